/*
 * qmpc_ground_run.h -- the fused launches of the fleet run and the loop run on terrain rows (qmpc_terrain.h) and on a
 * height-field bank (qmpc_field.h), as a per-handle switch (same library, same ABI version).
 *
 * Both run calls put everything between two MPC solves into one launch, and both were written for the flat plant: with
 * terrain rows or a bank bound they fall back to the per-tick sequence their headers spell out, four to ten launches a
 * tick, and say so in their info struct's `reason`.  With this switch on, a plant on rows and / or a bank with SCHEDULED
 * contact is served by a fused launch too: the same launch plan (one launch and one solve per 13 ticks in lockstep, two
 * small launches and the solve per tick with the per-robot schedule), and the per-tick sequence's result, bit for bit, in
 * every array the two run headers list and in the `support` and `ground` arrays of qmpc_terrain.h; for the loop run also
 * the episode manager's arrays, and the result log as a set.  The loop run's reset stage stands a finished robot on its
 * ground as qmpc_plant_reset does there.  (Bit for bit, with a NaN for a NaN: a robot that walks on NaNs -- a NaN mass,
 * say -- has NaN efforts on both paths, but the SIGN of a NaN that an instruction made of two NaNs is its operand order,
 * which two compilations of one source text need not share.)
 *
 * Covered with the switch on: rows alone, a bank alone, a bank on rows; both robot modes and both schedules; with or
 * without per-robot plant parameters and statistics; the loop run's actuator stage and episode step in any combination,
 * and neither (the fleet run).  The kernels are the loop run's kernel file compiled twice more, once for rows and once
 * for a bank (the build's QMPC_LOOP_GROUND 1 and 2); all sixteen instantiations hold the flat kernels' terms: no LDS, no
 * scratch, one wave per SIMD.  No combination of ground, parameters and statistics is routed back.
 *
 * NOT covered: contact decided by the ground (qmpc_contact.h).  Its step is a body of its own, already declared for one
 * wave per SIMD with 59 to 72 scalar spills, and it stays a fallback with the switch on: `reason` is then the contact bit
 * alone, whatever ground is bound under it.
 *
 * The default is 0, and qmpc_ctrl_init sets it: a handle that never calls this header behaves as before, reasons and
 * counts included.  The switch is read by the next run call; a captured graph keeps what it captured.  With the switch
 * on, `reason` in both info structs holds only the bits of what is bound AND the fused kernels do not cover; ticks
 * served on ground count as fused_ticks and fused_launches.
 *
 * Errors: QMPC_ERR_ARG for a null handle or pointer, QMPC_ERR_STATE before qmpc_ctrl_init.
 */
#ifndef QMPC_GROUND_RUN_H
#define QMPC_GROUND_RUN_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on: 0 (the default after qmpc_ctrl_init) / not 0. */
int qmpc_ground_run_enable(qmpc_handle h, int on);
/* *on: 0 / 1 as the next run call will read it. */
int qmpc_ground_run_enabled(qmpc_handle h, int* on);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_GROUND_RUN_H */
