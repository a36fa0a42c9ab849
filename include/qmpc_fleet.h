/*
 * qmpc_fleet.h -- the closed loop of qmpc_ctrl.h and qmpc_plant.h, many ticks in one call (same library, same ABI
 * version).  qmpc_fleet_run(ticks) leaves exactly what
 *
 *     for (k = 0; k < ticks; ++k) {
 *       qmpc_ctrl_tick_state(h, batch, state, motor, effort, stream);
 *       qmpc_plant_step(h, batch, effort, state, motor, stream);
 *     }
 *
 * leaves, bit for bit: effort, state and motor, every controller array qmpc_debug_ctrl_read knows (the due list's ORDER
 * excepted, which neither path defines: compare per robot), every array of qmpc_plant_view, the plant's statistics, T
 * and the per-robot counters.  What changes is how the work is enqueued.  The per-tick calls are four launches a tick
 * (and the solve on an MPC tick), each a dependent chain per lane behind a dispatch of its own.
 * Here everything between two MPC solves -- the leg command and plant step of the tick that solved, every stage of the
 * ticks that follow, the estimators and the locomotion stage of the next tick that solves -- is ONE launch of a kernel
 * that loops over the ticks (csrc/qmpc_span.hip): in lockstep one launch and one solve per 13 ticks, with the per-robot
 * schedule (a solve over the due list on every tick) two small launches and the solve per tick.
 *
 * The fused kernel covers the state-driven tick in both robot modes and both schedules, on the flat plant with
 * scheduled contact, with or without qmpc_plant_set_params and the statistics, at any `substeps` and any constants of the
 * handle (the kernel takes them at run time).  With terrain rows, contact decided by the ground or a height field
 * bound, the call FALLS BACK unless the handle's ground-run switch is on and contact is scheduled: it enqueues the
 * per-tick calls above, exactly, and says so in qmpc_fleet_info.reason.  qmpc_ground_run.h has the switch, which lets
 * terrain rows and height fields run fused too, and says what `reason` holds then.  The answer is the per-tick answer
 * either way.  Sensors, actuators and the episode managers
 * stand between the stages of a tick and keep their own loops (rollout_sensed, ... in the Python binding).
 *
 * The call only enqueues, on `stream`, and allocates nothing: it can be captured into a graph.  As with the per-tick
 * calls, the host decides the lockstep MPC ticks from its own count T, which a replay does not advance: in lockstep a
 * captured block holds a multiple of 13 ticks (qmpc_ctrl.h).  The first call starts the controller: it closes
 * qmpc_ctrl_set_schedule's window as a tick does.
 *
 * Errors: QMPC_ERR_STATE before qmpc_ctrl_init or qmpc_plant_init; QMPC_ERR_ARG for a batch other than the
 * controller's, ticks < 1 or a null pointer.  A refused call enqueues nothing and counts nothing; a call that stops on a
 * device error has counted the ticks it enqueued.
 */
#ifndef QMPC_FLEET_H
#define QMPC_FLEET_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Why a call fell back to the per-tick launches (qmpc_fleet_info.reason, a bit set; 0: it ran fused). */
enum {
  QMPC_FLEET_TERRAIN = 1, /* terrain rows are bound (qmpc_terrain.h) */
  QMPC_FLEET_CONTACT = 2, /* contact is decided by the ground (qmpc_contact.h) */
  QMPC_FLEET_FIELD = 4    /* a height field is bound (qmpc_field.h) */
};

/* `ticks` closed-loop ticks from where the pair stands.  effort[B][12], state[B][16], motor[B][24]: device, double, the
 * layouts of qmpc_ctrl_tick_state and qmpc_plant_step; on entry state and motor hold the plant's current read-out, on
 * return (of the stream) all three are as the last tick left them. */
int qmpc_fleet_run(qmpc_handle h, int batch, int ticks, double* effort, double* state, double* motor, void* stream);

/* How the ticks of qmpc_fleet_run were served since qmpc_ctrl_init (host-side counts of what was enqueued; a replayed
 * graph is not counted again). */
typedef struct {
  long long ticks;          /* ticks qmpc_fleet_run enqueued */
  long long fused_ticks;    /* ... served by the span kernel */
  long long fused_launches; /* launches of the span kernel */
  long long fallback_ticks; /* ... served by the per-tick launches */
  int reason;               /* QMPC_FLEET_* of the last call; 0: it ran fused */
} qmpc_fleet_info;
int qmpc_fleet_run_info(qmpc_handle h, qmpc_fleet_info* out);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_FLEET_H */
