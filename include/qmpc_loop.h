/*
 * qmpc_loop.h -- the fleet's long-running loop, many ticks in one call (same library, same ABI version): the closed loop
 * of controller and plant with the actuator stage and the episode manager INSIDE the launch that runs everything between
 * two MPC solves.  qmpc_loop_run(ticks, opts) leaves exactly what
 *
 *     for (k = 0; k < ticks; ++k) {
 *       qmpc_ctrl_tick_state(h, batch, state, motor, effort, stream);
 *       if (opts->actuators)  the actuator header's apply call (h, batch, effort, effort, stream);      // in place
 *       qmpc_plant_step(h, batch, effort, state, motor, stream);
 *       if (opts->episodes_every && (k + 1) % opts->episodes_every == 0) {
 *         qmpc_episode_step(h, batch, opts->episodes_every, stream);
 *         if (opts->actuators)  the actuator header's reset call (h, batch, the manager's mask, NULL,
 *                                                                opts->actuator_stats, stream);
 *       }
 *     }
 *
 * leaves, bit for bit: effort, state and motor; every controller array qmpc_debug_ctrl_read knows (the due list's ORDER
 * excepted, which neither path defines: compare per robot); every array of qmpc_plant_view and the plant's statistics;
 * the actuators' ring, head, age and seven accumulators; every array of qmpc_episode_view, the bound vel / gait arrays,
 * T and the per-robot counters; and the result log as a SET of rows keyed by (robot, episode) -- the done robots of a
 * wave take consecutive rows behind one atomic add, and a wave holds 16 robots here and 64 on the per-tick path, so the
 * order of the rows differs between the two as it may between two runs of either.
 *
 * What changes is how the work is enqueued.  On a check tick the sequence above is ten launches and the solve; here
 * everything between two MPC solves is ONE launch of a kernel that loops over the ticks (csrc/qmpc_loop.hip), under the
 * launch plan of the plain fused loop: in lockstep one launch and one solve per 13 ticks, with the per-robot schedule
 * two small launches and the solve per tick.  The actuator stage and the episode step add no launch.
 *
 * The fused kernel covers what the plain fused loop covers: the state-driven tick in both robot modes and both
 * schedules, on the flat plant with scheduled contact, with or without per-robot plant parameters and statistics.  With
 * terrain rows, contact decided by the ground or a height field bound the call FALLS BACK unless the handle's ground-run
 * switch is on and contact is scheduled: it enqueues the sequence above, exactly, and says so in qmpc_loop_info.reason.
 * qmpc_ground_run.h has the switch, which lets terrain rows and height fields run fused too -- the reset stage then
 * stands a robot on its ground -- and says what `reason` holds then.  With all three options 0 the call is the plain
 * fused loop.
 * Where the episode rule's `causes` are 0, qmpc_episode_step enqueues nothing and the fused call runs no reset stage.
 *
 * The call only enqueues, on `stream`, and allocates nothing: it can be captured into a graph.  The host decides the
 * lockstep MPC ticks, and the counter a robot reset in lockstep restarts at, from its own count T, which a replay does
 * not advance: in lockstep a captured block holds a multiple of 13 ticks (qmpc_ctrl.h).  The bound per-robot arrays of
 * the actuators, the plant and the manager are read at every tick, as on the per-tick path: rewrite them in place
 * between calls or replays.
 *
 * Errors.  QMPC_ERR_STATE: before qmpc_ctrl_init or qmpc_plant_init; with `actuators` before the actuators' init; with
 * `episodes_every` before qmpc_episode_init and qmpc_episode_set.  QMPC_ERR_ARG: a null handle, `opts` or pointer, a
 * batch other than the controller's, ticks < 1, a negative episodes_every, or ticks that are no multiple of it; with
 * episodes on, state / motor that are not the plant's own read-out rows (qmpc_plant_view.state / .motor: the plant's
 * reset writes only those, and the loop would carry on from stale caller rows); with actuators on, an effort buffer that
 * overlaps the plant's motor rows (the actuator stage reads the joint rates there while it writes the effort).  A
 * refused call enqueues nothing and counts nothing; a call that stops on a device error has counted what it enqueued.
 */
#ifndef QMPC_LOOP_H
#define QMPC_LOOP_H

#include "qmpc_episode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Why a call fell back to the per-tick launches (qmpc_loop_info.reason, a bit set; 0: it ran fused).  The values are
 * those of the plain fused loop's reasons. */
enum {
  QMPC_LOOP_TERRAIN = 1, /* terrain rows are bound (qmpc_terrain.h) */
  QMPC_LOOP_CONTACT = 2, /* contact is decided by the ground (qmpc_contact.h) */
  QMPC_LOOP_FIELD = 4    /* a height field is bound (qmpc_field.h) */
};

typedef struct {
  int actuators;      /* 0 / 1: the actuator stage between the leg command and the plant step */
  int episodes_every; /* 0: no episode manager; k >= 1: an episode step behind the plant step of every k-th tick of the call */
  int actuator_stats; /* with actuators and episodes: the reset of a finished robot also clears its accumulators */
} qmpc_loop_opts;

/* `ticks` ticks of the loop above from where the handle stands.  effort[B][12], state[B][16], motor[B][24]: device,
 * double, the layouts of qmpc_ctrl_tick_state and qmpc_plant_step; on entry state and motor hold the plant's current
 * read-out, on return (of the stream) all three are as the last tick left them. */
int qmpc_loop_run(qmpc_handle h, int batch, int ticks, const qmpc_loop_opts* opts, double* effort, double* state,
                  double* motor, void* stream);

/* How the ticks of qmpc_loop_run were served since qmpc_ctrl_init (host-side counts of what was enqueued; a replayed
 * graph is not counted again). */
typedef struct {
  long long ticks;          /* ticks qmpc_loop_run enqueued */
  long long fused_ticks;    /* ... served by a fused launch */
  long long fused_launches; /* fused launches */
  long long fallback_ticks; /* ... served by the per-tick launches */
  int reason;               /* QMPC_LOOP_* of the last call; 0: it ran fused */
} qmpc_loop_info;
int qmpc_loop_run_info(qmpc_handle h, qmpc_loop_info* out);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_LOOP_H */
