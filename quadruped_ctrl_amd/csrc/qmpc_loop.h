// qmpc_loop.h -- the argument block of the loop kernel (include/qmpc_loop.h; kernel: qmpc_loop.hip) and its launcher.
//
// The launch plan is the span's (qmpc_span.h: plan_spans), unchanged: a launch starts with C, P of the tick that has just
// solved, runs every stage of the ticks that follow, and ends behind E, L of the next tick that solves.  The loop kernel
// puts two more stages into a tick,  E  L  [solve]  C  A  P  R :  A, the actuators, between the leg command and the plant
// step; R, the episode step with the resets it orders, behind the plant step of a check tick.  Both stand behind the
// solve, so neither moves a launch boundary.
#ifndef QMPC_LOOP_DEV_H
#define QMPC_LOOP_DEV_H

#include "qmpc_act.h"
#include "qmpc_episode.h"
#include "qmpc_span.h"

// What the two stages read beside the span's block, filled in one place (qmpc_capi_ctrl.cpp: qmpc_loop_run).  By value.
struct QmpcLoopArgs {
  QmpcSpanArgs X;   // the span's block: controller, plant, the caller's three rows
  // stage A (act != 0)
  QmpcActArgs A;    // qmpc_act's block: motor = the plant's own motor rows, dt = 1 / freq
  int act;
  int act_stats;    // R's actuator reset also clears the accumulators
  // stage R (every != 0): behind P of the call's tick k where (k + 1) % every == 0
  int every;
  int decide;       // the rule has causes: the decision and the resets run (0: only the actuators' reset under the mask)
  QmpcEpisodeDev E;
  QmpcEpisodeIn In;
  qmpc_episode_rule R;
  qmpc_episode_bind Bd;
};

// The block of the kernel's ground compiles (qmpc_loop.hip with -DQMPC_LOOP_GROUND=1: terrain rows, =2: a height-field
// bank; include/qmpc_ground_run.h): the ground travels BEHIND the flat block, so the default compile's kernarg segment
// is the flat block alone, as it always was.  T.rows may be null under a bank (qmpc_field.hip).
struct QmpcLoopGroundArgs : QmpcLoopArgs {
  QmpcTerrainArgs T;  // the plant's ground(): rows as bound, ground[], support[], both bindings' flags
  QmpcFieldArgs Fd;   // the bank and the placement rows (QMPC_LOOP_GROUND == 1 reads none of it)
};

// robot_mode, vary, stats, first_at_c, ticks, last_after_l: as qmpc_launch_span.  tick0: the call's index of the launch's
// first tick (which ticks are check ticks); t_mod13: the controller's T modulo 13 when the launch is enqueued (lockstep:
// a reset robot's counter restarts at T mod 13 of ITS tick; the kernel counts its L stages on top).
extern "C" hipError_t qmpc_launch_loop(const QmpcLoopArgs* A, int robot_mode, int vary, int stats, int first_at_c,
                                       int ticks, int last_after_l, int tick0, int t_mod13, hipStream_t stream);
// ... and of the two ground compiles: the same file, the launcher's name by its define.  With act = every = 0 these serve
// the fleet run on ground: there is no ground compile of the span kernel.
extern "C" hipError_t qmpc_launch_loop_terrain(const QmpcLoopGroundArgs* A, int robot_mode, int vary, int stats,
                                               int first_at_c, int ticks, int last_after_l, int tick0, int t_mod13,
                                               hipStream_t stream);
extern "C" hipError_t qmpc_launch_loop_field(const QmpcLoopGroundArgs* A, int robot_mode, int vary, int stats,
                                             int first_at_c, int ticks, int last_after_l, int tick0, int t_mod13,
                                             hipStream_t stream);

#endif
