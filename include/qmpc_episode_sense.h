/*
 * qmpc_episode_sense.h -- fleet episodes on the SENSOR path: the episode manager of qmpc_episode.h and the sensor model
 * of qmpc_sense.h in one loop (same library, same handle, same ABI version: nothing of the other headers changes).
 * A run of
 *     qmpc_ctrl_tick -> qmpc_plant_step -> qmpc_episode_sense_step -> qmpc_sense
 * is a closed loop through the real estimators (VectorNav orientation, Kalman filter) in which a fallen robot is put
 * back on its feet AND warmed up, with no host in it.  qmpc_episode_sense_step allocates nothing and only enqueues, so
 * the loop can be captured into a graph (in lockstep a captured block holds a multiple of 13 ticks, see qmpc_ctrl.h);
 * the warm-up counters are device state and go on across replays.
 *
 * WHY.  A robot that has just been reset must see the warm-up of qmpc_sense.h for itself: W control periods of pre_work
 * only -- estimators and leg data -- on the standing plant, or its Kalman filter (xhat = 0, P = 100 I, the body at
 * 0.29 m) makes it fall again.  The controller's kernels run on the whole batch and take no mask.  So the whole tick
 * and the plant step run for everybody, and for a robot in warm-up this step then UNDOES everything except what
 * pre_work would have done:
 *   controller  every array is written as qmpc_ctrl_init writes it EXCEPT the pre_work set, which is kept: q, qd,
 *               leg_J, leg_p, leg_v, kf_p, kf_v, orientation, rpy, r_body, omega_body, omega_world, a_world,
 *               ori_ini_inv, xhat, P, position, v_world, v_body, first_visit.  Everything else is as after init:
 *               contact_phase 0.5, safe 1, f_ff = grf = 0, first_run 1, the gait state, status, the integrators, the
 *               commands (which step 3 below hands over again).  The counter restarts as under qmpc_ctrl_reset: at 0 with
 *               the per-robot schedule, at T mod 13 in lockstep.
 *   plant       qmpc_plant_reset's launches with the robot's row of qmpc_episode_view's xyyaw: the body stands where it
 *               was put, whatever the wasted step did to it; the statistics of qmpc_plant_vary.h are reset too while on.
 *   sensors     nothing: the qmpc_sense that follows reads the standing read-out and advances n, as in the warm-up.
 * A held period is, bit for bit, qmpc_sense -> qmpc_ctrl_prework on a fresh robot, and W of them are the warm-up of
 * qmpc_sense.h for that robot alone, while its neighbours walk.
 * COST.  A held robot's tick, solve and plant step are computed and thrown away, and a step is one launch more than
 * qmpc_episode_step's, plus qmpc_sense_reset's: the decision, the re-initialisation, the commands, the plant's reset
 * (two launches with contact on), the statistics' (while on), the sensors' -- five to seven small launches on every
 * tick.  A tick that skips held robots is out of scope.
 *
 * State per robot (device, allocated once for the handle's max_batch by qmpc_episode_sense_init):
 *   warm   int32   control periods of warm-up the robot still has in front of it
 *   hold   uint8   scratch: 1 for the robots the last qmpc_episode_sense_step held
 *
 * One qmpc_episode_sense_step (one control period: `elapsed` of qmpc_episode_step is 1 by definition):
 *  1. the decision kernel, one lane per robot.  warm[b] > 0: warm[b] -= 1, hold[b] = 1, mask[b] = 0 -- the robot is NOT
 *     judged: its age does not move, it gets no log row, no counter moves.  Otherwise hold[b] = 0 and exactly the
 *     decision of qmpc_episode_step(elapsed = 1) -- age, rule, log row, counters, draw (the same (seed, b, episode)),
 *     xyyaw, start, the vel / gait rows, mask, episode --, and a done robot also gets warm[b] = warm_ticks.  With
 *     causes == 0 nobody is judged; robots in warm-up are still held.
 *  2. the controller's re-initialisation in ONE launch: full for mask (what qmpc_ctrl_reset does), all but the pre_work
 *     set for hold.  Rows of `effort` (the tick's output; may be NULL) are zeroed for both sets.
 *  3. the bound vel / gait handed to the controller for the whole batch, as in qmpc_episode_step.
 *  4. the plant's reset under mask | hold with xyyaw, on flat ground, terrain, field and with contact.
 *  5. the statistics' reset under the same union, while they are enabled.
 *  6. qmpc_sense_reset's launch under mask only: a new noise epoch once per episode, not per held period.
 * A robot that finishes at step t is reset there, held at steps t+1 .. t+W (W pre_works), judged again from step
 * t+W+1, where its age becomes 1.  W = 0 is qmpc_episode_step followed by qmpc_sense_reset(mask).
 *
 * qmpc_episode_sense_hold puts robots into warm-up by hand: the initial settle of the whole fleet (mask NULL) through
 * the same mechanism, or the warm-up of robots the caller has reset themselves (qmpc_ctrl_reset, qmpc_plant_reset,
 * qmpc_sense_reset, then this, between qmpc_episode_sense_step and qmpc_sense).  It also writes the robot's row of xyyaw:
 * the plant's current x, y and yaw = 2 atan2(q_z, q_w), adjusted by at most four steps of a double so that a reset
 * reproduces q_w, q_z exactly -- a robot that a reset has just placed is held on the very pose it stands in; where no such
 * double exists (a body that is not upright) the yaw is the arc tangent's.  And it writes the robot's start = that x, y,
 * so that RANGE is judged from where the robot is held.  The age, the episode number, the counters and the log are the
 * manager's own and are left alone: a caller who resets robots by hand and wants a time limit counted from there lets
 * the manager end the episode instead.
 *
 * Out of scope: a tick that skips held robots; checking every k-th tick (`elapsed` > 1) on the sensor path; contact
 * sensing; the MPC warm start's per-robot working sets, which a held robot keeps as a robot under qmpc_ctrl_reset does.
 *
 * Errors as in qmpc_episode.h: QMPC_ERR_STATE before qmpc_episode_init or qmpc_sense_init, and before
 * qmpc_episode_sense_init for every call but qmpc_episode_sense_init itself; qmpc_episode_sense_step before
 * qmpc_episode_set is QMPC_ERR_STATE too.  QMPC_ERR_ARG for a batch other than the plant's, warm_ticks < 0, ticks < 0, or
 * a null view.
 */
#ifndef QMPC_EPISODE_SENSE_H
#define QMPC_EPISODE_SENSE_H

#include "qmpc_episode.h"
#include "qmpc_sense.h"

#ifdef __cplusplus
extern "C" {
#endif

/* After qmpc_episode_init and qmpc_sense_init.  Allocates warm and hold for the handle's max_batch (once), zeroes both on
 * the stream and keeps warm_ticks >= 0: the warm-up a robot gets when the manager resets it. */
int qmpc_episode_sense_init(qmpc_handle h, int batch, int warm_ticks, void* stream);

/* warm[b] = ticks >= 0, xyyaw[b] = the plant's x, y, yaw and start[b] = its x, y for the robots whose mask_dev[b] (uint8,
 * device) is non-zero, NULL: for all; one small kernel. */
int qmpc_episode_sense_hold(qmpc_handle h, int batch, const uint8_t* mask_dev, int ticks, void* stream);

/* One control period, between qmpc_plant_step and qmpc_sense on every tick.  effort: the tick's output [B][12] (device,
 * double), whose rows are zeroed for the robots reset or held; or NULL.  Allocates nothing and only enqueues. */
int qmpc_episode_sense_step(qmpc_handle h, int batch, double* effort, void* stream);

/* Device views of the state (valid until the handle is destroyed); read-only by contract. */
typedef struct {
  const int32_t* warm; /* [B] */
  const uint8_t* hold; /* [B] */
  int warm_ticks;
  int batch;
} qmpc_episode_sense_view;
int qmpc_episode_sense_view_get(qmpc_handle h, qmpc_episode_sense_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_EPISODE_SENSE_H */
