/*
 * qmpc_episode.h -- fleet episodes on the device for the closed loop of qmpc_ctrl.h and qmpc_plant.h (same library,
 * same handle, same ABI version: nothing of the other headers changes): who is done, where that robot starts again,
 * what it is told to do next, and a record of how each run ended.  A run of
 *     qmpc_ctrl_tick_state -> qmpc_plant_step -> qmpc_episode_step
 * is a closed loop in which a fallen robot is put back on its feet with no host in it.  qmpc_episode_step allocates
 * nothing and only enqueues, so the loop can be captured into a graph (in lockstep a captured block holds a multiple of
 * 13 ticks, see qmpc_ctrl.h); ages, episode numbers and the log go on across replays because they are device state.
 *
 * The model (fp64, no contraction, one operation at a time, no transcendental function; the decision and the draw are
 * the inline functions of csrc/qmpc_episode_rule.h, which the kernel and a host program compile from the same text, and
 * tests/episode_model.py restates them, the bookkeeping and the log in numpy and agrees bit for bit):
 *
 * State per robot (device, allocated once for the handle's max_batch by qmpc_episode_init):
 *   age         int32     control periods since the robot's last reset (it saturates at INT32_MAX)
 *   episode     int32     episodes finished so far: the index of the running one
 *   start[2]    double    world x, y of the running episode's start
 *   count[6]    int32     how often each cause (bit 0 .. 5 below) ended an episode; causes that hold at once all count
 *   ticks_sum   int64     the sum of the finished episodes' lengths (their age when they ended)
 *   last_cause, last_ticks  int32  the cause set and the length of the episode finished last (0 before the first)
 *   mask        uint8     scratch: 1 for the robots the last qmpc_episode_step reset
 *   xyyaw[3]    double    scratch: where such a robot was put (a row is rewritten only when its robot is reset)
 * and two device words, log_count (rows of the log written) and log_dropped (rows that found it full).
 *
 * Rule (qmpc_episode_rule; the scalars are host state and travel as kernel arguments, like qmpc_contact_params).
 * `causes` is the set of enabled criteria, all evaluated on the pose qmpc_plant_step left (qmpc_plant_view's p, q) and on
 * the controller's view after the tick (qmpc_ctrl_view's safe), with tilt = 1 - 2 (qx^2 + qy^2) -- the world-z component
 * of the body's z axis, computed as xx = qx qx, yy = qy qy, s = xx + yy, t = 2 s, tilt = 1 - t --, dx = p_x - start_x,
 * dy = p_y - start_y and height = p_z - ground_b, where ground_b is the plant's `ground` row (qmpc_terrain_view) while
 * the plant maintains it -- terrain rows or a height field bound, or contact flags set -- and 0 otherwise:
 *   QMPC_EP_UNSAFE     safe[b] == 0
 *   QMPC_EP_NONFINITE  any of p[0..2], q[0..3] is not finite
 *   QMPC_EP_TILT       tilt < cos_tilt_min
 *   QMPC_EP_HEIGHT     height < z_min
 *   QMPC_EP_RANGE      |dx| > range or |dy| > range, i.e. max(|dx|, |dy|) > range: a robot about to walk off its map
 *   QMPC_EP_TIMEOUT    age >= max_ticks
 * cause = the set of all enabled criteria that hold at once; a robot is done iff cause != 0.  A NaN compares false
 * everywhere except in NONFINITE, and a threshold that is not finite (cos_tilt_min, z_min, range: NaN or +-inf)
 * switches its criterion off: it never fires.  There is no atan2 or asin: a host restatement decides the same bits.
 *
 * Bindings (qmpc_episode_bind): caller-owned DEVICE arrays, read -- and vel, gait, log written -- at launch.  The
 * pointers are captured, the values are not (qmpc_plant_set_params' contract, including: rewrite them in place on the
 * stream, also between replays of a captured graph).
 *   vel[B][3], gait[B]   required: the fleet's commands as qmpc_ctrl_set_vel / qmpc_ctrl_set_gait take them.  The
 *                        manager hands them to the controller at every step, and writes a reset robot's rows.
 *   spawn[S][3]          (x, y, yaw), n_spawn = S >= 1; with the flag QMPC_EP_SPAWN_PER_ROBOT the table is [B][S][3]:
 *                        every robot has its own S rows (robots placed on maps of their own)
 *   commands[C][4]       (vx, vy, yaw rate, gait number), n_commands = C >= 1; or NULL: a reset robot keeps its rows
 *                        of vel / gait.  The gait column is clamped to [0, 31] (a NaN to 0) and then truncated to int32;
 *                        the velocities are copied as they are
 *   log[L][8]            log_rows = L >= 0; or NULL: nothing is logged and neither word moves
 *
 * Draws: counter-based, no generator state (the Philox4x32-10 of qmpc_sense.h).  A robot b that starts episode e
 * (e = 1 for the first one after a reset: the episode index AFTER the increment) draws
 *     w[0..3] = Philox4x32-10(counter = (b, e, 0, 0), key = (seed low word, seed high word))
 *     spawn row = floor(w0 S / 2^32)      command row = floor(w1 C / 2^32)        (the high word of the 64-bit product)
 * A draw is reproducible from (seed, b, e) alone.
 *
 * Log row of a finished episode, eight exact doubles: robot; episode index (before the increment); cause; age;
 * dx; dy; height; tilt.  Rows are appended wave by wave: the done lanes of a wave take consecutive places behind one
 * atomic add of its first done lane, so the order of the rows across waves is unspecified (sort by robot and episode).
 * A row that would land beyond L is not written and increments log_dropped; log_count never exceeds L.
 * qmpc_episode_log_clear zeroes both words on the stream.
 *
 * One qmpc_episode_step(elapsed):
 *  1. the decision kernel, one lane per robot: age += elapsed, evaluate the rule.  For a done robot: append the log
 *     row, update count / ticks_sum / last_*, draw, mask[b] = 1, xyyaw[b] = the spawn row, start = its x, y, age = 0,
 *     episode += 1, and with `commands` bound vel[b] and gait[b] = the command row.  Every other robot: mask[b] = 0.
 *  2. the existing resets with that mask, in this order: the controller's, exactly as qmpc_ctrl_reset does it (in
 *     lockstep the counter restarts at T mod 13); the commands, vel and gait, for the whole batch as qmpc_ctrl_set_vel
 *     / qmpc_ctrl_set_gait hand them over (qmpc_ctrl_reset zeroes a robot's commands; for the others this rewrites the
 *     values they have); the plant's with xyyaw, exactly as qmpc_plant_reset does it on flat ground, terrain, field
 *     and with contact; the statistics' of qmpc_plant_vary.h while they are enabled.
 *  With causes == 0 the step enqueues nothing and changes nothing.
 *
 * Out of scope here: episodes on the sensor path -- a reset robot needs the warm-up of qmpc_sense.h for itself, and
 * qmpc_ctrl_prework runs on the whole batch; nothing of qmpc_sense.h is called: qmpc_episode_sense.h does that, with this
 * header's rule, bindings, log and view.  Rewards and observations.  Anything inside the controller's or the plant's kernels.
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init, and before qmpc_episode_init for every call but
 * qmpc_episode_init itself; qmpc_episode_step before qmpc_episode_set is QMPC_ERR_STATE too.  QMPC_ERR_ARG for a batch
 * other than the plant's, unknown cause or flag bits, a null rule, bind, view, vel, gait or spawn, n_spawn < 1,
 * n_commands < 1 with commands bound, log_rows < 0, or elapsed < 1.  A later qmpc_plant_init with the same batch keeps
 * the episodes; with another batch they must be initialised again.
 */
#ifndef QMPC_EPISODE_H
#define QMPC_EPISODE_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the criteria: bits of qmpc_episode_rule.causes, of a log row's cause, and the index of count[] */
#define QMPC_EP_UNSAFE 1
#define QMPC_EP_NONFINITE 2
#define QMPC_EP_TILT 4
#define QMPC_EP_HEIGHT 8
#define QMPC_EP_RANGE 16
#define QMPC_EP_TIMEOUT 32
#define QMPC_EP_CAUSES 6 /* how many there are */

/* qmpc_episode_bind.flags */
#define QMPC_EP_SPAWN_PER_ROBOT 1

typedef struct {
  int causes;          /* QMPC_EP_* enabled; 0: the manager is off */
  int max_ticks;       /* TIMEOUT */
  double cos_tilt_min; /* TILT */
  double z_min;        /* HEIGHT, metres above the ground */
  double range;        /* RANGE, metres from the episode's start */
} qmpc_episode_rule;

typedef struct {
  double* vel;            /* [B][3] */
  int32_t* gait;          /* [B] */
  const double* spawn;    /* [S][3], or [B][S][3] with QMPC_EP_SPAWN_PER_ROBOT */
  const double* commands; /* [C][4], or NULL */
  double* log;            /* [L][8], or NULL */
  int n_spawn, n_commands, log_rows;
  int flags; /* QMPC_EP_SPAWN_PER_ROBOT */
} qmpc_episode_bind;

/* After qmpc_plant_init.  Allocates the state for the handle's max_batch (once), zeroes all of it on the stream, sets
 * start to the plant's p_x, p_y, keeps the seed; no rule is set and nothing is bound. */
int qmpc_episode_init(qmpc_handle h, int batch, uint64_t seed, void* stream);

/* The rule and the bindings (host state only: nothing is enqueued, nothing is copied). */
int qmpc_episode_set(qmpc_handle h, int batch, const qmpc_episode_rule* rule, const qmpc_episode_bind* bind);

/* After qmpc_plant_step: `elapsed` >= 1 control periods have passed since the previous call (a caller may check only
 * every k-th tick).  The decision kernel, then the resets above; allocates nothing and only enqueues. */
int qmpc_episode_step(qmpc_handle h, int batch, int elapsed, void* stream);

/* log_count = log_dropped = 0 on the stream: the next row lands in row 0 of the log. */
int qmpc_episode_log_clear(qmpc_handle h, void* stream);

/* Device views of the state (valid until the handle is destroyed); read-only by contract. */
typedef struct {
  const int32_t* age;         /* [B]    */
  const int32_t* episode;     /* [B]    */
  const double* start;        /* [B][2] */
  const int32_t* count;       /* [B][6] */
  const int64_t* ticks_sum;   /* [B]    */
  const int32_t* last_cause;  /* [B]    */
  const int32_t* last_ticks;  /* [B]    */
  const uint8_t* mask;        /* [B]    */
  const double* xyyaw;        /* [B][3] */
  const int32_t* log_count;   /* one word */
  const int32_t* log_dropped; /* one word */
  int batch;
  uint64_t seed;
} qmpc_episode_view;
int qmpc_episode_view_get(qmpc_handle h, qmpc_episode_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_EPISODE_H */
