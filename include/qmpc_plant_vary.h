/*
 * qmpc_plant_vary.h -- per-robot body, friction and pushes for the reduced-order plant of qmpc_plant.h, and per-robot
 * statistics of a run kept on the device.  Same library, same handle, same ABI version: nothing of qmpc_plant.h changes,
 * and a plant with nothing bound and the statistics off steps exactly as that header describes.
 *
 * qmpc_plant.h's plant reads the handle's own mass and inertia and one mu_plant: it is the model the MPC plans on.
 * Here the PLANT is given what the controller was not told -- a payload, another floor under each robot, a shove in the
 * side.  The controller and the solve are not told: qmpc_set_robot stays fleet-wide and stays the MPC's model.  That
 * mismatch is the point.
 *
 * The model changes only in step 2 of qmpc_plant.h's description (fp64, no contraction, one operation at a time; restated
 * in tests/plant_model_varied.py), for robot b:
 *   2a. cap = mu_b f_z (the cone of the robot's own floor).
 *   2b. F = ((f_0 + f_1) + (f_2 + f_3)) + force_b; n = ((n_0 + n_1) + (n_2 + n_3)) + torque_b, component by component
 *       after the quad sum, and only when the member is bound.  force_b acts on the body origin in the WORLD frame,
 *       torque_b is a moment in the BODY frame.
 *   2c. vdot = F / m_b + (0, 0, -g); wdot = I_b^-1 (n - w x I_b w).
 * The read-out is unchanged, so the accelerometer rows feel the push; the grf view stays the ground's reactions only.
 *
 * Still out of scope: per-robot constants in the MPC (the solve keeps one mass, inertia, mu and f_max per handle);
 * centre-of-mass offsets, slip, contact detection (the plant stays "not a physics engine").  (The sensor path closed
 * loop -- plant -> imu -> qmpc_ctrl_tick's estimators -- is qmpc_sense.h; per-robot slopes and stairs are qmpc_terrain.h.)
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init (and, for the statistics' reset and get, before the
 * first enable); QMPC_ERR_ARG for a batch other than the plant's or a null view.
 */
#ifndef QMPC_PLANT_VARY_H
#define QMPC_PLANT_VARY_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-owned DEVICE arrays, one row per robot.  A NULL member keeps qmpc_plant.h's value for every robot. */
typedef struct {
  const double* mass;    /* [B]     kg;            NULL: the handle's (qmpc_set_robot) */
  const double* ibody;   /* [B][3]  body inertia diagonal; NULL: the handle's */
  const double* mu;      /* [B]     ground friction; NULL: qmpc_plant_init's mu_plant */
  const double* force;   /* [B][3]  external force on the body origin, WORLD frame, N;  NULL: none */
  const double* torque;  /* [B][3]  external moment, BODY frame, N m;                   NULL: none */
} qmpc_plant_params;

/* Bind the arrays (host state only: nothing is enqueued, nothing is copied).  Every later qmpc_plant_step reads them at
 * launch: the pointers are captured, the values are not, so the caller changes a push by writing into its own array on
 * the stream, between eager steps or between replays of a captured graph.  prm == NULL or five NULL members unbind.
 * qmpc_plant_init unbinds (a new plant is the plain plant); qmpc_plant_reset keeps the binding.  The values are the
 * caller's responsibility like every device input: a non-finite or non-positive value affects that robot only. */
int qmpc_plant_set_params(qmpc_handle h, int batch, const qmpc_plant_params* prm);

/* Per-robot statistics, updated by every qmpc_plant_step while enabled, at the new pose, by the lane that writes the
 * robot's state row: n += 1; z_min / z_max over p_z; roll_max / pitch_max over |roll|, |pitch| with
 *     roll = atan2(2 (y z + w x), 1 - 2 (x^2 + y^2)),  pitch = asin(clamp(2 (w y - x z), -1, 1));
 * vx_sum += state[10], vy_sum += state[11] (body-frame velocity).  A window's mean is the difference of two reads
 * divided by the difference of n.  The statistics of a robot whose state is non-finite are unspecified; the other
 * robots' are not affected.
 *
 * The first enable allocates the arrays for the handle's max_batch and synchronises the device, once: every robot
 * starts with n = 0, z_min = +inf, z_max = -inf, roll_max = pitch_max = 0, sums 0.  After that enable / disable is
 * host state only (a disabled plant keeps the values).  qmpc_plant_init leaves the switch and the values alone. */
int qmpc_plant_stats_enable(qmpc_handle h, int on);

/* The initial values again for the robots whose mask_dev[b] (uint8, device) is non-zero, NULL: for all; one small
 * kernel on the stream. */
int qmpc_plant_stats_reset(qmpc_handle h, int batch, const uint8_t* mask_dev, void* stream);

/* Device views of the accumulators, [B] each (valid until the handle is destroyed); read-only by contract. */
typedef struct {
  const int32_t* n;
  const double* z_min;
  const double* z_max;
  const double* roll_max;
  const double* pitch_max;
  const double* vx_sum;
  const double* vy_sum;
  int batch;
  int enabled;
} qmpc_plant_stats;
int qmpc_plant_stats_get(qmpc_handle h, qmpc_plant_stats* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_PLANT_VARY_H */
