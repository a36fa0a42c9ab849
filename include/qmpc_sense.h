/*
 * qmpc_sense.h -- a sensor model on the device between the reduced-order plant of qmpc_plant.h and the controller's
 * sensor path (qmpc_ctrl_tick of qmpc_ctrl.h: VectorNav orientation estimator, Kalman filter, yaw re-basing).  Same
 * library, same handle, same ABI version: nothing of qmpc_ctrl.h, qmpc_plant.h or qmpc_plant_vary.h changes.
 *
 * One qmpc_sense per control period turns the plant's last read-out (qmpc_plant_view's state / motor) into what the
 * robot's sensors would report: imu[B][10] and motor[B][24] in qmpc_ctrl.h's layouts.  A run of
 *     qmpc_ctrl_tick -> qmpc_plant_step -> qmpc_sense
 * is a closed loop through the estimators with no host in it.  qmpc_sense allocates nothing and only enqueues one
 * kernel, so the loop can be captured into a graph (in lockstep a captured block holds a multiple of 13 ticks, see
 * qmpc_ctrl.h); the noise goes on across replays because its counter is device state.  qmpc_plant_vary.h varies what
 * the PLANT is not told; this header varies what the ESTIMATOR is told.
 *
 * The model (fp64, no contraction, one operation at a time; restated in tests/sense_model.py, which agrees with the
 * kernel bit for bit -- there is no transcendental function in the path):
 *
 * Ideal sensor (nothing bound): imu = (state[13..15], state[1], state[2], state[3], state[0], state[7..9]) -- the
 *   accelerometer's specific force, the quaternion as x y z w, the gyro -- and motor_out = motor, copied bit for bit.
 *   The quaternion is always passed through (attitude error is out of scope).
 * Channels of a robot: 0..2 accelerometer axes, 3..5 gyro axes, 6..17 joint angles, 18..29 joint rates.  A channel of
 *   robot b reads out = x + d, and only when a term of d is bound (otherwise out = x, the same bits):
 *       d = 0;   d = sigma_b * z   when the channel's sigma is bound;   d = bias_b + d   when its bias is bound
 *   (accelerometer and gyro only: the encoders have no bias term).
 * Noise: counter-based, no generator state.  For channel c of robot b, with the robot's counters n_b and epoch_b,
 *       w[0..3] = Philox4x32-10(counter = (b, n_b, c, epoch_b), key = (seed low word, seed high word))
 *       z = (double(w0 + w1 + w2 + w3, summed as uint64) - 8589934590.0) * (1.7320508075688772 * 2^-32):
 *   the centred sum of four uniform words scaled to unit variance (Irwin-Hall, n = 4: excess kurtosis -0.3), so
 *   |z| <= 2 sqrt(3) -- no outlier, whatever the seed.  Philox4x32-10 is Random123's: multipliers 0xD2511F53 (on counter
 *   word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9 / 0xBB67AE85 between the ten rounds, a round maps
 *   (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
 *   A reading is reproducible from (seed, b, epoch_b, n_b, c) alone.  qmpc_sense advances n_b; qmpc_sense_reset starts a
 *   new epoch, so a reset episode draws fresh noise and not the first episode's again.
 *
 * WARM-UP.  The Kalman filter starts at xhat = 0, P = 100 I while the body stands at 0.29 m.  Closing the loop from
 * tick 0 through the sensor path makes the fleet fall: on the 16 commands of the closed-loop tests, 650 ticks at
 * 500 Hz, 4 of 16 robots stay safe in robot mode 0 and 6 of 16 in mode 1 (CPU restatement with the reference's
 * qpOASES).  The reference's own protocol exists for this reason -- init_controller, pre_work ..., then torques: run
 * qmpc_sense -> qmpc_ctrl_prework on the standing plant first.  With 5, 13, 50 or 300 such calls all 16 robots stay
 * safe in both modes and every solve returns 0, ideal sensors or noisy ones (per-robot accelerometer bias within
 * +-0.2 m/s^2 with white noise sigma 0.3, gyro bias within +-0.02 rad/s with sigma 0.02, encoders sigma 0.002 rad and
 * 0.05 rad/s): heights stay in 0.245 .. 0.29 m, roll within 0.04 rad, pitch within 0.07 rad, the last second's mean
 * speed within 0.013 m/s of the command, the filter's height error at the end below 3 mm.  Other noise seeds move the
 * statistics by at most 0.39 of the closed-loop tests' envelope.
 *
 * Out of scope: sensor latency, attitude error, contact sensing.  (The warm-up of a single robot that is reset while its
 * neighbours walk: qmpc_episode_sense.h.)
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init, and before qmpc_sense_init for every call but
 * qmpc_sense_init itself; QMPC_ERR_ARG for a batch other than the plant's, a null output or view, or an output pointer
 * equal to one of the plant's own state / motor buffers (the kernel reads those while it writes the outputs).  A later
 * qmpc_plant_init with the same batch keeps the sensors; with another batch they must be initialised again.
 */
#ifndef QMPC_SENSE_H
#define QMPC_SENSE_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-owned DEVICE arrays, double, one row per robot.  A NULL member: that term is absent (not zero). */
typedef struct {
  const double* acc_bias;    /* [B][3] m/s^2, body frame   */
  const double* gyro_bias;   /* [B][3] rad/s               */
  const double* acc_sigma;   /* [B]                        */
  const double* gyro_sigma;  /* [B]                        */
  const double* q_sigma;     /* [B]    rad, all 12 joints  */
  const double* qd_sigma;    /* [B]    rad/s               */
} qmpc_sense_params;

/* After qmpc_plant_init.  Allocates the per-robot counters n[B] and epoch[B] for the handle's max_batch (once), sets
 * n = 0 and epoch = 0 on the stream, keeps the seed and unbinds the parameters. */
int qmpc_sense_init(qmpc_handle h, int batch, uint64_t seed, void* stream);

/* Bind the arrays (host state only: nothing is enqueued, nothing is copied).  Every later qmpc_sense reads them at
 * launch: the pointers are captured, the values are not (qmpc_plant_set_params' contract, including: a non-finite value
 * affects that robot only).  prm == NULL or six NULL members unbind. */
int qmpc_sense_set_params(qmpc_handle h, int batch, const qmpc_sense_params* prm);

/* For the robots whose mask_dev[b] (uint8, device) is non-zero, NULL: for all, epoch += 1 and n = 0; one small kernel. */
int qmpc_sense_reset(qmpc_handle h, int batch, const uint8_t* mask_dev, void* stream);

/* One control period: the plant's state / motor and (n, epoch) -> imu_out[B][10], motor_out[B][24] (device, double),
 * n += 1.  One kernel launch, nothing else; it writes nothing of the plant's or the controller's. */
int qmpc_sense(qmpc_handle h, int batch, double* imu_out, double* motor_out, void* stream);

/* Device views of the counters (valid until the handle is destroyed); read-only by contract. */
typedef struct {
  const int32_t* n;      /* [B] qmpc_sense calls since qmpc_sense_init or the robot's last reset */
  const int32_t* epoch;  /* [B] resets since qmpc_sense_init */
  int batch;
  uint64_t seed;
} qmpc_sense_view;
int qmpc_sense_view_get(qmpc_handle h, qmpc_sense_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_SENSE_H */
