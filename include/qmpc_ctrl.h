/*
 * qmpc_ctrl.h -- batched locomotion controller on top of the C ABI of qmpc.h (same library, same ABI version).
 *
 * GaitCtrller::TorqueCalculator (src/GaitCtrller.cpp:95-145) for `batch` robots: the orientation
 * estimator (src/Controllers/OrientationEstimator.cpp:46-110), the Kalman filter, the safety checks
 * (GaitCtrller.cpp:108-123, src/Controllers/SafetyChecker.cpp), ConvexMPCLocomotion::run
 * (src/MPC_Ctrl/ConvexMPCLocomotion.cpp:116-496) with the MPC every 13 ticks, and LegController::updateCommand.
 * Every piece of controller state lives on the device (allocated by qmpc_ctrl_init for the handle's max_batch
 * robots); a tick only enqueues kernels on `stream`, so a run of ticks can be captured into a graph.
 *
 * Scope: both robot modes of ConvexMPCLocomotion::run, one per controller (qmpc_ctrl_set_robot_mode), as the reference's
 * _robotMode is one per GaitCtrller.  Mode 0 (the default): the fixed gaits at horizonLength 14, picked by gait number
 * (ConvexMPCLocomotion.cpp:25-41, :149-172).  Mode 1 (what the reference's walking_simulation.py runs): the `aio` gait
 * (:173-233), re-timed from the filtered velocity command to standing, walking, walk-to-trot or trot with 10 .. 16
 * segments per robot; a robot's iterationCounter restarts when its segment count changes, so mode 1 needs the per-robot
 * schedule.  The MPC horizon does NOT vary: `int h = 10` is a local of every tick that only a phase-0 tick changes, a
 * tick that solves is never a phase-0 tick, so every solve of mode 1 runs at horizonLength 10 on the first ten rows of
 * the robot's n-row contact table -- one qmpc_setup horizon serves the batch (DESIGN.md section 0 has the derivation).
 * Not provided: robots of both modes in one batch, and a single-robot drop-in of the six GaitCtrller.h:63-99 symbols.
 *
 * Layouts (one row per robot, DEVICE pointers, the reference's own orders):
 *   imu[B][10]    double: accelerometer x y z, quaternion x y z w, gyro x y z (GaitCtrller.cpp:34-45,
 *                 OrientationEstimator.cpp:49-58)
 *   motor[B][24]  double: q[3*leg + joint], then qd[3*leg + joint] (GaitCtrller.cpp:47-56)
 *   state[B][16]  double: the simulator's ground truth in the member order of CheaterState<double>
 *                 (src/Utilities/IMUTypes.h:25-32): columns 0..3 orientation w x y z, 4..6 position, 7..9 omegaBody,
 *                 10..12 vBody, 13..15 acceleration (body frame).  Every value is rounded to float once
 *                 (.template cast<float>()); the quaternion is used as given, not normalised
 *   effort[B][12] double: tau[3*leg + joint]; zeros for a robot whose safety flag has latched (:130-144)
 *   vel[B][3]     double: x, y, yaw-rate command (SetRobotVel, :75-93: |v| < 0.03 reads 0)
 *   gait[B]       int32: gait number 0 .. 11 (:149-171; 1 bounding, 2 pronking, 4 standing, 5 trot running,
 *                 7 galloping, 8 pacing, 10 walking, 11 walking2, anything else trotting), +20 = omni mode (:129-132)
 *
 * MPC schedule (qmpc_ctrl_set_schedule), two modes:
 *
 * Lockstep (QMPC_CTRL_LOCKSTEP, the default): the handle counts ticks (T).  Every robot's iterationCounter is congruent
 * to T modulo 13, so the MPC runs for the whole batch on the same ticks -- one solve launch over the batch, decided on
 * the host from T.  qmpc_ctrl_reset deviates
 * from a fresh init_controller on exactly this point: a reset robot restarts with iterationCounter = T mod 13
 * (not 0), i.e. its gait clock starts part-way into the first MPC segment.  A graph captured from the tick
 * calls must hold a multiple of 13 ticks: T counts qmpc_ctrl_tick calls, captured ones included, and graph replays
 * do not advance it (qmpc_ctrl_view's `ticks` is T, not the number of ticks executed).
 *
 * Per-robot schedule (QMPC_CTRL_PER_ROBOT): each robot's own device-side counter decides.  Every tick enqueues the same
 * kernels -- estimator, Kalman filter, locomotion, solve, leg commands; the locomotion kernel writes due[b] =
 * (incremented counter % 13 == 0) and appends the due robots to a dense device-side list, and the solve's first launch
 * takes its robots from that list (workgroups beyond the device-side count leave at once).  A robot that is not due is not
 * scheduled: its command rows, world_position_desired / x_comp_integral bookkeeping of the MPC, grf, status and f_ff are
 * not touched by the solve.  qmpc_ctrl_reset is init_controller exactly: iterationCounter = 0, so the robot's first
 * solve comes 13 ticks after its reset, whatever T is -- the lockstep deviation does not apply.  T is still counted and
 * reported, but nothing depends on it: a captured graph may hold any number of ticks, and replays continue every
 * robot's schedule (the counters are device state).  To spread the solves of a fleet over the ticks, initialise,
 * select this mode, and reset group g on tick g (g = 0 .. 12): every robot stays in a state the reference can reach.
 *
 * Estimator source (qmpc_ctrl_prework_state / qmpc_ctrl_tick_state): a second way into the tick for simulated robots, whose
 * body state is known.  In place of the VectorNav orientation estimator and the Kalman filter it runs the reference's
 * CheaterOrientationEstimator::run (OrientationEstimator.cpp:21-39) and CheaterPositionVelocityEstimator::run
 * (PositionVelocityEstimator.cpp:229-238) on state[B][16]: orientation = the quaternion, rBody from it, omegaWorld =
 * rBody^T omegaBody, rpy, aWorld = rBody^T acceleration, position, vWorld = rBody^T vBody, vBody -- no yaw re-basing (the
 * cheater estimator has none) and no filter launch.  Everything after the estimators is the same tick: T and the
 * counters advance as with qmpc_ctrl_tick, and both schedules, both robot modes, qmpc_ctrl_reset, graph capture and
 * qmpc_ctrl_view_get work as described here.  The source is NOT a handle mode: a caller may alternate the two ticks.  A
 * state tick leaves the filter (xhat, P, the previous tick's leg data it reads) and the orientation estimator's
 * first-visit state (_b_first_visit, _ori_ini_inv) exactly where they were; the next IMU tick continues from them.  Only a
 * run of ticks of ONE kind is a state the reference can reach (it is built with one estimator set).
 *
 * Errors: a tick that returns QMPC_ERR_DEVICE may have advanced some of the controller state (T and the counters
 * advance together once the locomotion kernel is enqueued, so the MPC schedule stays consistent); re-initialise the
 * controller (qmpc_ctrl_init) before relying on its state again.
 *
 * Every call takes the batch given to qmpc_ctrl_init (QMPC_ERR_ARG otherwise); QMPC_ERR_STATE before
 * qmpc_ctrl_init.
 */
#ifndef QMPC_CTRL_H
#define QMPC_CTRL_H

#include "qmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GaitCtrller(freq, PIDParam) + init_controller: qmpc_setup(h, float(1 / freq) * 13, 14, 0.4, 120)
 * (ConvexMPCLocomotion.cpp:23-42, :629-630), device state for max_batch robots, and the initial state of
 * robots 0 .. batch-1: firstRun, firstSwing, f_ff = 0, Kalman filter setup(), contact phase 0.5
 * (GaitCtrller.cpp:21-24), orientation first visit, safety flag set, iteration counters 0, gait 0, velocity
 * command 0.  pid[2], pid[3] are the joint PD gains of LegController::updateCommand (ctrlParam(2..3)).
 * The handle's max_horizon must be at least 14.  Synchronises the device (allocation); resets T to 0.
 * Handle constants: the estimators read qmpc_set_leg_geometry's lengths at every prework / tick (so the setter may
 * come before or after this call), the solve reads qmpc_set_robot's body at every MPC tick; freq fixes dt and dt_mpc
 * here, and the Kalman filter keeps the reference's own dt = 0.002 at any freq. */
int qmpc_ctrl_init(qmpc_handle h, int batch, double freq, const double pid[4], void* stream);

/* The MPC schedule (see above).  qmpc_ctrl_init always leaves the handle in lockstep; the mode can be changed only
 * between qmpc_ctrl_init and the first qmpc_ctrl_tick or qmpc_ctrl_reset (QMPC_ERR_STATE afterwards, and before
 * qmpc_ctrl_init); an unknown mode is QMPC_ERR_ARG.  Host state only: nothing is enqueued. */
enum { QMPC_CTRL_LOCKSTEP = 0, QMPC_CTRL_PER_ROBOT = 1 };
int qmpc_ctrl_set_schedule(qmpc_handle h, int mode);

/* set_robot_mode (GaitCtrller.h, GaitCtrller::_robotMode) for the whole controller: 0 or 1 (QMPC_ERR_ARG otherwise).
 * Like the schedule, only between qmpc_ctrl_init and the first qmpc_ctrl_tick or qmpc_ctrl_reset (QMPC_ERR_STATE
 * afterwards and before qmpc_ctrl_init); qmpc_ctrl_prework calls may come first, as in the reference's protocol
 * (init_controller, pre_work ..., set_robot_mode(1)).  Mode 1 needs QMPC_CTRL_PER_ROBOT: QMPC_ERR_STATE on a handle in
 * lockstep (qmpc_last_error says so), and qmpc_ctrl_set_schedule(LOCKSTEP) is refused while mode 1 is selected.
 * Selecting a mode repeats qmpc_setup with its horizon (1: 10, 0: 14; same dt, 0.4, 120): host work, nothing is enqueued.
 * qmpc_ctrl_init always returns to mode 0.  In mode 1 the gait number still sets omni mode (>= 20) and the standing
 * transition test of :137; every other effect of it is overridden (:176-177).  A robot's gait state (segment count,
 * offsets, durations, phase) is device state and persists across ticks; qmpc_ctrl_reset restores the constructor's. */
int qmpc_ctrl_set_robot_mode(qmpc_handle h, int mode);

/* Re-initialise the robots whose mask_dev[b] (uint8, device) is non-zero exactly as qmpc_ctrl_init does -- in lockstep
 * except that their iteration counter restarts at T mod 13 (see Lockstep above); with the per-robot schedule without
 * exception (counter 0).  The other robots are untouched. */
int qmpc_ctrl_reset(qmpc_handle h, int batch, const uint8_t* mask_dev, void* stream);

/* set_gait_type for every robot (gait_dev: int32 [B], device). */
int qmpc_ctrl_set_gait(qmpc_handle h, int batch, const int32_t* gait_dev, void* stream);

/* set_robot_vel for every robot (vel_dev: double [B][3], device), with its 0.03 dead band. */
int qmpc_ctrl_set_vel(qmpc_handle h, int batch, const double* vel_dev, void* stream);

/* pre_work (GaitCtrller.cpp:58-63): the estimators (orientation, Kalman filter) and the leg data. */
int qmpc_ctrl_prework(qmpc_handle h, int batch, const double* imu, const double* motor, void* stream);

/* torque_calculator (GaitCtrller.cpp:95-145): pre_work, the safety checks, one ConvexMPCLocomotion::run tick
 * (the MPC when the incremented counter is a multiple of 13: for the whole batch in lockstep, for the due robots with
 * the per-robot schedule) and the leg commands -> effort[B][12]. */
int qmpc_ctrl_tick(qmpc_handle h, int batch, const double* imu, const double* motor, double* effort, void* stream);

/* pre_work with the cheater estimators (see Estimator source above): state[B][16] in place of imu, no Kalman filter. */
int qmpc_ctrl_prework_state(qmpc_handle h, int batch, const double* state, const double* motor, void* stream);

/* qmpc_ctrl_tick with qmpc_ctrl_prework_state as its pre_work; the same checks, ordering, schedule and outputs. */
int qmpc_ctrl_tick_state(qmpc_handle h, int batch, const double* state, const double* motor, double* effort, void* stream);

/* Read-only device views of the controller state (valid until the handle is destroyed or re-initialised). */
typedef struct {
  const float* position;      /* [B][3]  state estimate (StateEstimate<float>) */
  const float* v_world;       /* [B][3] */
  const float* orientation;   /* [B][4]  w, x, y, z */
  const float* rpy;           /* [B][3] */
  const float* r_body;        /* [B][9]  row-major */
  const float* omega_world;   /* [B][3] */
  const float* leg_q;         /* [B][12] datas[leg].q after checkJointLimit's clamp */
  const float* leg_p;         /* [B][12] datas[leg].p (hip frame) */
  const float* leg_v;         /* [B][12] datas[leg].v */
  const float* leg_J;         /* [B][4][9] datas[leg].J */
  const float* contact_state; /* [B][4]  gait->getContactState() of the last tick */
  const float* swing_state;   /* [B][4]  gait->getSwingState(); > 0: the foot swings */
  const float* p_des;         /* [B][12] commands[leg].pDes (hip frame) */
  const float* v_des;         /* [B][12] commands[leg].vDes */
  const float* f_ff;          /* [B][12] body-frame forces of the last MPC solve, f_ff[3*leg + axis] */
  const int32_t* safe;        /* [B]     GaitCtrller::_safetyCheck (1 = effort is passed on) */
  const int32_t* counter;     /* [B]     iterationCounter */
  int batch;                  /* robots initialised */
  int ticks;                  /* T */
} qmpc_ctrl_view;
int qmpc_ctrl_view_get(qmpc_handle h, qmpc_ctrl_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_CTRL_H */
