/*
 * qmpc_plant.h -- a reduced-order plant on the device for the batched locomotion controller of qmpc_ctrl.h (same
 * library, same ABI version): the single rigid body the MPC is designed on, with massless legs.  One qmpc_plant_step
 * consumes the controller's effort[B][12] and produces the next state[B][16] and motor[B][24] in the layouts of
 * qmpc_ctrl.h, so a run of qmpc_ctrl_tick_state -> qmpc_plant_step is a closed loop with no host in it.  A step
 * allocates nothing and only enqueues one kernel: the loop can be captured into a graph (in lockstep a captured block
 * holds a multiple of 13 ticks, see qmpc_ctrl.h).  The plant reads the controller's state and writes none of it.
 *
 * Limits: massless legs (a swing foot tracks its command exactly and its torque is ignored), scheduled contact (the
 * controller's gait decides which feet stand, not the ground), no slip (the force saturates, the foot stays), flat
 * ground at z = 0.  It closes the loop on the model the controller plans with; it is not a physics engine.
 * (qmpc_plant_vary.h gives each robot its own mass, inertia, friction and external pushes, and keeps per-robot
 * statistics on the device; qmpc_terrain.h puts per-robot slopes and stairs under the feet; qmpc_contact.h lifts the
 * two limits on contact, opt-in: the ground decides which feet stand -- early and late touch-down -- and a saturated
 * foot slips; with nothing bound or set in any of them, this header is the whole description.)
 *
 * The model, in double precision (every decision below is restated above the kernel in csrc/qmpc_plant.hip and in
 * tests/plant_model.py, which makes the same choices operation by operation):
 *
 * State per robot: body position p and velocity v (world), quaternion q (w x y z; R(q) maps body to world, rBody =
 *   R(q)^T = quaternionToRotationMatrix(q) maps world to body, as the cheater estimator uses it), body-frame angular
 *   velocity w; per foot a world position c_i and a stance flag; the ground reactions f_i of the last substep.
 * Constants: mass and body inertia of the handle (qmpc_set_robot; 9 kg, diag(0.07, 0.26, 0.242)); g = 9.81 (the
 *   plant's own constant: the handle's gravity is the MPC's model value, -9.8f); leg geometry qmpc_set_leg_geometry;
 *   hip locations (+-0.19, +-0.049, 0); dt = 1 / freq of qmpc_ctrl_init, h = dt / substeps.  Mass, inertia and
 *   geometry are read from the handle at every qmpc_plant_step / qmpc_plant_reset: a setter called between two
 *   steps takes effect on the next one (mu_plant and substeps are qmpc_plant_init's).
 *
 * One step, from effort and the controller's view after the tick that produced it (contact_state, p_des, v_des):
 *  1. Contact schedule.  Foot i stands iff contact_state[i] > 0.  On a swing -> stance edge c_i,z = 0 (x, y stay);
 *     on a stance -> swing edge only the flag changes.
 *  2. `substeps` times, with the torque held and everything else re-evaluated at the current pose:
 *     a. each stance foot: r_i = rBody (c_i - p) - hip_i; joint angles by the inverse kinematics below; J(angles);
 *        F_body = J^-T tau_i by cofactors; f_i = -rBody^T F_body.  If |det J| < 1e-5 m^3 (a knee within about a
 *        milliradian of straight at standing extension) or f_i,z <= 0, f_i = 0; otherwise, with t = sqrt(f_x^2 +
 *        f_y^2), if t > mu_plant f_z then f_x and f_y are scaled by (mu_plant f_z) / t.  A swing foot has f_i = 0.
 *     b. F = (f_0 + f_1) + (f_2 + f_3); n = sum in the same order of (rBody (c_i - p)) x (rBody f_i).
 *     c. vdot = F / m + (0, 0, -g); wdot = I^-1 (n - w x I w).
 *     d. semi-implicit Euler: v += h vdot; w += h wdot; then p += h v (the new v) and q <- normalise(q (x) dq), dq =
 *        (cos(a / 2), sin(a / 2) w / |w|) with a = |w| h for the new w (dq = (1, h w / 2) when |w| h < 1e-12).
 *  3. Swing feet, at the new pose: r_i = clamp(p_des_i), rdot_i = v_des_i, c_i = p + rBody^T (hip_i + r_i).  The clamp
 *     scales r_i radially into the shell a knee angle in [0.05, 2.6] rad reaches: |r_i|^2 in l1^2 + l2^2 + l3^2 +
 *     2 l2 l3 cos([2.6, 0.05]) with l1 = abad + knee_y.  (The direction is kept, so a command inside the cylinder
 *     y^2 + z^2 < l1^2 still has no exact solution; the inverse kinematics reads rho^2 = max(y^2 + z^2 - l1^2, 0).
 *     A zero command has no direction: it reads (0, 0, -|r|_min).)
 *  4. Read-out, at the new pose.  state = q, p, w, rBody v, rBody (vdot + (0, 0, g)) with the last substep's vdot: the
 *     specific force an accelerometer reads.  motor = joint angles by inverse kinematics of every foot's r_i on the
 *     branch of the standing pose (knee angle >= 0, qmpc_leg_fk's own branch -- the reference's computeLegIK is the
 *     OTHER branch):
 *         rho = sqrt(max(y^2 + z^2 - l1^2, 0)),  D = clamp((x^2 + rho^2 - l2^2 - l3^2) / (2 l2 l3), -1, 1),
 *         knee = atan2(sqrt(1 - D^2), D),  hip = atan2(x, rho) - atan2(l3 sqrt(1 - D^2), l2 + l3 D),
 *         abad = atan2(z, y) - atan2(-rho, side l1);
 *     joint rates = J^-1 rdot_i (zero when |det J| < 1e-5).  A pinned foot is fixed in the world and hip_i in the body,
 *     so r_i = rBody (c_i - p) - hip_i has rdot_i = -rBody v - w x (rBody (c_i - p)) = -rBody v - w x (r_i + hip_i):
 *     the lever arm is from the body origin, not from the hip.
 *
 * Initial state (init, reset): body at (x0, y0, 0.29) with yaw0 -- (0, 0, 0) without init_xyyaw -- zero velocities;
 * every foot at body-frame (hip_x, hip_y + side 0.065, -0.29), i.e. on the ground, in stance; f_i = 0; vdot = 0.
 *
 * Errors as in qmpc_ctrl.h: QMPC_ERR_STATE before qmpc_ctrl_init (init) or qmpc_plant_init (the rest); QMPC_ERR_ARG
 * for a batch other than the controller's, a null pointer where one is needed, substeps < 1, or mu_plant not >= 0.
 * A later qmpc_ctrl_init with the same batch keeps the plant; with another batch the plant must be initialised again.
 */
#ifndef QMPC_PLANT_H
#define QMPC_PLANT_H

#include "qmpc_ctrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Allocate the plant's state for the handle's max_batch (once) and put robots 0 .. batch-1 into the initial state.
 * mu_plant: friction coefficient of the ground (0.4, the MPC's, keeps the MPC's plan feasible); substeps >= 1;
 * init_xyyaw: double [B][3] (x, y, yaw) on the device, or NULL for zeros.  Synchronises the device on first use. */
int qmpc_plant_init(qmpc_handle h, int batch, double mu_plant, int substeps, const double* init_xyyaw, void* stream);

/* The initial state again for the robots whose mask_dev[b] (uint8, device) is non-zero; the others keep every bit. */
int qmpc_plant_reset(qmpc_handle h, int batch, const uint8_t* mask_dev, const double* init_xyyaw, void* stream);

/* One control period: effort[B][12] (device, as qmpc_ctrl_tick_state left it) and the controller's view ->
 * state_out[B][16], motor_out[B][24] (device, double) for the next tick.  One kernel launch, nothing else. */
int qmpc_plant_step(qmpc_handle h, int batch, const double* effort, double* state_out, double* motor_out, void* stream);

/* Device views of the plant's state (valid until the handle is destroyed); read-only by contract. */
typedef struct {
  const double* p;        /* [B][3]    body position, world */
  const double* v;        /* [B][3]    body velocity, world */
  const double* q;        /* [B][4]    w x y z */
  const double* omega;    /* [B][3]    body frame */
  const double* foot;     /* [B][4][3] foot positions, world */
  const int32_t* stance;  /* [B][4]    1: pinned */
  const double* grf;      /* [B][4][3] ground reactions on the body of the last substep, world */
  const double* state;    /* [B][16]   the plant's own copy of the last read-out: what init / reset / step left */
  const double* motor;    /* [B][24] */
  int batch;
  int substeps;
  double mu_plant;
} qmpc_plant_view;
int qmpc_plant_view_get(qmpc_handle h, qmpc_plant_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_PLANT_H */
