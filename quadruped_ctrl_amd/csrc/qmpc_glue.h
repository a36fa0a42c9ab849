// qmpc_glue.h -- float arithmetic of the per-tick glue either side of the MPC solve
// (SURVEY.md 8f-2), written operation by operation after the reference:
//   leg forward kinematics + Jacobian   src/Controllers/LegController.cpp:204-244, :89-110
//   leg command (Cartesian PD, J^T f)   src/Controllers/LegController.cpp:116-160
//   leg inverse kinematics              src/Controllers/LegController.cpp:255-285
//   swing-foot Bezier trajectory        src/Controllers/FootSwingTrajectory.cpp:17-37,
//                                       src/Utilities/Interpolation.h:27-67
// fp contraction is off inside every body (the reference's host code has no fma), so everything
// except the libm calls (sin / cos / atan2 / sqrt) rounds exactly like the reference's float code.
#ifndef QMPC_GLUE_H
#define QMPC_GLUE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qmpc.h"  // qmpc_leg_command, qmpc_kf_state

struct QmpcLegGeom {
  float abad, hip, knee, knee_y;  // _abadLinkLength, _hipLinkLength, _kneeLinkLength, _kneeLinkY_offset
};

// Quadruped::getSideSign (src/Dynamics/Quadruped.h:85-89)
__device__ __forceinline__ float qmpc_side_sign(int leg) { return (leg & 1) ? 1.f : -1.f; }

// computeLegJacobianAndPosition (:204-244).  J row-major 3x3.
__device__ __forceinline__ void qmpc_leg_fk(const QmpcLegGeom& g, int leg, float q0, float q1, float q2, float* J,
                                            float* p) {
#pragma clang fp contract(off)
  const float l1 = g.abad, l2 = g.hip, l3 = g.knee, l4 = g.knee_y;
  const float sideSign = qmpc_side_sign(leg);
  const float s1 = sinf(q0), s2 = sinf(q1), s3 = sinf(q2);
  const float c1 = cosf(q0), c2 = cosf(q1), c3 = cosf(q2);
  const float c23 = c2 * c3 - s2 * s3;
  const float s23 = s2 * c3 + c2 * s3;
  J[0] = 0.f;
  J[1] = l3 * c23 + l2 * c2;
  J[2] = l3 * c23;
  J[3] = l3 * c1 * c23 + l2 * c1 * c2 - (l1 + l4) * sideSign * s1;
  J[4] = -l3 * s1 * s23 - l2 * s1 * s2;
  J[5] = -l3 * s1 * s23;
  J[6] = l3 * s1 * c23 + l2 * c2 * s1 + (l1 + l4) * sideSign * c1;
  J[7] = l3 * c1 * s23 + l2 * c1 * s2;
  J[8] = l3 * c1 * s23;
  p[0] = l3 * s23 + l2 * s2;
  p[1] = (l1 + l4) * sideSign * c1 + l3 * (s1 * c23) + l2 * c2 * s1;
  p[2] = (l1 + l4) * sideSign * s1 - l3 * (c1 * c23) - l2 * c1 * c2;
}

// 3x3 row-major times 3-vector, accumulated left to right like Eigen's fixed-size product
__device__ __forceinline__ float qmpc_row3(const float* r, float x0, float x1, float x2) {
#pragma clang fp contract(off)
  return (r[0] * x0 + r[1] * x1) + r[2] * x2;
}

// computeLegIK (:255-285)
__device__ __forceinline__ void qmpc_leg_ik(const QmpcLegGeom& g, int leg, float px, float py, float pz, float* qdes) {
#pragma clang fp contract(off)
  const float l1 = g.abad + g.knee_y, l2 = g.hip, l3 = g.knee;
  const float sideSign = qmpc_side_sign(leg);
  float D = (px * px + py * py + pz * pz - l1 * l1 - l2 * l2 - l3 * l3) / (2 * l2 * l3);
  // ("D > 1.00001": double literals compared with the float widened)
  if ((double)D > 1.00001) D = (float)0.99999;
  if ((double)D < -1.00001) D = (float)-0.99999;
  const float gamma = atan2f(-sqrtf(1 - D * D), D);
  const float rad = sqrtf(py * py + pz * pz - l1 * l1);
  const float tetta = -atan2f(pz, py) - atan2f(rad, sideSign * l1);
  const float alpha = atan2f(-px, rad) - atan2f(l3 * sinf(gamma), l2 + l3 * cosf(gamma));
  qdes[0] = -tetta;
  qdes[1] = alpha;
  qdes[2] = gamma;
}

// Interpolate::cubicBezier and derivatives (Interpolation.h:27-67)
__device__ __forceinline__ float qmpc_bez(float y0, float yf, float x) {
#pragma clang fp contract(off)
  const float yDiff = yf - y0;
  const float bezier = x * x * x + 3.f * (x * x * (1.f - x));
  return y0 + bezier * yDiff;
}
__device__ __forceinline__ float qmpc_bez_d1(float y0, float yf, float x) {
#pragma clang fp contract(off)
  const float yDiff = yf - y0;
  const float bezier = 6.f * x * (1.f - x);
  return bezier * yDiff;
}
__device__ __forceinline__ float qmpc_bez_d2(float y0, float yf, float x) {
#pragma clang fp contract(off)
  const float yDiff = yf - y0;
  const float bezier = 6.f - 12.f * x;
  return bezier * yDiff;
}

// FootSwingTrajectory::computeSwingTrajectoryBezier (:17-37) for one axis
__device__ __forceinline__ void qmpc_swing_axis(int axis, float p0, float pf, float p0z, float pfz, float height,
                                                float phase, float swingTime, float& p, float& v, float& a) {
#pragma clang fp contract(off)
  if (axis < 2) {
    p = qmpc_bez(p0, pf, phase);
    v = qmpc_bez_d1(p0, pf, phase) / swingTime;
    a = qmpc_bez_d2(p0, pf, phase) / (swingTime * swingTime);
  } else if (phase < 0.5f) {
    p = qmpc_bez(p0z, p0z + height, phase * 2);
    v = qmpc_bez_d1(p0z, p0z + height, phase * 2) * 2 / swingTime;
    a = qmpc_bez_d2(p0z, p0z + height, phase * 2) * 4 / (swingTime * swingTime);
  } else {
    p = qmpc_bez(p0z + height, pfz, phase * 2 - 1);
    v = qmpc_bez_d1(p0z + height, pfz, phase * 2 - 1) * 2 / swingTime;
    a = qmpc_bez_d2(p0z + height, pfz, phase * 2 - 1) * 4 / (swingTime * swingTime);
  }
}

// ---------------------------------------------------------------------------------------------------
// Batched locomotion controller (include/qmpc_ctrl.h): the device state of GaitCtrller / ConvexMPCLocomotion for
// every robot, one row per robot in every array.  Views into two allocations made by qmpc_ctrl_init.
// The arrays are listed once, as X(element type, name, elements per robot): QmpcCtrlDev's members (in this order -- the
// struct is passed to kernels by value, so its layout is that of the kernel arguments), their carving out of the
// allocation (qmpc_capi_ctrl.cpp: carve) and the names of qmpc_debug_ctrl_read are generated from the list.
#define QMPC_CTRL_ARRAYS(X)                                                                                            \
  /* inputs of the tick, rounded to float like VectorNavData / LegData (GaitCtrller.cpp:34-56) */                      \
  X(float, q, 12)                 /* datas[leg].q (clamped by checkJointLimit) */                                      \
  X(float, qd, 12)                /* .qd */                                                                            \
  X(float, leg_J, 36)             /* datas[leg].J of this tick */                                                      \
  X(float, leg_p, 12)             /* .p of this tick */                                                                \
  X(float, leg_v, 12)             /* .v of this tick */                                                                \
  X(float, kf_p, 12)              /* the previous tick's .p: what the Kalman filter reads */                           \
  X(float, kf_v, 12)              /* the previous tick's .v */                                                         \
  /* StateEstimate */                                                                                                  \
  X(float, orientation, 4)                                                                                             \
  X(float, rpy, 3)                                                                                                     \
  X(float, r_body, 9)                                                                                                  \
  X(float, omega_body, 3)                                                                                              \
  X(float, omega_world, 3)                                                                                             \
  X(float, a_world, 3)                                                                                                 \
  X(float, ori_ini_inv, 4)        /* VectorNavOrientationEstimator::_ori_ini_inv */                                    \
  X(float, xhat, 18)              /* LinearKFPositionVelocityEstimator */                                              \
  X(float, P, 324)                                                                                                     \
  X(float, position, 3)                                                                                                \
  X(float, v_world, 3)                                                                                                 \
  X(float, v_body, 3)                                                                                                  \
  X(float, contact_phase, 4)      /* StateEstimatorContainer contactPhase */                                           \
  /* ConvexMPCLocomotion members */                                                                                    \
  X(float, vel_cmd, 3)            /* _gamepadCommand after SetRobotVel's dead band */                                  \
  X(float, vel_des, 3)            /* _x_vel_des, _y_vel_des, _yaw_turn_rate */                                         \
  X(float, yaw_des, 1)                                                                                                 \
  X(float, yaw_des_true, 1)                                                                                            \
  X(float, rpy_int, 2)                                                                                                 \
  X(float, rpy_comp, 2)                                                                                                \
  X(float, stand_traj, 6)                                                                                              \
  X(float, wpd, 2)                /* world_position_desired */                                                         \
  X(float, xci, 1)                /* x_comp_integral */                                                                \
  X(float, p_foot, 12)            /* pFoot */                                                                          \
  X(float, r_cmd, 9)              /* rBody for the MPC command (identity in omni mode, see qmpc_ctrl_tick) */          \
  X(float, sw_p0, 12)             /* footSwingTrajectories[leg] _p0 */                                                 \
  X(float, sw_pf, 12)             /* _pf */                                                                            \
  X(float, sw_p, 12)              /* _p */                                                                             \
  X(float, sw_v, 12)              /* _v */                                                                             \
  X(float, swing_time, 4)         /* swingTimes */                                                                     \
  X(float, swing_rem, 4)          /* swingTimeRemaining */                                                             \
  X(float, contact_state, 4)                                                                                           \
  X(float, swing_state, 4)                                                                                             \
  X(float, p_des, 12)             /* commands[leg].pDes */                                                             \
  X(float, v_des, 12)             /* commands[leg].vDes */                                                             \
  X(float, f_ff, 12)              /* f_ff (body frame) */                                                              \
  X(float, grf, 12)               /* grf (the solve's world-frame forces) */                                           \
  X(float, pf_rel, 8)             /* pfx_rel, pfy_rel per leg after the clamp (:346-365), for tests */                 \
  X(int, counter, 1)                                                                                                   \
  X(int, first_run, 1)                                                                                                 \
  X(int, first_swing, 4)                                                                                               \
  X(int, first_visit, 1)          /* VectorNavOrientationEstimator::_b_first_visit */                                  \
  X(int, gait_num, 1)             /* set_gait_type's number */                                                         \
  X(int, current_gait, 1)         /* current_gait (-1: none yet) */                                                    \
  X(int, offsets, 4)              /* the selected gait (OffsetDurationGait) */                                         \
  X(int, durations, 4)                                                                                                 \
  X(int, iteration, 1)                                                                                                 \
  X(int, safe, 1)                 /* _safetyCheck */                                                                   \
  X(int, status, 1)               /* status of the last solve */                                                       \
  /* the MPC schedule of the tick (qmpc_ctrl_set_schedule) */                                                          \
  X(int, due, 1)                  /* 1: the incremented counter is a multiple of 13 (this tick solves for the robot) */\
  X(int, due_list, 1)             /* per-robot schedule: the due robots of the tick, dense, [0 .. due_count[0]) */      \
  X(int, due_count, 1)            /* ... their number, in element 0 (the rest of the row-per-robot array is unused) */ \
  /* robot mode 1 (qmpc_ctrl_set_robot_mode): the `aio` gait's state beside offsets / durations, which persist there */ \
  X(int, nseg, 1)                 /* OffsetDurationGait::_nIterations of the robot's gait (14 in mode 0) */            \
  X(float, gait_phase, 1)         /* _phase as the last setIterations left it (0 in a fresh robot: see qmpc_glue.hip) */\
  X(int, mpc_offsets, 4)          /* the 10 rows the solve reads of the nseg-row table, as a 10-segment gait ... */    \
  X(int, mpc_durations, 4)        /* ... (qmpc_ctrl_window_gait); written on the robot's due ticks */

struct QmpcCtrlDev {
#define QMPC_CTRL_MEMBER(T, name, per_robot) T* name;
  QMPC_CTRL_ARRAYS(QMPC_CTRL_MEMBER)
#undef QMPC_CTRL_MEMBER
  float dt, dt_mpc;                       // ConvexMPCLocomotion::dt, dtMPC
  float kp_joint, kd_joint;               // ctrlParam(2), ctrlParam(3)
};

// Mini Cheetah _abadLocation (MiniCheetah.h:25-26,105), Quadruped::getHipLocation (Quadruped.h:95-101)
__device__ __forceinline__ void qmpc_hip_location(int leg, float* h) {
  h[0] = (leg == 0 || leg == 1) ? 0.19f : -0.19f;
  h[1] = (leg == 1 || leg == 3) ? 0.049f : -0.049f;
  h[2] = 0.f;
}

// The reference's gaits at horizonLength 14 (ConvexMPCLocomotion.cpp:27-41) as picked by gait number in robot mode 0
// (:149-172).  Vec4<int>(double) truncates: walking is offsets (0, 7, 3, 10), durations 10 (:37-38).
__device__ __forceinline__ void qmpc_ctrl_gait(int gn, int* off, int* dur) {
  int o0 = 0, o1 = 7, o2 = 7, o3 = 0, d = 7;  // trotting (0, 3, 6, 9 and everything unlisted)
  if (gn == 1) { o0 = 7; o1 = 7; o2 = 0; o3 = 0; d = 6; }         // bounding
  else if (gn == 2) { o1 = 0; o2 = 0; d = 6; }                    // pronking
  else if (gn == 4) { o1 = 0; o2 = 0; d = 14; }                   // standing
  else if (gn == 5) { d = 6; }                                    // trotRunning
  else if (gn == 7) { o1 = 4; o2 = 7; o3 = 11; d = 7; }           // galloping
  else if (gn == 8) { o0 = 7; o1 = 0; o2 = 7; o3 = 0; d = 7; }    // pacing
  else if (gn == 10) { o1 = 7; o2 = 3; o3 = 10; d = 10; }         // walking
  else if (gn == 11) { d = 10; }                                  // walking2
  off[0] = o0; off[1] = o1; off[2] = o2; off[3] = o3;
  dur[0] = dur[1] = dur[2] = dur[3] = d;
}

// Robot mode 1: the phase-0 branch of ConvexMPCLocomotion::run (:174-232) -- the `aio` gait re-timed from the filtered
// command.  xv, yv, yr: _x_vel_des, _y_vel_des, _yaw_turn_rate of this tick.  -> the segment count h; off / dur; the
// return value is gaitNumber (4 inside the standing case only, 9 otherwise).
//   vBody (:175) is `sqrt(x*x) + (y*y)`: float products, the DOUBLE sqrt (see the overload decision in qmpc_glue.hip), a
//   double sum -- not a norm.  abs(_yaw_turn_rate) (:180) is the float overload, compared with the double 0.01.
//   h / 2, h / 4, 3 * h / 4 are integer divisions; the walk-to-trot case (:209-211) and h = -20.0 * vBody + 42.0 (:221)
//   are double expressions truncated by the conversion to int (Vec4<int>(double ...)).
__device__ __forceinline__ int qmpc_ctrl_aio_gait(float xv, float yv, float yr, int& h, int* off, int* dur) {
#pragma clang fp contract(off)
  const double vBody = sqrt((double)(xv * xv)) + (double)(yv * yv);
  int gaitNumber = 9;
  h = 10;
  int o1, o2, o3, d;
  if (vBody < 0.002) {
    if ((double)fabsf(yr) < 0.01) {  // standing (:181-185)
      gaitNumber = 4;
      o1 = 0; o2 = 0; o3 = 0; d = h;
    } else {                         // turning on the spot: trot (:187-192)
      h = 10;
      o1 = h / 2; o2 = h / 2; o3 = 0; d = h / 2;
    }
  } else if (vBody <= 0.2) {         // walking (:196-202)
    h = 16;
    o1 = 1 * h / 2; o2 = 1 * h / 4; o3 = 3 * h / 4; d = 3 * h / 4;
  } else if (vBody > 0.2 && vBody <= 0.4) {  // walking to trotting (:204-211)
    h = 16;
    o1 = 1 * h / 2;
    o2 = (int)((double)h * ((5.0 / 4.0) * vBody));
    o3 = (int)((double)h * ((5.0 / 4.0) * vBody + (1.0 / 2.0)));
    d = (int)((double)h * ((-5.0 / 4.0) * vBody + 1.0));
  } else if (vBody > 0.4 && vBody <= 1.4) {  // trotting (:213-218)
    h = 14;
    o1 = h / 2; o2 = h / 2; o3 = 0; d = h / 2;
  } else {                           // fast trot, 13 .. 10 segments (:221-227)
    h = (int)(-20.0 * vBody + 42.0);
    if (h < 10) h = 10;
    o1 = h / 2; o2 = h / 2; o3 = 0; d = h / 2;
  }
  off[0] = 0; off[1] = o1; off[2] = o2; off[3] = o3;
  dur[0] = dur[1] = dur[2] = dur[3] = d;
  return gaitNumber;
}

// OffsetDurationGait::getContactState / getSwingState (Gait.cpp:61-123) of one leg at _phase
__device__ __forceinline__ void qmpc_ctrl_gait_state(float phase, int off, int dur, int n, float& contact, float& swing) {
#pragma clang fp contract(off)
  const float offF = (float)off / (float)n, durF = (float)dur / (float)n;  // setGaitParam (:36-37)
  float pr = phase - offF;
  if (pr < 0) pr = pr + 1.f;
  contact = (pr > durF) ? 0.f : pr / durF;
  float so = offF + durF;
  if (so > 1) so = so - 1.f;
  const float sd = 1.f - durF;
  pr = phase - so;
  if (pr < 0) pr = pr + 1.f;
  if (pr > sd) swing = 0.f;
  else swing = ((double)sd < 0.0000000001) ? 0.f : pr / sd;
}

// The state of a fresh GaitCtrller for robot b, every array of QMPC_CTRL_ARRAYS exactly once: what qmpc_ctrl_init and
// qmpc_ctrl_reset write (FULL = true, qmpc_glue.hip), and what a robot in warm-up on the sensor path gets after a tick
// that is to count as pre_work alone (FULL = false, qmpc_episode_sense.hip): everything EXCEPT the pre_work set -- what
// qmpc_ctrl_prework writes: the inputs, the leg data, the state estimate, both estimators' own state --, which is kept.
// One function with a compile-time switch, so that the two lists cannot drift: an array is either inside the FULL block
// or behind it (tests/test_episode_sense_cpu.py holds the partition to the array list).  The partial form does not touch
// the 324-float P row.
template <bool FULL>
__device__ __forceinline__ void qmpc_ctrl_init_robot(const QmpcCtrlDev& S, const int b, const int counter0) {
  if constexpr (FULL) {  // the pre_work set
    for (int e = 0; e < 18 * 18; ++e) S.P[(size_t)b * 324 + e] = (e / 18 == e % 18) ? 100.f : 0.f;
    for (int k = 0; k < 18; ++k) S.xhat[(size_t)b * 18 + k] = 0.f;
    for (int k = 0; k < 36; ++k) S.leg_J[(size_t)b * 36 + k] = 0.f;
    for (int k = 0; k < 12; ++k) {
      S.q[(size_t)b * 12 + k] = 0.f;
      S.qd[(size_t)b * 12 + k] = 0.f;
      S.leg_p[(size_t)b * 12 + k] = 0.f;
      S.leg_v[(size_t)b * 12 + k] = 0.f;
      S.kf_p[(size_t)b * 12 + k] = 0.f;
      S.kf_v[(size_t)b * 12 + k] = 0.f;
    }
    for (int k = 0; k < 9; ++k) S.r_body[(size_t)b * 9 + k] = 0.f;
    for (int k = 0; k < 4; ++k) {
      S.orientation[(size_t)b * 4 + k] = 0.f;
      S.ori_ini_inv[(size_t)b * 4 + k] = 0.f;
    }
    for (int k = 0; k < 3; ++k) {
      S.rpy[(size_t)b * 3 + k] = 0.f;
      S.omega_body[(size_t)b * 3 + k] = 0.f;
      S.omega_world[(size_t)b * 3 + k] = 0.f;
      S.a_world[(size_t)b * 3 + k] = 0.f;
      S.position[(size_t)b * 3 + k] = 0.f;
      S.v_world[(size_t)b * 3 + k] = 0.f;
      S.v_body[(size_t)b * 3 + k] = 0.f;
    }
    S.first_visit[b] = 1;
  }
  // everything else
  for (int k = 0; k < 12; ++k) {
    S.p_foot[(size_t)b * 12 + k] = 0.f;
    S.sw_p0[(size_t)b * 12 + k] = 0.f;
    S.sw_pf[(size_t)b * 12 + k] = 0.f;
    S.sw_p[(size_t)b * 12 + k] = 0.f;
    S.sw_v[(size_t)b * 12 + k] = 0.f;
    S.p_des[(size_t)b * 12 + k] = 0.f;
    S.v_des[(size_t)b * 12 + k] = 0.f;
    S.f_ff[(size_t)b * 12 + k] = 0.f;
    S.grf[(size_t)b * 12 + k] = 0.f;
  }
  for (int k = 0; k < 8; ++k) S.pf_rel[(size_t)b * 8 + k] = 0.f;
  for (int k = 0; k < 9; ++k) S.r_cmd[(size_t)b * 9 + k] = 0.f;
  for (int k = 0; k < 4; ++k) {
    S.contact_phase[(size_t)b * 4 + k] = 0.5f;  // GaitCtrller.cpp:22-24
    S.swing_time[(size_t)b * 4 + k] = 0.f;
    S.swing_rem[(size_t)b * 4 + k] = 0.f;
    S.contact_state[(size_t)b * 4 + k] = 0.f;
    S.swing_state[(size_t)b * 4 + k] = 0.f;
    S.first_swing[(size_t)b * 4 + k] = 1;
    S.offsets[(size_t)b * 4 + k] = 0;
    S.durations[(size_t)b * 4 + k] = 0;
  }
  for (int k = 0; k < 3; ++k) {
    S.vel_cmd[(size_t)b * 3 + k] = 0.f;
    S.vel_des[(size_t)b * 3 + k] = 0.f;
  }
  for (int k = 0; k < 2; ++k) {
    S.rpy_int[(size_t)b * 2 + k] = 0.f;
    S.rpy_comp[(size_t)b * 2 + k] = 0.f;
    S.wpd[(size_t)b * 2 + k] = 0.f;
  }
  for (int k = 0; k < 6; ++k) S.stand_traj[(size_t)b * 6 + k] = 0.f;
  S.yaw_des[b] = 0.f;
  S.yaw_des_true[b] = 0.f;
  S.xci[b] = 0.f;
  S.counter[b] = counter0;
  S.first_run[b] = 1;
  S.gait_num[b] = 0;
  S.current_gait[b] = -1;
  S.iteration[b] = 0;
  S.safe[b] = 1;
  S.status[b] = 0;
  S.due[b] = 0;
  S.due_list[b] = 0;
  S.nseg[b] = 14;  // the `aio` gait as its constructor leaves it (ConvexMPCLocomotion.cpp:41); its offsets 0 and
  S.gait_phase[b] = 0.f;  // durations 14 are replaced by the first tick's selection before anything reads them
  for (int k = 0; k < 4; ++k) {
    S.mpc_offsets[(size_t)b * 4 + k] = 0;
    S.mpc_durations[(size_t)b * 4 + k] = 0;
  }
  S.due_count[b] = 0;  // (element 0 is the count of a tick, rebuilt by every tick; the rest is never used)
}

// ---------------------------------------------------------------------------------------------------
// Launchers of qmpc_glue.hip, declared once: qmpc_glue.hip (which defines them) and the host units qmpc_capi*.cpp (which call them)
// both read these lines, so a signature that drifts fails to compile.
extern "C" hipError_t qmpc_launch_leg_kin(const float geom[4], const float* q, const float* qd, float* J, float* p,
                                          float* v, int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_leg_cmd(const float geom[4], const qmpc_leg_command* c, float* tau, float* q_des,
                                          int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_swing(const float* p0, const float* pf, const float* height, const float* phase,
                                        const float* swing_time, float* p, float* v, float* a, int n_feet,
                                        hipStream_t stream);
extern "C" hipError_t qmpc_launch_kf(const qmpc_kf_state* st, const float hip[3], int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_kf_init(float* xhat, float* P, int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_init(const QmpcCtrlDev* S, const uint8_t* mask, int counter0, int batch,
                                            hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_set(const QmpcCtrlDev* S, const int32_t* gait, const double* vel, int batch,
                                           hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_est(const QmpcCtrlDev* S, const float geom[4], const double* imu,
                                           const double* motor, int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_est_state(const QmpcCtrlDev* S, const float geom[4], const double* state,
                                                 const double* motor, int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_loco(const QmpcCtrlDev* S, int batch, int build_list, hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_loco_aio(const QmpcCtrlDev* S, int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_ctrl_legcmd(const QmpcCtrlDev* S, double* effort, int batch, hipStream_t stream);

#endif
