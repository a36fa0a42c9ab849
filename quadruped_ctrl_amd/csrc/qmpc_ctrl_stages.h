// qmpc_ctrl_stages.h -- device code of the batched locomotion controller's stages (include/qmpc_ctrl.h), shared by the
// per-tick kernels of qmpc_glue.hip (one launch per stage) and the span kernel of qmpc_span.hip (every stage between
// two MPC solves in one launch): the estimators' helpers, and the BODIES of the stages of a state-driven tick,
//   E  qmpc_ctrl_est_state_body   the cheater estimators + LegController::updateData, lane t = robot * 4 + leg
//   L  (qmpc_ctrl_loco_body.h, text: it costs the per-tick kernel registers as a function), whose helper is here, and
//      qmpc_ctrl_due_append       the wave's due robots onto the due list (per-robot schedule)
//   C  qmpc_ctrl_legcmd_body      f_ff, the gains, LegController::updateCommand, the latch, lane t = robot * 4 + leg
// as force-inlined functions: one text behind both users, so the two cannot drift.  A body neither returns from the
// kernel nor tests the lane against the batch: its caller decides which lanes run it (the per-tick kernels leave early,
// the span kernel keeps every lane alive for its barriers and shuffles).  qmpc_ctrl_due_append holds a ballot and a
// shuffle and is called by every lane of the wave, with due = false in the lanes that ran no L.
// Everything lives in an unnamed namespace, like qmpc_plant_dev.h: each translation unit gets its own copy.  The
// decisions where the reference's C++ does not say what it computes at first sight are listed in qmpc_glue.hip.
#ifndef QMPC_CTRL_STAGES_H
#define QMPC_CTRL_STAGES_H

#include "qmpc_cmd.h"
#include "qmpc_glue.h"

namespace {

// Eigen-order 3x3 products (row-major), ((a0 b0 + a1 b1) + a2 b2) like qmpc_row3
__device__ __forceinline__ void qmpc_mat3_mul(const float* A, const float* B, float* C) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// ori::quatToRPY (orientation_tools.h:195-208)
__device__ __forceinline__ void qmpc_quat_to_rpy(const float* q, float* rpy) {
#pragma clang fp contract(off)
  const double m = -2. * (double)(q[1] * q[3] - q[0] * q[2]);
  // std::min(m, .99999) in its operand order, (b < a) ? b : a: a NaN m (NaN quaternion) stays NaN, so that rpy is NaN and
  // the orientation check, abs(NaN) >= 0.5, does not latch -- as in the reference
  const float as = (float)(.99999 < m ? .99999 : m);
  rpy[2] = atan2f(2 * (q[1] * q[2] + q[0] * q[3]), ((q[0] * q[0] + q[1] * q[1]) - q[2] * q[2]) - q[3] * q[3]);
  rpy[1] = asinf(as);
  rpy[0] = atan2f(2 * (q[2] * q[3] + q[0] * q[1]), ((q[0] * q[0] - q[1] * q[1]) - q[2] * q[2]) + q[3] * q[3]);
}

// rpyToQuat(-rpy_ini) with rpy_ini = (0, 0, yaw) (OrientationEstimator.cpp:55-61): rpyToRotMat (:93-100) as the
// product of three coordinateRotation's (:58-76), then rotationMatrixToQuaternion (:129-162)
__device__ __forceinline__ void qmpc_yaw_inverse_quat(float yaw, float* q) {
#pragma clang fp contract(off)
  const float v0 = -0.f, v1 = -0.f, v2 = -yaw;
  float s = sinf(v0), c = cosf(v0);
  const float Rx[9] = {1, 0, 0, 0, c, s, 0, -s, c};
  s = sinf(v1);
  c = cosf(v1);
  const float Ry[9] = {c, 0, -s, 0, 1, 0, s, 0, c};
  s = sinf(v2);
  c = cosf(v2);
  const float Rz[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
  float T[9], R[9];
  qmpc_mat3_mul(Rx, Ry, T);
  qmpc_mat3_mul(T, Rz, R);
  // r = R^T: r(i, j) = R[3 j + i]
#define QR(i, j) R[3 * (j) + (i)]
  const float tr = (QR(0, 0) + QR(1, 1)) + QR(2, 2);
  if (tr > 0.0) {
    const float S = (float)(sqrt((double)tr + 1.0) * 2.0);
    q[0] = (float)(0.25 * S);
    q[1] = (QR(2, 1) - QR(1, 2)) / S;
    q[2] = (QR(0, 2) - QR(2, 0)) / S;
    q[3] = (QR(1, 0) - QR(0, 1)) / S;
  } else if ((QR(0, 0) > QR(1, 1)) && (QR(0, 0) > QR(2, 2))) {
    const float S = (float)(sqrt(((1.0 + QR(0, 0)) - QR(1, 1)) - QR(2, 2)) * 2.0);
    q[0] = (QR(2, 1) - QR(1, 2)) / S;
    q[1] = (float)(0.25 * S);
    q[2] = (QR(0, 1) + QR(1, 0)) / S;
    q[3] = (QR(0, 2) + QR(2, 0)) / S;
  } else if (QR(1, 1) > QR(2, 2)) {
    const float S = (float)(sqrt(((1.0 + QR(1, 1)) - QR(0, 0)) - QR(2, 2)) * 2.0);
    q[0] = (QR(0, 2) - QR(2, 0)) / S;
    q[1] = (QR(0, 1) + QR(1, 0)) / S;
    q[2] = (float)(0.25 * S);
    q[3] = (QR(1, 2) + QR(2, 1)) / S;
  } else {
    const float S = (float)(sqrt(((1.0 + QR(2, 2)) - QR(0, 0)) - QR(1, 1)) * 2.0);
    q[0] = (QR(1, 0) - QR(0, 1)) / S;
    q[1] = (QR(0, 2) + QR(2, 0)) / S;
    q[2] = (QR(1, 2) + QR(2, 1)) / S;
    q[3] = (float)(0.25 * S);
  }
#undef QR
}

// ori::quaternionToRotationMatrix (orientation_tools.h:170-189) BEFORE its final transpose: R with rBody = R^T, so that
// row k of R is column k of rBody (rBody^T * v is a row of R times v).  q is used as given, not normalised.
__device__ __forceinline__ void qmpc_quat_to_rot(const float* q, float* R) {
#pragma clang fp contract(off)
  const float e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3];
  R[0] = 1 - 2 * (e2 * e2 + e3 * e3);
  R[1] = 2 * (e1 * e2 - e0 * e3);
  R[2] = 2 * (e1 * e3 + e0 * e2);
  R[3] = 2 * (e1 * e2 + e0 * e3);
  R[4] = 1 - 2 * (e1 * e1 + e3 * e3);
  R[5] = 2 * (e2 * e3 - e0 * e1);
  R[6] = 2 * (e1 * e3 - e0 * e2);
  R[7] = 2 * (e2 * e3 + e0 * e1);
  R[8] = 1 - 2 * (e1 * e1 + e2 * e2);
}

// VectorNavOrientationEstimator::run for robot b
__device__ __forceinline__ void qmpc_ctrl_orientation(const QmpcCtrlDev& S, int b, const double* u) {
#pragma clang fp contract(off)
  float o[4] = {(float)u[6], (float)u[3], (float)u[4], (float)u[5]};  // result->orientation = (quat[3], quat[0..2])
  float* inv = S.ori_ini_inv + (size_t)b * 4;
  if (S.first_visit[b]) {
    float rpy_ini[3];
    qmpc_quat_to_rpy(o, rpy_ini);
    qmpc_yaw_inverse_quat(rpy_ini[2], inv);
    S.first_visit[b] = 0;
  }
  // ori::quatProduct(_ori_ini_inv, orientation) (orientation_tools.h:272-285)
  const float r1 = inv[0], r2 = o[0];
  const float a0 = inv[1], a1 = inv[2], a2 = inv[3], b0 = o[1], b1 = o[2], b2 = o[3];
  const float dot = (a0 * b0 + a1 * b1) + a2 * b2;
  float q[4];
  q[0] = r1 * r2 - dot;
  q[1] = (r1 * b0 + r2 * a0) + (a1 * b2 - a2 * b1);
  q[2] = (r1 * b1 + r2 * a1) + (a2 * b0 - a0 * b2);
  q[3] = (r1 * b2 + r2 * a2) + (a0 * b1 - a1 * b0);
  float rpy[3];
  qmpc_quat_to_rpy(q, rpy);
  float R[9];
  qmpc_quat_to_rot(q, R);
  float* rB = S.r_body + (size_t)b * 9;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) rB[3 * i + j] = R[3 * j + i];
  const float w[3] = {(float)u[7], (float)u[8], (float)u[9]}, acc[3] = {(float)u[0], (float)u[1], (float)u[2]};
  for (int k = 0; k < 4; ++k) S.orientation[(size_t)b * 4 + k] = q[k];
  for (int k = 0; k < 3; ++k) {
    S.rpy[(size_t)b * 3 + k] = rpy[k];
    S.omega_body[(size_t)b * 3 + k] = w[k];
    // rBody^T * v: column k of rBody = row k of R
    S.omega_world[(size_t)b * 3 + k] = (R[3 * k] * w[0] + R[3 * k + 1] * w[1]) + R[3 * k + 2] * w[2];
    S.a_world[(size_t)b * 3 + k] = (R[3 * k] * acc[0] + R[3 * k + 1] * acc[1]) + R[3 * k + 2] * acc[2];
  }
}

// CheaterOrientationEstimator::run (OrientationEstimator.cpp:21-39), then CheaterPositionVelocityEstimator::run
// (PositionVelocityEstimator.cpp:229-238) for robot b.  u: the robot's CheaterState<double> row (IMUTypes.h:25-32) --
// orientation w x y z, position, omegaBody, vBody, acceleration -- every member rounded to float once (.cast<T>()).
// No yaw re-basing (the cheater estimator has none), no filter: nothing of the VectorNav / Kalman state is touched.
__device__ __forceinline__ void qmpc_ctrl_cheater(const QmpcCtrlDev& S, int b, const double* u) {
#pragma clang fp contract(off)
  float x[16];
  for (int k = 0; k < 16; ++k) x[k] = (float)u[k];
  const float* q = x;
  const float *pos = x + 4, *w = x + 7, *vb = x + 10, *acc = x + 13;
  float R[9], rpy[3];
  qmpc_quat_to_rot(q, R);
  qmpc_quat_to_rpy(q, rpy);
  float* rB = S.r_body + (size_t)b * 9;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) rB[3 * i + j] = R[3 * j + i];
  for (int k = 0; k < 4; ++k) S.orientation[(size_t)b * 4 + k] = q[k];
  for (int k = 0; k < 3; ++k) {
    const size_t o = (size_t)b * 3 + k;
    S.rpy[o] = rpy[k];
    S.omega_body[o] = w[k];
    // rBody^T * v: column k of rBody = row k of R
    S.omega_world[o] = (R[3 * k] * w[0] + R[3 * k + 1] * w[1]) + R[3 * k + 2] * w[2];
    S.a_world[o] = (R[3 * k] * acc[0] + R[3 * k + 1] * acc[1]) + R[3 * k + 2] * acc[2];
    S.position[o] = pos[k];
    S.v_world[o] = (R[3 * k] * vb[0] + R[3 * k + 1] * vb[1]) + R[3 * k + 2] * vb[2];
    S.v_body[o] = vb[k];
  }
}

// The leg's joint angles and rates of the robot's motor row m, rounded to float (GaitCtrller.cpp:47-56)
struct QmpcLegJoints {
  float q0, q1, q2, d0, d1, d2;
};
__device__ __forceinline__ QmpcLegJoints qmpc_ctrl_leg_joints(const double* m, int leg) {
  return {(float)m[3 * leg],      (float)m[3 * leg + 1],      (float)m[3 * leg + 2],
          (float)m[12 + 3 * leg], (float)m[12 + 3 * leg + 1], (float)m[12 + 3 * leg + 2]};
}

// LegController::updateData for thread t = robot * 4 + leg: q, qd, J, p, v of the leg
__device__ __forceinline__ void qmpc_ctrl_leg_update(const QmpcCtrlDev& S, const QmpcLegGeom& g, int t, int leg,
                                                     const QmpcLegJoints& j) {
#pragma clang fp contract(off)
  const size_t o3 = (size_t)t * 3;
  const float q0 = j.q0, q1 = j.q1, q2 = j.q2, d0 = j.d0, d1 = j.d1, d2 = j.d2;
  float J[9], p[3];
  qmpc_leg_fk(g, leg, q0, q1, q2, J, p);
  for (int k = 0; k < 9; ++k) S.leg_J[(size_t)t * 9 + k] = J[k];
  for (int k = 0; k < 3; ++k) {
    S.leg_p[o3 + k] = p[k];
    S.leg_v[o3 + k] = qmpc_row3(J + 3 * k, d0, d1, d2);
  }
  S.q[o3 + 0] = q0;
  S.q[o3 + 1] = q1;
  S.q[o3 + 2] = q2;
  S.qd[o3 + 0] = d0;
  S.qd[o3 + 1] = d1;
  S.qd[o3 + 2] = d2;
}

// pre_work of a tick driven by simulator ground truth (qmpc_ctrl_tick_state): the same leg data, and the two cheater
// estimators in place of the VectorNav estimator and the Kalman filter.  state: [B][16] double.  Memory-shaped: per
// robot 320 B in (one thread reads the 128 B state row, the four leg threads 48 B each of the motor row) and 504 B out.
// Stage E for lane t = robot * 4 + leg.  (The reset of the tick's due list is not part of it: see its two callers.)
__device__ __forceinline__ void qmpc_ctrl_est_state_body(const QmpcCtrlDev& S, const QmpcLegGeom& g, const double* state,
                                                         const double* motor, const int t) {
#pragma clang fp contract(off)
  const int b = t >> 2, leg = t & 3;
  qmpc_ctrl_leg_update(S, g, t, leg, qmpc_ctrl_leg_joints(motor + (size_t)b * 24, leg));
  if (leg == 0) qmpc_ctrl_cheater(S, b, state + (size_t)b * 16);
}

// Robot mode 1, the solve's contact table.  Every solve of mode 1 runs at horizonLength 10 and
// reads rows i = 0 .. 9 of the robot's n-row table (getMpcTable, Gait.cpp:142-166), n = 10 .. 16.  The command stage
// of the solve builds its table from (iteration, offset, duration) with n_segments = horizon (qmpc_cmd_gait_bit), so
// it is handed a 10-segment gait with the SAME ten rows: row i of a leg sits at place p = (i + iteration + 1) % 10 of
// a cycle of ten; the leg's contact rows are one run of that cycle (ten consecutive rows of a cycle of n >= 10 meet
// the contact arc in one piece, or in two pieces that touch the two ends of the window, which are neighbours in the
// cycle of ten), so offset' = the place where the run starts and duration' = its length reproduce every row.
// tests/test_ctrl_mode1_cpu.py checks the identity for every n, offset, duration and iteration.
__device__ __forceinline__ void qmpc_ctrl_window_gait(int iteration, int off, int dur, int n, int& off10, int& dur10) {
  unsigned m = 0;  // bit p: contact at place p
  for (int i = 0; i < 10; ++i)
    if (qmpc_cmd_gait_bit(i, iteration, off, dur, n)) m |= 1u << ((i + iteration + 1) % 10);
  const unsigned prev = ((m << 1) | (m >> 9)) & 0x3ffu;  // bit p: contact at place p - 1
  const unsigned start = m & ~prev;
  off10 = start ? __ffs((int)start) - 1 : 0;
  dur10 = __popc(m);
}

// Per-robot schedule: the dense list of the due robots (what the solve's first launch consumes).  The wave's due lanes
// take consecutive places behind one atomic add of its first due lane; at most `batch` entries (every robot appends at
// most once a tick).  Every lane that is still alive in the wave calls it; b is read in the due lanes only.
__device__ __forceinline__ void qmpc_ctrl_due_append(const QmpcCtrlDev& S, const int b, const bool due) {
  const unsigned long long m = __ballot(due);
  if (m) {
    const int lane = (int)__lane_id(), leader = __ffsll(m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(S.due_count, __popcll(m));
    base = __shfl(base, leader);
    if (due) S.due_list[base + __popcll(m & ((1ull << lane) - 1ull))] = b;
  }
}

// qmpc_ctrl_set_gait / qmpc_ctrl_set_vel for robot b (null: that command is left alone).  One text behind the set kernel of
// qmpc_glue.hip and the reset stage of qmpc_loop.hip.
__device__ __forceinline__ void qmpc_ctrl_set_robot(const QmpcCtrlDev& S, const int32_t* gait, const double* vel, const int b) {
  if (gait) S.gait_num[b] = gait[b];
  if (vel)  // SetRobotVel (GaitCtrller.cpp:75-93): abs(double) there is the double overload (<math.h>)
    for (int k = 0; k < 3; ++k) {
      const double v = vel[(size_t)b * 3 + k];
      S.vel_cmd[(size_t)b * 3 + k] = (float)(fabs(v) < 0.03 ? 0.0 : v * 1.0);
    }
}

// Stage C for lane t = robot * 4 + leg: f_ff (on MPC ticks), the gains of :378-382, LegController::updateCommand and the
// latch
__device__ __forceinline__ void qmpc_ctrl_legcmd_body(const QmpcCtrlDev& S, double* effort, const int t) {
#pragma clang fp contract(off)
  const int b = t >> 2, leg = t & 3;
  const size_t o3 = (size_t)t * 3, o9 = (size_t)t * 9;
  float* ffl = S.f_ff + o3;
  if (S.counter[b] % 13 == 0) {  // this tick solved: f_ff = -rBody grf (ConvexMPCLocomotion.cpp:672-680)
    const float* g = S.grf + o3;
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    for (int i = 0; i < 3; ++i) ffl[i] = qmpc_cmd_f2b(S.r_body + (size_t)b * 9 + 3 * i, g0, g1, g2);
  }
  const bool swing = S.swing_state[(size_t)b * 4 + leg] > 0;
  float ff[3], dp[3], dv[3];
  for (int k = 0; k < 3; ++k) {
    ff[k] = swing ? 0.f : ffl[k];  // stance: forceFeedForward = f_ff[foot] (:456); zeroCommand otherwise
    dp[k] = S.p_des[o3 + k] - S.leg_p[o3 + k];
    dv[k] = S.v_des[o3 + k] - S.leg_v[o3 + k];
  }
  // kpCartesian = Kp = diag(700, 700, 200) in swing, 0 in stance; kdCartesian = Kd = diag(10, 10, 10)
  const float kp[3] = {swing ? 700.f : 0.f, swing ? 700.f : 0.f, swing ? 200.f : 0.f};
  float add[3];
  for (int k = 0; k < 3; ++k) {
    float r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    r[4 * k] = kp[k];
    add[k] = qmpc_row3(r + 3 * k, dp[0], dp[1], dp[2]);
  }
  for (int k = 0; k < 3; ++k) ff[k] = ff[k] + add[k];
  for (int k = 0; k < 3; ++k) {
    float r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    r[4 * k] = 10.f;
    add[k] = qmpc_row3(r + 3 * k, dv[0], dv[1], dv[2]);
  }
  for (int k = 0; k < 3; ++k) ff[k] = ff[k] + add[k];
  const float* Jl = S.leg_J + o9;
  float lt[3];
  for (int k = 0; k < 3; ++k) lt[k] = 0.f + ((Jl[k] * ff[0] + Jl[3 + k] * ff[1]) + Jl[6 + k] * ff[2]);
  const bool safe = S.safe[b] != 0;
  for (int k = 0; k < 3; ++k) {
    const float tau = (float)((double)S.kp_joint * (0.0 - (double)S.q[o3 + k]) - (double)(S.kd_joint * S.qd[o3 + k]) +
                              (double)lt[k]);
    effort[o3 + k] = safe ? (double)tau : 0.0;
  }
}

}  // namespace

#endif
