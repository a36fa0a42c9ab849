// qmpc_glue.hip -- per-tick glue either side of the MPC solve, batched on the GPU:
//   qmpc_leg_kin_kernel    LegController::updateData (src/Controllers/LegController.cpp:89-110):
//                          foot position and Jacobian of every leg from the joint angles
//                          (computeLegJacobianAndPosition, :204-244) and foot velocity v = J qd
//   qmpc_leg_cmd_kernel    LegController::updateCommand (:116-160): Cartesian PD on the foot,
//                          tau = tauFF + J^T (forceFF + Kp (pDes - p) + Kd (vDes - v)), the joint PD
//                          of GaitCtrller's ctrlParam(2..3), and the desired joint angles (computeLegIK)
//   qmpc_swing_kernel      FootSwingTrajectory::computeSwingTrajectoryBezier
//                          (src/Controllers/FootSwingTrajectory.cpp:17-37)
// One thread per (robot, leg): small fixed-size float algebra, pure streaming of narrow rows
// (kinematics 96 B in / 240 B out per robot).  The arithmetic lives in qmpc_glue.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qmpc.h"

#include "qmpc_cmd.h"
#include "qmpc_glue.h"

namespace {

__global__ __launch_bounds__(256) void qmpc_leg_kin_kernel(const QmpcLegGeom g, const float* __restrict__ q,
                                                           const float* __restrict__ qd, float* __restrict__ J,
                                                           float* __restrict__ p, float* __restrict__ v, const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;  // robot * 4 + leg
  if (t >= n) return;
  const int leg = t & 3;
  const float q0 = q[(size_t)t * 3 + 0], q1 = q[(size_t)t * 3 + 1], q2 = q[(size_t)t * 3 + 2];
  float Jl[9], pl[3];
  qmpc_leg_fk(g, leg, q0, q1, q2, Jl, pl);
#pragma unroll
  for (int k = 0; k < 9; ++k) J[(size_t)t * 9 + k] = Jl[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[(size_t)t * 3 + k] = pl[k];
  if (v) {
    const float d0 = qd[(size_t)t * 3 + 0], d1 = qd[(size_t)t * 3 + 1], d2 = qd[(size_t)t * 3 + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[(size_t)t * 3 + k] = qmpc_row3(Jl + 3 * k, d0, d1, d2);  // datas[leg].v = J * qd  (:108)
  }
}

__global__ __launch_bounds__(256) void qmpc_leg_cmd_kernel(const QmpcLegGeom g, const qmpc_leg_command c,
                                                           float* __restrict__ tau, float* __restrict__ q_des,
                                                           const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;  // robot * 4 + leg
  if (t >= n) return;
  const int leg = t & 3;
  const size_t o3 = (size_t)t * 3, o9 = (size_t)t * 9;
  float lt[3], ff[3], dp[3], dv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lt[k] = c.tau_ff ? c.tau_ff[o3 + k] : 0.f;      // legTorque = tauFeedForward            (:121)
    ff[k] = c.force_ff ? c.force_ff[o3 + k] : 0.f;  // footForce = forceFeedForward          (:124)
    dp[k] = c.p_des[o3 + k] - c.p[o3 + k];
    dv[k] = c.v_des[o3 + k] - c.v[o3 + k];
  }
  // footForce += kpCartesian * (pDes - p); footForce += kdCartesian * (vDes - v)             (:128-131)
  float add[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) add[k] = qmpc_row3(c.kp_cart + o9 + 3 * k, dp[0], dp[1], dp[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) ff[k] = ff[k] + add[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) add[k] = qmpc_row3(c.kd_cart + o9 + 3 * k, dv[0], dv[1], dv[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) ff[k] = ff[k] + add[k];
  // legTorque += J^T * footForce                                                             (:134)
  const float* Jl = c.J + o9;
#pragma unroll
  for (int k = 0; k < 3; ++k) lt[k] = lt[k] + ((Jl[k] * ff[0] + Jl[3 + k] * ff[1]) + Jl[6 + k] * ff[2]);
  // tau_*_ff[leg] = crtlParam(2) * (0 - q) - crtlParam(3) * qd + legTorque                   (:138-158)
#pragma unroll
  for (int k = 0; k < 3; ++k)
    // (LegController.cpp:147-154 writes `crtlParam(2) * (0.0 - q)` with a DOUBLE literal: the joint-PD term and the sum
    //  are evaluated in double there and rounded to float once; kd * qd is a float product)
    tau[o3 + k] = (float)((double)c.kp_joint * (0.0 - (double)c.q[o3 + k]) - (double)(c.kd_joint * c.qd[o3 + k]) + (double)lt[k]);
  if (q_des) {  // computeLegIK(_quadruped, commands[leg].pDes, &qDes, leg)                  (:137)
    float qd3[3];
    qmpc_leg_ik(g, leg, c.p_des[o3 + 0], c.p_des[o3 + 1], c.p_des[o3 + 2], qd3);
#pragma unroll
    for (int k = 0; k < 3; ++k) q_des[o3 + k] = qd3[k];
  }
}

__global__ __launch_bounds__(256) void qmpc_swing_kernel(const float* __restrict__ p0, const float* __restrict__ pf,
                                                         const float* __restrict__ height, const float* __restrict__ phase,
                                                         const float* __restrict__ swing_time, float* __restrict__ p,
                                                         float* __restrict__ v, float* __restrict__ a, const int n) {
  const int t = blockIdx.x * 256 + threadIdx.x;  // foot index (robot * 4 + foot), one thread per axis triple
  if (t >= n) return;
  const size_t o = (size_t)t * 3;
  const float a0 = p0[o], a1 = p0[o + 1], a2 = p0[o + 2], b0 = pf[o], b1 = pf[o + 1], b2 = pf[o + 2];
  const float hgt = height[t], ph = phase[t], st = swing_time[t];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    float pp, vv, aa;
    qmpc_swing_axis(ax, ax == 0 ? a0 : a1, ax == 0 ? b0 : b1, a2, b2, hgt, ph, st, pp, vv, aa);
    p[o + ax] = pp;
    v[o + ax] = vv;
    a[o + ax] = aa;
  }
}

// ---------------------------------------------------------------------------------------------------
// LinearKFPositionVelocityEstimator<float>::run (src/Controllers/PositionVelocityEstimator.cpp:66-221):
// the 18-state / 28-measurement Kalman filter that turns leg kinematics + IMU into body position and
// velocity, one WAVE per robot, every matrix of the filter in LDS (12 KB).  The measurement matrix C is
// never stored: each of its rows has one +1 and at most one -1 (:28-46), so C Pm, C Pm C^T and Pm C^T
// are differences of rows / columns of Pm.  The two S.lu().solve() calls (:183, :186) are ONE LU with
// partial pivoting on the augmented matrix [S | ey | C].  Every output element is computed by one lane
// with its inner sums in index order and no fma, i.e. the same float operations in the same order as the
// restatement (oracle/glue_oracle.c) -- bit-identical results.
constexpr int KF_N = 18, KF_M = 28, KF_W = KF_M + 1 + KF_N;

__device__ __forceinline__ int kf_ca(int r) { return r < 12 ? r % 3 : (r < 24 ? 3 + r % 3 : 8 + 3 * (r - 24)); }
__device__ __forceinline__ int kf_cb(int r) { return r < 12 ? 6 + r : -1; }

__global__ __launch_bounds__(64) void qmpc_kf_kernel(const qmpc_kf_state s, const float hx, const float hy, const float hz,
                                                     const int batch) {
#pragma clang fp contract(off)
  __shared__ float Pm[KF_N * KF_N], AP[KF_N * KF_N], K1[KF_N * KF_M], CP[KF_M * KF_N], Sa[KF_M * KF_W];
  __shared__ float xh[KF_N], Q[KF_N], R[KF_M], y[KF_M];
  __shared__ int pivrow;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= batch) return;
  const float dt = 0.002f;
  float* Pg = s.P + (size_t)b * KF_N * KF_N;
  if (lane < KF_N) {
    xh[lane] = s.xhat[(size_t)b * KF_N + lane];
    // run() :73-76 with _Q0 of setup() :56-60
    Q[lane] = lane < 3 ? (dt / 20.f) * 0.02f : (lane < 6 ? (dt * 9.8f / 20.f) * 0.02f : dt * 0.002f);
  }
  if (lane < KF_M) R[lane] = 1.f * (lane < 12 ? 0.001f : (lane < 24 ? 0.1f : 0.001f));
  __syncthreads();
  if (lane < 4) {  // per leg :118-166
    const int i = lane;
    const float* rB = s.r_body + (size_t)b * 9;
    const float* om = s.omega_body + (size_t)b * 3;
    const float ph[3] = {(i == 0 || i == 1) ? hx : -hx, (i == 1 || i == 3) ? hy : -hy, hz};
    float p_rel[3], dp_rel[3], w[3], p_f[3], dp_f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p_rel[k] = ph[k] + s.leg_p[(size_t)b * 12 + 3 * i + k];
      dp_rel[k] = s.leg_v[(size_t)b * 12 + 3 * i + k];
    }
    w[0] = (om[1] * p_rel[2] - om[2] * p_rel[1]) + dp_rel[0];
    w[1] = (om[2] * p_rel[0] - om[0] * p_rel[2]) + dp_rel[1];
    w[2] = (om[0] * p_rel[1] - om[1] * p_rel[0]) + dp_rel[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // Rbod = rBody^T
      p_f[k] = (rB[0 * 3 + k] * p_rel[0] + rB[1 * 3 + k] * p_rel[1]) + rB[2 * 3 + k] * p_rel[2];
      dp_f[k] = (rB[0 * 3 + k] * w[0] + rB[1 * 3 + k] * w[1]) + rB[2 * 3 + k] * w[2];
    }
    float trust = 1.f;
    const float phase = fminf(s.contact_phase[(size_t)b * 4 + i], 1.f);
    const float trust_window = 0.2f;
    if (phase < trust_window) trust = phase / trust_window;
    else if (phase > (1.f - trust_window)) trust = (1.f - phase) / trust_window;
    const float factor = 1.f + (1.f - trust) * 100.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Q[6 + 3 * i + k] = factor * Q[6 + 3 * i + k];
      R[3 * i + k] = 1 * R[3 * i + k];
      R[12 + 3 * i + k] = factor * R[12 + 3 * i + k];
      y[3 * i + k] = -p_f[k];
      y[12 + 3 * i + k] = (1.0f - trust) * xh[3 + k] + trust * (-dp_f[k]);
    }
    R[24 + i] = factor * R[24 + i];
    y[24 + i] = (1.0f - trust) * (xh[2] + p_f[2]);
  }
  __syncthreads();
  if (lane < 3) {  // _xhat = _A * _xhat + _B * a  (:170), a = aWorld + (0, 0, -9.81)  (:95)
    const float ak = s.a_world[(size_t)b * 3 + lane] + (lane == 2 ? -9.81f : 0.f);
    const float xp = xh[lane], xv = xh[3 + lane];
    xh[lane] = xp + dt * xv;
    xh[3 + lane] = xv + dt * ak;
  }
  for (int e = lane; e < KF_N * KF_N; e += 64) {  // A P
    const int i = e / KF_N, j = e - KF_N * i;
    AP[e] = (i < 3) ? Pg[e] + dt * Pg[(i + 3) * KF_N + j] : Pg[e];
  }
  __syncthreads();
  for (int e = lane; e < KF_N * KF_N; e += 64) {  // Pm = (A P) A^T + Q  (:172)
    const int i = e / KF_N, j = e - KF_N * i;
    float v = (j < 3) ? AP[e] + dt * AP[e + 3] : AP[e];
    if (i == j) v = v + Q[i];
    Pm[e] = v;
  }
  __syncthreads();
  for (int e = lane; e < KF_M * KF_N; e += 64) {  // C Pm and Pm C^T
    const int r = e / KF_N, j = e - KF_N * r;
    CP[e] = (kf_cb(r) >= 0) ? Pm[kf_ca(r) * KF_N + j] - Pm[kf_cb(r) * KF_N + j] : Pm[kf_ca(r) * KF_N + j];
    const int i = e / KF_M, c = e - KF_M * i;
    K1[e] = (kf_cb(c) >= 0) ? Pm[i * KF_N + kf_ca(c)] - Pm[i * KF_N + kf_cb(c)] : Pm[i * KF_N + kf_ca(c)];
  }
  __syncthreads();
  for (int e = lane; e < KF_M * KF_W; e += 64) {  // [ S | ey | C ],  S = C Pm C^T + R (:177), ey = y - C xhat (:175-176)
    const int r = e / KF_W, c = e - KF_W * r;
    float v;
    if (c < KF_M) {
      v = (kf_cb(c) >= 0) ? CP[r * KF_N + kf_ca(c)] - CP[r * KF_N + kf_cb(c)] : CP[r * KF_N + kf_ca(c)];
      if (r == c) v = v + R[r];
    } else if (c == KF_M) {
      const float ym = (kf_cb(r) >= 0) ? xh[kf_ca(r)] - xh[kf_cb(r)] : xh[kf_ca(r)];
      v = y[r] - ym;
    } else {
      const int j = c - KF_M - 1;
      v = (j == kf_ca(r)) ? 1.f : ((j == kf_cb(r)) ? -1.f : 0.f);
    }
    Sa[e] = v;
  }
  __syncthreads();
  for (int k = 0; k < KF_M; ++k) {  // LU with partial pivoting (first largest wins), every right-hand side carried along
    if (lane == 0) {
      int piv = k;
      float best = fabsf(Sa[k * KF_W + k]);
      for (int r = k + 1; r < KF_M; ++r) {
        const float a = fabsf(Sa[r * KF_W + k]);
        if (a > best) {
          best = a;
          piv = r;
        }
      }
      pivrow = piv;
    }
    __syncthreads();
    const int piv = pivrow;
    if (piv != k && lane < KF_W) {
      const float t = Sa[k * KF_W + lane];
      Sa[k * KF_W + lane] = Sa[piv * KF_W + lane];
      Sa[piv * KF_W + lane] = t;
    }
    __syncthreads();
    const float dkk = Sa[k * KF_W + k];
    const int ncol = KF_W - (k + 1), nel = (KF_M - (k + 1)) * ncol;
    for (int e = lane; e < nel; e += 64) {
      const int r = k + 1 + e / ncol, c = k + 1 + e % ncol;
      const float l = Sa[r * KF_W + k] / dkk;
      Sa[r * KF_W + c] = Sa[r * KF_W + c] - l * Sa[k * KF_W + c];
    }
    __syncthreads();
  }
  if (lane < KF_W - KF_M) {  // back substitution: one right-hand side per lane
    const int c = KF_M + lane;
    for (int r = KF_M - 1; r >= 0; --r) {
      float acc = Sa[r * KF_W + c];
      for (int j = r + 1; j < KF_M; ++j) acc = acc - Sa[r * KF_W + j] * Sa[j * KF_W + c];
      Sa[r * KF_W + c] = acc / Sa[r * KF_W + r];
    }
  }
  __syncthreads();
  if (lane < KF_N) {  // _xhat += Pm C^T S_ey  (:184)
    float acc = 0.f;
    for (int c = 0; c < KF_M; ++c) acc = acc + K1[lane * KF_M + c] * Sa[c * KF_W + KF_M];
    xh[lane] = xh[lane] + acc;
  }
  for (int e = lane; e < KF_N * KF_N; e += 64) {  // T1 = I - Pm C^T S_C
    const int i = e / KF_N, j = e - KF_N * i;
    float acc = 0.f;
    for (int c = 0; c < KF_M; ++c) acc = acc + K1[i * KF_M + c] * Sa[c * KF_W + KF_M + 1 + j];
    AP[e] = ((i == j) ? 1.f : 0.f) - acc;
  }
  __syncthreads();
  for (int e = lane; e < KF_N * KF_N; e += 64) {  // _P = T1 Pm  (:187)
    const int i = e / KF_N, j = e - KF_N * i;
    float acc = 0.f;
    for (int k = 0; k < KF_N; ++k) acc = acc + AP[i * KF_N + k] * Pm[k * KF_N + j];
    CP[e] = acc;  // (C Pm is dead)
  }
  __syncthreads();
  for (int e = lane; e < KF_N * KF_N; e += 64) {  // (_P + _P^T) / 2  (:189-190)
    const int i = e / KF_N, j = e - KF_N * i;
    Pm[e] = (CP[e] + CP[j * KF_N + i]) / 2.f;
  }
  __syncthreads();
  const bool reset = Pm[0] * Pm[KF_N + 1] - Pm[1] * Pm[KF_N] > 0.000001f;  // :192-196
  for (int e = lane; e < KF_N * KF_N; e += 64) {
    const int i = e / KF_N, j = e - KF_N * i;
    float v = Pm[e];
    if (reset) {
      if ((i < 2) != (j < 2)) v = 0.f;
      else if (i < 2 && j < 2) v = v / 10.f;
    }
    Pg[e] = v;
  }
  if (lane < KF_N) s.xhat[(size_t)b * KF_N + lane] = xh[lane];
  if (lane < 3) {
    s.position[(size_t)b * 3 + lane] = xh[lane];
    s.v_world[(size_t)b * 3 + lane] = xh[3 + lane];
    const float* rB = s.r_body + (size_t)b * 9;  // vBody = rBody * vWorld  (:212-214)
    if (s.v_body) s.v_body[(size_t)b * 3 + lane] = (rB[3 * lane] * xh[3] + rB[3 * lane + 1] * xh[4]) + rB[3 * lane + 2] * xh[5];
  }
}

__global__ __launch_bounds__(256) void qmpc_kf_init_kernel(float* __restrict__ xhat, float* __restrict__ P, const int batch) {
  const int t = blockIdx.x * 256 + threadIdx.x;  // setup() :22-24, :52-53: xhat = 0, P = 100 I
  if (t >= batch * KF_N * KF_N) return;
  const int e = t % (KF_N * KF_N), b = t / (KF_N * KF_N);
  P[t] = (e / KF_N == e % KF_N) ? 100.f : 0.f;
  if (e < KF_N) xhat[(size_t)b * KF_N + e] = 0.f;
}

}  // namespace

extern "C" hipError_t qmpc_launch_leg_kin(const float geom[4], const float* q, const float* qd, float* J, float* p,
                                          float* v, int batch, hipStream_t stream) {
  const QmpcLegGeom g{geom[0], geom[1], geom[2], geom[3]};
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_leg_kin_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, g, q, qd, J, p, v, n);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_leg_cmd(const float geom[4], const qmpc_leg_command* c, float* tau, float* q_des,
                                          int batch, hipStream_t stream) {
  const QmpcLegGeom g{geom[0], geom[1], geom[2], geom[3]};
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_leg_cmd_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, g, *c, tau, q_des, n);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_swing(const float* p0, const float* pf, const float* height, const float* phase,
                                        const float* swing_time, float* p, float* v, float* a, int n_feet,
                                        hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_swing_kernel, dim3((n_feet + 255) / 256), dim3(256), 0, stream, p0, pf, height, phase,
                     swing_time, p, v, a, n_feet);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_kf(const qmpc_kf_state* st, const float hip[3], int batch, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_kf_kernel, dim3(batch), dim3(64), 0, stream, *st, hip[0], hip[1], hip[2], batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_kf_init(float* xhat, float* P, int batch, hipStream_t stream) {
  const int n = batch * 18 * 18;
  hipLaunchKernelGGL(qmpc_kf_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, xhat, P, batch);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Batched locomotion controller (include/qmpc_ctrl.h): GaitCtrller::TorqueCalculator (src/GaitCtrller.cpp:95-145)
// in robot mode 0 or 1 (qmpc_ctrl_set_robot_mode: the locomotion kernel's template argument), as five launches per tick:
//   qmpc_ctrl_est_kernel     pre_work: VectorNavOrientationEstimator::run (OrientationEstimator.cpp:46-110) and
//                            LegController::updateData (one thread per (robot, leg); leg 0 also runs the estimator)
//   (qmpc_ctrl_est_state_kernel  in its place AND the filter's on a tick driven by simulator ground truth,
//                            qmpc_ctrl_tick_state: the reference's two Cheater estimators and the same updateData)
//   qmpc_kf_kernel           the Kalman filter above, on the previous tick's leg data (the estimators run before
//                            updateData, GaitCtrller.cpp:58-63) and the contact phase of the previous tick
//   qmpc_ctrl_loco_kernel    the safety checks and ConvexMPCLocomotion::run up to the MPC (one thread per robot):
//                            writes the qmpc_command rows
//   (the solve               lockstep: qmpc_solve_commands on the ticks whose incremented counter is a multiple of 13,
//                            decided on the host from T; per-robot schedule: every tick, over the list of due
//                            robots the locomotion kernel left -- qmpc_capi.cpp: solve_impl's due list)
//   qmpc_ctrl_legcmd_kernel  f_ff from the solve, the swing / stance gains, LegController::updateCommand, the latch
// Decisions where the reference's C++ does not say what it computes at first sight (pinned by
// tests/test_gpu_controller.py and tests/test_ctrl_cpu.py):
//  * overload resolution.  SafetyChecker.cpp and ConvexMPCLocomotion.cpp include Eigen (Utilities/cppTypes.h), which on
//    x86-64 vectorises with SSE2 by default and so includes <emmintrin.h> -> <xmmintrin.h> -> <mm_malloc.h> -> <stdlib.h>;
//    in C++ that is libstdc++'s wrapper, whose `using std::abs;` puts the float overload into the global namespace.
//    Unqualified abs(float) therefore binds to float abs(float) (GCC 11: decltype(abs(0.7f)) is int with <cmath> and
//    <cstdlib> alone, float once <emmintrin.h> is included): the orientation check trips at |roll| or |pitch| >= 0.5,
//    and the yaw re-anchor at |rpy[2] - yaw_des_true| > 5.0.  No header of the chain brings sqrt's float overload into
//    the global namespace: unqualified sqrt(float) binds to double sqrt(double).
//  * double promotion.  pfx_rel / pfy_rel (:346-356) are evaluated in double -- `(.5 + 0.0)`, `.5 * stance_time * 1.0`
//    and the double sqrt -- with the float sub-expressions rounded first, and stored to float once.
//  * truncated gait integers: Vec4<int>(double) makes walking offsets (0, 7, 3, 10), durations 10 (:37-38).
//  * timing: setIterations sees the counter before the increment (:239), the increment comes before
//    updateMPCIfNeeded (:375, :387): the first solve is at the 13th tick, on table iteration 0.
//  * swing state: setInitialPosition also sets _p; a stance foot's pDes is the trajectory's last _p / _v.
//  * robot mode 1 reads OffsetDurationGait::_phase (Gait.h:57) on its first tick before anything wrote it (undefined in
//    the reference): here it starts at 0, so the first tick takes the phase-0 branch; qmpc_ctrl_reset restores that.
//  * omni mode per robot: qmpc_command carries ONE omni flag; the command's rBody row is the identity for omni
//    robots (v_des_world = v_des_robot, :505-507) and f_ff = -rBody grf is formed here with the true rBody
//    (qmpc_cmd_f2b, the solve's own arithmetic).
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

__global__ __launch_bounds__(256) void qmpc_ctrl_est_kernel(const QmpcCtrlDev S, const QmpcLegGeom g,
                                                            const double* __restrict__ imu,
                                                            const double* __restrict__ motor, const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;  // robot * 4 + leg
  if (t >= n) return;
  const int b = t >> 2, leg = t & 3;
  const size_t o3 = (size_t)t * 3;
  if (t == 0) S.due_count[0] = 0;  // the tick's list of due robots starts empty (filled by the locomotion kernel)
  const QmpcLegJoints j = qmpc_ctrl_leg_joints(motor + (size_t)b * 24, leg);
  for (int k = 0; k < 3; ++k) {  // what the Kalman filter of this tick reads: updateData has not run yet
    S.kf_p[o3 + k] = S.leg_p[o3 + k];
    S.kf_v[o3 + k] = S.leg_v[o3 + k];
  }
  qmpc_ctrl_leg_update(S, g, t, leg, j);
  if (leg == 0) qmpc_ctrl_orientation(S, b, imu + (size_t)b * 10);
}

// pre_work of a tick driven by simulator ground truth (qmpc_ctrl_tick_state): the same leg data, and the two cheater
// estimators in place of the VectorNav estimator and the Kalman filter.  state: [B][16] double.  Memory-shaped: per
// robot 320 B in (one thread reads the 128 B state row, the four leg threads 48 B each of the motor row) and 504 B out.
__global__ __launch_bounds__(256) void qmpc_ctrl_est_state_kernel(const QmpcCtrlDev S, const QmpcLegGeom g,
                                                                  const double* __restrict__ state,
                                                                  const double* __restrict__ motor, const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;  // robot * 4 + leg
  if (t >= n) return;
  const int b = t >> 2, leg = t & 3;
  if (t == 0) S.due_count[0] = 0;  // the tick's list of due robots starts empty (filled by the locomotion kernel)
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

// The safety checks and ConvexMPCLocomotion::run up to updateMPCIfNeeded, one thread per robot
// build_list (per-robot schedule): the due robots also append themselves to S.due_list, one atomic per wave
// MODE: the controller's robot mode (qmpc_ctrl_set_robot_mode).  0: the gait picked by number, 14 segments (:150-172).
// 1: the `aio` gait (:173-233), whose segment count, offsets and durations are the robot's own rows and change on
// phase-0 ticks only; everything below the gait selection reads them where mode 0 has the literal 14.
template <int MODE>
__global__ __launch_bounds__(256) void qmpc_ctrl_loco_kernel(const QmpcCtrlDev S, const int batch, const int build_list) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const float dt = S.dt, dtMPC = S.dt_mpc;
  const float* rB = S.r_body + (size_t)b * 9;
  float pos[3], vW[3], rpy[3];
  for (int k = 0; k < 3; ++k) {
    pos[k] = S.position[(size_t)b * 3 + k];
    vW[k] = S.v_world[(size_t)b * 3 + k];
    rpy[k] = S.rpy[(size_t)b * 3 + k];
  }
  // ---- safety (GaitCtrller.cpp:108-123) on the zeroed commands: checkPDesFoot and checkForceFeedForward pass;
  //      checkSafeOrientation's abs is the float overload (see the header of this section); checkJointLimit clamps q
  if ((double)fabsf(rpy[0]) >= 0.5 || (double)fabsf(rpy[1]) >= 0.5) {
    S.safe[b] = 0;
  } else {
    const float max_ab_ad = 1.0472f, max_hip = 0.174533f, min_hip = -1.8f, max_knee = 2.79253f, min_knee = -0.174533f;
    bool ok = true;
    float* q = S.q + (size_t)b * 12;
    for (int leg = 0; leg < 4; ++leg) {  // SafetyChecker.cpp checkJointLimit, in its order
      float* ql = q + 3 * leg;
      if (ql[0] < -max_ab_ad) { ql[0] = -max_ab_ad; ok = false; }
      if (ql[0] > max_ab_ad) { ql[0] = max_ab_ad; ok = false; }
      if (ql[1] < min_hip) { ql[1] = min_hip; ok = false; }
      if (ql[1] > max_hip) { ql[1] = max_hip; ok = false; }
      if (ql[2] > max_knee) { ql[2] = max_knee; ok = false; }
      if (ql[2] < min_knee) { ql[2] = min_knee; ok = false; }
    }
    if (!ok) S.safe[b] = 0;
  }
  // ---- _SetupCommand (ConvexMPCLocomotion.cpp:76-114; _body_height = 0.25 is the command's body_height)
  float* vd = S.vel_des + (size_t)b * 3;
  const float xc = S.vel_cmd[(size_t)b * 3], yc = S.vel_cmd[(size_t)b * 3 + 1], wc = S.vel_cmd[(size_t)b * 3 + 2];
  const float x_filter = 0.01f, y_filter = 0.006f, yaw_filter = 0.03f;
  float xv = vd[0] * (1 - x_filter) + xc * x_filter;
  float yv = vd[1] * (1 - y_filter) + yc * y_filter;
  const float yr = vd[2] * (1 - yaw_filter) + wc * yaw_filter;
  if ((double)xv > 2.0) xv = 2.f;
  else if ((double)xv < -1.0) xv = -1.f;
  if ((double)yv > 0.6) yv = (float)0.6;
  else if ((double)yv < -0.6) yv = (float)-0.6;
  vd[0] = xv;
  vd[1] = yv;
  vd[2] = yr;
  S.yaw_des[b] = rpy[2] + dt * yr;
  float ydt = S.yaw_des_true[b];
  if ((double)fabsf(rpy[2] - ydt) > 5.0) ydt = rpy[2];  // abs(float) (:106)
  ydt = ydt + dt * yr;
  S.yaw_des_true[b] = ydt;
  // ---- run (:116-496)
  int gn = S.gait_num[b];
  const bool omni = gn >= 20;
  if (omni) gn -= 20;
  float* wpd = S.wpd + (size_t)b * 2;
  float* st = S.stand_traj + (size_t)b * 6;
  const bool first_run = S.first_run[b] != 0;
  if ((gn == 4 && S.current_gait[b] != 4) || first_run) {  // :137-146
    st[0] = pos[0];
    st[1] = pos[1];
    st[2] = 0.21f;
    st[3] = 0.f;
    st[4] = 0.f;
    st[5] = rpy[2];
    wpd[0] = st[0];
    wpd[1] = st[1];
  }
  int off[4], dur[4];
  int cnt = S.counter[b];
  int nseg = 14;
  const int ibm = 13;
  bool standing;
  if constexpr (MODE == 0) {
    qmpc_ctrl_gait(gn, off, dur);
    standing = gn == 4;
    S.current_gait[b] = gn;
  } else {
    // gait = &aio; gaitNumber = 9 (:176-177).  The gait keeps its parameters from tick to tick: setGaitParam is
    // called only where the phase the PREVIOUS tick's setIterations left is 0 (:178).  A fresh robot's phase is 0
    // (the reference reads an uninitialised float there: INTEGRATION.md section F), so its first tick selects.
    nseg = S.nseg[b];
    for (int l = 0; l < 4; ++l) {
      off[l] = S.offsets[(size_t)b * 4 + l];
      dur[l] = S.durations[(size_t)b * 4 + l];
    }
    int cg = 9;
    if (S.gait_phase[b] == 0.f) {
      int h;
      cg = qmpc_ctrl_aio_gait(xv, yv, yr, h, off, dur);
      if (nseg != h) cnt = 0;  // if (gait->getGaitHorizon() != h) iterationCounter = 0
      nseg = h;
      S.nseg[b] = h;
    }
    // (horizonLength = h (:233) is 10 on every tick that solves: such a tick is never a phase-0 tick)
    standing = false;          // `gait != &standing` (:277) holds for &aio, its standing case included
    S.current_gait[b] = cg;    // 4 only on a phase-0 tick of the standing case: never on a tick that solves
  }
  S.iteration[b] = (cnt / ibm) % nseg;  // setIterations (Gait.cpp:187-193) with the counter before the increment
  const float phase = (float)(cnt % (ibm * nseg)) / (float)(ibm * nseg);
  if constexpr (MODE == 1) S.gait_phase[b] = phase;
  for (int l = 0; l < 4; ++l) {
    S.offsets[(size_t)b * 4 + l] = off[l];
    S.durations[(size_t)b * 4 + l] = dur[l];
  }
  float vw0, vw1;
  qmpc_cmd_vdes_world(rB, xv, yv, omni ? 1 : 0, vw0, vw1);
  float* ri = S.rpy_int + (size_t)b * 2;
  float* rc = S.rpy_comp + (size_t)b * 2;
  if ((double)fabsf(vW[0]) > .2) ri[1] = ri[1] + (dt * (0.f - rpy[1])) / vW[0];
  if ((double)fabsf(vW[1]) > 0.1) ri[0] = ri[0] + (dt * (0.f - rpy[0])) / vW[1];
  ri[0] = fminf(fmaxf(ri[0], -.25f), .25f);
  ri[1] = fminf(fmaxf(ri[1], -.25f), .25f);
  rc[1] = vW[0] * ri[1];
  rc[0] = vW[1] * ri[0];
  float pF[12];
  for (int i = 0; i < 4; ++i) {  // pFoot = position + rBody^T (hip + p)
    float h[3];
    qmpc_hip_location(i, h);
    float x[3];
    for (int k = 0; k < 3; ++k) x[k] = h[k] + S.leg_p[(size_t)b * 12 + 3 * i + k];
    for (int k = 0; k < 3; ++k) pF[3 * i + k] = pos[k] + ((rB[k] * x[0] + rB[3 + k] * x[1]) + rB[6 + k] * x[2]);
  }
  for (int k = 0; k < 12; ++k) S.p_foot[(size_t)b * 12 + k] = pF[k];
  if (!standing) {
    wpd[0] = wpd[0] + dt * vw0;
    wpd[1] = wpd[1] + dt * vw1;
  }
  float* p0 = S.sw_p0 + (size_t)b * 12;
  float* pf = S.sw_pf + (size_t)b * 12;
  float* sp = S.sw_p + (size_t)b * 12;
  float* sv = S.sw_v + (size_t)b * 12;
  if (first_run) {
    wpd[0] = pos[0];
    wpd[1] = pos[1];
    for (int k = 0; k < 12; ++k) {
      p0[k] = pF[k];
      sp[k] = pF[k];
      pf[k] = pF[k];
    }
    S.first_run[b] = 0;
  }
  // foot placement (:297-372)
  float* swt = S.swing_time + (size_t)b * 4;
  float* rem = S.swing_rem + (size_t)b * 4;
  int* fs = S.first_swing + (size_t)b * 4;
  for (int l = 0; l < 4; ++l) swt[l] = dtMPC * (float)(nseg - dur[l]);
  const float interleave_y[4] = {-0.08f, 0.08f, 0.02f, -0.02f};
  const float interleave_gain = -0.2f;
  const float v_abs = fabsf(xv);
  const double sqrt_term = 0.5f * sqrt((double)(pos[2] / 9.81f));  // double sqrt(double) -- see above
  for (int i = 0; i < 4; ++i) {
    if (fs[i]) rem[i] = swt[i];
    else rem[i] = rem[i] - dt;
    float pr[3];
    qmpc_hip_location(i, pr);
    pr[1] = pr[1] + (float)((double)qmpc_side_sign(i) * .065);
    pr[1] = pr[1] + (interleave_y[i] * v_abs) * interleave_gain;
    const float stance_time = dtMPC * (float)dur[i];
    const float th = ((-yr) * stance_time) / 2;
    const float s = sinf(th), c = cosf(th);  // coordinateRotation(Z, th) = [c s 0; -s c 0; 0 0 1]
    float py[3];
    py[0] = (c * pr[0] + s * pr[1]) + 0.f * pr[2];
    py[1] = (-s * pr[0] + c * pr[1]) + 0.f * pr[2];
    py[2] = (0.f * pr[0] + 0.f * pr[1]) + 1.f * pr[2];
    const float dv[3] = {xv, yv, 0.f};
    float x[3];
    for (int k = 0; k < 3; ++k) x[k] = py[k] + dv[k] * rem[i];
    float P[3];
    for (int k = 0; k < 3; ++k) P[k] = pos[k] + ((rB[k] * x[0] + rB[3 + k] * x[1]) + rB[6 + k] * x[2]);
    const float p_rel_max = 0.3f;
    float pfx = (float)((((double)vW[0] * (.5 + 0.0)) * (double)stance_time + (double)(.03f * (vW[0] - vw0))) +
                        sqrt_term * (double)(vW[1] * yr));
    float pfy = (float)(((((double)vW[1] * .5) * (double)stance_time) * 1.0 + (double)(.03f * (vW[1] - vw1))) +
                        sqrt_term * (double)((-vW[0]) * yr));
    pfx = fminf(fmaxf(pfx, -p_rel_max), p_rel_max);
    pfy = fminf(fmaxf(pfy, -p_rel_max), p_rel_max);
    S.pf_rel[(size_t)b * 8 + 2 * i] = pfx;
    S.pf_rel[(size_t)b * 8 + 2 * i + 1] = pfy;
    P[0] = P[0] + pfx;
    P[1] = P[1] + pfy;
    P[2] = 0.f;
    for (int k = 0; k < 3; ++k) pf[3 * i + k] = P[k];
  }
  S.counter[b] = cnt + 1;  // :375
  // gait states (:384-385) and the swing / stance state machine (:394-472)
  float* cs = S.contact_state + (size_t)b * 4;
  float* ss = S.swing_state + (size_t)b * 4;
  const float height = 0.06f;
  for (int foot = 0; foot < 4; ++foot) {
    float contact, swing;
    qmpc_ctrl_gait_state(phase, off[foot], dur[foot], nseg, contact, swing);
    cs[foot] = contact;
    ss[foot] = swing;
    float* fp = sp + 3 * foot;
    float* fv = sv + 3 * foot;
    if (swing > 0) {
      if (fs[foot]) {
        fs[foot] = 0;
        for (int k = 0; k < 3; ++k) {
          p0[3 * foot + k] = pF[3 * foot + k];
          fp[k] = pF[3 * foot + k];
        }
      }
      for (int ax = 0; ax < 3; ++ax) {
        float pp, vv, aa;
        qmpc_swing_axis(ax, p0[3 * foot + ax], pf[3 * foot + ax], p0[3 * foot + 2], pf[3 * foot + 2], height, swing,
                        swt[foot], pp, vv, aa);
        fp[ax] = pp;
        fv[ax] = vv;
      }
      S.contact_phase[(size_t)b * 4 + foot] = 0.f;
    } else {
      fs[foot] = 1;
      S.contact_phase[(size_t)b * 4 + foot] = contact;
    }
    // pDesLeg = rBody (pDesFootWorld - position) - hip; vDesLeg = rBody (vDesFootWorld - vWorld)
    float h[3], dp[3], dvv[3];
    qmpc_hip_location(foot, h);
    for (int k = 0; k < 3; ++k) {
      dp[k] = fp[k] - pos[k];
      dvv[k] = fv[k] - vW[k];
    }
    for (int k = 0; k < 3; ++k) {
      S.p_des[(size_t)b * 12 + 3 * foot + k] = qmpc_row3(rB + 3 * k, dp[0], dp[1], dp[2]) - h[k];
      S.v_des[(size_t)b * 12 + 3 * foot + k] = qmpc_row3(rB + 3 * k, dvv[0], dvv[1], dvv[2]);
    }
  }
  // the MPC command's rBody: the identity for omni robots (v_des_world = v_des_robot); f_ff uses the true rBody
  float* rc9 = S.r_cmd + (size_t)b * 9;
  for (int k = 0; k < 9; ++k) rc9[k] = omni ? ((k % 4 == 0) ? 1.f : 0.f) : rB[k];
  // the MPC schedule: updateMPCIfNeeded solves when the incremented counter is a multiple of 13 (:387)
  const bool due = (cnt + 1) % ibm == 0;
  S.due[b] = due ? 1 : 0;
  if constexpr (MODE == 1) {
    if (due) {  // the ten rows of the robot's table that the horizon-10 solve reads, as a 10-segment gait
      const int it = (cnt / ibm) % nseg;
      for (int l = 0; l < 4; ++l) {
        int o10, d10;
        qmpc_ctrl_window_gait(it, off[l], dur[l], nseg, o10, d10);
        S.mpc_offsets[(size_t)b * 4 + l] = o10;
        S.mpc_durations[(size_t)b * 4 + l] = d10;
      }
    }
  }
  if (build_list) {
    // dense list of the due robots (what the solve's first launch consumes): the wave's due lanes take consecutive
    // places behind one atomic add of its first due lane; at most `batch` entries (every robot appends at most once)
    const unsigned long long m = __ballot(due);
    if (m) {
      const int lane = (int)__lane_id(), leader = __ffsll(m) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(S.due_count, __popcll(m));
      base = __shfl(base, leader);
      if (due) S.due_list[base + __popcll(m & ((1ull << lane) - 1ull))] = b;
    }
  }
}

// f_ff (on MPC ticks), the gains of :378-382, LegController::updateCommand and the latch; one thread per (robot, leg)
__global__ __launch_bounds__(256) void qmpc_ctrl_legcmd_kernel(const QmpcCtrlDev S, double* __restrict__ effort,
                                                               const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
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

// qmpc_ctrl_init / qmpc_ctrl_reset: the state of a fresh GaitCtrller (mask == NULL: every robot), qmpc_glue.h's list
__global__ __launch_bounds__(256) void qmpc_ctrl_init_kernel(const QmpcCtrlDev S, const uint8_t* __restrict__ mask,
                                                             const int counter0, const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (mask && !mask[b]) return;
  qmpc_ctrl_init_robot<true>(S, b, counter0);
}

__global__ __launch_bounds__(256) void qmpc_ctrl_set_kernel(const QmpcCtrlDev S, const int32_t* __restrict__ gait,
                                                            const double* __restrict__ vel, const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (gait) S.gait_num[b] = gait[b];
  if (vel)  // SetRobotVel (GaitCtrller.cpp:75-93): abs(double) there is the double overload (<math.h>)
    for (int k = 0; k < 3; ++k) {
      const double v = vel[(size_t)b * 3 + k];
      S.vel_cmd[(size_t)b * 3 + k] = (float)(fabs(v) < 0.03 ? 0.0 : v * 1.0);
    }
}

}  // namespace

extern "C" hipError_t qmpc_launch_ctrl_init(const QmpcCtrlDev* S, const uint8_t* mask, int counter0, int batch,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_ctrl_init_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, mask, counter0, batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_ctrl_set(const QmpcCtrlDev* S, const int32_t* gait, const double* vel, int batch,
                                           hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_ctrl_set_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, gait, vel, batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_ctrl_est(const QmpcCtrlDev* S, const float geom[4], const double* imu,
                                           const double* motor, int batch, hipStream_t stream) {
  const QmpcLegGeom g{geom[0], geom[1], geom[2], geom[3]};
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_ctrl_est_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *S, g, imu, motor, n);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_ctrl_est_state(const QmpcCtrlDev* S, const float geom[4], const double* state,
                                                 const double* motor, int batch, hipStream_t stream) {
  const QmpcLegGeom g{geom[0], geom[1], geom[2], geom[3]};
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_ctrl_est_state_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *S, g, state, motor, n);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_ctrl_loco(const QmpcCtrlDev* S, int batch, int build_list, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_ctrl_loco_kernel<0>, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, batch, build_list);
  return hipGetLastError();
}

// robot mode 1 (always with the per-robot schedule: the list of due robots is built)
extern "C" hipError_t qmpc_launch_ctrl_loco_aio(const QmpcCtrlDev* S, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_ctrl_loco_kernel<1>, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, batch, 1);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_ctrl_legcmd(const QmpcCtrlDev* S, double* effort, int batch, hipStream_t stream) {
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_ctrl_legcmd_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *S, effort, n);
  return hipGetLastError();
}
