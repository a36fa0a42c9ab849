// qmpc_plant.hip -- the reduced-order plant of include/qmpc_plant.h: one launch per control period, one lane per
// (robot, leg) as in the glue kernels.  Every lane of a robot's quad carries a copy of the body state; a leg's force and
// moment are summed over the quad with two xor-shuffles, (f_0 + f_1) + (f_2 + f_3) in every lane (the sum is
// commutative, so the four lanes hold the same bits), and the four lanes integrate the same body redundantly -- no
// broadcast, no LDS, no atomics.  Lane 0 of the quad stores the body; every lane stores its own foot and joints.
// fp contraction is off, as in the glue code: tests/plant_model.py restates every expression in the same order.
//
// Decisions the model leaves open (the same list as in include/qmpc_plant.h):
//  * order inside a step: contact edges (touch-down sets c_z = 0) -> `substeps` x [stance forces at the current pose
//    with the torque held -> quad sums -> vdot, wdot -> v, w -> p, q] -> swing feet placed at the new pose -> read-out.
//  * forces: F_body = J^-T tau by cofactors of the fp64 Jacobian at the plant's own angles (IK of the pinned foot);
//    |det J| < QMPC_PLANT_DET_MIN = 1e-5 m^3 (det = l2 l3 sin(knee) rho up to sign: a straight knee) -> f = 0; f_z <= 0
//    -> f = 0; tangential part scaled to mu f_z when larger.  The foot stays pinned whatever the force.
//  * quaternion: q (x) dq with dq from the new body-frame w, exponential map, first-order below |w| h = 1e-12, then
//    normalised.
//  * swing clamp: radial scaling of p_des into |r|^2 in [r2_lo, r2_hi] (knee angle 2.6 .. 0.05 rad); a zero command
//    reads (0, 0, -sqrt(r2_lo)).  IK clamps rho^2 at 0 and D to [-1, 1], so it returns angles for every input.
//  * IK branch: knee >= 0 (qmpc_leg_fk's standing pose); no wrapping of the abad angle (the two atan2 terms cancel
//    near the standing pose).
//  * pinned foot's hip-frame velocity: -rBody v - w x (rBody (c - p)), lever arm from the body origin.
//  * accelerometer: rBody_new (vdot_last + (0, 0, g)).
#include "qmpc_plant.h"

namespace {

struct PlantLeg {
  double ang[3];  // abad, hip, knee
  double C[9];    // cofactors of J (row-major): J^-1 = C^T / det
  double det;
};

// R(q), row-major, body -> world (ori::quaternionToRotationMatrix before its transpose); rBody = R^T
__device__ __forceinline__ void plant_rot(const double* q, double* R) {
#pragma clang fp contract(off)
  const double e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3];
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
// y = R x (body -> world)
__device__ __forceinline__ void plant_mul(const double* R, const double* x, double* y) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) y[k] = (R[3 * k] * x[0] + R[3 * k + 1] * x[1]) + R[3 * k + 2] * x[2];
}
// y = R^T x = rBody x (world -> body)
__device__ __forceinline__ void plant_mulT(const double* R, const double* x, double* y) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) y[k] = (R[k] * x[0] + R[3 + k] * x[1]) + R[6 + k] * x[2];
}
__device__ __forceinline__ void plant_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void plant_hip(int leg, double* h) {
  h[0] = (double)((leg == 0 || leg == 1) ? 0.19f : -0.19f);
  h[1] = (double)((leg == 1 || leg == 3) ? 0.049f : -0.049f);
  h[2] = 0.0;
}

// Inverse kinematics of the hip-frame foot position r (knee >= 0), the Jacobian of qmpc_leg_fk at those angles in fp64,
// its cofactors and determinant
__device__ __forceinline__ void plant_leg(const QmpcPlantConst& K, double side, const double* r, PlantLeg& L) {
#pragma clang fp contract(off)
  const double l1 = K.geom[0] + K.geom[3], l2 = K.geom[1], l3 = K.geom[2];
  const double x = r[0], y = r[1], z = r[2];
  double rho2 = (y * y + z * z) - l1 * l1;
  if (rho2 < 0.0) rho2 = 0.0;
  const double rho = sqrt(rho2);
  double D = (((x * x + rho2) - l2 * l2) - l3 * l3) / (2 * l2 * l3);
  if (D > 1.0) D = 1.0;
  if (D < -1.0) D = -1.0;
  const double sk = sqrt(1 - D * D);
  L.ang[2] = atan2(sk, D);
  L.ang[1] = atan2(x, rho) - atan2(l3 * sk, l2 + l3 * D);
  L.ang[0] = atan2(z, y) - atan2(-rho, side * l1);
  // computeLegJacobianAndPosition (LegController.cpp:204-244) in double
  const double s1 = sin(L.ang[0]), s2 = sin(L.ang[1]), s3 = sin(L.ang[2]);
  const double c1 = cos(L.ang[0]), c2 = cos(L.ang[1]), c3 = cos(L.ang[2]);
  const double c23 = c2 * c3 - s2 * s3;
  const double s23 = s2 * c3 + c2 * s3;
  const double J0 = 0.0;
  const double J1 = l3 * c23 + l2 * c2;
  const double J2 = l3 * c23;
  const double J3 = l3 * c1 * c23 + l2 * c1 * c2 - l1 * side * s1;
  const double J4 = -l3 * s1 * s23 - l2 * s1 * s2;
  const double J5 = -l3 * s1 * s23;
  const double J6 = l3 * s1 * c23 + l2 * c2 * s1 + l1 * side * c1;
  const double J7 = l3 * c1 * s23 + l2 * c1 * s2;
  const double J8 = l3 * c1 * s23;
  L.C[0] = J4 * J8 - J5 * J7;
  L.C[1] = J5 * J6 - J3 * J8;
  L.C[2] = J3 * J7 - J4 * J6;
  L.C[3] = J2 * J7 - J1 * J8;
  L.C[4] = J0 * J8 - J2 * J6;
  L.C[5] = J1 * J6 - J0 * J7;
  L.C[6] = J1 * J5 - J2 * J4;
  L.C[7] = J2 * J3 - J0 * J5;
  L.C[8] = J0 * J4 - J1 * J3;
  L.det = (J0 * L.C[0] + J1 * L.C[1]) + J2 * L.C[2];
}

// (f_0 + f_1) + (f_2 + f_3) over the quad, in every lane
__device__ __forceinline__ double plant_quad_sum(double x) {
#pragma clang fp contract(off)
  x = x + __shfl_xor(x, 1);
  x = x + __shfl_xor(x, 2);
  return x;
}

// The read-out of lane tt = robot * 4 + leg at pose (p, v, q, w): the foot's hip-frame position and velocity -> joint
// angles and rates; leg 0 also writes the body's state row.  A swing foot (stance == 0) takes r, rdot from pdes / vdes
// (clamped) and moves c to it.  Rows go to the plant's own copy and, when given, to the caller's.
__device__ __forceinline__ void plant_readout(const QmpcPlantDev& S, const QmpcPlantConst& K, int tt, bool live,
                                              const double* p, const double* v, const double* q, const double* w,
                                              double* c, bool stance, const double* vdot, const float* pdes,
                                              const float* vdes, double* state_out, double* motor_out) {
#pragma clang fp contract(off)
  const int b = tt >> 2, leg = tt & 3;
  const double side = (leg & 1) ? 1.0 : -1.0;
  double hip[3], R[9], r[3], rdot[3], vb[3];
  plant_hip(leg, hip);
  plant_rot(q, R);
  plant_mulT(R, v, vb);
  if (stance) {
    const double d[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    double rb[3], wx[3];
    plant_mulT(R, d, rb);
    plant_cross(w, rb, wx);
    for (int k = 0; k < 3; ++k) {
      r[k] = rb[k] - hip[k];
      rdot[k] = -vb[k] - wx[k];
    }
  } else {
    for (int k = 0; k < 3; ++k) {
      r[k] = (double)pdes[k];
      rdot[k] = (double)vdes[k];
    }
    const double rr2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (rr2 == 0.0) {
      r[2] = -sqrt(K.r2_lo);
    } else if (rr2 > K.r2_hi) {
      const double s = sqrt(K.r2_hi / rr2);
      for (int k = 0; k < 3; ++k) r[k] = r[k] * s;
    } else if (rr2 < K.r2_lo) {
      const double s = sqrt(K.r2_lo / rr2);
      for (int k = 0; k < 3; ++k) r[k] = r[k] * s;
    }
    const double hb[3] = {hip[0] + r[0], hip[1] + r[1], hip[2] + r[2]};
    double hw[3];
    plant_mul(R, hb, hw);
    for (int k = 0; k < 3; ++k) c[k] = p[k] + hw[k];
  }
  PlantLeg L;
  plant_leg(K, side, r, L);
  double qd[3] = {0.0, 0.0, 0.0};
  if (fabs(L.det) >= QMPC_PLANT_DET_MIN)
    for (int k = 0; k < 3; ++k) qd[k] = ((L.C[k] * rdot[0] + L.C[3 + k] * rdot[1]) + L.C[6 + k] * rdot[2]) / L.det;
  if (!live) return;
  for (int k = 0; k < 3; ++k) {
    S.foot[(size_t)tt * 3 + k] = c[k];
    S.motor[(size_t)b * 24 + 3 * leg + k] = L.ang[k];
    S.motor[(size_t)b * 24 + 12 + 3 * leg + k] = qd[k];
    if (motor_out) {
      motor_out[(size_t)b * 24 + 3 * leg + k] = L.ang[k];
      motor_out[(size_t)b * 24 + 12 + 3 * leg + k] = qd[k];
    }
  }
  if (leg != 0) return;
  const double sf[3] = {vdot[0], vdot[1], vdot[2] + QMPC_PLANT_GRAVITY};
  double acc[3];
  plant_mulT(R, sf, acc);
  double row[16];
  for (int k = 0; k < 4; ++k) row[k] = q[k];
  for (int k = 0; k < 3; ++k) {
    row[4 + k] = p[k];
    row[7 + k] = w[k];
    row[10 + k] = vb[k];
    row[13 + k] = acc[k];
  }
  for (int k = 0; k < 16; ++k) {
    S.state[(size_t)b * 16 + k] = row[k];
    if (state_out) state_out[(size_t)b * 16 + k] = row[k];
  }
  for (int k = 0; k < 3; ++k) {
    S.p[(size_t)b * 3 + k] = p[k];
    S.v[(size_t)b * 3 + k] = v[k];
    S.omega[(size_t)b * 3 + k] = w[k];
  }
  for (int k = 0; k < 4; ++k) S.q[(size_t)b * 4 + k] = q[k];
}

// qmpc_plant_init / qmpc_plant_reset (mask == NULL: every robot).  n = batch * 4 lanes.
__global__ __launch_bounds__(256) void qmpc_plant_init_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ xyyaw, const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int b = t >> 2, leg = t & 3;
  if (mask && !mask[b]) return;
  const double x0 = xyyaw ? xyyaw[(size_t)b * 3] : 0.0, y0 = xyyaw ? xyyaw[(size_t)b * 3 + 1] : 0.0;
  const double yaw = xyyaw ? xyyaw[(size_t)b * 3 + 2] : 0.0;
  const double p[3] = {x0, y0, QMPC_PLANT_HEIGHT}, v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
  const double side = (leg & 1) ? 1.0 : -1.0;
  double hip[3], R[9], fw[3];
  plant_hip(leg, hip);
  plant_rot(q, R);
  const double fb[3] = {hip[0], hip[1] + side * QMPC_PLANT_SIDE_OFFSET, -QMPC_PLANT_HEIGHT};
  plant_mul(R, fb, fw);
  double c[3] = {p[0] + fw[0], p[1] + fw[1], 0.0};
  for (int k = 0; k < 3; ++k) S.grf[(size_t)t * 3 + k] = 0.0;
  S.stance[t] = 1;
  plant_readout(S, K, t, true, p, v, q, w, c, true, v /* vdot = 0 */, nullptr, nullptr, nullptr, nullptr);
}

// One control period.  n = batch * 4 lanes; the lanes past n in the last wave repeat lane n - 1 and store nothing, so
// that every shuffle has its partner.
// VARY (include/qmpc_plant_vary.h): the robot's own mass, inertia and friction where the caller bound an array (every
// lane of the quad loads its robot's values once, before the substeps: the same address in four lanes), and an external
// force / moment added to the quad sums.  STATS: the lane that writes the state row folds the new pose into the robot's
// accumulators.  <false, false> reads nothing of V and is the plain step.
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) void qmpc_plant_step_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const double* __restrict__ effort,
                                                              const float* __restrict__ contact_state,
                                                              const float* __restrict__ p_des,
                                                              const float* __restrict__ v_des, double* state_out,
                                                              double* motor_out, const int n, const QmpcPlantVary V) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n;
  const int tt = live ? t : n - 1;
  const int b = tt >> 2, leg = tt & 3;
  const size_t o3 = (size_t)tt * 3;
  const double side = (leg & 1) ? 1.0 : -1.0;
  double p[3], v[3], q[4], w[3], c[3], tau[3], hip[3];
  for (int k = 0; k < 3; ++k) {
    p[k] = S.p[(size_t)b * 3 + k];
    v[k] = S.v[(size_t)b * 3 + k];
    w[k] = S.omega[(size_t)b * 3 + k];
    c[k] = S.foot[o3 + k];
    tau[k] = effort[o3 + k];
  }
  for (int k = 0; k < 4; ++k) q[k] = S.q[(size_t)b * 4 + k];
  plant_hip(leg, hip);
  const bool stance = contact_state[tt] > 0.f;
  if (stance && !S.stance[tt]) c[2] = 0.0;  // touch-down: pinned on the ground plane
  double f[3] = {0.0, 0.0, 0.0}, vdot[3] = {0.0, 0.0, 0.0};
  // the robot's own constants and the external wrench (VARY only; a member that is not bound keeps the handle's value)
  double mass_b = K.mass, mu_b = K.mu, ib_b[3] = {K.ibody[0], K.ibody[1], K.ibody[2]};
  double fext[3] = {0.0, 0.0, 0.0}, text[3] = {0.0, 0.0, 0.0};
  if constexpr (VARY) {
    if (V.mass) mass_b = V.mass[b];
    if (V.mu) mu_b = V.mu[b];
    for (int k = 0; k < 3; ++k) {
      if (V.ibody) ib_b[k] = V.ibody[(size_t)b * 3 + k];
      if (V.force) fext[k] = V.force[(size_t)b * 3 + k];
      if (V.torque) text[k] = V.torque[(size_t)b * 3 + k];
    }
  }
  // (the plain step reads K where it always did: with the inertia copied into a local array in front of the loop it
  //  took 225 VGPRs and parked 17 scalar registers in scratch -- tests/test_plant_varied_cpu.py holds 221 and none)
  const double mass = VARY ? mass_b : K.mass, mu = VARY ? mu_b : K.mu;
  const double* ib = VARY ? ib_b : K.ibody;
  for (int s = 0; s < K.substeps; ++s) {
    double R[9], rb[3], fb[3], m[3];
    plant_rot(q, R);
    const double d[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    plant_mulT(R, d, rb);
    f[0] = f[1] = f[2] = 0.0;
    if (stance) {
      const double r[3] = {rb[0] - hip[0], rb[1] - hip[1], rb[2] - hip[2]};
      PlantLeg L;
      plant_leg(K, side, r, L);
      if (fabs(L.det) >= QMPC_PLANT_DET_MIN) {
        double Fb[3], Fw[3];
        for (int k = 0; k < 3; ++k)
          Fb[k] = ((L.C[3 * k] * tau[0] + L.C[3 * k + 1] * tau[1]) + L.C[3 * k + 2] * tau[2]) / L.det;
        plant_mul(R, Fb, Fw);
        if (-Fw[2] > 0.0) {
          f[0] = -Fw[0];
          f[1] = -Fw[1];
          f[2] = -Fw[2];
          const double ft = sqrt(f[0] * f[0] + f[1] * f[1]), cap = mu * f[2];
          if (ft > cap) {
            const double sc = cap / ft;
            f[0] = f[0] * sc;
            f[1] = f[1] * sc;
          }
        }
      }
    }
    plant_mulT(R, f, fb);
    plant_cross(rb, fb, m);
    double F[3], N[3];
    for (int k = 0; k < 3; ++k) {
      F[k] = plant_quad_sum(f[k]);
      N[k] = plant_quad_sum(m[k]);
    }
    if constexpr (VARY) {
      if (V.force)
        for (int k = 0; k < 3; ++k) F[k] = F[k] + fext[k];
      if (V.torque)
        for (int k = 0; k < 3; ++k) N[k] = N[k] + text[k];
    }
    vdot[0] = F[0] / mass;
    vdot[1] = F[1] / mass;
    vdot[2] = F[2] / mass - QMPC_PLANT_GRAVITY;
    const double Iw[3] = {ib[0] * w[0], ib[1] * w[1], ib[2] * w[2]};
    double wIw[3];
    plant_cross(w, Iw, wIw);
    for (int k = 0; k < 3; ++k) {
      v[k] = v[k] + K.h * vdot[k];
      w[k] = w[k] + K.h * ((N[k] - wIw[k]) / ib[k]);
    }
    for (int k = 0; k < 3; ++k) p[k] = p[k] + K.h * v[k];
    const double wn = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double a = wn * K.h;
    double d0, ds;  // dq = (d0, ds * w)
    if (a < 1e-12) {
      d0 = 1.0;
      ds = 0.5 * K.h;
    } else {
      d0 = cos(0.5 * a);
      ds = sin(0.5 * a) / wn;
    }
    const double d1 = ds * w[0], d2 = ds * w[1], d3 = ds * w[2];
    const double n0 = ((q[0] * d0 - q[1] * d1) - q[2] * d2) - q[3] * d3;
    const double n1 = ((q[0] * d1 + q[1] * d0) + q[2] * d3) - q[3] * d2;
    const double n2 = ((q[0] * d2 - q[1] * d3) + q[2] * d0) + q[3] * d1;
    const double n3 = ((q[0] * d3 + q[1] * d2) - q[2] * d1) + q[3] * d0;
    const double nn = sqrt(((n0 * n0 + n1 * n1) + n2 * n2) + n3 * n3);
    q[0] = n0 / nn;
    q[1] = n1 / nn;
    q[2] = n2 / nn;
    q[3] = n3 / nn;
  }
  if (live) {
    for (int k = 0; k < 3; ++k) S.grf[o3 + k] = f[k];
    S.stance[tt] = stance ? 1 : 0;
  }
  plant_readout(S, K, tt, live, p, v, q, w, c, stance, vdot, p_des + o3, v_des + o3, state_out, motor_out);
  if constexpr (STATS) {
    if (live && leg == 0) {
      // the state row's own numbers: p_z, the quaternion, rBody v (the read-out's expression again: the same bits)
      double R[9], vb[3];
      plant_rot(q, R);
      plant_mulT(R, v, vb);
      const double roll = atan2(2 * (q[2] * q[3] + q[0] * q[1]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]));
      double sp = 2 * (q[0] * q[2] - q[1] * q[3]);
      if (sp > 1.0) sp = 1.0;
      if (sp < -1.0) sp = -1.0;
      const double pitch = asin(sp);
      double* a = V.acc + b;  // a[k * acc_stride]: QMPC_PLANT_STAT_*
      const size_t M = (size_t)V.acc_stride;
      V.n[b] = V.n[b] + 1;
      a[QMPC_PLANT_STAT_Z_MIN * M] = fmin(a[QMPC_PLANT_STAT_Z_MIN * M], p[2]);
      a[QMPC_PLANT_STAT_Z_MAX * M] = fmax(a[QMPC_PLANT_STAT_Z_MAX * M], p[2]);
      a[QMPC_PLANT_STAT_ROLL_MAX * M] = fmax(a[QMPC_PLANT_STAT_ROLL_MAX * M], fabs(roll));
      a[QMPC_PLANT_STAT_PITCH_MAX * M] = fmax(a[QMPC_PLANT_STAT_PITCH_MAX * M], fabs(pitch));
      a[QMPC_PLANT_STAT_VX_SUM * M] = a[QMPC_PLANT_STAT_VX_SUM * M] + vb[0];
      a[QMPC_PLANT_STAT_VY_SUM * M] = a[QMPC_PLANT_STAT_VY_SUM * M] + vb[1];
    }
  }
}

// qmpc_plant_stats_reset (mask == NULL: every robot): one lane per robot
__global__ __launch_bounds__(256) void qmpc_plant_stats_reset_kernel(const QmpcPlantVary V,
                                                                     const uint8_t* __restrict__ mask, const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (mask && !mask[b]) return;
  double* a = V.acc + b;
  const size_t M = (size_t)V.acc_stride;
  V.n[b] = 0;
  a[QMPC_PLANT_STAT_Z_MIN * M] = __builtin_inf();
  a[QMPC_PLANT_STAT_Z_MAX * M] = -__builtin_inf();
  a[QMPC_PLANT_STAT_ROLL_MAX * M] = 0.0;
  a[QMPC_PLANT_STAT_PITCH_MAX * M] = 0.0;
  a[QMPC_PLANT_STAT_VX_SUM * M] = 0.0;
  a[QMPC_PLANT_STAT_VY_SUM * M] = 0.0;
}

}  // namespace

extern "C" hipError_t qmpc_launch_plant_init(const QmpcPlantDev* S, const QmpcPlantConst* K, const uint8_t* mask,
                                             const double* xyyaw, int batch, hipStream_t stream) {
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_plant_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *S, *K, mask, xyyaw, n);
  return hipGetLastError();
}

// V == NULL: the plain step.  Otherwise vary (per-robot parameters bound) and stats (statistics on) pick the instantiation.
extern "C" hipError_t qmpc_launch_plant_step(const QmpcPlantDev* S, const QmpcPlantConst* K, const double* effort,
                                             const float* contact_state, const float* p_des, const float* v_des,
                                             double* state_out, double* motor_out, int batch, hipStream_t stream,
                                             const QmpcPlantVary* V, int vary, int stats) {
  const int n = batch * 4;
  const dim3 grid((n + 255) / 256), block(256);
  const QmpcPlantVary none{};
  vary = V && vary;
  stats = V && stats;
#define QMPC_PLANT_STEP(VARY, STATS, v)                                                                            \
  hipLaunchKernelGGL((qmpc_plant_step_kernel<VARY, STATS>), grid, block, 0, stream, *S, *K, effort, contact_state, \
                     p_des, v_des, state_out, motor_out, n, v)
  if (vary && stats)
    QMPC_PLANT_STEP(true, true, *V);
  else if (vary)
    QMPC_PLANT_STEP(true, false, *V);
  else if (stats)
    QMPC_PLANT_STEP(false, true, *V);
  else
    QMPC_PLANT_STEP(false, false, none);
#undef QMPC_PLANT_STEP
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_plant_stats_reset(const QmpcPlantVary* V, const uint8_t* mask, int batch,
                                                    hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_plant_stats_reset_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *V, mask, batch);
  return hipGetLastError();
}
