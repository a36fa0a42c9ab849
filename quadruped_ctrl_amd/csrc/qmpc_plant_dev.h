// qmpc_plant_dev.h -- device code of the reduced-order plant shared by qmpc_plant.hip (include/qmpc_plant.h: flat
// ground), qmpc_terrain.hip (include/qmpc_terrain.h: per-robot slopes and stairs), qmpc_contact.hip (include/qmpc_contact.h)
// and qmpc_field.hip (include/qmpc_field.h: height fields from memory): the leg helpers, the terrain's height, the
// field's sampler and per-foot normal, and the read-out.  (The statements of one control period are qmpc_plant_step_body.h, which a step kernel
// includes as text.)  One lane per (robot, leg) as in the glue kernels.  Every lane of a robot's quad carries a copy of
// the body state; a leg's force and moment are summed over the quad with two xor-shuffles, (f_0 + f_1) + (f_2 + f_3) in
// every lane (the sum is commutative, so the four lanes hold the same bits), and the four lanes integrate the same body
// redundantly -- no broadcast, no LDS, no atomics.  Lane 0 of the quad stores the body; every lane stores its own foot
// and joints.  fp contraction is off, as in the glue code: tests/plant_model.py (and tests/plant_model_terrain.py for
// TERRAIN) restates every expression in the same order.
//
// Everything here is force-inlined and lives in an unnamed namespace: each translation unit gets its own copy and
// defines only its own kernels.  TERRAIN = false reads nothing of the terrain and is the flat plant, bit for bit;
// FIELD = false reads nothing of the field and leaves every kernel of the other three files as it was.
#ifndef QMPC_PLANT_DEV_CODE_H
#define QMPC_PLANT_DEV_CODE_H

#include <type_traits>

#include "qmpc_plant.h"
#include "qmpc_field_index.h"

namespace {

struct PlantLeg {
  double ang[3];  // abad, hip, knee
  double C[9];    // cofactors of J (row-major): J^-1 = C^T / det
  double det;
};

// A robot's terrain row (include/qmpc_terrain.h) in registers, with what is computed once per step: cos / sin of the
// flight's heading and the contact normal; `support` is filled in after the contact edges.
struct PlantGround {
  double z0, gx, gy, rise, run, count, s0, cpsi, spsi;
  double n[3];
  double support;
  int flags;
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
// (i_0 + i_1) + (i_2 + i_3) over the quad, in every lane
__device__ __forceinline__ int contact_quad_count(int x) {
  x = x + __shfl_xor(x, 1);
  x = x + __shfl_xor(x, 2);
  return x;
}

// The terrain row of a robot -> registers.  n_x = -gx / norm: a zero slope gives -0.0, the additive identity that keeps
// the sign of the other operand (the flat plant's bits under an all-zero row).
__device__ __forceinline__ void plant_ground_load(const double* __restrict__ row, int flags, PlantGround& G) {
#pragma clang fp contract(off)
  G.z0 = row[0];
  G.gx = row[1];
  G.gy = row[2];
  G.rise = row[3];
  G.run = row[4];
  G.count = row[5];
  G.s0 = row[6];
  const double psi = row[7];
  G.cpsi = cos(psi);
  G.spsi = sin(psi);
  const double norm = sqrt((G.gx * G.gx + G.gy * G.gy) + 1);
  G.n[0] = -G.gx / norm;
  G.n[1] = -G.gy / norm;
  G.n[2] = 1 / norm;
  G.support = 0.0;
  G.flags = flags;
}

// height(x, y) of include/qmpc_terrain.h
__device__ __forceinline__ double plant_height(const PlantGround& G, double x, double y) {
#pragma clang fp contract(off)
  double k = 0.0;
  if (!(G.count <= 0.0) && G.run > 0.0) {
    k = floor(((x * G.cpsi + y * G.spsi) - G.s0) / G.run) + 1;
    if (k < 0.0) k = 0.0;
    if (k > G.count) k = G.count;
  }
  return ((G.z0 + G.gx * x) + G.gy * y) + G.rise * k;
}

// No terrain bound: an all-zero row under flags 0 (height 0, n = (-0, -0, 1): the additive identities of qmpc_terrain.h)
__device__ __forceinline__ void plant_ground_flat(PlantGround& G) {
  G.z0 = G.gx = G.gy = G.rise = G.run = G.count = G.s0 = 0.0;
  G.cpsi = 1.0;
  G.spsi = 0.0;
  G.n[0] = -0.0;
  G.n[1] = -0.0;
  G.n[2] = 1.0;
  G.support = 0.0;
  G.flags = 0;
}

// A robot's placement on the height-field bank (include/qmpc_field.h) in registers: its map's first sample, the origin,
// the scale and the grid.  Loaded once per step (the same address in the four lanes of a quad).  An empty struct's worth
// of dead registers where FIELD is false.
struct PlantField {
  const float* z;  // the robot's own map: bank + m ny nx
  double ox, oy, zs, cell;
  int nx, ny;
};

__device__ __forceinline__ void plant_field_load(const QmpcFieldArgs& Fd, int b, PlantField& Fl) {
  const double* __restrict__ row = Fd.place + (size_t)b * 4;
  const double map = row[0];
  Fl.ox = row[1];
  Fl.oy = row[2];
  Fl.zs = row[3];
  Fl.z = Fd.z + qmpc_field_base(qmpc_field_map(map, Fd.count), Fd.nx, Fd.ny);
  Fl.cell = Fd.cell;
  Fl.nx = Fd.nx;
  Fl.ny = Fd.ny;
}

// f, fx, fy of include/qmpc_field.h at (x, y), from one set of four taps.  The taps are dependent gathers (their address
// hangs on the foot's position): all four loads are issued before the first use, so they share one wait.
__device__ __forceinline__ void plant_field_sample(const PlantField& Fl, double x, double y, double& f, double& fx,
                                                   double& fy) {
#pragma clang fp contract(off)
  double a, b;
  bool in_x, in_y;
  const int i = qmpc_field_axis((x - Fl.ox) / Fl.cell, Fl.nx, &a, &in_x);
  const int j = qmpc_field_axis((y - Fl.oy) / Fl.cell, Fl.ny, &b, &in_y);
  const float* __restrict__ t = Fl.z + qmpc_field_tap(i, j, Fl.nx);
  const float s00 = t[0], s10 = t[1], s01 = t[Fl.nx], s11 = t[Fl.nx + 1];
  const double z00 = (double)s00, z10 = (double)s10, z01 = (double)s01, z11 = (double)s11;
  const double d0 = z10 - z00, d1 = z11 - z01;
  const double e0 = z00 + a * d0, e1 = z01 + a * d1;
  const double e = e1 - e0;
  f = Fl.zs * (e0 + b * e);
  fx = in_x ? Fl.zs * ((d0 + b * (d1 - d0)) / Fl.cell) : 0.0;
  fy = in_y ? Fl.zs * (e / Fl.cell) : 0.0;
}

// height(x, y) of include/qmpc_field.h from the analytic height h and the field's f: f == 0 (either sign) leaves h's bits
__device__ __forceinline__ double plant_field_add(double h, double f) {
#pragma clang fp contract(off)
  return f == 0.0 ? h : h + f;
}

// The summed surface at (x, y) where only the height is wanted
__device__ __forceinline__ double plant_field_height(const PlantGround& G, const PlantField& Fl, double x, double y) {
  double f, fx, fy;
  plant_field_sample(Fl, x, y, f, fx, fy);
  return plant_field_add(plant_height(G, x, y), f);
}

// The summed surface at a foot's (x, y) and the contact normal there, into G.n: this lane's own foot, so G.n is per foot
// from here on.  fx == fy == 0 gives plant_ground_load's bits.
__device__ __forceinline__ double plant_field_foot(PlantGround& G, const PlantField& Fl, double x, double y) {
#pragma clang fp contract(off)
  double f, fx, fy;
  plant_field_sample(Fl, x, y, f, fx, fy);
  const double gx = fx == 0.0 ? G.gx : G.gx + fx, gy = fy == 0.0 ? G.gy : G.gy + fy;
  const double norm = sqrt((gx * gx + gy * gy) + 1);
  G.n[0] = -gx / norm;
  G.n[1] = -gy / norm;
  G.n[2] = 1 / norm;
  return plant_field_add(plant_height(G, x, y), f);
}

// The surface of a kernel: the summed one with FIELD, the analytic one without
template <bool FIELD>
__device__ __forceinline__ double plant_surface(const PlantGround& G, const PlantField& Fl, double x, double y) {
  if constexpr (FIELD)
    return plant_field_height(G, Fl, x, y);
  else
    return plant_height(G, x, y);
}

// The read-out of lane tt = robot * 4 + leg at pose (p, v, q, w): the foot's hip-frame position and velocity -> joint
// angles and rates; leg 0 also writes the body's state row.  A swing foot (stance == 0) takes r, rdot from pdes / vdes
// (clamped) and moves c to it.  Rows go to the plant's own copy and, when given, to the caller's.
// TERRAIN: with QMPC_TERRAIN_CLAMP_SWING a swing foot placed below the surface is lifted onto it and r follows; with
// QMPC_TERRAIN_REBASE_Z column 6 of the state row is p_z - G.support (the view's p stays world truth).
// FIELD (include/qmpc_field.h): the surface the swing foot is lifted onto is the summed one, through Fl.
template <bool TERRAIN, bool FIELD = false>
__device__ __forceinline__ void plant_readout(const QmpcPlantDev& S, const QmpcPlantConst& K, int tt, bool live,
                                              const double* p, const double* v, const double* q, const double* w,
                                              double* c, bool stance, const double* vdot, const float* pdes,
                                              const float* vdes, double* state_out, double* motor_out,
                                              const PlantGround& G, const PlantField& Fl = PlantField{}) {
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
    if constexpr (TERRAIN) {
      if (G.flags & 1 /* QMPC_TERRAIN_CLAMP_SWING */) {
        const double hz = plant_surface<FIELD>(G, Fl, c[0], c[1]);
        if (c[2] < hz) {
          c[2] = hz;  // the encoders see the shortened leg; rdot stays v_des
          const double d[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
          double rb[3];
          plant_mulT(R, d, rb);
          for (int k = 0; k < 3; ++k) r[k] = rb[k] - hip[k];
        }
      }
    }
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
  if constexpr (TERRAIN) {
    if (G.flags & 2 /* QMPC_TERRAIN_REBASE_Z */) row[6] = p[2] - G.support;
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

// qmpc_plant_init / qmpc_plant_reset of lane t = robot * 4 + leg on flat ground: the robot stands at (x0, y0) with the
// attitude q (a yaw: the caller builds it from its xyyaw row) at QMPC_PLANT_HEIGHT, its feet under the hips, every foot in
// stance, and the read-out goes to the plant's own rows.  One text behind the init kernel of qmpc_plant.hip and the reset
// stage of qmpc_loop.hip; the caller decides which lanes run it.
__device__ __forceinline__ void plant_init_lane(const QmpcPlantDev& S, const QmpcPlantConst& K, const double x0,
                                                const double y0, const double* q, const int t) {
#pragma clang fp contract(off)
  const int leg = t & 3;
  const double p[3] = {x0, y0, QMPC_PLANT_HEIGHT}, v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  const double side = (leg & 1) ? 1.0 : -1.0;
  double hip[3], R[9], fw[3];
  plant_hip(leg, hip);
  plant_rot(q, R);
  const double fb[3] = {hip[0], hip[1] + side * QMPC_PLANT_SIDE_OFFSET, -QMPC_PLANT_HEIGHT};
  plant_mul(R, fb, fw);
  double c[3] = {p[0] + fw[0], p[1] + fw[1], 0.0};
  for (int k = 0; k < 3; ++k) S.grf[(size_t)t * 3 + k] = 0.0;
  S.stance[t] = 1;
  const PlantGround flat{};
  plant_readout<false>(S, K, t, true, p, v, q, w, c, true, v /* vdot = 0 */, nullptr, nullptr, nullptr, nullptr,
                       flat);
}

// qmpc_plant_reset of lane tt = robot * 4 + leg while terrain rows (FIELD false) or a height-field bank (FIELD true;
// T.rows may be null: the field alone) are bound.  The body stands level at (x0, y0, 0.29 + height(x0, y0)) under the
// yaw, every foot at its usual body-frame xy on the surface; support is the mean of the four feet, (c_0 + c_1) +
// (c_2 + c_3) over 4, so EVERY lane of a quad calls this (the shuffles need their partners) and `live` says whether the
// lane stores; the leg-0 lane writes support[b] and ground[b].  q: the yaw as a quaternion, built by the caller from its
// xyyaw row, as for plant_init_lane.  One text behind the init kernels of qmpc_terrain.hip and
// qmpc_field.hip and the reset stage of qmpc_loop.hip on ground.
template <bool FIELD>
__device__ __forceinline__ void plant_ground_init_lane(const QmpcPlantDev& S, const QmpcPlantConst& K,
                                                       const QmpcTerrainArgs& T, const QmpcFieldArgs& Fd, const double x0,
                                                       const double y0, const double* q, const int tt, const bool live) {
#pragma clang fp contract(off)
  const int b = tt >> 2, leg = tt & 3;
  PlantGround G;
  PlantField Fl{};
  if constexpr (FIELD) {
    if (T.rows)
      plant_ground_load(T.rows + (size_t)b * 8, T.flags, G);
    else
      plant_ground_flat(G);
    G.flags = T.flags;
    plant_field_load(Fd, b, Fl);
  } else {
    plant_ground_load(T.rows + (size_t)b * 8, T.flags, G);
  }
  const double ground = plant_surface<FIELD>(G, Fl, x0, y0);
  const double p[3] = {x0, y0, QMPC_PLANT_HEIGHT + ground}, v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  const double side = (leg & 1) ? 1.0 : -1.0;
  double hip[3], R[9], fw[3];
  plant_hip(leg, hip);
  plant_rot(q, R);
  const double fb[3] = {hip[0], hip[1] + side * QMPC_PLANT_SIDE_OFFSET, -QMPC_PLANT_HEIGHT};
  plant_mul(R, fb, fw);
  double c[3] = {p[0] + fw[0], p[1] + fw[1], 0.0};
  c[2] = plant_surface<FIELD>(G, Fl, c[0], c[1]);
  G.support = plant_quad_sum(c[2]) / 4.0;
  if (live) {
    for (int k = 0; k < 3; ++k) S.grf[(size_t)tt * 3 + k] = 0.0;
    S.stance[tt] = 1;
    if (leg == 0) {
      T.support[b] = G.support;
      T.ground[b] = ground;
    }
  }
  plant_readout<true, FIELD>(S, K, tt, live, p, v, q, w, c, true, v /* vdot = 0 */, nullptr, nullptr, nullptr, nullptr, G,
                             Fl);
}

// qmpc_plant_stats_reset of robot b: the accumulators as qmpc_plant_stats_enable leaves them
__device__ __forceinline__ void plant_stats_reset_robot(const QmpcPlantVary& V, const int b) {
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

// Host side of every launcher here: 256 lanes per block over n = batch * 4 lanes ...
inline dim3 plant_grid(int n) { return dim3((n + 255) / 256); }

// ... and the <VARY, STATS> instantiation of a step kernel from the launcher's two flags: launch(VARY, STATS) is called
// with two std::bool_constants, whose ::value a generic lambda can use as a template argument.
template <class Launch>
void plant_vary_stats(bool vary, bool stats, Launch launch) {
  if (vary && stats)
    launch(std::true_type{}, std::true_type{});
  else if (vary)
    launch(std::true_type{}, std::false_type{});
  else if (stats)
    launch(std::false_type{}, std::true_type{});
  else
    launch(std::false_type{}, std::false_type{});
}

}  // namespace

#endif
