// qmpc_plant_step_body.h -- the statements of one control period of the plant, as TEXT: included inside the body of a
// step kernel (qmpc_plant.hip: TERRAIN false; qmpc_terrain.hip: TERRAIN true) after qmpc_plant_dev.h, with in scope
//   #pragma clang fp contract(off) at the head of the kernel's body (the pragma is only allowed there);
//   the template parameters bool VARY, bool STATS, and constexpr bool TERRAIN, FIELD (qmpc_field.hip: both true);
//   the names S, K, effort, contact_state, p_des, v_des, state_out, motor_out, n, V of qmpc_plant.h's QmpcPlantStepArgs:
//   the launchers spread the block's members, so in the step kernels these are separate kernel parameters (in
//   qmpc_span.hip the span kernel's own parameters and locals, contact_state / p_des / v_des the controller's arrays);
//   T (QmpcTerrainArgs: a parameter of the terrain kernels, an empty local of the flat ones) and
//   Fd (QmpcFieldArgs: a parameter of the field kernels, an empty local of the others).
// It is text and not a function on purpose.  As a force-inlined function template plant_step_body<VARY, STATS, TERRAIN>
// the same statements cost the plain step 225 VGPRs and 17 scalar registers parked in scratch (arguments by value or by
// reference, with or without __restrict__), against 221 and none when the kernel holds them itself -- the figures
// tests/test_plant_varied_cpu.py keeps.  Piece by piece it is no different: the per-robot constants, J^-T tau, the cone
// about the normal, the quad sums with the wrench, the body update, the quaternion step and the statistics fold are the
// same statements here and in qmpc_contact_step_body.h, and each of them was tried as a function of qmpc_plant_dev.h.
// Most cost registers, spills or scratch; the three that did not moved the --vary and --contact plant step by 0.02 to
// 0.08 us on an MI355X, past the parent's own repeats (profiles/plant_kernel_resources.txt lists the forms and the
// figures, profiles/plant_substep_shared_ab.json the runs).  So they stay text in both bodies: a change to one of them
// is made in both.  No include guard: it is included once per kernel.
//
// One control period of lane t = blockIdx.x * 256 + threadIdx.x.  n = batch * 4 lanes; the lanes past n in the last wave
// repeat lane n - 1 and store nothing, so that every shuffle has its partner.
// VARY (include/qmpc_plant_vary.h): the robot's own mass, inertia and friction where the caller bound an array (every
// lane of the quad loads its robot's values once, before the substeps: the same address in four lanes), and an external
// force / moment added to the quad sums.  STATS: the lane that writes the state row folds the new pose into the robot's
// accumulators.  TERRAIN (include/qmpc_terrain.h): the robot's terrain row is loaded once in front of the substeps (the
// same address in four lanes), touch-down lands on height(c_x, c_y), the cone is taken about the contact normal, and the
// stance feet's mean height and the ground under the body are kept.  FIELD (include/qmpc_field.h, with TERRAIN): the
// robot's place row is loaded once beside the terrain row (T.rows may be null: the field alone), every height is the
// summed surface, and the contact normal is this lane's own foot's, from the taps of its touch-down.  VARY = STATS =
// TERRAIN = false reads nothing of V or T and is the plain step; FIELD = false reads nothing of Fd.
// QMPC_PLANT_STEP_LANE: the lane's index where the including file's workgroups are not 256 lanes (qmpc_span.hip).
#ifndef QMPC_PLANT_STEP_LANE
#define QMPC_PLANT_STEP_LANE (blockIdx.x * 256 + threadIdx.x)
#endif
  const int t = QMPC_PLANT_STEP_LANE;
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
  PlantGround G;
  PlantField Fl;
  if constexpr (TERRAIN) {
    if constexpr (FIELD) {
      if (T.rows)
        plant_ground_load(T.rows + (size_t)b * 8, T.flags, G);
      else
        plant_ground_flat(G);
      G.flags = T.flags;
      plant_field_load(Fd, b, Fl);
      // the surface and the contact normal under this lane's foot, from one set of taps
      const double hz = plant_field_foot(G, Fl, c[0], c[1]);
      if (stance && !S.stance[tt]) c[2] = hz;  // touch-down: pinned on the surface
    } else {
      plant_ground_load(T.rows + (size_t)b * 8, T.flags, G);
      if (stance && !S.stance[tt]) c[2] = plant_height(G, c[0], c[1]);  // touch-down: pinned on the surface
    }
    // the stance feet's mean height (the previous value through a flight phase)
    const double cnt = plant_quad_sum(stance ? 1.0 : 0.0);
    const double sum = plant_quad_sum(stance ? c[2] : 0.0);
    G.support = cnt > 0.0 ? sum / cnt : T.support[b];
  } else {
    if (stance && !S.stance[tt]) c[2] = 0.0;  // touch-down: pinned on the ground plane
  }
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
        if constexpr (TERRAIN) {
          // the cone about the contact normal: f = fn n + t, |t| <= mu fn; an unsaturated force is left untouched
          const double g[3] = {-Fw[0], -Fw[1], -Fw[2]};
          const double fn = (g[0] * G.n[0] + g[1] * G.n[1]) + g[2] * G.n[2];
          if (fn > 0.0) {
            const double tg[3] = {g[0] - fn * G.n[0], g[1] - fn * G.n[1], g[2] - fn * G.n[2]};
            const double ft = sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]), cap = mu * fn;
            f[0] = g[0];
            f[1] = g[1];
            f[2] = g[2];
            if (ft > cap) {
              const double sc = cap / ft;
              for (int k = 0; k < 3; ++k) f[k] = fn * G.n[k] + tg[k] * sc;
            }
          }
        } else {
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
  plant_readout<TERRAIN, FIELD>(S, K, tt, live, p, v, q, w, c, stance, vdot, p_des + o3, v_des + o3, state_out, motor_out,
                                G, Fl);
  if constexpr (TERRAIN) {
    if (live && leg == 0) {
      T.support[b] = G.support;
      T.ground[b] = plant_surface<FIELD>(G, Fl, p[0], p[1]);
    }
  }
  if constexpr (STATS) {
    if (live && leg == 0) {
      // the state row's own numbers: column 6, the quaternion, rBody v (the read-out's expression again: the same bits)
      double R[9], vb[3];
      plant_rot(q, R);
      plant_mulT(R, v, vb);
      const double roll = atan2(2 * (q[2] * q[3] + q[0] * q[1]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]));
      double sp = 2 * (q[0] * q[2] - q[1] * q[3]);
      if (sp > 1.0) sp = 1.0;
      if (sp < -1.0) sp = -1.0;
      const double pitch = asin(sp);
      double zc = p[2];
      if constexpr (TERRAIN) {
        if (G.flags & 2 /* QMPC_TERRAIN_REBASE_Z */) zc = p[2] - G.support;
      }
      double* a = V.acc + b;  // a[k * acc_stride]: QMPC_PLANT_STAT_*
      const size_t M = (size_t)V.acc_stride;
      V.n[b] = V.n[b] + 1;
      a[QMPC_PLANT_STAT_Z_MIN * M] = fmin(a[QMPC_PLANT_STAT_Z_MIN * M], zc);
      a[QMPC_PLANT_STAT_Z_MAX * M] = fmax(a[QMPC_PLANT_STAT_Z_MAX * M], zc);
      a[QMPC_PLANT_STAT_ROLL_MAX * M] = fmax(a[QMPC_PLANT_STAT_ROLL_MAX * M], fabs(roll));
      a[QMPC_PLANT_STAT_PITCH_MAX * M] = fmax(a[QMPC_PLANT_STAT_PITCH_MAX * M], fabs(pitch));
      a[QMPC_PLANT_STAT_VX_SUM * M] = a[QMPC_PLANT_STAT_VX_SUM * M] + vb[0];
      a[QMPC_PLANT_STAT_VY_SUM * M] = a[QMPC_PLANT_STAT_VY_SUM * M] + vb[1];
    }
  }
