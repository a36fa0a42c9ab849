// qmpc_contact_step_body.h -- the statements of one control period with contact decided by the ground, as TEXT: included
// inside the body of a contact step kernel (qmpc_contact.hip: FIELD false; qmpc_field.hip: FIELD true) after
// qmpc_plant_dev.h, for the reason qmpc_plant_step_body.h gives, with in scope
//   #pragma clang fp contract(off) at the head of the kernel's body;
//   the template parameters bool VARY, bool STATS, and constexpr bool FIELD;
//   the kernel's one parameter A and its type StepArgs (qmpc_plant.h's QmpcPlantStepArgs in both files), and
//   Fd (QmpcFieldArgs: A's member in the field kernels, an empty local of the others).
// The numbered comments are the steps of include/qmpc_contact.h.  FIELD (include/qmpc_field.h): the robot's place row is
// loaded once beside the terrain row, every height is the summed surface, and G.n is this lane's own foot's normal,
// evaluated after the edges and again after each slide move from the taps of the height it needs there anyway.
// FIELD = false reads nothing of Fd.  The per-robot constants, J^-T tau, the cone about the normal, the quad sums with the
// wrench, the body update, the quaternion step and the statistics fold are qmpc_plant_step_body.h's statements again, as
// text, for the reasons its header gives: a change to one of them is made in both.  No include guard: it is included once
// per kernel.
  const QmpcPlantConst& K = A.K;
  const QmpcContactArgs& C = A.C;
  const int n = A.n;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n;
  const int tt = live ? t : n - 1;
  const int b = tt >> 2, leg = tt & 3;
  const size_t o3 = (size_t)tt * 3;
  const double side = (leg & 1) ? 1.0 : -1.0;
  const bool f_early = (C.flags & 1) != 0, f_late = (C.flags & 2) != 0, f_slip = (C.flags & 4) != 0;
  double p[3], v[3], q[4], w[3], c[3], tau[3], hip[3];
  for (int k = 0; k < 3; ++k) {
    p[k] = A.S.p[(size_t)b * 3 + k];
    v[k] = A.S.v[(size_t)b * 3 + k];
    w[k] = A.S.omega[(size_t)b * 3 + k];
    c[k] = A.S.foot[o3 + k];
    tau[k] = A.effort[o3 + k];
  }
  for (int k = 0; k < 4; ++k) q[k] = A.S.q[(size_t)b * 4 + k];
  plant_hip(leg, hip);
  const bool sched = A.contact_state[tt] > 0.f;
  bool pin = A.S.stance[tt] != 0;
  double drop = C.drop[tt], slip = C.slip[b];
  PlantGround G;
  PlantField Fl;
  if (A.T.rows)
    plant_ground_load(A.T.rows + (size_t)b * 8, A.T.flags, G);
  else
    plant_ground_flat(G);
  if constexpr (FIELD) {
    G.flags = A.T.flags;  // (the OR of both bindings' flags)
    plant_field_load(Fd, b, Fl);
  }
  // 1. edges
  if constexpr (FIELD) {
    // the surface and the contact normal under this lane's foot, from one set of taps (c_x, c_y do not move here)
    const double hz = plant_field_foot(G, Fl, c[0], c[1]);
    if (sched && !pin) {
      if (!f_late || c[2] <= hz) {
        c[2] = hz;  // touch-down: pinned on the surface
        pin = true;
      }
    } else if (!sched && pin && !f_early) {
      pin = false;
    }
  } else {
    if (sched && !pin) {
      const double hz = plant_height(G, c[0], c[1]);
      if (!f_late || c[2] <= hz) {
        c[2] = hz;  // touch-down: pinned on the surface
        pin = true;
      }
    } else if (!sched && pin && !f_early) {
      pin = false;
    }
  }
  {
    const double cnt = plant_quad_sum(pin ? 1.0 : 0.0);
    const double sum = plant_quad_sum(pin ? c[2] : 0.0);
    G.support = cnt > 0.0 ? sum / cnt : A.T.support[b];
  }
  double f[3] = {0.0, 0.0, 0.0}, vdot[3] = {0.0, 0.0, 0.0}, cd[3] = {0.0, 0.0, 0.0};
  // (the robot's own constants as in qmpc_plant_step_body.h: without VARY the launch's K is read where it is used)
  double mass_b = K.mass, mu_b = K.mu, ib_b[3] = {K.ibody[0], K.ibody[1], K.ibody[2]};
  double fext[3] = {0.0, 0.0, 0.0}, text[3] = {0.0, 0.0, 0.0};
  if constexpr (VARY) {
    if (A.V.mass) mass_b = A.V.mass[b];
    if (A.V.mu) mu_b = A.V.mu[b];
    for (int k = 0; k < 3; ++k) {
      if (A.V.ibody) ib_b[k] = A.V.ibody[(size_t)b * 3 + k];
      if (A.V.force) fext[k] = A.V.force[(size_t)b * 3 + k];
      if (A.V.torque) text[k] = A.V.torque[(size_t)b * 3 + k];
    }
  }
  const double mass = VARY ? mass_b : K.mass, mu = VARY ? mu_b : K.mu;
  const double* ib = VARY ? ib_b : K.ibody;
  // 2. substeps
  for (int s = 0; s < K.substeps; ++s) {
    double R[9], rb[3], fb[3], m[3];
    plant_rot(q, R);
    const double d[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    plant_mulT(R, d, rb);
    f[0] = f[1] = f[2] = 0.0;
    cd[0] = cd[1] = cd[2] = 0.0;
    bool slid = false;
    double sv = 0.0;
    if (pin) {
      const double r[3] = {rb[0] - hip[0], rb[1] - hip[1], rb[2] - hip[2]};
      PlantLeg L;
      plant_leg(K, side, r, L);
      if (fabs(L.det) >= QMPC_PLANT_DET_MIN) {
        double Fb[3], Fw[3];
        for (int k = 0; k < 3; ++k)
          Fb[k] = ((L.C[3 * k] * tau[0] + L.C[3 * k + 1] * tau[1]) + L.C[3 * k + 2] * tau[2]) / L.det;
        plant_mul(R, Fb, Fw);
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
            if (f_slip) {
              // the foot slides against the friction it receives
              slid = true;
              sv = C.slip_gain * (ft - cap);
              if (sv > C.slip_vmax) sv = C.slip_vmax;
              for (int k = 0; k < 3; ++k) cd[k] = -(sv * (tg[k] / ft));
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
      if (A.V.force)
        for (int k = 0; k < 3; ++k) F[k] = F[k] + fext[k];
      if (A.V.torque)
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
    if (f_slip) {
      if (slid) {
        c[0] = c[0] + K.h * cd[0];
        c[1] = c[1] + K.h * cd[1];
        if constexpr (FIELD)
          c[2] = plant_field_foot(G, Fl, c[0], c[1]);  // ... and the normal at the new place
        else
          c[2] = plant_height(G, c[0], c[1]);
      }
      slip = slip + plant_quad_sum(slid ? K.h * sv : 0.0);
    }
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
  // 3. unpinned feet and release, at the new pose
  double R[9], r[3], rdot[3], vb[3];
  plant_rot(q, R);
  plant_mulT(R, v, vb);
  const bool late = sched && !pin;
  bool lifted = false;  // qmpc_terrain.h's swing clamp acted: r follows the foot
  if (!(sched && pin)) {
    for (int k = 0; k < 3; ++k) r[k] = (double)A.p_des[o3 + k];
    if (late) {
      drop = drop + C.drop_speed * C.dt;
      for (int k = 0; k < 3; ++k) r[k] = r[k] - drop * R[6 + k];  // rBody e_z
    }
    const double rr2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (rr2 == 0.0) {
      r[2] = -sqrt(K.r2_lo);
    } else if (rr2 > K.r2_hi) {
      const double sc = sqrt(K.r2_hi / rr2);
      for (int k = 0; k < 3; ++k) r[k] = r[k] * sc;
    } else if (rr2 < K.r2_lo) {
      const double sc = sqrt(K.r2_lo / rr2);
      for (int k = 0; k < 3; ++k) r[k] = r[k] * sc;
    }
    const double hb[3] = {hip[0] + r[0], hip[1] + r[1], hip[2] + r[2]};
    double hw[3];
    plant_mul(R, hb, hw);
    const double cs[3] = {p[0] + hw[0], p[1] + hw[1], p[2] + hw[2]};
    const double hz = plant_surface<FIELD>(G, Fl, cs[0], cs[1]);
    if ((sched || f_early) && cs[2] <= hz) {
      if (!pin) {  // it lands here; a pinned swing foot stays where it is
        c[0] = cs[0];
        c[1] = cs[1];
        c[2] = hz;
        pin = true;
      }
    } else {
      c[0] = cs[0];
      c[1] = cs[1];
      c[2] = cs[2];
      pin = false;
      if ((G.flags & 1 /* QMPC_TERRAIN_CLAMP_SWING */) && c[2] < hz) {
        c[2] = hz;
        lifted = true;
      }
    }
  }
  const int n_early = contact_quad_count(!sched && pin ? 1 : 0);
  const int n_late = contact_quad_count(late ? 1 : 0);
  if (pin || !sched) drop = 0.0;
  // 4. read-out
  if (pin || lifted) {
    const double d[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    double rb[3];
    plant_mulT(R, d, rb);
    for (int k = 0; k < 3; ++k) r[k] = rb[k] - hip[k];
    if (pin) {
      double wx[3], rcd[3];
      plant_cross(w, rb, wx);
      plant_mulT(R, cd, rcd);
      for (int k = 0; k < 3; ++k) rdot[k] = (-vb[k] - wx[k]) + rcd[k];
    }
  }
  if (!pin)
    for (int k = 0; k < 3; ++k) rdot[k] = (double)A.v_des[o3 + k];
  PlantLeg L;
  plant_leg(K, side, r, L);
  double qd[3] = {0.0, 0.0, 0.0};
  if (fabs(L.det) >= QMPC_PLANT_DET_MIN)
    for (int k = 0; k < 3; ++k) qd[k] = ((L.C[k] * rdot[0] + L.C[3 + k] * rdot[1]) + L.C[6 + k] * rdot[2]) / L.det;
  if (!live) return;
  // the stores: their pointers, from the kernarg segment again
  typedef const __attribute__((address_space(4))) StepArgs* KernargPtr;
  KernargPtr again = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(again));
  QmpcPlantDev S;
#define QMPC_CONTACT_AGAIN(T, name, per_robot) S.name = again->S.name;
  QMPC_PLANT_ARRAYS(QMPC_CONTACT_AGAIN)
#undef QMPC_CONTACT_AGAIN
  struct {
    double *acc, *support, *ground, *drop, *slip;
    int32_t *early, *late;
    int* n;
    int acc_stride;
  } Z = {again->V.acc, again->T.support, again->T.ground, again->C.drop, again->C.slip,
         again->C.early, again->C.late, again->V.n, again->V.acc_stride};
  double *const state_out = again->state_out, *const motor_out = again->motor_out;
  for (int k = 0; k < 3; ++k) {
    S.grf[o3 + k] = f[k];
    S.foot[o3 + k] = c[k];
    S.motor[(size_t)b * 24 + 3 * leg + k] = L.ang[k];
    S.motor[(size_t)b * 24 + 12 + 3 * leg + k] = qd[k];
    if (motor_out) {
      motor_out[(size_t)b * 24 + 3 * leg + k] = L.ang[k];
      motor_out[(size_t)b * 24 + 12 + 3 * leg + k] = qd[k];
    }
  }
  S.stance[tt] = pin ? 1 : 0;
  Z.drop[tt] = drop;
  if (leg != 0) return;
  Z.early[b] = Z.early[b] + n_early;
  Z.late[b] = Z.late[b] + n_late;
  Z.slip[b] = slip;
  Z.support[b] = G.support;
  Z.ground[b] = plant_surface<FIELD>(G, Fl, p[0], p[1]);
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
  if (G.flags & 2 /* QMPC_TERRAIN_REBASE_Z */) row[6] = p[2] - G.support;
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
  if constexpr (STATS) {
    // the state row's own numbers (qmpc_plant_step_body.h)
    const double roll = atan2(2 * (q[2] * q[3] + q[0] * q[1]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]));
    double sp = 2 * (q[0] * q[2] - q[1] * q[3]);
    if (sp > 1.0) sp = 1.0;
    if (sp < -1.0) sp = -1.0;
    const double pitch = asin(sp);
    const double zc = row[6];
    double* a = Z.acc + b;  // a[k * acc_stride]: QMPC_PLANT_STAT_*
    const size_t M = (size_t)Z.acc_stride;
    Z.n[b] = Z.n[b] + 1;
    a[QMPC_PLANT_STAT_Z_MIN * M] = fmin(a[QMPC_PLANT_STAT_Z_MIN * M], zc);
    a[QMPC_PLANT_STAT_Z_MAX * M] = fmax(a[QMPC_PLANT_STAT_Z_MAX * M], zc);
    a[QMPC_PLANT_STAT_ROLL_MAX * M] = fmax(a[QMPC_PLANT_STAT_ROLL_MAX * M], fabs(roll));
    a[QMPC_PLANT_STAT_PITCH_MAX * M] = fmax(a[QMPC_PLANT_STAT_PITCH_MAX * M], fabs(pitch));
    a[QMPC_PLANT_STAT_VX_SUM * M] = a[QMPC_PLANT_STAT_VX_SUM * M] + vb[0];
    a[QMPC_PLANT_STAT_VY_SUM * M] = a[QMPC_PLANT_STAT_VY_SUM * M] + vb[1];
  }
