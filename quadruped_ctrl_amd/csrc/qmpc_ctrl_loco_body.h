// qmpc_ctrl_loco_body.h -- stage L of a tick for one robot, as TEXT: the safety checks and ConvexMPCLocomotion::run up to
// updateMPCIfNeeded.  Included inside the body of qmpc_ctrl_loco_kernel<MODE> (qmpc_glue.hip) and of the span kernel
// (qmpc_span.hip) after qmpc_ctrl_stages.h, with in scope
//   #pragma clang fp contract(off) at the head of the kernel's body (the pragma is only allowed there);
//   the template parameter int MODE, S (the QmpcCtrlDev) and b (the robot).
// It leaves `const bool due` behind: the robot's incremented counter is a multiple of 13, this tick solves for it.
// It is text and not a function for the reason at the head of qmpc_plant_step_body.h: as a force-inlined function the
// same statements cost qmpc_ctrl_loco_kernel<0> 92 VGPRs against 84 when the kernel holds them itself (by reference or
// by value, with or without the due-list append inside) -- the figure tests/test_fleet_run_cpu.py keeps.  No include
// guard: it is included once per kernel.  No statement in it returns.
// MODE: the controller's robot mode (qmpc_ctrl_set_robot_mode).  0: the gait picked by number, 14 segments (:150-172).
// 1: the `aio` gait (:173-233), whose segment count, offsets and durations are the robot's own rows and change on
// phase-0 ticks only; everything below the gait selection reads them where mode 0 has the literal 14.
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
