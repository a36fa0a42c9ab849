// qmpc_act_model.h -- the per-joint arithmetic and the ring indexing of include/qmpc_act.h in plain C++, __host__ and
// __device__: the kernel of qmpc_act.hip computes through it, and a CPU program (tests/act_dump.cpp) compiles it under
// the sanitizers.  fp64, contraction off, one operation at a time, nothing transcendental: tests/act_model.py restates
// every statement in the same order and agrees bit for bit.  The motor is the reference's ActuatorModel<T>::getTorque
// (src/Dynamics/ActuatorModel.h:54-71) with its coerce (two compares: a NaN passes through) and its sgn.
#ifndef QMPC_ACT_MODEL_H
#define QMPC_ACT_MODEL_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QMPC_ACT_HD __host__ __device__ __forceinline__
#else
#define QMPC_ACT_HD inline
#endif

// the motor of one robot: the config's scalars with the robot's bound values in their places
struct QmpcActMotor {
  double kt, R;
  double V, tmax, damp, dry;  // battery voltage, motor-side torque cap, joint damping, dry friction
  double strength;            // read only when has_strength
  int has_strength, friction;
};

// what one joint contributes to a control period
struct QmpcActJoint {
  double tau;    // the torque at the joint
  double heat;   // 1.5 i^2 R, i = tc / (1.5 kt)
  double power;  // tau qd
  int vsat;      // vact != vdes
  int tsat;      // tc != tam
};

// the reference's coerce(in, min, max)
QMPC_ACT_HD double qmpc_act_coerce(double in, double lo, double hi) {
  if (in < lo) in = lo;
  if (in > hi) in = hi;
  return in;
}

// the reference's sgn: (0 < x) - (x < 0), so sgn(+-0) = 0 and sgn(NaN) = 0
QMPC_ACT_HD double qmpc_act_sgn(double x) { return (double)((0.0 < x) - (x < 0.0)); }

// getTorque for gear ratio g, the command tau_cmd at the joint and the joint rate qd
QMPC_ACT_HD QmpcActJoint qmpc_act_joint(const QmpcActMotor& M, double g, double tau_cmd, double qd) {
#pragma clang fp contract(off)
  QmpcActJoint J;
  const double tm = tau_cmd / g;
  const double k15 = M.kt * 1.5;
  const double ides = tm / k15;
  const double bemf = ((qd * g) * M.kt) * 2.0;
  const double vdes = ides * M.R + bemf;
  const double vact = qmpc_act_coerce(vdes, -M.V, M.V);
  const double tam = (k15 * (vact - bemf)) / M.R;
  const double tc = qmpc_act_coerce(tam, -M.tmax, M.tmax);
  double tau = g * tc;
  if (M.has_strength) tau = M.strength * tau;
  if (M.friction) tau = (tau - M.damp * qd) - M.dry * qmpc_act_sgn(qd);
  const double i = tc / k15;
  J.tau = tau;
  J.heat = ((1.5 * i) * i) * M.R;
  J.power = tau * qd;
  J.vsat = vact != vdes;
  J.tsat = tc != tam;
  return J;
}

// A control period's subtotals over a robot's joints, taken in joint order k = 0 .. 11 (the order is part of the
// contract): |tau| enters the peak only when it is larger, so a NaN never does; a power that is NaN counts 0 in pos.
struct QmpcActSums {
  double peak;  // starts at the robot's tau_peak
  double heat, mech, pos;  // start at 0.0
};
QMPC_ACT_HD void qmpc_act_sums_add(QmpcActSums& S, double tau, double heat, double power) {
#pragma clang fp contract(off)
  const double a = tau < 0.0 ? -tau : tau;
  S.peak = a > S.peak ? a : S.peak;
  S.heat = S.heat + heat;
  S.mech = S.mech + power;
  S.pos = S.pos + (power > 0.0 ? power : 0.0);
}
// The same subtotals where a lane holds THREE joints of its robot (the loop kernel of qmpc_loop.hip: lane = leg, four lanes
// a robot): every lane of the quad takes the twelve terms in joint order, term k from lane k / 3, component k % 3.
// shfl(own value, source lane, slot) returns the source lane's value of that slot (3 * component + 0 / 1 / 2 for tau,
// heat, power): a width-4 shuffle in the kernel, a table lookup in the CPU program (tests/loop_dump.cpp), which compares
// the result with the sixteen-lane order above bit for bit.
template <class Shfl>
QMPC_ACT_HD void qmpc_act_sums_quad(QmpcActSums& S, const QmpcActJoint* J, Shfl shfl) {
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 0; k < 12; ++k) {
    const int c = k % 3, src = k / 3;
    qmpc_act_sums_add(S, shfl(J[c].tau, src, 3 * c), shfl(J[c].heat, src, 3 * c + 1), shfl(J[c].power, src, 3 * c + 2));
  }
}
// an energy after the period: e + dt * subtotal
QMPC_ACT_HD double qmpc_act_energy(double e, double dt, double subtotal) {
#pragma clang fp contract(off)
  const double d = dt * subtotal;
  return e + d;
}

// The ring of max_delay + 1 rows.  head: the row this period's command is stored in (the call count modulo the ring's
// length); age: periods since init or the robot's last reset, saturated at max_delay.  The row that is applied lies
// min(clamp(delay, 0, max_delay), age) rows back: 0 <= row <= max_delay for any delay, 0 <= head, age <= max_delay.
QMPC_ACT_HD int qmpc_act_row(int head, int age, int delay, int max_delay) {
  int d = delay < 0 ? 0 : delay;
  if (d > max_delay) d = max_delay;
  if (age < d) d = age;
  const int r = head - d;
  return r < 0 ? r + max_delay + 1 : r;
}
QMPC_ACT_HD int qmpc_act_next_head(int head, int max_delay) { return head >= max_delay ? 0 : head + 1; }
QMPC_ACT_HD int qmpc_act_next_age(int age, int max_delay) { return age < max_delay ? age + 1 : max_delay; }

#endif
