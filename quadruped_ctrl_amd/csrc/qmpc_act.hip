// qmpc_act.hip -- the actuator stage of include/qmpc_act.h: one launch per control period, 16 lanes per robot (four
// robots per wave).  Lanes 0..11 take one joint each: a robot's twelve commands, its ring row and its output are
// contiguous, so a wave reads and writes four runs of 96 bytes.  A lane touches only its own column of effort and of
// the ring, and reads it before it writes it: effort_out may be effort_in.  Lanes 12..15 compute on zeros and store
// nothing; they stay so that the sixteen lanes of a robot reach the shuffles together.
// The accumulators' sums are taken by every lane of the robot over the twelve joints' terms, broadcast one after the
// other in joint order (the order is part of the contract); lane 0 stores them.  All sixteen lanes load head and age
// with ONE wave instruction each in front of the first branch, and lane 0's stores come after: program order inside a
// wave is enough.  No LDS allocation, no atomics, no scratch.  fp contraction is off: tests/act_model.py restates every
// expression in the same order and agrees bit for bit.
#include "qmpc_act.h"
#include "qmpc_act_model.h"

namespace {

__global__ __launch_bounds__(256) void qmpc_act_kernel(const QmpcActArgs A, const double* effort_in, double* effort_out,
                                                       const int batch) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int b = t >> 4, lane = t & 15;
  if (b >= batch) return;
  const int D = A.cfg.max_delay;
  int head = A.d.head[b], age = A.d.age[b];
  // (the state is this library's own; a row index is still never taken on trust)
  if ((unsigned)head > (unsigned)D) head = 0;
  if ((unsigned)age > (unsigned)D) age = D;
  const bool joint = lane < 12;
  const size_t at = (size_t)b * 12 + lane, row_stride = (size_t)batch * 12;
  double cmd = 0.0, qd = 0.0;
  if (joint) {
    const double e = effort_in[at];
    A.ring[(size_t)head * row_stride + at] = e;
    const int row = qmpc_act_row(head, age, A.delay ? A.delay[b] : 0, D);
    cmd = row == head ? e : A.ring[(size_t)row * row_stride + at];
    qd = A.motor[(size_t)b * 24 + 12 + lane];
  }
  QmpcActMotor M;
  M.kt = A.cfg.kt;
  M.R = A.cfg.R;
  M.V = A.battery_v ? A.battery_v[b] : A.cfg.battery_v;
  M.tmax = A.tau_max ? A.tau_max[b] : A.cfg.tau_max;
  M.damp = A.damping ? A.damping[b] : A.cfg.damping;
  M.dry = A.dry_friction ? A.dry_friction[b] : A.cfg.dry_friction;
  M.has_strength = A.strength != nullptr;
  M.strength = A.strength ? A.strength[b] : 1.0;
  M.friction = A.cfg.friction;
  const int j = lane % 3;
  const double g = j == 0 ? A.cfg.gear[0] : j == 1 ? A.cfg.gear[1] : A.cfg.gear[2];
  const QmpcActJoint J = qmpc_act_joint(M, g, cmd, qd);
  if (joint) effort_out[at] = J.tau;

  // the robot's sixteen bits of the wave's two ballots
  const int shift = (threadIdx.x & 63) & ~15;
  const int n_vsat = __popcll((__ballot(joint && J.vsat) >> shift) & 0xFFFFull);
  const int n_tsat = __popcll((__ballot(joint && J.tsat) >> shift) & 0xFFFFull);
  QmpcActSums S{lane == 0 ? A.d.tau_peak[b] : 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 12; ++k)
    qmpc_act_sums_add(S, __shfl(J.tau, k, 16), __shfl(J.heat, k, 16), __shfl(J.power, k, 16));
  if (lane != 0) return;
  A.d.head[b] = qmpc_act_next_head(head, D);
  A.d.age[b] = qmpc_act_next_age(age, D);
  A.d.n[b] = A.d.n[b] + 1;
  A.d.n_vsat[b] = A.d.n_vsat[b] + n_vsat;
  A.d.n_tsat[b] = A.d.n_tsat[b] + n_tsat;
  A.d.tau_peak[b] = S.peak;
  A.d.e_heat[b] = qmpc_act_energy(A.d.e_heat[b], A.dt, S.heat);
  A.d.e_mech[b] = qmpc_act_energy(A.d.e_mech[b], A.dt, S.mech);
  A.d.e_pos[b] = qmpc_act_energy(A.d.e_pos[b], A.dt, S.pos);
}

// qmpc_act_init's zeroing is a memset; this is qmpc_act_reset: one lane per robot
__global__ __launch_bounds__(256) void qmpc_act_reset_kernel(const QmpcActDev S, const uint8_t* __restrict__ mask_a,
                                                             const uint8_t* __restrict__ mask_b, const int stats,
                                                             const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const bool all = !mask_a && !mask_b;
  if (!all && !((mask_a && mask_a[b]) || (mask_b && mask_b[b]))) return;
  qmpc_act_reset_robot(S, b, stats);
}

}  // namespace

extern "C" hipError_t qmpc_launch_act(const QmpcActArgs* A, const double* effort_in, double* effort_out, int batch,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_act_kernel, dim3((batch * 16 + 255) / 256), dim3(256), 0, stream, *A, effort_in, effort_out,
                     batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_act_reset(const QmpcActDev* S, const uint8_t* mask_a, const uint8_t* mask_b, int stats,
                                            int batch, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_act_reset_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, mask_a, mask_b, stats,
                     batch);
  return hipGetLastError();
}
