// qmpc_sense.hip -- the sensor model of include/qmpc_sense.h: one launch per control period, 16 lanes per robot (four
// robots per wave).  Lanes 0..11 take one joint each (angle and rate), lanes 12..14 one body axis each (accelerometer
// and gyro): two channels per lane, each at most one Philox4x32-10 call.  Lane 15 copies the quaternion and stores
// n + 1.  All sixteen lanes load n with ONE wave instruction in front of the first branch, and lane 15's store needs
// the value that load returns: every lane has read the old count before the new one is written -- program order
// inside a wave is enough.
// No LDS, no atomics, no shuffles.  fp contraction is off: tests/sense_model.py restates every expression in the same
// order and agrees bit for bit (integer arithmetic up to the one conversion, then a subtraction and a multiplication).
// <false> is the ideal sensor: nothing bound, no generator call.
#include "qmpc_philox.h"  // Random123's Philox4x32 with ten rounds
#include "qmpc_sense.h"

namespace {

// the centred sum of the four words, scaled to unit variance: |z| <= 2 sqrt(3)
__device__ __forceinline__ double sense_z(const QmpcSenseArgs& A, int b, int n, int channel, int epoch) {
#pragma clang fp contract(off)
  uint32_t w[4];
  qmpc_philox4x32_10((uint32_t)b, (uint32_t)n, (uint32_t)channel, (uint32_t)epoch, A.key0, A.key1, w);
  const uint64_t s = ((uint64_t)w[0] + (uint64_t)w[1]) + ((uint64_t)w[2] + (uint64_t)w[3]);
  return ((double)s - 8589934590.0) * (1.7320508075688772 * 0x1p-32);
}

// out = x + d, only when a term of d is bound: d = sigma z (sigma bound), d = bias + d (bias bound)
__device__ __forceinline__ double sense_channel(const QmpcSenseArgs& A, double x, const double* sigma,
                                                const double* bias, int b, int n, int channel, int epoch) {
#pragma clang fp contract(off)
  if (!sigma && !bias) return x;
  double d = 0.0;
  if (sigma) d = *sigma * sense_z(A, b, n, channel, epoch);
  if (bias) d = *bias + d;
  return x + d;
}

template <bool NOISY>
__global__ __launch_bounds__(256) void qmpc_sense_kernel(const QmpcSenseArgs A, double* __restrict__ imu_out,
                                                         double* __restrict__ motor_out, const int batch) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int b = t >> 4, lane = t & 15;
  if (b >= batch) return;
  const double* st = A.state + (size_t)b * 16;
  const double* mo = A.motor + (size_t)b * 24;
  double* imu = imu_out + (size_t)b * 10;
  double* out = motor_out + (size_t)b * 24;
  // every lane reads the count here, in front of the branch: lane 15's store below cannot overtake a load of its robot
  const int n = A.n[b];
  if (lane == 15) {
    imu[3] = st[1];
    imu[4] = st[2];
    imu[5] = st[3];
    imu[6] = st[0];
    A.n[b] = n + 1;
    return;
  }
  // the lane's two channels: (joint angle, joint rate) or (accelerometer axis, gyro axis)
  const bool joint = lane < 12;
  const int k = joint ? lane : lane - 12;
  const double* src0 = joint ? mo + k : st + 13 + k;
  const double* src1 = joint ? mo + 12 + k : st + 7 + k;
  double* dst0 = joint ? out + k : imu + k;
  double* dst1 = joint ? out + 12 + k : imu + 7 + k;
  double x0 = *src0, x1 = *src1;
  if constexpr (NOISY) {
    const int epoch = A.epoch[b];
    const double* sg0 = joint ? A.q_sigma : A.acc_sigma;
    const double* sg1 = joint ? A.qd_sigma : A.gyro_sigma;
    const double* bs0 = joint ? nullptr : A.acc_bias;
    const double* bs1 = joint ? nullptr : A.gyro_bias;
    x0 = sense_channel(A, x0, sg0 ? sg0 + b : nullptr, bs0 ? bs0 + (size_t)b * 3 + k : nullptr, b, n,
                       (joint ? QMPC_SENSE_CH_Q : QMPC_SENSE_CH_ACC) + k, epoch);
    x1 = sense_channel(A, x1, sg1 ? sg1 + b : nullptr, bs1 ? bs1 + (size_t)b * 3 + k : nullptr, b, n,
                       (joint ? QMPC_SENSE_CH_QD : QMPC_SENSE_CH_GYRO) + k, epoch);
  }
  *dst0 = x0;
  *dst1 = x1;
}

// qmpc_sense_init's zeroing is a memset; this is qmpc_sense_reset (mask == NULL: every robot): one lane per robot
__global__ __launch_bounds__(256) void qmpc_sense_reset_kernel(const QmpcSenseArgs A, const uint8_t* __restrict__ mask,
                                                               const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (mask && !mask[b]) return;
  A.epoch[b] = A.epoch[b] + 1;
  A.n[b] = 0;
}

}  // namespace

// noisy: at least one of the six parameter pointers is bound
extern "C" hipError_t qmpc_launch_sense(const QmpcSenseArgs* A, double* imu_out, double* motor_out, int batch, int noisy,
                                        hipStream_t stream) {
  const dim3 grid((batch * 16 + 255) / 256), block(256);
  if (noisy)
    hipLaunchKernelGGL((qmpc_sense_kernel<true>), grid, block, 0, stream, *A, imu_out, motor_out, batch);
  else
    hipLaunchKernelGGL((qmpc_sense_kernel<false>), grid, block, 0, stream, *A, imu_out, motor_out, batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_sense_reset(const QmpcSenseArgs* A, const uint8_t* mask, int batch,
                                              hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_sense_reset_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *A, mask, batch);
  return hipGetLastError();
}
