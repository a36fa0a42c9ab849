// qmpc_episode_sense.hip -- episodes on the sensor path (include/qmpc_episode_sense.h): the decision kernel of one
// control period, the controller's re-initialisation (full for a robot that finished, all but the pre_work set for a
// robot in warm-up), the hold kernel and the init kernel.  One lane per robot everywhere; no LDS, no scratch.
// The decision of a robot that is not in warm-up is qmpc_episode.hip's, from the same text
// (qmpc_episode_decide_body.h): same rule, same log, same draws.  The ballot in it is reached by every lane of every
// wave: a held lane, a lane past the batch and a lane of a manager that is off all carry judge == false through it.
// The two forms of the re-initialisation are qmpc_glue.h's qmpc_ctrl_init_robot<true / false>, the list
// qmpc_ctrl_init_kernel writes.
#include "qmpc_episode_sense.h"
#include "qmpc_episode_rule.h"

namespace {

__global__ __launch_bounds__(256) void qmpc_episode_sense_decide_kernel(const QmpcEpisodeSenseDev W, const QmpcEpisodeDev S,
                                                                        const QmpcEpisodeIn In, const qmpc_episode_rule R,
                                                                        const qmpc_episode_bind Bd, const int warm_ticks,
                                                                        const int batch) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool in = b < batch;
  const int warm = in ? W.warm[b] : 0;
  const bool held = warm > 0;
  const bool judge = in && !held && R.causes != 0;
  const int elapsed = 1;
#include "qmpc_episode_decide_body.h"
  if (!in) return;
  if (held) {  // not judged: no age, no log row, no counter
    W.warm[b] = warm - 1;
    S.mask[b] = 0;
  } else if (done) {
    W.warm[b] = warm_ticks;
  } else if (!judge) {
    S.mask[b] = 0;  // (the manager is off: the body wrote nothing)
  }
  W.hold[b] = held ? 1 : 0;
  W.both[b] = (held || done) ? 1 : 0;
}

__global__ __launch_bounds__(256) void qmpc_episode_sense_reinit_kernel(const uint8_t* __restrict__ mask,
                                                                        const uint8_t* __restrict__ hold,
                                                                        const QmpcCtrlDev C, const int counter0,
                                                                        double* __restrict__ effort, const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const bool full = mask[b] != 0, part = hold[b] != 0;
  if (!full && !part) return;
  if (full) qmpc_ctrl_init_robot<true>(C, b, counter0);
  else qmpc_ctrl_init_robot<false>(C, b, counter0);
  if (effort)
    for (int k = 0; k < 12; ++k) effort[(size_t)b * 12 + k] = 0.0;
}

// The yaw that qmpc_plant_reset turns into (qw, 0, 0, qz): 2 atan2(qz, qw), and of the doubles within four steps of it
// the first whose half angle gives these very bits back through the reset's own cos and sin -- a robot that a reset has
// just placed is then held on exactly the pose it stands in.  None does (a body that is not upright): the arc tangent.
// This leans on the plant's three reset kernels (qmpc_plant.hip, qmpc_terrain.hip, qmpc_field.hip) building q as
// (cos(yaw / 2), 0, 0, sin(yaw / 2)); tests/test_episode_sense_cpu.py holds their text to that, and
// tests/test_gpu_episode_sense.py holds the round trip over the whole circle of yaw.
__device__ __forceinline__ double hold_yaw(const double qw, const double qz) {
#pragma clang fp contract(off)
  const double y0 = 2.0 * atan2(qz, qw);
  const long long bits = __double_as_longlong(y0);
  double yaw = y0;
  bool found = false;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const int d = (k & 1) ? (k + 1) / 2 : -(k / 2);  // 0, 1, -1, 2, -2, ...
    const double c = __longlong_as_double(bits + d);
    const bool hit = !found && cos(c / 2) == qw && sin(c / 2) == qz;
    yaw = hit ? c : yaw;
    found = found || hit;
  }
  return yaw;
}

__global__ __launch_bounds__(256) void qmpc_episode_sense_hold_kernel(const QmpcEpisodeSenseDev W, const QmpcEpisodeDev S,
                                                                      const double* __restrict__ p,
                                                                      const double* __restrict__ q,
                                                                      const uint8_t* __restrict__ mask, const int ticks,
                                                                      const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (mask && !mask[b]) return;
  W.warm[b] = ticks;
  S.xyyaw[(size_t)b * 3 + 0] = p[(size_t)b * 3 + 0];
  S.xyyaw[(size_t)b * 3 + 1] = p[(size_t)b * 3 + 1];
  S.xyyaw[(size_t)b * 3 + 2] = hold_yaw(q[(size_t)b * 4 + 0], q[(size_t)b * 4 + 3]);
  // ... and the episode's start: RANGE is judged from where the robot is held, not from where an earlier episode began
  S.start[(size_t)b * 2 + 0] = p[(size_t)b * 3 + 0];
  S.start[(size_t)b * 2 + 1] = p[(size_t)b * 3 + 1];
}

__global__ __launch_bounds__(256) void qmpc_episode_sense_init_kernel(const QmpcEpisodeSenseDev W, const int max_batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= max_batch) return;
  W.warm[b] = 0;
  W.hold[b] = 0;
  W.both[b] = 0;
}

}  // namespace

extern "C" hipError_t qmpc_launch_episode_sense_init(const QmpcEpisodeSenseDev* W, int max_batch, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_sense_init_kernel, dim3((max_batch + 255) / 256), dim3(256), 0, stream, *W, max_batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_episode_sense_hold(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S, const double* p,
                                                     const double* q, const uint8_t* mask, int ticks, int batch,
                                                     hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_sense_hold_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *W, *S, p, q, mask,
                     ticks, batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_episode_sense_decide(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S,
                                                       const QmpcEpisodeIn* In, const qmpc_episode_rule* R,
                                                       const qmpc_episode_bind* Bd, int warm_ticks, int batch,
                                                       hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_sense_decide_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *W, *S, *In, *R, *Bd,
                     warm_ticks, batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_episode_sense_reinit(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S,
                                                       const QmpcCtrlDev* C, int counter0, double* effort, int batch,
                                                       hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_sense_reinit_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, S->mask, W->hold, *C,
                     counter0, effort, batch);
  return hipGetLastError();
}
