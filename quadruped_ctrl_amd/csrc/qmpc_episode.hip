// qmpc_episode.hip -- the episode manager of include/qmpc_episode.h: the decision kernel (one lane per robot, one launch
// per qmpc_episode_step), the init kernel and the log clear.  The decision and the draw are the inline functions of
// qmpc_episode_rule.h, the same text a host program compiles; fp contraction is off, and tests/episode_model.py
// restates every expression in the same order and agrees bit for bit.
// No LDS, no scratch.  The only atomics are the log's: the done lanes of a wave take consecutive rows behind ONE add of
// the wave's first done lane (qmpc_glue.hip's due list does the same), and a wave that runs past the end of the log gives
// back what it could not use, so log_count never stays above log_rows.  The ballot is reached by every lane of every
// wave: no lane returns in front of it.  The decision's statements are qmpc_episode_decide_body.h, which the decision
// kernel of qmpc_episode_sense.hip includes too.
#include "qmpc_episode.h"
#include "qmpc_episode_rule.h"

namespace {

__global__ __launch_bounds__(256) void qmpc_episode_decide_kernel(const QmpcEpisodeDev S, const QmpcEpisodeIn In,
                                                                  const qmpc_episode_rule R, const qmpc_episode_bind Bd,
                                                                  const int elapsed, const int batch) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool judge = b < batch;  // every robot is judged
#include "qmpc_episode_decide_body.h"
}

// one lane per robot of the allocation: everything zero; start = the plant's p_x, p_y for the robots initialised
__global__ __launch_bounds__(256) void qmpc_episode_init_kernel(const QmpcEpisodeDev S, const double* __restrict__ p,
                                                                const int batch, const int max_batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < 2) S.log_words[b] = 0;  // (in front of the return: a handle of one robot has no lane 1 below it)
  if (b >= max_batch) return;
  const bool live = b < batch;
  S.start[(size_t)b * 2 + 0] = live ? p[(size_t)b * 3 + 0] : 0.0;
  S.start[(size_t)b * 2 + 1] = live ? p[(size_t)b * 3 + 1] : 0.0;
  for (int k = 0; k < 3; ++k) S.xyyaw[(size_t)b * 3 + k] = 0.0;
  S.ticks_sum[b] = 0;
  S.age[b] = 0;
  S.episode[b] = 0;
  for (int k = 0; k < QMPC_EP_CAUSES; ++k) S.count[(size_t)b * QMPC_EP_CAUSES + k] = 0;
  S.last_cause[b] = 0;
  S.last_ticks[b] = 0;
  S.mask[b] = 0;
}

__global__ void qmpc_episode_log_clear_kernel(const QmpcEpisodeDev S) {
  if (threadIdx.x < 2) S.log_words[threadIdx.x] = 0;
}

}  // namespace

extern "C" hipError_t qmpc_launch_episode_init(const QmpcEpisodeDev* S, const double* p, int batch, int max_batch,
                                               hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_init_kernel, dim3((max_batch + 255) / 256), dim3(256), 0, stream, *S, p, batch, max_batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_episode_decide(const QmpcEpisodeDev* S, const QmpcEpisodeIn* In,
                                                 const qmpc_episode_rule* R, const qmpc_episode_bind* Bd, int elapsed,
                                                 int batch, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_decide_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *S, *In, *R, *Bd, elapsed,
                     batch);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_episode_log_clear(const QmpcEpisodeDev* S, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_episode_log_clear_kernel, dim3(1), dim3(64), 0, stream, *S);
  return hipGetLastError();
}
