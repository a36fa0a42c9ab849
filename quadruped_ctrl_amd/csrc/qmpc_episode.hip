// qmpc_episode.hip -- the episode manager of include/qmpc_episode.h: the decision kernel (one lane per robot, one launch
// per qmpc_episode_step), the init kernel and the log clear.  The decision and the draw are the inline functions of
// qmpc_episode_rule.h, the same text a host program compiles; fp contraction is off, and tests/episode_model.py
// restates every expression in the same order and agrees bit for bit.
// No LDS, no scratch.  The only atomics are the log's: the done lanes of a wave take consecutive rows behind ONE add of
// the wave's first done lane (qmpc_glue.hip's due list does the same), and a wave that runs past the end of the log gives
// back what it could not use, so log_count never stays above log_rows.  The ballot is reached by every lane of every
// wave: no lane returns in front of it.
#include "qmpc_episode.h"
#include "qmpc_episode_rule.h"

namespace {

__global__ __launch_bounds__(256) void qmpc_episode_decide_kernel(const QmpcEpisodeDev S, const QmpcEpisodeIn In,
                                                                  const qmpc_episode_rule R, const qmpc_episode_bind Bd,
                                                                  const int elapsed, const int batch) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool in = b < batch;
  int cause = 0, age = 0;
  QmpcEpisodeFacts F{};
  if (in) {
    double p[3], q[4], start[2];
    for (int k = 0; k < 3; ++k) p[k] = In.p[(size_t)b * 3 + k];
    for (int k = 0; k < 4; ++k) q[k] = In.q[(size_t)b * 4 + k];
    for (int k = 0; k < 2; ++k) start[k] = S.start[(size_t)b * 2 + k];
    const double ground = In.ground ? In.ground[b] : 0.0;
    age = qmpc_episode_age(S.age[b], elapsed);
    cause = qmpc_episode_cause(R, In.safe[b], p, q, ground, start, age, &F);
  }
  const bool done = cause != 0;
  const int episode = done ? S.episode[b] : 0;
  if (Bd.log) {
    // the wave's done lanes take consecutive rows; a row at or beyond log_rows is not written
    const unsigned long long m = __ballot(done);
    if (m) {
      const int lane = (int)__lane_id(), leader = __ffsll(m) - 1, n = __popcll(m);
      int base = 0;
      if (lane == leader) {
        base = atomicAdd(S.log_words, n);
        const long long end = (long long)base + n, cap = (long long)Bd.log_rows;
        if (end > cap) {
          const int beyond = (int)(end - (base > cap ? (long long)base : cap));
          atomicSub(S.log_words, beyond);
          atomicAdd(S.log_words + 1, beyond);
        }
      }
      base = __shfl(base, leader);
      const long long row = (long long)base + __popcll(m & ((1ull << lane) - 1ull));
      if (done && row < (long long)Bd.log_rows) {
        double* out = Bd.log + (size_t)row * 8;
        out[0] = (double)b;
        out[1] = (double)episode;
        out[2] = (double)cause;
        out[3] = (double)age;
        out[4] = F.dx;
        out[5] = F.dy;
        out[6] = F.height;
        out[7] = F.tilt;
      }
    }
  }
  if (!in) return;
  if (!done) {
    S.age[b] = age;
    S.mask[b] = 0;
    return;
  }
  for (int k = 0; k < QMPC_EP_CAUSES; ++k)
    if (cause & (1 << k)) S.count[(size_t)b * QMPC_EP_CAUSES + k] += 1;
  S.ticks_sum[b] += (int64_t)age;
  S.last_cause[b] = cause;
  S.last_ticks[b] = age;
  const int next = (int)((uint32_t)episode + 1u);
  int spawn_row, command_row;
  qmpc_episode_draw(In.key0, In.key1, b, next, Bd.n_spawn, Bd.commands ? Bd.n_commands : 0, &spawn_row, &command_row);
  const double* sp = Bd.spawn + qmpc_episode_spawn_at(b, spawn_row, Bd.n_spawn, Bd.flags);
  const double x = sp[0], y = sp[1];
  S.xyyaw[(size_t)b * 3 + 0] = x;
  S.xyyaw[(size_t)b * 3 + 1] = y;
  S.xyyaw[(size_t)b * 3 + 2] = sp[2];
  S.start[(size_t)b * 2 + 0] = x;
  S.start[(size_t)b * 2 + 1] = y;
  S.mask[b] = 1;
  S.age[b] = 0;
  S.episode[b] = next;
  if (Bd.commands) {
    const double* cm = Bd.commands + (size_t)command_row * 4;
    for (int k = 0; k < 3; ++k) Bd.vel[(size_t)b * 3 + k] = cm[k];
    Bd.gait[b] = qmpc_episode_gait(cm[3]);
  }
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
