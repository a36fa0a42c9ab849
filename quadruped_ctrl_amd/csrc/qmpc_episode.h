// qmpc_episode.h -- device state and launch arguments of the episode manager (include/qmpc_episode.h), shared by
// qmpc_episode.hip (kernels) and qmpc_capi_stages.cpp (entry points).  Views into one allocation made by qmpc_episode_init for the
// handle's max_batch.
#ifndef QMPC_EPISODE_DEV_H
#define QMPC_EPISODE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qmpc_episode.h"

// X(element type, name, elements per robot): members, carving and the view are generated from the list (8-byte types
// first; every array starts 256-byte aligned)
#define QMPC_EPISODE_ARRAYS(X)                                                       \
  X(double, start, 2)       /* world x, y of the running episode's start */          \
  X(double, xyyaw, 3)       /* scratch: where a reset robot is put */                \
  X(int64_t, ticks_sum, 1)  /* the finished episodes' lengths, summed */             \
  X(int32_t, age, 1)        /* control periods since the last reset */               \
  X(int32_t, episode, 1)    /* episodes finished */                                  \
  X(int32_t, count, 6)      /* per cause */                                          \
  X(int32_t, last_cause, 1)                                                          \
  X(int32_t, last_ticks, 1)                                                          \
  X(uint8_t, mask, 1)       /* scratch: the robots the last step reset */

struct QmpcEpisodeDev {
#define QMPC_EPISODE_MEMBER(T, name, per_robot) T* name;
  QMPC_EPISODE_ARRAYS(QMPC_EPISODE_MEMBER)
#undef QMPC_EPISODE_MEMBER
  int32_t* log_words;  // [2] log_count, log_dropped (behind the arrays, in the same allocation)
};

// what the decision kernel reads of the handle's other state (by value)
struct QmpcEpisodeIn {
  const double* p;       // [B][3] QmpcPlantDev::p
  const double* q;       // [B][4] QmpcPlantDev::q
  const int32_t* safe;   // [B]    QmpcCtrlDev::safe
  const double* ground;  // [B]    QmpcTerrainArgs::ground while the plant maintains it, else null: 0
  uint32_t key0, key1;   // the seed's low and high word
};

// Launchers of qmpc_episode.hip, declared once for the file that defines them and for qmpc_capi_stages.cpp, which calls them: a
// signature that drifts fails to compile.
// every array of S zeroed for robots 0 .. max_batch-1 and both log words; start = p_x, p_y for robots 0 .. batch-1
extern "C" hipError_t qmpc_launch_episode_init(const QmpcEpisodeDev* S, const double* p, int batch, int max_batch,
                                               hipStream_t stream);
extern "C" hipError_t qmpc_launch_episode_decide(const QmpcEpisodeDev* S, const QmpcEpisodeIn* In,
                                                 const qmpc_episode_rule* R, const qmpc_episode_bind* Bd, int elapsed,
                                                 int batch, hipStream_t stream);
extern "C" hipError_t qmpc_launch_episode_log_clear(const QmpcEpisodeDev* S, hipStream_t stream);

#endif
