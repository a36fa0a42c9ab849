// qmpc_episode_sense.h -- device state and launchers of episodes on the sensor path (include/qmpc_episode_sense.h), shared
// by qmpc_episode_sense.hip (kernels) and qmpc_capi_stages.cpp (entry points).  Views into one allocation made by
// qmpc_episode_sense_init for the handle's max_batch.
#ifndef QMPC_EPISODE_SENSE_DEV_H
#define QMPC_EPISODE_SENSE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qmpc_episode_sense.h"
#include "qmpc_episode.h"
#include "qmpc_glue.h"

// X(element type, name, elements per robot), as QMPC_EPISODE_ARRAYS
#define QMPC_EPISODE_SENSE_ARRAYS(X)                                                                   \
  X(int32_t, warm, 1)  /* control periods of warm-up the robot still has in front of it */             \
  X(uint8_t, hold, 1)  /* scratch: 1 for the robots the last step held */                              \
  X(uint8_t, both, 1)  /* scratch: mask | hold of the last step, what the plant's reset is given */

struct QmpcEpisodeSenseDev {
#define QMPC_EPISODE_SENSE_MEMBER(T, name, per_robot) T* name;
  QMPC_EPISODE_SENSE_ARRAYS(QMPC_EPISODE_SENSE_MEMBER)
#undef QMPC_EPISODE_SENSE_MEMBER
};

// Launchers of qmpc_episode_sense.hip, declared once for the file that defines them and for qmpc_capi_stages.cpp, which calls
// them: a signature that drifts fails to compile.
// warm = hold = both = 0 for robots 0 .. max_batch-1
extern "C" hipError_t qmpc_launch_episode_sense_init(const QmpcEpisodeSenseDev* W, int max_batch, hipStream_t stream);
// warm = ticks, xyyaw = the plant's x, y, yaw (p [B][3], q [B][4]) and start = its x, y for the masked robots (NULL: all)
extern "C" hipError_t qmpc_launch_episode_sense_hold(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S, const double* p,
                                                     const double* q, const uint8_t* mask, int ticks, int batch,
                                                     hipStream_t stream);
// the decision of one control period: warm / hold / both, and for the robots not in warm-up qmpc_episode.hip's decision
extern "C" hipError_t qmpc_launch_episode_sense_decide(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S,
                                                       const QmpcEpisodeIn* In, const qmpc_episode_rule* R,
                                                       const qmpc_episode_bind* Bd, int warm_ticks, int batch,
                                                       hipStream_t stream);
// the controller's re-initialisation: full where S->mask is set, all but the pre_work set where W->hold is set; rows of
// effort (null: none) zeroed for both
extern "C" hipError_t qmpc_launch_episode_sense_reinit(const QmpcEpisodeSenseDev* W, const QmpcEpisodeDev* S,
                                                       const QmpcCtrlDev* C, int counter0, double* effort, int batch,
                                                       hipStream_t stream);

#endif
