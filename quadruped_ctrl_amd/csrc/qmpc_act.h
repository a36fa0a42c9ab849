// qmpc_act.h -- device state, launch arguments and launchers of the actuator stage (include/qmpc_act.h), shared by
// qmpc_act.hip (kernels) and qmpc_capi_stages.cpp (entry points).  The per-robot arrays are views into one allocation made by
// qmpc_act_init for the handle's max_batch; the ring is an allocation of its own.
#ifndef QMPC_ACT_DEV_H
#define QMPC_ACT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qmpc_act.h"

// X(element type, name, elements per robot), as QMPC_EPISODE_ARRAYS.  All zero after qmpc_act_init.
#define QMPC_ACT_ARRAYS(X)                                                                            \
  X(int32_t, head, 1)     /* the ring row this period's command goes into */                          \
  X(int32_t, age, 1)      /* periods since init or the robot's last reset, saturated at max_delay */  \
  X(int32_t, n, 1)        /* the accumulators of include/qmpc_act.h */                                \
  X(int64_t, n_vsat, 1)                                                                               \
  X(int64_t, n_tsat, 1)                                                                               \
  X(double, tau_peak, 1)                                                                              \
  X(double, e_heat, 1)                                                                                \
  X(double, e_mech, 1)                                                                                \
  X(double, e_pos, 1)

struct QmpcActDev {
#define QMPC_ACT_MEMBER(T, name, per_robot) T* name;
  QMPC_ACT_ARRAYS(QMPC_ACT_MEMBER)
#undef QMPC_ACT_MEMBER
};

#if defined(__HIPCC__)
// qmpc_act_reset of robot b: the ring fills again; with stats the accumulators start at zero.  One text behind the reset
// kernel of qmpc_act.hip and the reset stage of qmpc_loop.hip.
__device__ __forceinline__ void qmpc_act_reset_robot(const QmpcActDev& S, const int b, const int stats) {
  S.age[b] = 0;
  if (!stats) return;
  S.n[b] = 0;
  S.n_vsat[b] = 0;
  S.n_tsat[b] = 0;
  S.tau_peak[b] = 0.0;
  S.e_heat[b] = 0.0;
  S.e_mech[b] = 0.0;
  S.e_pos[b] = 0.0;
}
#endif

// by value; the six parameter pointers are the caller's arrays as bound (null: the config's value / absent / 0)
struct QmpcActArgs {
  QmpcActDev d;
  double* ring;         // [max_delay + 1][batch][12]
  const double* motor;  // [B][24] the plant's last read-out (QmpcPlantDev::motor): the rates are columns 12..23
  const double* battery_v;
  const double* tau_max;
  const double* strength;
  const double* damping;
  const double* dry_friction;
  const int32_t* delay;
  qmpc_act_config cfg;
  double dt;
};

// Launchers of qmpc_act.hip, declared once for the file that defines them and for qmpc_capi_stages.cpp, which calls them: a
// signature that drifts fails to compile.
// one control period; effort_out may be effort_in
extern "C" hipError_t qmpc_launch_act(const QmpcActArgs* A, const double* effort_in, double* effort_out, int batch,
                                      hipStream_t stream);
// age = 0 (and with stats the accumulators' zeros) where mask_a | mask_b is set; both null: every robot
extern "C" hipError_t qmpc_launch_act_reset(const QmpcActDev* D, const uint8_t* mask_a, const uint8_t* mask_b, int stats,
                                            int batch, hipStream_t stream);

#endif
