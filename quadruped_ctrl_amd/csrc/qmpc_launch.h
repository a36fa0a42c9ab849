// qmpc_launch.h -- launchers that qmpc_capi.cpp calls and that have no per-unit header of their own (those of
// qmpc_glue.hip, qmpc_plant.hip, qmpc_sense.hip and qmpc_episode.hip are declared in qmpc_glue.h, qmpc_plant.h, qmpc_sense.h
// and qmpc_episode.h).
#ifndef QMPC_LAUNCH_H
#define QMPC_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/qmpc.h"
#include "qmpc_device.h"

// qmpc_pack.hip -- checked: the file includes this header, so a signature that drifts fails to compile
extern "C" hipError_t qmpc_launch_pack(const qmpc_command* c, const qmpc_record* rec, int batch, int horizon, float dt_mpc,
                                       hipStream_t stream);
extern "C" hipError_t qmpc_launch_f2b(const float* r_body, const float* grf, float* f_ff, int batch, hipStream_t stream);

// qmpc_kernels.hip (one translation unit per size class) and qmpc_engine.hip -- the CALLER'S side only.  The defining
// side is UNCHECKED: those two files (with qmpc_wave.h, qmpc_cmd.h and qmpc_device.h) are hashed into the kernel-source
// stamp that ties the committed profiles to the tree (bench.py: KERNEL_SOURCES), so they do not include this header; with
// C linkage a definition that drifts from these lines still links.  Whoever changes one of these signatures changes both
// places.
#define QMPC_DECLARE_CLASS(RB)                                                                  \
  extern "C" size_t qmpc_c##RB##_smem(void);                                                    \
  extern "C" hipError_t qmpc_c##RB##_prepare(void);                                             \
  extern "C" int qmpc_c##RB##_resident(void);                                                   \
  extern "C" hipError_t qmpc_c##RB##_launch(const QmpcParams* P, int grid, hipStream_t stream);   \
  extern "C" int qmpc_c##RB##_resident_sweep(void);                                              \
  extern "C" hipError_t qmpc_c##RB##_launch_sweep(const QmpcParams* P, int grid, hipStream_t stream);
QMPC_DECLARE_CLASS(1)
QMPC_DECLARE_CLASS(2)
QMPC_DECLARE_CLASS(3)
QMPC_DECLARE_CLASS(4)
QMPC_DECLARE_CLASS(6)
#undef QMPC_DECLARE_CLASS
extern "C" hipError_t qmpc_launch_keys(const QmpcParams* P, int* nst, float* score, float* demand, hipStream_t stream);
extern "C" hipError_t qmpc_big_prepare(void);
extern "C" hipError_t qmpc_big_launch(const QmpcParams* P, int grid, hipStream_t stream);
// the decoupled path's consumer (qmpc_engine.hip)
extern "C" hipError_t qmpc_engine_prepare(void);
extern "C" int qmpc_engine_resident(int rb);
extern "C" int qmpc_engine_capacity(int rb);
extern "C" hipError_t qmpc_engine_launch(int rb, const QmpcParams* P, int grid, hipStream_t stream);
extern "C" hipError_t qmpc_admm_big_launch(const QmpcParams* P, int grid, hipStream_t stream);

#endif
