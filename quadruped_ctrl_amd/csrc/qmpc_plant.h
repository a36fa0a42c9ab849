// qmpc_plant.h -- device state of the reduced-order plant (include/qmpc_plant.h), shared by qmpc_plant.hip (kernels)
// and qmpc_capi_plant.cpp (entry points).  Views into one allocation made by qmpc_plant_init for the handle's max_batch.
#ifndef QMPC_PLANT_DEV_H
#define QMPC_PLANT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmpc_plant_pick.h"

// X(element type, name, elements per robot): members, carving and the view are generated from the list
#define QMPC_PLANT_ARRAYS(X)                                                        \
  X(double, p, 3)       /* body position, world */                                  \
  X(double, v, 3)       /* body velocity, world */                                  \
  X(double, q, 4)       /* w x y z */                                               \
  X(double, omega, 3)   /* body frame */                                            \
  X(double, foot, 12)   /* world */                                                 \
  X(double, grf, 12)    /* ground reactions of the last substep, world */           \
  X(double, state, 16)  /* the last read-out (qmpc_ctrl.h: state[B][16]) */         \
  X(double, motor, 24)  /* ... motor[B][24] */                                      \
  X(int, stance, 4)

struct QmpcPlantDev {
#define QMPC_PLANT_MEMBER(T, name, per_robot) T* name;
  QMPC_PLANT_ARRAYS(QMPC_PLANT_MEMBER)
#undef QMPC_PLANT_MEMBER
};

// the constants of a launch (by value)
struct QmpcPlantConst {
  double mass, ibody[3];     // qmpc_set_robot
  double geom[4];            // abad, hip, knee, knee_y (the handle's floats, widened)
  double mu;                 // mu_plant
  double h;                  // dt / substeps
  double r2_lo, r2_hi;       // the swing clamp's shell: |r|^2 at knee angle QMPC_PLANT_KNEE_MAX / _MIN
  int substeps;
};

// include/qmpc_plant_vary.h: the caller's per-robot arrays (null: the handle's value / none) and the statistics'
// accumulators (one allocation for max_batch robots, made by the first qmpc_plant_stats_enable: acc[k][max_batch] in the
// order of QMPC_PLANT_STAT_*, then n[max_batch]).  By value, after the step's other arguments; the plain instantiation
// reads none of it.
struct QmpcPlantVary {
  const double* mass;    // [B]
  const double* ibody;   // [B][3]
  const double* mu;      // [B]
  const double* force;   // [B][3] world
  const double* torque;  // [B][3] body
  double* acc;           // [QMPC_PLANT_STATS][acc_stride]
  int* n;                // [B] steps accumulated
  int acc_stride;        // max_batch
};
enum {
  QMPC_PLANT_STAT_Z_MIN, QMPC_PLANT_STAT_Z_MAX, QMPC_PLANT_STAT_ROLL_MAX, QMPC_PLANT_STAT_PITCH_MAX,
  QMPC_PLANT_STAT_VX_SUM, QMPC_PLANT_STAT_VY_SUM, QMPC_PLANT_STATS
};

// include/qmpc_terrain.h: the caller's terrain rows as bound (null: flat ground, the kernels of qmpc_plant.hip), the
// plant's ground[max_batch] and support[max_batch] (one allocation made by qmpc_plant_init) and the flags.  By value.
struct QmpcTerrainArgs {
  const double* rows;  // [B][8] z0, gx, gy, rise, run, count, s0, psi
  double* ground;      // [B] height under the body origin at the last pose
  double* support;     // [B] mean height of the stance feet (kept through a flight phase)
  int flags;           // QMPC_TERRAIN_*
};

// include/qmpc_contact.h: the flags and scalars as set (flags 0: off, the kernels of qmpc_plant.hip / qmpc_terrain.hip), dt =
// 1 / freq, and the plant's counters (one allocation made by qmpc_plant_init for max_batch robots).  By value.
struct QmpcContactArgs {
  double drop_speed, slip_gain, slip_vmax, dt;
  int32_t* early;  // [B] foot-ticks pinned while scheduled to swing
  int32_t* late;   // [B] foot-ticks unpinned while scheduled to stand
  double* slip;    // [B] metres slid
  double* drop;    // [B][4] how far a late foot has been lowered
  int flags;       // QMPC_CONTACT_*
};

// include/qmpc_field.h: the caller's bank and placements as bound (z null: no field, the kernels above).  By value.  The
// flags of the binding are OR-ed into the QmpcTerrainArgs a field launcher is given.
struct QmpcFieldArgs {
  const float* z;       // [count][ny][nx], x fastest
  const double* place;  // [B][4] map, ox, oy, zs
  double cell;
  int nx, ny, count;
};

#define QMPC_PLANT_GRAVITY 9.81
#define QMPC_PLANT_HEIGHT 0.29      /* ConvexMPCLocomotion::_body_height */
#define QMPC_PLANT_SIDE_OFFSET 0.065
#define QMPC_PLANT_DET_MIN 1e-5     /* |det J| below this: no force, no joint rates */
#define QMPC_PLANT_KNEE_MIN 0.05    /* the swing clamp's shell, as knee angles */
#define QMPC_PLANT_KNEE_MAX 2.6

// The arguments of a step, filled in one place (qmpc_capi_plant.cpp: plant_step_args) and given to every step launcher.  The
// contact kernels take this struct itself, by value: it IS their kernarg segment, which they read a second time
// (qmpc_contact_step_body.h), so a member a kernel does not read costs it kernarg bytes and no instruction.  The
// scheduled-contact kernels keep separate parameters (profiles/plant_kernel_resources.txt); their launchers spread the
// members they take.  V is an empty QmpcPlantVary when nothing is bound and the statistics are off; T carries the OR of
// the terrain's and the field's flags; n = batch * 4 lanes.
struct QmpcPlantStepArgs {
  QmpcPlantDev S;
  QmpcPlantConst K;
  const double* effort;
  const float *contact_state, *p_des, *v_des;
  double *state_out, *motor_out;
  int n;
  QmpcPlantVary V;
  QmpcTerrainArgs T;
  QmpcContactArgs C;
  QmpcFieldArgs Fd;
};

// ... and of a reset that stands the masked robots on the ground (mask == NULL: every robot; xyyaw == NULL: the origin).
struct QmpcPlantResetArgs {
  QmpcPlantDev S;
  QmpcPlantConst K;
  const uint8_t* mask;
  const double* xyyaw;
  int n;
  QmpcTerrainArgs T;  // qmpc_launch_plant_init reads neither T nor Fd
  QmpcFieldArgs Fd;   // qmpc_launch_terrain_init does not read Fd
};

// Launchers, declared once for the files that define them and for qmpc_capi_plant.cpp (the resets: qmpc_capi_stages.cpp too), which calls them: a signature that
// drifts fails to compile.  One step and one reset launcher per entry of qmpc_plant_pick.h's lists, all of one signature;
// vary (per-robot parameters bound) and stats (statistics on) pick the step's instantiation.
#define QMPC_PLANT_DECLARE(NAME, name)                                                                             \
  extern "C" hipError_t qmpc_launch_##name##_step(const QmpcPlantStepArgs* A, int vary, int stats, hipStream_t stream);
QMPC_PLANT_STEP_KINDS(QMPC_PLANT_DECLARE)
#undef QMPC_PLANT_DECLARE
#define QMPC_PLANT_DECLARE(NAME, name) \
  extern "C" hipError_t qmpc_launch_##name##_init(const QmpcPlantResetArgs* A, hipStream_t stream);
QMPC_PLANT_RESET_KINDS(QMPC_PLANT_DECLARE)
#undef QMPC_PLANT_DECLARE
extern "C" hipError_t qmpc_launch_plant_stats_reset(const QmpcPlantVary* V, const uint8_t* mask, int batch,
                                                    hipStream_t stream);
// qmpc_contact.hip: the reset of the contact counters, enqueued before the ground's own reset (T->rows may be null)
extern "C" hipError_t qmpc_launch_contact_reset(const uint8_t* mask, int batch, hipStream_t stream,
                                                const QmpcTerrainArgs* T, const QmpcContactArgs* C);

#endif
