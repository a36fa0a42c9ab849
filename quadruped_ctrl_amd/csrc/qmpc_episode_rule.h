// qmpc_episode_rule.h -- the decision and the draw of include/qmpc_episode.h in plain C++, __host__ and __device__: the
// kernel of qmpc_episode.hip decides through it, and a CPU program (tests/episode_rule_dump.cpp) compiles it under the
// sanitizers.  fp64, contraction off, one operation at a time; comparisons only, so a NaN fires nothing but NONFINITE.
// Every row index is the high word of a 32 x 32 bit product with the table's length: 0 <= row <= n - 1 for n >= 1.
#ifndef QMPC_EPISODE_RULE_H
#define QMPC_EPISODE_RULE_H

#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/qmpc_episode.h"
#include "qmpc_philox.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QMPC_EP_HD __host__ __device__ __forceinline__
#else
#define QMPC_EP_HD inline
#endif

// what the rule reads of a robot beside its pose, and what a log row records
struct QmpcEpisodeFacts {
  double dx, dy;  // p_x - start_x, p_y - start_y
  double height;  // p_z - ground
  double tilt;    // 1 - 2 (qx^2 + qy^2)
};

// x is neither NaN nor +-inf (x - x is 0 exactly then, and NaN otherwise)
QMPC_EP_HD bool qmpc_episode_finite(double x) {
#pragma clang fp contract(off)
  return x - x == 0.0;
}

// age + elapsed for elapsed >= 1, saturating
QMPC_EP_HD int qmpc_episode_age(int age, int elapsed) { return age > INT_MAX - elapsed ? INT_MAX : age + elapsed; }

// The cause set of a robot (0: it goes on) and the facts of its log row.  p[3], q[4] (w x y z), start[2]; `age` after
// this step's increment.
QMPC_EP_HD int qmpc_episode_cause(const qmpc_episode_rule& R, int safe, const double* p, const double* q, double ground,
                                  const double* start, int age, QmpcEpisodeFacts* F) {
#pragma clang fp contract(off)
  const double xx = q[1] * q[1];
  const double yy = q[2] * q[2];
  const double s = xx + yy;
  const double t = 2.0 * s;
  F->tilt = 1.0 - t;
  F->dx = p[0] - start[0];
  F->dy = p[1] - start[1];
  F->height = p[2] - ground;
  int cause = 0;
  if (safe == 0) cause |= QMPC_EP_UNSAFE;
  bool finite = true;
  for (int k = 0; k < 3; ++k) finite = finite && qmpc_episode_finite(p[k]);
  for (int k = 0; k < 4; ++k) finite = finite && qmpc_episode_finite(q[k]);
  if (!finite) cause |= QMPC_EP_NONFINITE;
  if (qmpc_episode_finite(R.cos_tilt_min) && F->tilt < R.cos_tilt_min) cause |= QMPC_EP_TILT;
  if (qmpc_episode_finite(R.z_min) && F->height < R.z_min) cause |= QMPC_EP_HEIGHT;
  if (qmpc_episode_finite(R.range) && (fabs(F->dx) > R.range || fabs(F->dy) > R.range)) cause |= QMPC_EP_RANGE;
  if (age >= R.max_ticks) cause |= QMPC_EP_TIMEOUT;
  return cause & R.causes;
}

// the gait column of a command row -> a gait number: clamped to [0, 31] (a NaN to 0) in front of the conversion, then
// truncated, so the conversion is defined for any bits in the caller's table (qmpc_ctrl.h: gait numbers 0 .. 11, + 20 omni)
QMPC_EP_HD int32_t qmpc_episode_gait(double g) {
  if (!(g >= 0.0)) g = 0.0;
  if (g > 31.0) g = 31.0;
  return (int32_t)g;
}

// a 32-bit word -> a row of a table of n >= 1 rows
QMPC_EP_HD int qmpc_episode_row(uint32_t w, int n) { return (int)(((uint64_t)w * (uint64_t)(uint32_t)n) >> 32); }

// The draw of robot b for its episode `episode` (the index after the increment): rows of a spawn table of n_spawn and a
// command table of n_commands rows (n_commands < 1: no table, row 0)
QMPC_EP_HD void qmpc_episode_draw(uint32_t key0, uint32_t key1, int b, int episode, int n_spawn, int n_commands,
                                  int* spawn_row, int* command_row) {
  uint32_t w[4];
  qmpc_philox4x32_10((uint32_t)b, (uint32_t)episode, 0u, 0u, key0, key1, w);
  *spawn_row = qmpc_episode_row(w[0], n_spawn);
  *command_row = n_commands >= 1 ? qmpc_episode_row(w[1], n_commands) : 0;
}

// the offset of row `row` of robot b's spawn table: the table is [n_spawn][3], or [B][n_spawn][3] per robot
QMPC_EP_HD size_t qmpc_episode_spawn_at(int b, int row, int n_spawn, int flags) {
  const size_t r = (flags & QMPC_EP_SPAWN_PER_ROBOT) ? (size_t)b * (size_t)n_spawn + (size_t)row : (size_t)row;
  return r * 3;
}

#endif
