// qmpc_terrain.hip -- the plant of include/qmpc_plant.h on the per-robot terrain of include/qmpc_terrain.h: an inclined
// plane plus a flight of stairs per robot, analytic, read from the caller's terrain[B][8] at every launch.  The device
// code is shared with the flat plant of qmpc_plant.hip (qmpc_plant_dev.h): the kernels here are the statements of
// qmpc_plant_step_body.h with TERRAIN = true in the four <VARY, STATS> combinations, and the reset that stands the
// robots on their terrain.  One lane per (robot, leg); the lanes past n in the last wave repeat lane n - 1 and store
// nothing; quad sums through two xor-shuffles; no LDS, no atomics.  tests/plant_model_terrain.py restates every
// expression in the same order.
#include "qmpc_plant_dev.h"

namespace {

// qmpc_plant_reset while terrain is bound (mask == NULL: every robot).  n = batch * 4 lanes.  The reset of a lane is
// qmpc_plant_dev.h's plant_ground_init_lane, which the loop kernel's reset stage calls too.  Every lane computes (the
// shuffles need their partners); masked ones store.
__global__ __launch_bounds__(256) void qmpc_terrain_init_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                                const uint8_t* __restrict__ mask,
                                                                const double* __restrict__ xyyaw, const int n,
                                                                const QmpcTerrainArgs T) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool in = t < n;
  const int tt = in ? t : n - 1;
  const int b = tt >> 2;
  const bool live = in && (!mask || mask[b]);
  const double x0 = xyyaw ? xyyaw[(size_t)b * 3] : 0.0, y0 = xyyaw ? xyyaw[(size_t)b * 3 + 1] : 0.0;
  const double yaw = xyyaw ? xyyaw[(size_t)b * 3 + 2] : 0.0;
  const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
  plant_ground_init_lane<false>(S, K, T, QmpcFieldArgs{}, x0, y0, q, tt, live);
}

// One control period on terrain: qmpc_plant_step_body.h with TERRAIN = true
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) void qmpc_terrain_step_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                                const double* __restrict__ effort,
                                                                const float* __restrict__ contact_state,
                                                                const float* __restrict__ p_des,
                                                                const float* __restrict__ v_des, double* state_out,
                                                                double* motor_out, const int n, const QmpcPlantVary V,
                                                                const QmpcTerrainArgs T) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = true;
  constexpr bool FIELD = false;
  const QmpcFieldArgs Fd{};
#include "qmpc_plant_step_body.h"
}

}  // namespace

extern "C" hipError_t qmpc_launch_terrain_init(const QmpcPlantResetArgs* A, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_terrain_init_kernel, plant_grid(A->n), dim3(256), 0, stream, A->S, A->K, A->mask, A->xyyaw,
                     A->n, A->T);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_terrain_step(const QmpcPlantStepArgs* A, int vary, int stats, hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_terrain_step_kernel<VARY.value, STATS.value>), plant_grid(A->n), dim3(256), 0, stream, A->S,
                       A->K, A->effort, A->contact_state, A->p_des, A->v_des, A->state_out, A->motor_out, A->n, A->V,
                       A->T);
  });
  return hipGetLastError();
}
