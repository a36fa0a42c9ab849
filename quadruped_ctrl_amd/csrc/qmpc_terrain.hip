// qmpc_terrain.hip -- the plant of include/qmpc_plant.h on the per-robot terrain of include/qmpc_terrain.h: an inclined
// plane plus a flight of stairs per robot, analytic, read from the caller's terrain[B][8] at every launch.  The device
// code is shared with the flat plant of qmpc_plant.hip (qmpc_plant_dev.h): the kernels here are the statements of
// qmpc_plant_step_body.h with TERRAIN = true in the four <VARY, STATS> combinations, and the reset that stands the
// robots on their terrain.  One lane per (robot, leg); the lanes past n in the last wave repeat lane n - 1 and store
// nothing; quad sums through two xor-shuffles; no LDS, no atomics.  tests/plant_model_terrain.py restates every
// expression in the same order.
#include "qmpc_plant_dev.h"

namespace {

// qmpc_plant_reset while terrain is bound (mask == NULL: every robot).  n = batch * 4 lanes.  The body stands level at
// (x0, y0, 0.29 + height(x0, y0)), every foot at its usual body-frame xy on the surface; support is the mean of the four
// feet, (c_0 + c_1) + (c_2 + c_3) over 4.  Every lane computes (the shuffles need their partners); masked ones store.
__global__ __launch_bounds__(256) void qmpc_terrain_init_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                                const uint8_t* __restrict__ mask,
                                                                const double* __restrict__ xyyaw, const int n,
                                                                const QmpcTerrainArgs T) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool in = t < n;
  const int tt = in ? t : n - 1;
  const int b = tt >> 2, leg = tt & 3;
  const bool live = in && (!mask || mask[b]);
  const double x0 = xyyaw ? xyyaw[(size_t)b * 3] : 0.0, y0 = xyyaw ? xyyaw[(size_t)b * 3 + 1] : 0.0;
  const double yaw = xyyaw ? xyyaw[(size_t)b * 3 + 2] : 0.0;
  PlantGround G;
  plant_ground_load(T.rows + (size_t)b * 8, T.flags, G);
  const double ground = plant_height(G, x0, y0);
  const double p[3] = {x0, y0, QMPC_PLANT_HEIGHT + ground}, v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
  const double side = (leg & 1) ? 1.0 : -1.0;
  double hip[3], R[9], fw[3];
  plant_hip(leg, hip);
  plant_rot(q, R);
  const double fb[3] = {hip[0], hip[1] + side * QMPC_PLANT_SIDE_OFFSET, -QMPC_PLANT_HEIGHT};
  plant_mul(R, fb, fw);
  double c[3] = {p[0] + fw[0], p[1] + fw[1], 0.0};
  c[2] = plant_height(G, c[0], c[1]);
  G.support = plant_quad_sum(c[2]) / 4.0;
  if (live) {
    for (int k = 0; k < 3; ++k) S.grf[(size_t)tt * 3 + k] = 0.0;
    S.stance[tt] = 1;
    if (leg == 0) {
      T.support[b] = G.support;
      T.ground[b] = ground;
    }
  }
  plant_readout<true>(S, K, tt, live, p, v, q, w, c, true, v /* vdot = 0 */, nullptr, nullptr, nullptr, nullptr, G);
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
