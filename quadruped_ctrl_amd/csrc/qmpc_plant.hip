// qmpc_plant.hip -- the reduced-order plant of include/qmpc_plant.h: one launch per control period, one lane per
// (robot, leg) as in the glue kernels.  The device code is shared with the terrain kernels of qmpc_terrain.hip: the leg
// helpers and the read-out in qmpc_plant_dev.h, the statements of a control period in qmpc_plant_step_body.h; the
// kernels here are the flat plant (TERRAIN = false).  fp contraction is off, as in the glue code: tests/plant_model.py
// restates every expression in the same order.
//
// Decisions the model leaves open (the same list as in include/qmpc_plant.h):
//  * order inside a step: contact edges (touch-down sets c_z = 0) -> `substeps` x [stance forces at the current pose
//    with the torque held -> quad sums -> vdot, wdot -> v, w -> p, q] -> swing feet placed at the new pose -> read-out.
//  * forces: F_body = J^-T tau by cofactors of the fp64 Jacobian at the plant's own angles (IK of the pinned foot);
//    |det J| < QMPC_PLANT_DET_MIN = 1e-5 m^3 (det = l2 l3 sin(knee) rho up to sign: a straight knee) -> f = 0; f_z <= 0
//    -> f = 0; tangential part scaled to mu f_z when larger.  The foot stays pinned whatever the force.
//  * quaternion: q (x) dq with dq from the new body-frame w, exponential map, first-order below |w| h = 1e-12, then
//    normalised.
//  * swing clamp: radial scaling of p_des into |r|^2 in [r2_lo, r2_hi] (knee angle 2.6 .. 0.05 rad); a zero command
//    reads (0, 0, -sqrt(r2_lo)).  IK clamps rho^2 at 0 and D to [-1, 1], so it returns angles for every input.
//  * IK branch: knee >= 0 (qmpc_leg_fk's standing pose); no wrapping of the abad angle (the two atan2 terms cancel
//    near the standing pose).
//  * pinned foot's hip-frame velocity: -rBody v - w x (rBody (c - p)), lever arm from the body origin.
//  * accelerometer: rBody_new (vdot_last + (0, 0, g)).
#include "qmpc_plant_dev.h"

namespace {

// qmpc_plant_init / qmpc_plant_reset (mask == NULL: every robot).  n = batch * 4 lanes.
__global__ __launch_bounds__(256) void qmpc_plant_init_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ xyyaw, const int n) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int b = t >> 2;
  if (mask && !mask[b]) return;
  const double x0 = xyyaw ? xyyaw[(size_t)b * 3] : 0.0, y0 = xyyaw ? xyyaw[(size_t)b * 3 + 1] : 0.0;
  const double yaw = xyyaw ? xyyaw[(size_t)b * 3 + 2] : 0.0;
  const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
  plant_init_lane(S, K, x0, y0, q, t);
}

// One control period on flat ground: qmpc_plant_step_body.h with TERRAIN = false.  <false, false> reads nothing of V
// and is the plain step.
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) void qmpc_plant_step_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const double* __restrict__ effort,
                                                              const float* __restrict__ contact_state,
                                                              const float* __restrict__ p_des,
                                                              const float* __restrict__ v_des, double* state_out,
                                                              double* motor_out, const int n, const QmpcPlantVary V) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = false;
  const QmpcTerrainArgs T{};
  constexpr bool FIELD = false;
  const QmpcFieldArgs Fd{};
#include "qmpc_plant_step_body.h"
}

// qmpc_plant_stats_reset (mask == NULL: every robot): one lane per robot
__global__ __launch_bounds__(256) void qmpc_plant_stats_reset_kernel(const QmpcPlantVary V,
                                                                     const uint8_t* __restrict__ mask, const int batch) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (mask && !mask[b]) return;
  plant_stats_reset_robot(V, b);
}

}  // namespace

extern "C" hipError_t qmpc_launch_plant_init(const QmpcPlantResetArgs* A, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_plant_init_kernel, plant_grid(A->n), dim3(256), 0, stream, A->S, A->K, A->mask, A->xyyaw, A->n);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_plant_step(const QmpcPlantStepArgs* A, int vary, int stats, hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_plant_step_kernel<VARY.value, STATS.value>), plant_grid(A->n), dim3(256), 0, stream, A->S,
                       A->K, A->effort, A->contact_state, A->p_des, A->v_des, A->state_out, A->motor_out, A->n, A->V);
  });
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_plant_stats_reset(const QmpcPlantVary* V, const uint8_t* mask, int batch,
                                                    hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_plant_stats_reset_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, *V, mask, batch);
  return hipGetLastError();
}
