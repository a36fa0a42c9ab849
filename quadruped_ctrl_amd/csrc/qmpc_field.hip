// qmpc_field.hip -- the plant of include/qmpc_plant.h on height-field terrain from memory (include/qmpc_field.h): a bank
// of float maps in device memory, every robot placed on one of them, added to the analytic ground of
// include/qmpc_terrain.h.  The host picks these kernels only while a bank is bound; with none the plant launches the
// kernels of qmpc_plant.hip / qmpc_terrain.hip / qmpc_contact.hip as it always did, with the arguments it always gave.
//
// Nothing here is a step of its own: the scheduled-contact step is the statements of qmpc_plant_step_body.h with
// TERRAIN = FIELD = true, the contact step those of qmpc_contact_step_body.h with FIELD = true, each in the four
// <VARY, STATS> combinations, and the reset is qmpc_terrain.hip's on the summed surface.  The sampler and the per-foot
// normal are qmpc_plant_dev.h's plant_field_*; the index logic is qmpc_field_index.h, which tests/field_index_dump.cpp
// compiles for the CPU.  One lane per (robot, leg): a lane's foot has its own four taps, so the per-foot normal costs no
// shuffle.  The taps are dependent gathers of 4 bytes each from a map that, at the reference's 256 x 256, is 256 KiB and
// lives in L2; the sampler issues the four loads before the first use, and the place row is loaded once per step.
// tests/plant_model_field.py restates every expression in the same order.
#include "qmpc_plant_dev.h"

namespace {

// qmpc_plant_reset while a field is bound (mask == NULL: every robot): qmpc_terrain_init_kernel on the summed surface,
// qmpc_plant_dev.h's plant_ground_init_lane with FIELD.  T.rows may be null (the field alone).  Every lane computes (the
// shuffles need their partners); masked ones store.
__global__ __launch_bounds__(256) void qmpc_field_init_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ xyyaw, const int n,
                                                              const QmpcTerrainArgs T, const QmpcFieldArgs Fd) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool in = t < n;
  const int tt = in ? t : n - 1;
  const int b = tt >> 2;
  const bool live = in && (!mask || mask[b]);
  const double x0 = xyyaw ? xyyaw[(size_t)b * 3] : 0.0, y0 = xyyaw ? xyyaw[(size_t)b * 3 + 1] : 0.0;
  const double yaw = xyyaw ? xyyaw[(size_t)b * 3 + 2] : 0.0;
  const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
  plant_ground_init_lane<true>(S, K, T, Fd, x0, y0, q, tt, live);
}

// One control period with scheduled contact on the summed surface: qmpc_plant_step_body.h with TERRAIN = FIELD = true
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) void qmpc_field_step_kernel(const QmpcPlantDev S, const QmpcPlantConst K,
                                                              const double* __restrict__ effort,
                                                              const float* __restrict__ contact_state,
                                                              const float* __restrict__ p_des,
                                                              const float* __restrict__ v_des, double* state_out,
                                                              double* motor_out, const int n, const QmpcPlantVary V,
                                                              const QmpcTerrainArgs T, const QmpcFieldArgs Fd) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = true;
  constexpr bool FIELD = true;
#include "qmpc_plant_step_body.h"
}

// One control period with contact decided by the summed surface: qmpc_contact_step_body.h with FIELD = true, under the
// launch bounds of qmpc_contact_step_kernel.
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void qmpc_field_contact_step_kernel(
    const QmpcPlantStepArgs A) {
#pragma clang fp contract(off)
  constexpr bool FIELD = true;
  const QmpcFieldArgs& Fd = A.Fd;
  typedef QmpcPlantStepArgs StepArgs;
#include "qmpc_contact_step_body.h"
}

}  // namespace

extern "C" hipError_t qmpc_launch_field_init(const QmpcPlantResetArgs* A, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_field_init_kernel, plant_grid(A->n), dim3(256), 0, stream, A->S, A->K, A->mask, A->xyyaw, A->n,
                     A->T, A->Fd);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_field_step(const QmpcPlantStepArgs* A, int vary, int stats, hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_field_step_kernel<VARY.value, STATS.value>), plant_grid(A->n), dim3(256), 0, stream, A->S,
                       A->K, A->effort, A->contact_state, A->p_des, A->v_des, A->state_out, A->motor_out, A->n, A->V,
                       A->T, A->Fd);
  });
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_field_contact_step(const QmpcPlantStepArgs* A, int vary, int stats,
                                                     hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_field_contact_step_kernel<VARY.value, STATS.value>), plant_grid(A->n), dim3(256), 0, stream,
                       *A);
  });
  return hipGetLastError();
}
