// qmpc_contact.hip -- the plant of include/qmpc_plant.h with contact decided by the ground (include/qmpc_contact.h):
// early and late touch-down and slipping feet, on the per-robot terrain of include/qmpc_terrain.h or, with no rows bound,
// on flat ground.  The host picks these kernels only while contact flags are set; with the flags 0 the plant launches
// the kernels of qmpc_plant.hip / qmpc_terrain.hip as it always did.
//
// Same shape as the other step kernels and the same helpers (qmpc_plant_dev.h): one lane per (robot, leg); the lanes past
// n in the last wave repeat lane n - 1 and store nothing, so that every shuffle has its partner; every lane of a quad
// integrates its robot's body redundantly; quad sums through two xor-shuffles; no LDS, no atomics.  The step is a body
// of its own and not qmpc_plant_step_body.h with one more switch: the flat and the terrain steps keep their registers
// (tests/test_plant_varied_cpu.py, tests/test_terrain_cpu.py), and here the pinned flag, not the schedule, decides what a
// foot does.  Its statements are qmpc_contact_step_body.h, text like the other body, which qmpc_field.hip includes a
// second time for the height field of include/qmpc_field.h (FIELD = true); here FIELD is false and nothing of the field
// is read.  tests/plant_model_contact.py restates every expression in the same order.
#include "qmpc_plant_dev.h"

namespace {

// qmpc_plant_reset while contact is on, before the ground's own reset kernel (mask == NULL: every robot): the masked
// robots' counters and drop are zeroed; with no terrain bound so are support and ground, which the flat reset does not
// know and the field's reset writes afterwards.  n = batch * 4 lanes, one per (robot, leg).
__global__ __launch_bounds__(256) void qmpc_contact_reset_kernel(const uint8_t* __restrict__ mask, const int n,
                                                                 const QmpcTerrainArgs T, const QmpcContactArgs C) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int b = t >> 2;
  if (mask && !mask[b]) return;
  C.drop[t] = 0.0;
  if ((t & 3) != 0) return;
  C.early[b] = 0;
  C.late[b] = 0;
  C.slip[b] = 0.0;
  if (!T.rows) {
    T.support[b] = 0.0;
    T.ground[b] = 0.0;
  }
}

// One control period with contact decided by the ground.  The arguments are one struct by value, qmpc_plant.h's
// QmpcPlantStepArgs: it IS the kernarg segment, so the kernel can read it a second time (its last member, the field's
// arguments, is kernarg bytes this kernel never loads).  The step holds the registers of the terrain step plus the
// sliding velocity, the drop and the counters: one wave per SIMD, which a launch of this size (bound by its launch gap)
// does not feel.  The two dozen pointers that only the stores at the end need would sit in scalar registers through
// the whole step and push others out; they are read from the kernarg segment again behind the arithmetic instead (the
// empty asm keeps the compiler from hoisting those loads to the top).
template <bool VARY, bool STATS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void qmpc_contact_step_kernel(
    const QmpcPlantStepArgs A) {
#pragma clang fp contract(off)
  constexpr bool FIELD = false;
  const QmpcFieldArgs Fd{};
  typedef QmpcPlantStepArgs StepArgs;
#include "qmpc_contact_step_body.h"
}

}  // namespace

extern "C" hipError_t qmpc_launch_contact_reset(const uint8_t* mask, int batch, hipStream_t stream,
                                                const QmpcTerrainArgs* T, const QmpcContactArgs* C) {
  const int n = batch * 4;
  hipLaunchKernelGGL(qmpc_contact_reset_kernel, plant_grid(n), dim3(256), 0, stream, mask, n, *T, *C);
  return hipGetLastError();
}

extern "C" hipError_t qmpc_launch_contact_step(const QmpcPlantStepArgs* A, int vary, int stats, hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_contact_step_kernel<VARY.value, STATS.value>), plant_grid(A->n), dim3(256), 0, stream, *A);
  });
  return hipGetLastError();
}
