// qmpc_span.hip -- the closed loop between two MPC solves in ONE launch (include/qmpc_fleet.h, plan: qmpc_span.h).
//
// A tick is  E (cheater estimators + leg data)  L (safety + locomotion)  [solve]  C (leg command)  P (plant step); the
// per-tick path enqueues E, L, C (qmpc_glue.hip) and P (qmpc_plant.hip) one launch each: four dispatches and their gaps
// a tick, around stages that are one dependent chain per lane.  Nothing in E, L, C, P couples two robots, so the span
// kernel loops over the ticks: C, P of the tick that has just solved (first_at_c), then E, L, C, P of every following
// tick, up to E, L of the next tick that solves (last_after_l).  (Measured: INTEGRATION.md section G -- 23 us a tick
// against 37 to 39; L and P themselves are 18 and 12 us of kernel time on the per-tick path.)
//
// The stage code is the per-tick kernels' own: E and C are the bodies of qmpc_ctrl_stages.h, L is qmpc_ctrl_loco_body.h
// and P is qmpc_plant_step_body.h as text with TERRAIN = FIELD = false -- the same expressions in the same order, fp contraction
// off, so a fused run leaves the bits of the per-tick run in every array.
//
// Thread mapping: lane t = robot * 4 + leg, as in those kernels; L runs in the leg-0 lane of its robot.  A workgroup is
// QMPC_SPAN_WG lanes, a multiple of the wave, so a robot's four lanes always share a wave (the plant's quad sums are
// shuffles) and EVERYTHING a robot's stages hand over stays inside that wave: E's leg rows and state estimate to L, L's
// command rows to C and P, C's effort to P, P's state and motor rows to the next E.  The hand-off goes through the same
// global arrays as between the per-tick launches; each stage boundary is a __syncthreads(), i.e. a workgroup-scope
// release fence, the barrier, and a workgroup-scope acquire fence, which is what the AMDGPU memory model asks for between
// a plain store of one lane and a plain load of another lane of the same workgroup.  No lane leaves before the last
// barrier: lanes past n run no E, L, C and are P's stand-ins for lane n - 1 (qmpc_plant_step_body.h), storing nothing.
//
// The one fleet-wide word, the due list's count (per-robot schedule), is NOT reset here: workgroups run at their own pace,
// and one workgroup's L could append before another's reset landed.  The host resets it in front of the launch
// (qmpc_span.h: reset_due); L appends as in the per-tick kernel.  The order of the list is undefined there and here.
#include "qmpc_plant_dev.h"
#include "qmpc_ctrl_stages.h"
#include "qmpc_span.h"

// Lanes per workgroup.  64 and 256 were measured against each other on an MI355X: the loop is
// latency-bound, and the smaller workgroup spreads a small fleet over more CUs.
#ifndef QMPC_SPAN_WG
#define QMPC_SPAN_WG 64
#endif
static_assert(QMPC_SPAN_WG % 64 == 0 && QMPC_SPAN_WG >= 64 && QMPC_SPAN_WG <= 1024, "whole waves: a robot's quad shares one");
#define QMPC_PLANT_STEP_LANE (blockIdx.x * QMPC_SPAN_WG + threadIdx.x)

namespace {

template <int MODE, bool VARY, bool STATS>
__global__ __launch_bounds__(QMPC_SPAN_WG) void qmpc_span_kernel(const QmpcCtrlDev Cd, const QmpcLegGeom g,
                                                                 const QmpcPlantDev S, const QmpcPlantConst K,
                                                                 double* effort, double* state_out, double* motor_out,
                                                                 const int n, const QmpcPlantVary V, const int build_list,
                                                                 const int first_at_c, const int ticks,
                                                                 const int last_after_l) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = false;
  const QmpcTerrainArgs T{};
  constexpr bool FIELD = false;
  const QmpcFieldArgs Fd{};
  // what P reads of the controller (qmpc_capi_plant.cpp: plant_step_args)
  const float* contact_state = Cd.contact_state;
  const float* p_des = Cd.p_des;
  const float* v_des = Cd.v_des;
  const int lane_t = QMPC_PLANT_STEP_LANE;  // robot * 4 + leg
  const bool alive = lane_t < n;
  const int robot = lane_t >> 2;
  for (int i = 0; i < ticks; ++i) {  // (every condition on i and the arguments is uniform over the grid)
    if (i > 0 || !first_at_c) {
      if (alive) qmpc_ctrl_est_state_body(Cd, g, state_out, motor_out, lane_t);
      __syncthreads();
      bool due = false;
      if (alive && (lane_t & 3) == 0) {
        const QmpcCtrlDev& S = Cd;  // (the text's names; the plant's S is out of sight in here)
        const int b = robot;
        bool& span_due = due;
        {
#include "qmpc_ctrl_loco_body.h"
          span_due = due;
        }
      }
      if (build_list) qmpc_ctrl_due_append(Cd, robot, due);
      __syncthreads();
      if (i == ticks - 1 && last_after_l) break;
    }
    if (alive) qmpc_ctrl_legcmd_body(Cd, effort, lane_t);
    __syncthreads();
    {
#include "qmpc_plant_step_body.h"
    }
    __syncthreads();
  }
}

template <int MODE>
hipError_t launch_mode(const QmpcSpanArgs* A, int vary, int stats, int first_at_c, int ticks, int last_after_l,
                       hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_span_kernel<MODE, VARY.value, STATS.value>), dim3((A->n + QMPC_SPAN_WG - 1) / QMPC_SPAN_WG),
                       dim3(QMPC_SPAN_WG), 0, stream, A->C, A->g, A->S, A->K, A->effort, A->state, A->motor, A->n, A->V,
                       A->build_list, first_at_c, ticks, last_after_l);
  });
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t qmpc_launch_span(const QmpcSpanArgs* A, int robot_mode, int vary, int stats, int first_at_c,
                                       int ticks, int last_after_l, hipStream_t stream) {
  return robot_mode == 1 ? launch_mode<1>(A, vary, stats, first_at_c, ticks, last_after_l, stream)
                         : launch_mode<0>(A, vary, stats, first_at_c, ticks, last_after_l, stream);
}
