// qmpc_loop.hip -- the fleet's long-running loop between two MPC solves in ONE launch (include/qmpc_loop.h, arguments:
// qmpc_loop.h).  It is the span kernel's loop (qmpc_span.hip: read its head first) with two more stages in a tick:
//
//   E  L  [solve]  C  A  P  R
//
// A (actuators) stands between the leg command and the plant step; R (the episode step and the resets it orders) behind
// the plant step of a check tick.  The thread mapping is the span's, lane t = robot * 4 + leg in workgroups of whole
// waves, so a robot's quad shares a wave and everything a robot's stages hand over stays inside it; the hand-off goes
// through the same global arrays as between the per-tick launches, with a __syncthreads() at the stage boundaries where
// one lane reads what another wrote.  E, L, C, P are the single texts the span kernel and the per-tick kernels include;
// fp contraction is off; no LDS, no scratch.
//
// Stage A is new device code: the per-tick kernel (qmpc_act.hip) gives a robot sixteen lanes, one per joint; here a leg
// lane takes its three joints.  The arithmetic is qmpc_act_model.h's, the ring and the head / age advance are
// qmpc_act.hip's statements.  The accumulators' order is part of the contract (include's actuator header): twelve terms
// in joint order k = 0 .. 11, left to right.  Every lane of the quad takes them through width-4 shuffles -- source lane
// k / 3, component k % 3 -- and the leg-0 lane stores.  A reads the command C wrote in the same lane, the joint rates P
// wrote in the same lane (the plant's own motor rows), and head / age, which the leg-0 lane stored a tick (several
// barriers) ago: no barrier stands between C and A.
//
// Stage R: the decision is qmpc_episode_decide_body.h in the leg-0 lane (every lane reaches its ballot: a wave holds 16
// robots, so the log's rows come in another order than from the per-tick kernel's 64 -- the log is a set).  Behind a
// barrier the robot's lanes do what qmpc_episode_step enqueues behind its decision, under the mask the decision left:
// the controller's reset (leg-0 lane), the commands of EVERY robot from the bound arrays (leg-0 lane), the flat plant's
// reset (four lanes), the statistics' reset, and the actuators' reset.
//
// Two words are fleet-wide.  The log's counter is an atomic, as in the per-tick kernel.  The due list's count (per-robot
// schedule) is reset by the host in front of the launch, as for the span; but the controller's reset of robot b also
// writes due_list[b] and due_count[b], rows of the fleet's list, and another workgroup may already be appending to that
// list in the L stage of the next tick.  Where L stages follow in the launch, the reset therefore writes those two zeros
// into the robot's own due[b] instead (which it zeroes anyway): the count was reset in front of the launch, the next L
// rebuilds the list, and the list's entries past its count are not defined on either path.
//
// A and R are run-time switches, uniform over the grid: as template arguments they would make 24 more instantiations of
// a kernel that takes 10 s to compile, for stages that are short beside L and P.
//
// The ground is a compile-time switch of the FILE (include/qmpc_ground_run.h): the build compiles it three times, as
// qmpc_kernels.hip is compiled once per size class.  QMPC_LOOP_GROUND undefined or 0 is the flat plant, P with TERRAIN =
// FIELD = false and empty T / Fd; 1 is terrain rows (TERRAIN); 2 a height-field bank on any rows (TERRAIN and FIELD,
// T.rows may be null).  The ground compiles take the ground behind the flat block (qmpc_loop.h: QmpcLoopGroundArgs), their
// launcher has its own name, and their stage R stands a reset robot on its ground with the init kernels' own text
// (qmpc_plant_dev.h).  With A and R off they are the fleet run's kernels on ground.
#include "qmpc_plant_dev.h"
#include "qmpc_ctrl_stages.h"
#include "qmpc_act_model.h"
#include "qmpc_episode_rule.h"
#include "qmpc_loop.h"

#ifndef QMPC_LOOP_GROUND
#define QMPC_LOOP_GROUND 0
#endif
#if QMPC_LOOP_GROUND == 0
#define QMPC_LOOP_LAUNCHER qmpc_launch_loop
typedef QmpcLoopArgs LoopArgs;
#elif QMPC_LOOP_GROUND == 1
#define QMPC_LOOP_LAUNCHER qmpc_launch_loop_terrain
typedef QmpcLoopGroundArgs LoopArgs;
#elif QMPC_LOOP_GROUND == 2
#define QMPC_LOOP_LAUNCHER qmpc_launch_loop_field
typedef QmpcLoopGroundArgs LoopArgs;
#else
#error "QMPC_LOOP_GROUND: 0 (flat), 1 (terrain rows) or 2 (height field)"
#endif

// Lanes per workgroup: the span's choice
#ifndef QMPC_LOOP_WG
#define QMPC_LOOP_WG 64
#endif
static_assert(QMPC_LOOP_WG % 64 == 0 && QMPC_LOOP_WG >= 64 && QMPC_LOOP_WG <= 1024, "whole waves: a robot's quad shares one");
#define QMPC_PLANT_STEP_LANE (blockIdx.x * QMPC_LOOP_WG + threadIdx.x)

namespace {

// Stage A for lane t = robot * 4 + leg; every lane of the wave calls it (shuffles), the lanes past n compute on zeros and
// store nothing.
__device__ __forceinline__ void qmpc_loop_act_body(const QmpcActArgs& A, double* effort, const int t, const bool alive,
                                                   const int batch) {
#pragma clang fp contract(off)
  const int b = t >> 2, leg = t & 3;
  const int D = A.cfg.max_delay;
  int head = 0, age = 0;
  if (alive) {
    head = A.d.head[b];
    age = A.d.age[b];
  }
  // (the state is this library's own; a row index is still never taken on trust)
  if ((unsigned)head > (unsigned)D) head = 0;
  if ((unsigned)age > (unsigned)D) age = D;
  const size_t at = (size_t)t * 3, row_stride = (size_t)batch * 12;
  double cmd[3] = {0.0, 0.0, 0.0}, qd[3] = {0.0, 0.0, 0.0};
  QmpcActMotor M;
  M.kt = A.cfg.kt;
  M.R = A.cfg.R;
  M.V = A.cfg.battery_v;
  M.tmax = A.cfg.tau_max;
  M.damp = A.cfg.damping;
  M.dry = A.cfg.dry_friction;
  M.has_strength = A.strength != nullptr;
  M.strength = 1.0;
  M.friction = A.cfg.friction;
  if (alive) {
    const int row = qmpc_act_row(head, age, A.delay ? A.delay[b] : 0, D);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double e = effort[at + j];
      A.ring[(size_t)head * row_stride + at + j] = e;
      cmd[j] = row == head ? e : A.ring[(size_t)row * row_stride + at + j];
      qd[j] = A.motor[(size_t)b * 24 + 12 + 3 * leg + j];
    }
    if (A.battery_v) M.V = A.battery_v[b];
    if (A.tau_max) M.tmax = A.tau_max[b];
    if (A.damping) M.damp = A.damping[b];
    if (A.dry_friction) M.dry = A.dry_friction[b];
    if (A.strength) M.strength = A.strength[b];
  }
  QmpcActJoint J[3];
  int n_vsat = 0, n_tsat = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    J[j] = qmpc_act_joint(M, A.cfg.gear[j], cmd[j], qd[j]);
    if (alive) effort[at + j] = J[j].tau;
    n_vsat += J[j].vsat;
    n_tsat += J[j].tsat;
  }
  n_vsat = contact_quad_count(n_vsat);
  n_tsat = contact_quad_count(n_tsat);
  const bool store = alive && leg == 0;
  QmpcActSums S{store ? A.d.tau_peak[b] : 0.0, 0.0, 0.0, 0.0};
  qmpc_act_sums_quad(S, J, [](double x, int src, int) { return __shfl(x, src, 4); });
  if (!store) return;
  A.d.head[b] = qmpc_act_next_head(head, D);
  A.d.age[b] = qmpc_act_next_age(age, D);
  A.d.n[b] = A.d.n[b] + 1;
  A.d.n_vsat[b] = A.d.n_vsat[b] + n_vsat;
  A.d.n_tsat[b] = A.d.n_tsat[b] + n_tsat;
  A.d.tau_peak[b] = S.peak;
  A.d.e_heat[b] = qmpc_act_energy(A.d.e_heat[b], A.dt, S.heat);
  A.d.e_mech[b] = qmpc_act_energy(A.d.e_mech[b], A.dt, S.mech);
  A.d.e_pos[b] = qmpc_act_energy(A.d.e_pos[b], A.dt, S.pos);
}

// The argument block is the kernel's first parameter: it IS the head of the kernarg segment.  Stages A and R read their
// part of it there AGAIN, through a pointer the compiler cannot see through: left to itself it hoists every pointer of
// the block out of the tick loop into scalar registers, four hundred of which then spill into vector registers and
// push the plant step into scratch (qmpc_contact.hip reads its store pointers a second time for the same reason).
// R, which writes some seventy arrays, reads it through a pointer in a VECTOR register: the array pointers then come by
// vector loads, into the registers the stores address with, and take no scalar register at all.
#define QMPC_LOOP_ARGS_AGAIN(name, reg)                                             \
  typedef const __attribute__((address_space(4))) LoopArgs* KernargPtr_##name;      \
  KernargPtr_##name again_##name = (KernargPtr_##name)__builtin_amdgcn_kernarg_segment_ptr(); \
  asm volatile("" : reg(again_##name));                                             \
  const LoopArgs& name = *(const LoopArgs*)again_##name

template <int MODE, bool VARY, bool STATS>
__global__ __launch_bounds__(QMPC_LOOP_WG) void qmpc_loop_kernel(const LoopArgs W, const int first_at_c, const int ticks,
                                                                 const int last_after_l, const int tick0,
                                                                 const int t_mod13) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = QMPC_LOOP_GROUND >= 1;
  constexpr bool FIELD = QMPC_LOOP_GROUND == 2;
#if !QMPC_LOOP_GROUND
  const QmpcTerrainArgs T{};
  const QmpcFieldArgs Fd{};
#endif
  // the span's names (qmpc_span.hip)
  const QmpcCtrlDev& Cd = W.X.C;
  const QmpcLegGeom& g = W.X.g;
  const QmpcPlantDev& S = W.X.S;
  const QmpcPlantConst& K = W.X.K;
  const QmpcPlantVary& V = W.X.V;
  double* const effort = W.X.effort;
  double* const state_out = W.X.state;
  double* const motor_out = W.X.motor;
  const int n = W.X.n;
  const int build_list = W.X.build_list;
  const float* contact_state = Cd.contact_state;
  const float* p_des = Cd.p_des;
  const float* v_des = Cd.v_des;
  const int lane_t = QMPC_PLANT_STEP_LANE;  // robot * 4 + leg
  const bool alive = lane_t < n;
  const int robot = lane_t >> 2;
  int locos = 0;  // L stages run so far: T of the current tick is T of the launch + locos
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
      ++locos;
      __syncthreads();
      if (i == ticks - 1 && last_after_l) break;
    }
    if (alive) qmpc_ctrl_legcmd_body(Cd, effort, lane_t);
    if (W.act) {
      QMPC_LOOP_ARGS_AGAIN(Wa, "+s");
      int lane_a = lane_t;
      asm volatile("" : "+v"(lane_a));
      qmpc_loop_act_body(Wa.A, effort, lane_a, alive, n >> 2);
    }
    __syncthreads();
    {
#if QMPC_LOOP_GROUND
      // (the ground's pointers are read again too: nothing of T or Fd is carried around the tick loop)
      QMPC_LOOP_ARGS_AGAIN(Wp, "+s");
      const QmpcTerrainArgs& T = Wp.T;
      const QmpcFieldArgs& Fd = Wp.Fd;
#endif
#include "qmpc_plant_step_body.h"
    }
    __syncthreads();
    if (W.every && (tick0 + i + 1) % W.every == 0) {
      QMPC_LOOP_ARGS_AGAIN(Wr, "+v");
      // (... and its lane index: the addresses of the sixty arrays a reset writes are not carried around the loop either)
      int lane_r = lane_t;
      asm volatile("" : "+v"(lane_r));
      const int robot_r = lane_r >> 2;
      const bool leg0 = alive && (lane_r & 3) == 0;
      if (W.decide) {
        {
          const QmpcEpisodeDev& S = Wr.E;  // (the text's names)
          const QmpcEpisodeIn& In = Wr.In;
          const qmpc_episode_rule& R = Wr.R;
          const qmpc_episode_bind& Bd = Wr.Bd;
          const int elapsed = W.every;
          const int b = robot_r;
          const bool judge = leg0;
#include "qmpc_episode_decide_body.h"
        }
        __syncthreads();  // mask, xyyaw, the commands: the leg-0 lane's stores, read by the quad
        const bool hit = alive && Wr.E.mask[robot_r] != 0;
        if (leg0) {
          if (hit) {
            // lockstep: T mod 13 of this tick, so that the robot keeps solving with the batch; per robot: 0
            const bool later = i + 1 < ticks;  // L stages follow in this launch (see the head of the file)
            QmpcCtrlDev Cr = Wr.X.C;
            if (build_list && later) Cr.due_list = Cr.due_count = Cr.due;
            qmpc_ctrl_init_robot<true>(Cr, robot_r, build_list ? 0 : (t_mod13 + locos) % 13);
          }
          qmpc_ctrl_set_robot(Wr.X.C, Wr.Bd.gait, Wr.Bd.vel, robot_r);
        }
        if (hit) {  // (the plant's reset kernel on this ground: the robot's row of the manager's xyyaw)
          const double* row = Wr.E.xyyaw + (size_t)robot_r * 3;
          const double yaw = row[2];
          const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};
#if QMPC_LOOP_GROUND
          // (hit is the robot's: a quad is in here whole, so the reset's shuffles have their partners)
          plant_ground_init_lane<FIELD>(Wr.X.S, Wr.X.K, Wr.T, Wr.Fd, row[0], row[1], q, lane_r, true);
#else
          plant_init_lane(Wr.X.S, Wr.X.K, row[0], row[1], q, lane_r);
#endif
        }
        if constexpr (STATS) {
          if (hit && leg0) plant_stats_reset_robot(Wr.X.V, robot_r);
        }
      }
      if (W.act && leg0 && Wr.E.mask[robot_r] != 0) qmpc_act_reset_robot(Wr.A.d, robot_r, W.act_stats);
      __syncthreads();
    }
  }
}
#undef QMPC_LOOP_ARGS_AGAIN

template <int MODE>
hipError_t launch_mode(const LoopArgs* A, int vary, int stats, int first_at_c, int ticks, int last_after_l, int tick0,
                       int t_mod13, hipStream_t stream) {
  plant_vary_stats(vary, stats, [&](auto VARY, auto STATS) {
    hipLaunchKernelGGL((qmpc_loop_kernel<MODE, VARY.value, STATS.value>), dim3((A->X.n + QMPC_LOOP_WG - 1) / QMPC_LOOP_WG),
                       dim3(QMPC_LOOP_WG), 0, stream, *A, first_at_c, ticks, last_after_l, tick0, t_mod13);
  });
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t QMPC_LOOP_LAUNCHER(const LoopArgs* A, int robot_mode, int vary, int stats, int first_at_c,
                                         int ticks, int last_after_l, int tick0, int t_mod13, hipStream_t stream) {
  return robot_mode == 1 ? launch_mode<1>(A, vary, stats, first_at_c, ticks, last_after_l, tick0, t_mod13, stream)
                         : launch_mode<0>(A, vary, stats, first_at_c, ticks, last_after_l, tick0, t_mod13, stream);
}
