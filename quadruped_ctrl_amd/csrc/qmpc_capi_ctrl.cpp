// qmpc_capi_ctrl.cpp -- host side of include/qmpc_ctrl.h (the batched locomotion controller; the kernels are in
// qmpc_glue.hip), of include/qmpc_fleet.h (the closed loop of controller and plant; the kernel is in qmpc_span.hip) and of
// include/qmpc_loop.h (that loop with the actuators and the episode manager inside the launch; qmpc_loop.hip), with the
// switch of include/qmpc_ground_run.h (both on terrain rows and height fields: qmpc_loop.hip's ground compiles).
#include <cstring>

#include "../../include/qmpc_debug.h"  // qmpc_debug_ctrl_read
#include "../../include/qmpc_plant.h"  // qmpc_plant_step: the fleet run's fallback is the per-tick calls themselves
#include "../../include/qmpc_act.h"    // ... and the loop run's: qmpc_act, qmpc_act_reset
#include "../../include/qmpc_ground_run.h"  // the switch that lets both run calls serve rows and a field fused
#include "qmpc_host.h"
#include "qmpc_span.h"      // the fleet run's plan (host-only) and the span kernel's launcher
#include "qmpc_loop.h"      // the loop kernel's argument blocks and launchers
#include "qmpc_run_pick.h"  // which of them serves a call (host-only)
using namespace qmpc_host;

size_t qmpc_host::carve(QmpcCtrlDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_CTRL_ARRAYS(QMPC_CARVE)
  return off;
}

// Where a reset robot's counter restarts (qmpc_ctrl_reset, and both episode managers'): in lockstep at T mod 13 (the
// batch keeps solving on the same ticks), with the per-robot schedule at 0, as init_controller leaves it.  A reset
// starts the controller (qmpc_ctrl_set_schedule's window closes).
int qmpc_host::ctrl_reset_counter0(qmpc_ctx::Ctrl* k) {
  k->started = true;
  return k->schedule == QMPC_CTRL_PER_ROBOT ? 0 : (int)(k->ticks % 13);
}

// The controller's reset of the masked robots (qmpc_ctrl_reset, and the episode manager's).
int qmpc_host::ctrl_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, hipStream_t stream) {
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const int counter0 = ctrl_reset_counter0(k);
  HIP_TRY(c, qmpc_launch_ctrl_init(&k->d, mask_dev, counter0, batch, stream));
  return QMPC_OK;
}

namespace {

int ctrl_check(qmpc_ctx* c, int batch) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->ctrl->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

// The solve of an MPC tick, behind the locomotion stage that wrote the command rows (and, with the per-robot schedule, the
// list of due robots): the per-tick path's and the fleet run's.  This and ctrl_after_prework are called as qmpc_host.h's
// *_enqueue are: with the DeviceGuard held and the stream ordered.
int ctrl_solve_enqueue(qmpc_ctx* c, int batch, hipStream_t stream) {
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const QmpcCtrlDev& d = k->d;
  const bool per_robot = k->schedule == QMPC_CTRL_PER_ROBOT;
  const bool aio = k->robot_mode == 1;  // (per_robot holds: qmpc_ctrl_set_robot_mode)
  qmpc_command cmd{};
  cmd.position = d.position;
  cmd.v_world = d.v_world;
  cmd.omega_world = d.omega_world;
  cmd.orientation = d.orientation;
  cmd.rpy = d.rpy;
  cmd.r_body = d.r_cmd;
  cmd.p_foot = d.p_foot;
  cmd.vel_des = d.vel_des;
  cmd.yaw_des_true = d.yaw_des_true;
  cmd.rpy_comp = d.rpy_comp;
  cmd.stand_traj = d.stand_traj;
  cmd.rp_des = nullptr;  // _roll_des = _pitch_des = 0 (:112-113)
  cmd.gait_type = d.current_gait;
  // robot mode 1: the ten rows the horizon-10 solve reads of the robot's own table, as a 10-segment gait (qmpc_glue.hip:
  // qmpc_ctrl_window_gait); gait_type is 9 for every due robot there
  cmd.gait_offsets = aio ? d.mpc_offsets : d.offsets;
  cmd.gait_durations = aio ? d.mpc_durations : d.durations;
  cmd.gait_iteration = d.iteration;
  cmd.world_position_desired = d.wpd;
  cmd.x_comp_integral = d.xci;
  cmd.body_height = 0.25f;  // _SetupCommand (:79)
  cmd.omni_mode = 0;        // per robot through r_cmd
  qmpc_outputs out{d.grf, nullptr, d.status, nullptr};
  return solve_impl(c, batch, nullptr, &cmd, &out, nullptr, stream, per_robot ? d.due_list : nullptr,
                    per_robot ? d.due_count : nullptr);
}

// A tick after its pre_work, whichever estimators that ran: the locomotion kernel, the solve by the handle's schedule, the
// leg commands.
int ctrl_after_prework(qmpc_ctx* c, int batch, double* effort, hipStream_t stream) {
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const QmpcCtrlDev& d = k->d;
  const bool per_robot = k->schedule == QMPC_CTRL_PER_ROBOT;
  const bool aio = k->robot_mode == 1;  // (per_robot holds: qmpc_ctrl_set_robot_mode)
  if (aio) HIP_TRY(c, qmpc_launch_ctrl_loco_aio(&d, batch, stream));
  else HIP_TRY(c, qmpc_launch_ctrl_loco(&d, batch, per_robot ? 1 : 0, stream));
  // the locomotion kernel advances every robot's counter: T follows it here, before the launches that can still fail,
  // so that the host's MPC schedule and the device's `counter % 13` test never disagree
  // lockstep: every robot's incremented counter is a multiple of 13 on the same ticks, known from T alone.
  // per-robot schedule: nothing depends on T -- every tick enqueues the solve over the list of due robots the locomotion
  // kernel has just built (d.due_list, d.due_count[0]); a tick on which nobody is due costs launches that find no entry
  const bool mpc_tick = (++k->ticks % 13 == 0) || per_robot;
  if (mpc_tick)
    if (const int rc = ctrl_solve_enqueue(c, batch, stream)) return rc;
  HIP_TRY(c, qmpc_launch_ctrl_legcmd(&d, effort, batch, stream));
  return QMPC_OK;
}

// The one body of qmpc_ctrl_prework / _tick and their _state pair: pre_work through the estimator launch `est`, then, when
// `tick`, the rest of the tick.
//   qmpc_launch_ctrl_est (in = imu): orientation estimator + leg data, then the Kalman filter (previous tick's leg data and
//   contact phase);  qmpc_launch_ctrl_est_state (in = simulator ground truth): the cheater estimators + leg data in one
//   launch, no filter
using EstLaunch = hipError_t (*)(const QmpcCtrlDev*, const float*, const double*, const double*, int, hipStream_t);
int ctrl_tick(qmpc_ctx* c, int batch, EstLaunch est, const double* in, const double* motor, double* effort, bool tick,
              void* stream_) {
  if (const int rc = ctrl_check(c, batch)) return rc;
  if (!in || !motor || (tick && !effort)) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  if (tick) c->ctrl->started = true;
  const QmpcCtrlDev& d = c->ctrl->d;
  HIP_TRY(c, est(&d, c->leg_geom, in, motor, batch, q.stream));
  if (est == qmpc_launch_ctrl_est) {
    qmpc_kf_state st{d.xhat, d.P, d.r_body, d.a_world, d.omega_body, d.contact_phase, d.kf_p, d.kf_v,
                     d.position, d.v_world, d.v_body};
    HIP_TRY(c, qmpc_launch_kf(&st, kAbadLocation, batch, q.stream));
  }
  return tick ? ctrl_after_prework(c, batch, effort, q.stream) : QMPC_OK;
}

}  // namespace

extern "C" {

int qmpc_ctrl_init(qmpc_handle c, int batch, double freq, const double pid[4], void* stream_) {
  if (!c || !pid || batch <= 0 || batch > c->max_batch || !(freq > 0) || c->max_horizon < 14) return QMPC_ERR_ARG;
  // ConvexMPCLocomotion(1.0 / freq, 13): float dt, dtMPC = dt * iterationsBetweenMPC (:23-42); setup_problem(dtMPC, 14,
  // 0.4, 120) (:629-630)
  const float dt = (float)(1.0 / freq);
  const float dt_mpc = dt * 13;
  if (const int rc = qmpc_setup(c, (double)dt_mpc, 14, 0.4, 120.0)) return rc;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::Ctrl* k = made(c->ctrl);
  HIP_TRY(c, carve_block(k->buf, k->d, c->max_batch));
  k->d.dt = dt;
  k->d.dt_mpc = dt_mpc;
  k->d.kp_joint = (float)pid[2];  // Vec4<float> ctrlParam (GaitCtrller.cpp:14-16)
  k->d.kd_joint = (float)pid[3];
  if (const int rc = order_after_previous(c, stream)) return rc;
  HIP_TRY(c, qmpc_launch_ctrl_init(&k->d, nullptr, 0, batch, stream));
  k->batch = batch;
  k->freq = freq;
  k->ticks = 0;
  k->schedule = QMPC_CTRL_LOCKSTEP;
  k->robot_mode = 0;
  k->started = false;
  k->fleet = qmpc_fleet_info{};
  k->loop = qmpc_loop_info{};
  k->ground_run = false;
  return QMPC_OK;
}

int qmpc_ctrl_reset(qmpc_handle c, int batch, const uint8_t* mask_dev, void* stream_) {
  if (const int rc = ctrl_check(c, batch)) return rc;
  if (!mask_dev) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  return ctrl_reset_enqueue(c, batch, mask_dev, q.stream);
}

int qmpc_ctrl_set_schedule(qmpc_handle c, int mode) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (mode != QMPC_CTRL_LOCKSTEP && mode != QMPC_CTRL_PER_ROBOT) return QMPC_ERR_ARG;
  if (c->ctrl->started) return QMPC_ERR_STATE;
  if (mode == QMPC_CTRL_LOCKSTEP && c->ctrl->robot_mode == 1) {
    c->err = "robot mode 1 needs the per-robot schedule (select robot mode 0 first)";
    return QMPC_ERR_STATE;
  }
  c->ctrl->schedule = mode;
  return QMPC_OK;
}

int qmpc_ctrl_set_robot_mode(qmpc_handle c, int mode) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (mode != 0 && mode != 1) return QMPC_ERR_ARG;
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  if (k->started) return QMPC_ERR_STATE;
  if (mode == 1 && k->schedule != QMPC_CTRL_PER_ROBOT) {
    // a robot's counter restarts whenever its gait is re-timed (ConvexMPCLocomotion.cpp:182-224): no common MPC tick
    c->err = "robot mode 1 needs the per-robot schedule: the handle is in lockstep (qmpc_ctrl_set_schedule first)";
    return QMPC_ERR_STATE;
  }
  // every solve of mode 1 runs at horizonLength 10 (:174, :233), mode 0 at 14: setup_problem(dtMPC,
  // horizonLength, 0.4, 120) (:629-630).  Host work and a table upload; nothing is enqueued
  if (const int rc = qmpc_setup(c, (double)k->d.dt_mpc, mode == 1 ? 10 : 14, 0.4, 120.0)) return rc;
  k->robot_mode = mode;
  return QMPC_OK;
}

int qmpc_ctrl_set_gait(qmpc_handle c, int batch, const int32_t* gait_dev, void* stream_) {
  if (const int rc = ctrl_check(c, batch)) return rc;
  if (!gait_dev) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_ctrl_set(&c->ctrl->d, gait_dev, nullptr, batch, q.stream));
  return QMPC_OK;
}

int qmpc_ctrl_set_vel(qmpc_handle c, int batch, const double* vel_dev, void* stream_) {
  if (const int rc = ctrl_check(c, batch)) return rc;
  if (!vel_dev) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_ctrl_set(&c->ctrl->d, nullptr, vel_dev, batch, q.stream));
  return QMPC_OK;
}

int qmpc_ctrl_prework(qmpc_handle c, int batch, const double* imu, const double* motor, void* stream) {
  return ctrl_tick(c, batch, qmpc_launch_ctrl_est, imu, motor, nullptr, false, stream);
}

int qmpc_ctrl_tick(qmpc_handle c, int batch, const double* imu, const double* motor, double* effort, void* stream) {
  return ctrl_tick(c, batch, qmpc_launch_ctrl_est, imu, motor, effort, true, stream);
}

int qmpc_ctrl_prework_state(qmpc_handle c, int batch, const double* state, const double* motor, void* stream) {
  return ctrl_tick(c, batch, qmpc_launch_ctrl_est_state, state, motor, nullptr, false, stream);
}

int qmpc_ctrl_tick_state(qmpc_handle c, int batch, const double* state, const double* motor, double* effort,
                         void* stream) {
  return ctrl_tick(c, batch, qmpc_launch_ctrl_est_state, state, motor, effort, true, stream);
}

int qmpc_debug_ctrl_read(qmpc_handle c, const char* name, void* dst, long long cap_bytes, int* per_robot) {
  if (!c || !name || !dst) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  const QmpcCtrlDev& d = c->ctrl->d;
  struct Arr {
    const char* n;
    const void* p;
    int per;
  };
#define QMPC_CTRL_ENTRY(T, name, per_robot) {#name, d.name, per_robot},
  const Arr tab[] = {QMPC_CTRL_ARRAYS(QMPC_CTRL_ENTRY)};
#undef QMPC_CTRL_ENTRY
  for (const Arr& a : tab) {
    if (std::strcmp(a.n, name) != 0) continue;
    const size_t bytes = (size_t)4 * a.per * (size_t)c->ctrl->batch;
    if (per_robot) *per_robot = a.per;
    if (cap_bytes < 0 || (size_t)cap_bytes < bytes) return QMPC_ERR_ARG;
    DeviceGuard g(c->device);
    if (c->has_last) HIP_TRY(c, hipStreamSynchronize(c->last_stream));
    HIP_TRY(c, hipMemcpy(dst, a.p, bytes, hipMemcpyDefault));
    return QMPC_OK;
  }
  return QMPC_ERR_ARG;
}

int qmpc_ctrl_view_get(qmpc_handle c, qmpc_ctrl_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  const QmpcCtrlDev& d = c->ctrl->d;
  v->position = d.position;
  v->v_world = d.v_world;
  v->orientation = d.orientation;
  v->rpy = d.rpy;
  v->r_body = d.r_body;
  v->omega_world = d.omega_world;
  v->leg_q = d.q;
  v->leg_p = d.leg_p;
  v->leg_v = d.leg_v;
  v->leg_J = d.leg_J;
  v->contact_state = d.contact_state;
  v->swing_state = d.swing_state;
  v->p_des = d.p_des;
  v->v_des = d.v_des;
  v->f_ff = d.f_ff;
  v->safe = d.safe;
  v->counter = d.counter;
  v->batch = c->ctrl->batch;
  v->ticks = (int)c->ctrl->ticks;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// The fused launches behind both run calls.  Which kernel serves a call, and what its `reason` says, is qmpc_run_pick.h's
// pure function of the handle's switch (include/qmpc_ground_run.h), what is bound and the call's options.
namespace {

static_assert(QMPC_RUN_REASON_TERRAIN == QMPC_FLEET_TERRAIN && QMPC_RUN_REASON_CONTACT == QMPC_FLEET_CONTACT &&
                  QMPC_RUN_REASON_FIELD == QMPC_FLEET_FIELD && QMPC_RUN_REASON_TERRAIN == QMPC_LOOP_TERRAIN &&
                  QMPC_RUN_REASON_CONTACT == QMPC_LOOP_CONTACT && QMPC_RUN_REASON_FIELD == QMPC_LOOP_FIELD,
              "qmpc_run_pick.h's reason bits are both headers'");

QmpcRunPick run_pick(const qmpc_ctx* c, bool actuators, bool episodes) {
  const qmpc_ctx::Plant* pl = c->plant.get();
  return qmpc_run_pick(c->ctrl->ground_run, pl->terrain.rows != nullptr, pl->contact.flags != 0, pl->field.z != nullptr,
                       actuators, episodes);
}

// `ticks` ticks under the span's plan through `kernel` (not QMPC_RUN_PER_TICK).  A: the stages' part as the caller
// filled it (the fleet run: none); the span's block and the ground are filled here.  info: the call's own counts.
template <class Info>
int run_fused(qmpc_ctx* c, int batch, int ticks, QmpcRunKernel kernel, QmpcLoopGroundArgs& A, double* effort,
              double* state, double* motor, Info& info, void* stream_) {
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const qmpc_ctx::Plant* pl = c->plant.get();
  k->started = true;
  info.reason = 0;
  const bool per_robot = k->schedule == QMPC_CTRL_PER_ROBOT;
  const QmpcPlantStepArgs P = plant_step_args(c, batch, effort, state, motor);
  A.X.C = k->d;
  A.X.g = QmpcLegGeom{c->leg_geom[0], c->leg_geom[1], c->leg_geom[2], c->leg_geom[3]};
  A.X.S = P.S;
  A.X.K = P.K;
  A.X.effort = effort;
  A.X.state = state;
  A.X.motor = motor;
  A.X.n = P.n;
  A.X.V = P.V;
  A.X.build_list = per_robot ? 1 : 0;
  A.T = P.T;  // (the flat kernels are given neither)
  A.Fd = P.Fd;
  int cur = 0;  // the call's index of the launch's first tick
  for (const SpanLaunch& l : plan_spans(k->ticks, ticks, per_robot)) {
    // (a kernel, not a memset node: see fill_ints)
    if (l.reset_due) HIP_TRY(c, fill_ints(k->d.due_count, 1, 0, q.stream));
    const int t_mod13 = (int)(k->ticks % 13);
    switch (kernel) {
      case QMPC_RUN_SPAN:
        HIP_TRY(c, qmpc_launch_span(&A.X, k->robot_mode, pl->bound, pl->stats_on, l.first_at_c, l.ticks, l.last_after_l, q.stream));
        break;
      case QMPC_RUN_LOOP:
        HIP_TRY(c, qmpc_launch_loop(&A, k->robot_mode, pl->bound, pl->stats_on, l.first_at_c, l.ticks, l.last_after_l, cur,
                                    t_mod13, q.stream));
        break;
      case QMPC_RUN_LOOP_TERRAIN:
        HIP_TRY(c, qmpc_launch_loop_terrain(&A, k->robot_mode, pl->bound, pl->stats_on, l.first_at_c, l.ticks,
                                            l.last_after_l, cur, t_mod13, q.stream));
        break;
      case QMPC_RUN_LOOP_FIELD:
        HIP_TRY(c, qmpc_launch_loop_field(&A, k->robot_mode, pl->bound, pl->stats_on, l.first_at_c, l.ticks,
                                          l.last_after_l, cur, t_mod13, q.stream));
        break;
      default:
        return QMPC_ERR_STATE;  // (not reached: the caller serves QMPC_RUN_PER_TICK itself)
    }
    // T follows the locomotion stages as they are enqueued, in front of the solve that can still fail (ctrl_after_prework)
    k->ticks += l.locos;
    info.ticks += l.locos;
    info.fused_ticks += l.locos;
    ++info.fused_launches;
    if (l.solve) {
      if (const int rc = ctrl_solve_enqueue(c, batch, q.stream)) return rc;
      cur += l.ticks - 1;
    }
  }
  return QMPC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Fleet run (include/qmpc_fleet.h): qmpc_ctrl_tick_state -> qmpc_plant_step, `ticks` times, with everything between two
// solves in one launch.  The plan is qmpc_span.h's, the kernel qmpc_span.hip's; on ground (include/qmpc_ground_run.h)
// qmpc_loop.hip's ground compile with its two stages off.
extern "C" {

int qmpc_fleet_run(qmpc_handle c, int batch, int ticks, double* effort, double* state, double* motor, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (ticks < 1 || !effort || !state || !motor) return QMPC_ERR_ARG;
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const QmpcRunPick pick = run_pick(c, false, false);
  // (the counts follow what has been enqueued: a call refused here, or one that stops half way, counts no tick it did not
  //  enqueue)
  if (pick.kernel == QMPC_RUN_PER_TICK) {
    // what the fused kernels do not cover: the per-tick calls themselves, so the launches are theirs exactly
    for (int i = 0; i < ticks; ++i) {
      if (const int rc = qmpc_ctrl_tick_state(c, batch, state, motor, effort, stream_)) return rc;
      k->fleet.reason = pick.reason;  // (the call has enqueued something: it is the last call now)
      if (const int rc = qmpc_plant_step(c, batch, effort, state, motor, stream_)) return rc;
      ++k->fleet.ticks;
      ++k->fleet.fallback_ticks;
    }
    return QMPC_OK;
  }
  QmpcLoopGroundArgs A{};
  return run_fused(c, batch, ticks, pick.kernel, A, effort, state, motor, k->fleet, stream_);
}

int qmpc_fleet_run_info(qmpc_handle c, qmpc_fleet_info* out) {
  if (!c || !out) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  *out = c->ctrl->fleet;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Loop run (include/qmpc_loop.h): the fleet run's loop with the actuator stage and the episode step inside the launch.
// The plan is the span's, unchanged; the kernel is qmpc_loop.hip's, or the span's own where no option is set.
extern "C" {

int qmpc_loop_run(qmpc_handle c, int batch, int ticks, const qmpc_loop_opts* o, double* effort, double* state,
                  double* motor, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!o || ticks < 1 || !effort || !state || !motor) return QMPC_ERR_ARG;
  const bool act = o->actuators != 0;
  const int every = o->episodes_every;
  if (every < 0 || (every && ticks % every != 0)) return QMPC_ERR_ARG;
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  qmpc_ctx::Plant* pl = c->plant.get();
  if (act) {
    if (!ready(c->act)) return QMPC_ERR_STATE;
    if (batch != c->act->batch) return QMPC_ERR_ARG;
    // the actuator stage reads the rates in the plant's motor rows while it writes the effort (qmpc_act's own check)
    const double* m = pl->d.motor;
    if (effort < m + (size_t)batch * 24 && m < effort + (size_t)batch * 12) return QMPC_ERR_ARG;
  }
  if (every) {
    if (!ready(c->episode) || !c->episode->is_set) return QMPC_ERR_STATE;
    if (batch != c->episode->batch) return QMPC_ERR_ARG;
    // the plant's reset writes its own read-out rows only: the loop would carry on from stale caller rows
    if (state != pl->d.state || motor != pl->d.motor) return QMPC_ERR_ARG;
  }
  QmpcLoopGroundArgs A{};
  if (act) {
    A.A = c->act->a;
    A.A.motor = pl->d.motor;
    A.A.dt = 1.0 / k->freq;
    A.act = 1;
    A.act_stats = o->actuator_stats;
  }
  if (every) {
    const qmpc_ctx::Episode* e = c->episode.get();
    A.decide = e->rule.causes ? 1 : 0;  // (causes 0: qmpc_episode_step enqueues nothing)
    A.every = A.decide || act ? every : 0;
    A.E = e->d;
    A.In = episode_inputs(c);
    A.R = e->rule;
    A.Bd = e->bind;
  }
  // (neither stage in the launch: nothing of this header's, the span kernel itself on the flat plant)
  const QmpcRunPick pick = run_pick(c, A.act != 0, A.every != 0);
  if (pick.kernel == QMPC_RUN_PER_TICK) {
    // what the fused kernels do not cover: the per-tick calls themselves, so the launches are theirs exactly
    for (int i = 0; i < ticks; ++i) {
      if (const int rc = qmpc_ctrl_tick_state(c, batch, state, motor, effort, stream_)) return rc;
      k->loop.reason = pick.reason;  // (the call has enqueued something: it is the last call now)
      if (act)
        if (const int rc = qmpc_act(c, batch, effort, effort, stream_)) return rc;
      if (const int rc = qmpc_plant_step(c, batch, effort, state, motor, stream_)) return rc;
      ++k->loop.ticks;
      ++k->loop.fallback_ticks;
      if (every && (i + 1) % every == 0) {
        if (const int rc = qmpc_episode_step(c, batch, every, stream_)) return rc;
        if (act)
          if (const int rc = qmpc_act_reset(c, batch, c->episode->d.mask, nullptr, o->actuator_stats, stream_)) return rc;
      }
    }
    return QMPC_OK;
  }
  return run_fused(c, batch, ticks, pick.kernel, A, effort, state, motor, k->loop, stream_);
}

int qmpc_loop_run_info(qmpc_handle c, qmpc_loop_info* out) {
  if (!c || !out) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  *out = c->ctrl->loop;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// The switch of include/qmpc_ground_run.h: host state only, read by the next run call.
extern "C" {

int qmpc_ground_run_enable(qmpc_handle c, int on) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  c->ctrl->ground_run = on != 0;
  return QMPC_OK;
}

int qmpc_ground_run_enabled(qmpc_handle c, int* on) {
  if (!c || !on) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  *on = c->ctrl->ground_run ? 1 : 0;
  return QMPC_OK;
}

}  // extern "C"
