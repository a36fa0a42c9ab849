// qmpc_capi_stages.cpp -- host side of the stages around the closed loop of controller and plant: the sensor model
// (include/qmpc_sense.h), the actuator stage (qmpc_act.h) and the episode manager in both forms (qmpc_episode.h,
// qmpc_episode_sense.h).  Each has its kernels in the .hip file of its name.
#include "../../include/qmpc_sense.h"
#include "../../include/qmpc_act.h"
#include "../../include/qmpc_episode.h"
#include "../../include/qmpc_episode_sense.h"
#include "qmpc_host.h"
using namespace qmpc_host;

size_t qmpc_host::carve(QmpcActDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_ACT_ARRAYS(QMPC_CARVE)
  return off;
}
size_t qmpc_host::carve(QmpcEpisodeDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_EPISODE_ARRAYS(QMPC_CARVE)
  carve_array(d.log_words, base, off, 2, 1);
  return off;
}
size_t qmpc_host::carve(QmpcEpisodeSenseDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_EPISODE_SENSE_ARRAYS(QMPC_CARVE)
  return off;
}

namespace {

// A stage's check: the controller and the plant stand for this batch (plant_check; c may be null, so the stage is named by
// its member), and so does the stage
template <class S>
int stage_check(qmpc_ctx* c, int batch, std::unique_ptr<S> qmpc_ctx::*stage) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!ready(c->*stage)) return QMPC_ERR_STATE;
  if (batch != (c->*stage)->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Sensor model (include/qmpc_sense.h).  The kernels are in qmpc_sense.hip.
namespace {

int sense_check(qmpc_ctx* c, int batch) { return stage_check(c, batch, &qmpc_ctx::sense); }

void sense_unbind(QmpcSenseArgs& a) {
  a.acc_bias = a.gyro_bias = a.acc_sigma = a.gyro_sigma = a.q_sigma = a.qd_sigma = nullptr;
}

}  // namespace

extern "C" {

int qmpc_sense_init(qmpc_handle c, int batch, uint64_t seed, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::Sense* k = made(c->sense);
  if (!k->buf) HIP_TRY(c, k->buf.alloc(2 * (size_t)c->max_batch));  // n[max_batch], epoch[max_batch]
  if (const int rc = order_after_previous(c, stream)) return rc;
  HIP_TRY(c, fill_ints(k->buf, (int)k->buf.n, 0, stream));
  k->a.n = k->buf;
  k->a.epoch = k->a.n + c->max_batch;
  k->a.key0 = (uint32_t)(seed & 0xFFFFFFFFu);
  k->a.key1 = (uint32_t)(seed >> 32);
  sense_unbind(k->a);
  k->bound = false;
  k->seed = seed;
  k->batch = batch;
  return QMPC_OK;
}

int qmpc_sense_set_params(qmpc_handle c, int batch, const qmpc_sense_params* prm) {
  if (const int rc = sense_check(c, batch)) return rc;
  QmpcSenseArgs& a = c->sense->a;
  sense_unbind(a);
  if (prm) {
    a.acc_bias = prm->acc_bias;
    a.gyro_bias = prm->gyro_bias;
    a.acc_sigma = prm->acc_sigma;
    a.gyro_sigma = prm->gyro_sigma;
    a.q_sigma = prm->q_sigma;
    a.qd_sigma = prm->qd_sigma;
  }
  c->sense->bound = a.acc_bias || a.gyro_bias || a.acc_sigma || a.gyro_sigma || a.q_sigma || a.qd_sigma;
  return QMPC_OK;
}

int qmpc_sense_reset(qmpc_handle c, int batch, const uint8_t* mask_dev, void* stream_) {
  if (const int rc = sense_check(c, batch)) return rc;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_sense_reset(&c->sense->a, mask_dev, batch, q.stream));
  return QMPC_OK;
}

int qmpc_sense(qmpc_handle c, int batch, double* imu_out, double* motor_out, void* stream_) {
  if (const int rc = sense_check(c, batch)) return rc;
  const QmpcPlantDev& p = c->plant->d;
  if (!imu_out || !motor_out) return QMPC_ERR_ARG;
  // the kernel reads the plant's rows while it writes the outputs
  if (imu_out == p.state || imu_out == p.motor || motor_out == p.state || motor_out == p.motor) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  QmpcSenseArgs a = c->sense->a;
  a.state = p.state;
  a.motor = p.motor;
  HIP_TRY(c, qmpc_launch_sense(&a, imu_out, motor_out, batch, c->sense->bound, q.stream));
  return QMPC_OK;
}

int qmpc_sense_view_get(qmpc_handle c, qmpc_sense_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c) || !ready(c->sense)) return QMPC_ERR_STATE;
  v->n = c->sense->a.n;
  v->epoch = c->sense->a.epoch;
  v->batch = c->sense->batch;
  v->seed = c->sense->seed;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Actuator stage (include/qmpc_act.h).  The kernels are in qmpc_act.hip.
namespace {

int act_check(qmpc_ctx* c, int batch) { return stage_check(c, batch, &qmpc_ctx::act); }

void act_unbind(QmpcActArgs& a) {
  a.battery_v = a.tau_max = a.strength = a.damping = a.dry_friction = nullptr;
  a.delay = nullptr;
}

}  // namespace

extern "C" {

int qmpc_act_config_default(qmpc_act_config* cfg) {
  if (!cfg) return QMPC_ERR_ARG;
  // MiniCheetah.h:28-46 as Quadruped::buildActuatorModels assembles them (abad and hip share a gear ratio)
  *cfg = qmpc_act_config{{6.0, 6.0, 9.33}, 0.05, 0.173, 24.0, 0.01, 0.2, 3.0, 1, 0};
  return QMPC_OK;
}

int qmpc_act_init(qmpc_handle c, int batch, const qmpc_act_config* cfg_, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  qmpc_act_config cfg;
  qmpc_act_config_default(&cfg);
  if (cfg_) cfg = *cfg_;
  if (cfg.max_delay < 0 || cfg.max_delay > QMPC_ACT_MAX_DELAY) return QMPC_ERR_ARG;
  if (!(cfg.kt > 0.0) || !(cfg.R > 0.0)) return QMPC_ERR_ARG;
  for (const double g : cfg.gear)
    if (!(g > 0.0)) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::Act* k = made(c->act);
  HIP_TRY(c, carve_block(k->buf, k->a.d, c->max_batch));
  const size_t ring_n = (size_t)(cfg.max_delay + 1) * (size_t)c->max_batch * 12;
  if (k->ring.n < ring_n) {
    // (a longer ring than the handle has had so far: the old block goes, after the device has finished with it)
    k->batch = 0;
    DevBuf<double> grown;
    HIP_TRY(c, grown.alloc(ring_n));
    k->ring = std::move(grown);
  }
  if (const int rc = order_after_previous(c, stream)) return rc;
  HIP_TRY(c, hipMemsetAsync(k->buf, 0, k->buf.n, stream));
  HIP_TRY(c, hipMemsetAsync(k->ring, 0, sizeof(double) * (size_t)(cfg.max_delay + 1) * (size_t)batch * 12, stream));
  k->a.ring = k->ring;
  k->a.cfg = cfg;
  act_unbind(k->a);
  k->batch = batch;
  return QMPC_OK;
}

int qmpc_act_set_params(qmpc_handle c, int batch, const qmpc_act_params* prm) {
  if (const int rc = act_check(c, batch)) return rc;
  QmpcActArgs& a = c->act->a;
  act_unbind(a);
  if (prm) {
    a.battery_v = prm->battery_v;
    a.tau_max = prm->tau_max;
    a.strength = prm->strength;
    a.damping = prm->damping;
    a.dry_friction = prm->dry_friction;
    a.delay = prm->delay;
  }
  return QMPC_OK;
}

int qmpc_act_reset(qmpc_handle c, int batch, const uint8_t* mask_a, const uint8_t* mask_b, int stats, void* stream_) {
  if (const int rc = act_check(c, batch)) return rc;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_act_reset(&c->act->a.d, mask_a, mask_b, stats, batch, q.stream));
  return QMPC_OK;
}

int qmpc_act(qmpc_handle c, int batch, const double* effort_in, double* effort_out, void* stream_) {
  if (const int rc = act_check(c, batch)) return rc;
  if (!effort_in || !effort_out) return QMPC_ERR_ARG;
  // the kernel reads the rates in the plant's motor rows while it writes the output
  const double* motor = c->plant->d.motor;
  if (effort_out < motor + (size_t)batch * 24 && motor < effort_out + (size_t)batch * 12) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  QmpcActArgs a = c->act->a;
  a.motor = motor;
  a.dt = 1.0 / c->ctrl->freq;
  HIP_TRY(c, qmpc_launch_act(&a, effort_in, effort_out, batch, q.stream));
  return QMPC_OK;
}

int qmpc_act_view_get(qmpc_handle c, qmpc_act_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!ctrl_ready(c) || !plant_ready(c) || !ready(c->act)) return QMPC_ERR_STATE;
  const QmpcActArgs& a = c->act->a;
  v->ring = a.ring;
  v->head = a.d.head;
  v->age = a.d.age;
  v->n = a.d.n;
  v->n_vsat = a.d.n_vsat;
  v->n_tsat = a.d.n_tsat;
  v->tau_peak = a.d.tau_peak;
  v->e_heat = a.d.e_heat;
  v->e_mech = a.d.e_mech;
  v->e_pos = a.d.e_pos;
  v->config = a.cfg;
  v->dt = 1.0 / c->ctrl->freq;
  v->batch = c->act->batch;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Episode manager (include/qmpc_episode.h).  The kernels are in qmpc_episode.hip.
// what a decision kernel reads of the handle's other state
QmpcEpisodeIn qmpc_host::episode_inputs(const qmpc_ctx* c) {
  const qmpc_ctx::Plant* pl = c->plant.get();
  // the plant writes ground[b] on terrain, on a field and with contact on (there 0 without rows); the flat plant never does
  const bool ground = pl->terrain.rows || pl->field.z || pl->contact.flags;
  return QmpcEpisodeIn{pl->d.p, pl->d.q, c->ctrl->d.safe, ground ? pl->terrain.ground : nullptr,
                       (uint32_t)(c->episode->seed & 0xFFFFFFFFu), (uint32_t)(c->episode->seed >> 32)};
}

namespace {

int episode_check(qmpc_ctx* c, int batch) { return stage_check(c, batch, &qmpc_ctx::episode); }

const int kEpisodeCauses = QMPC_EP_UNSAFE | QMPC_EP_NONFINITE | QMPC_EP_TILT | QMPC_EP_HEIGHT | QMPC_EP_RANGE | QMPC_EP_TIMEOUT;

}  // namespace

extern "C" {

int qmpc_episode_init(qmpc_handle c, int batch, uint64_t seed, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::Episode* k = made(c->episode);
  HIP_TRY(c, carve_block(k->buf, k->d, c->max_batch));
  if (const int rc = order_after_previous(c, stream)) return rc;
  HIP_TRY(c, qmpc_launch_episode_init(&k->d, c->plant->d.p, batch, c->max_batch, stream));
  k->rule = qmpc_episode_rule{};
  k->bind = qmpc_episode_bind{};
  k->is_set = false;
  k->seed = seed;
  k->batch = batch;
  return QMPC_OK;
}

int qmpc_episode_set(qmpc_handle c, int batch, const qmpc_episode_rule* rule, const qmpc_episode_bind* bind) {
  if (const int rc = episode_check(c, batch)) return rc;
  if (!rule || !bind) return QMPC_ERR_ARG;
  if ((rule->causes & ~kEpisodeCauses) || (bind->flags & ~QMPC_EP_SPAWN_PER_ROBOT)) return QMPC_ERR_ARG;
  if (!bind->vel || !bind->gait || !bind->spawn || bind->n_spawn < 1) return QMPC_ERR_ARG;
  if ((bind->commands && bind->n_commands < 1) || bind->log_rows < 0) return QMPC_ERR_ARG;
  qmpc_ctx::Episode* k = c->episode.get();
  k->rule = *rule;
  k->bind = *bind;
  k->is_set = true;
  return QMPC_OK;
}

int qmpc_episode_step(qmpc_handle c, int batch, int elapsed, void* stream_) {
  if (const int rc = episode_check(c, batch)) return rc;
  qmpc_ctx::Episode* k = c->episode.get();
  if (!k->is_set) return QMPC_ERR_STATE;
  if (elapsed < 1) return QMPC_ERR_ARG;
  if (!k->rule.causes) return QMPC_OK;  // the manager is off: nothing is enqueued
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  const qmpc_ctx::Plant* pl = c->plant.get();
  const QmpcEpisodeIn in = episode_inputs(c);
  HIP_TRY(c, qmpc_launch_episode_decide(&k->d, &in, &k->rule, &k->bind, elapsed, batch, q.stream));
  // the existing resets under the kernel's mask: controller, its commands (the reset zeroed them), plant, statistics
  if (const int rc = ctrl_reset_enqueue(c, batch, k->d.mask, q.stream)) return rc;
  HIP_TRY(c, qmpc_launch_ctrl_set(&c->ctrl->d, k->bind.gait, k->bind.vel, batch, q.stream));
  if (const int rc = plant_reset_enqueue(c, batch, k->d.mask, k->d.xyyaw, q.stream)) return rc;
  if (pl->stats_on) HIP_TRY(c, qmpc_launch_plant_stats_reset(&pl->vary, k->d.mask, batch, q.stream));
  return QMPC_OK;
}

int qmpc_episode_log_clear(qmpc_handle c, void* stream_) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c) || !plant_ready(c) || !ready(c->episode)) return QMPC_ERR_STATE;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_episode_log_clear(&c->episode->d, q.stream));
  return QMPC_OK;
}

int qmpc_episode_view_get(qmpc_handle c, qmpc_episode_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c) || !ready(c->episode)) return QMPC_ERR_STATE;
  const QmpcEpisodeDev& d = c->episode->d;
  v->age = d.age;
  v->episode = d.episode;
  v->start = d.start;
  v->count = d.count;
  v->ticks_sum = d.ticks_sum;
  v->last_cause = d.last_cause;
  v->last_ticks = d.last_ticks;
  v->mask = d.mask;
  v->xyyaw = d.xyyaw;
  v->log_count = d.log_words;
  v->log_dropped = d.log_words + 1;
  v->batch = c->episode->batch;
  v->seed = c->episode->seed;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Episodes on the sensor path (include/qmpc_episode_sense.h).  The kernels are in qmpc_episode_sense.hip.
namespace {

// the three inits this header stands on, then its own (own == false: qmpc_episode_sense_init itself)
int episode_sense_check(qmpc_ctx* c, int batch, bool own = true) {
  if (const int rc = episode_check(c, batch)) return rc;
  if (const int rc = sense_check(c, batch)) return rc;
  return own ? stage_check(c, batch, &qmpc_ctx::episode_sense) : QMPC_OK;
}

}  // namespace

extern "C" {

int qmpc_episode_sense_init(qmpc_handle c, int batch, int warm_ticks, void* stream_) {
  if (const int rc = episode_sense_check(c, batch, false)) return rc;
  if (warm_ticks < 0) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::EpisodeSense* k = made(c->episode_sense);
  HIP_TRY(c, carve_block(k->buf, k->d, c->max_batch));
  if (const int rc = order_after_previous(c, stream)) return rc;
  HIP_TRY(c, qmpc_launch_episode_sense_init(&k->d, c->max_batch, stream));
  k->warm_ticks = warm_ticks;
  k->batch = batch;
  return QMPC_OK;
}

int qmpc_episode_sense_hold(qmpc_handle c, int batch, const uint8_t* mask_dev, int ticks, void* stream_) {
  if (const int rc = episode_sense_check(c, batch)) return rc;
  if (ticks < 0) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  const QmpcPlantDev& p = c->plant->d;
  HIP_TRY(c, qmpc_launch_episode_sense_hold(&c->episode_sense->d, &c->episode->d, p.p, p.q, mask_dev, ticks, batch, q.stream));
  return QMPC_OK;
}

int qmpc_episode_sense_step(qmpc_handle c, int batch, double* effort, void* stream_) {
  if (const int rc = episode_sense_check(c, batch)) return rc;
  qmpc_ctx::Episode* k = c->episode.get();
  const qmpc_ctx::EpisodeSense* w = c->episode_sense.get();
  if (!k->is_set) return QMPC_ERR_STATE;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  const qmpc_ctx::Plant* pl = c->plant.get();
  const QmpcEpisodeIn in = episode_inputs(c);
  // (with causes == 0 nobody is judged, but the robots in warm-up are still held: the launches are the same)
  HIP_TRY(c, qmpc_launch_episode_sense_decide(&w->d, &k->d, &in, &k->rule, &k->bind, w->warm_ticks, batch, q.stream));
  // the controller: full under mask, all but the pre_work set under hold, one launch; then its commands, as
  // qmpc_episode_step hands them over (both forms zeroed them)
  const int counter0 = ctrl_reset_counter0(c->ctrl.get());
  HIP_TRY(c, qmpc_launch_episode_sense_reinit(&w->d, &k->d, &c->ctrl->d, counter0, effort, batch, q.stream));
  HIP_TRY(c, qmpc_launch_ctrl_set(&c->ctrl->d, k->bind.gait, k->bind.vel, batch, q.stream));
  // the plant and its statistics under the union; the sensors' new epoch for the robots that finished only
  if (const int rc = plant_reset_enqueue(c, batch, w->d.both, k->d.xyyaw, q.stream)) return rc;
  if (pl->stats_on) HIP_TRY(c, qmpc_launch_plant_stats_reset(&pl->vary, w->d.both, batch, q.stream));
  HIP_TRY(c, qmpc_launch_sense_reset(&c->sense->a, k->d.mask, batch, q.stream));
  return QMPC_OK;
}

int qmpc_episode_sense_view_get(qmpc_handle c, qmpc_episode_sense_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c) || !ready(c->episode_sense)) return QMPC_ERR_STATE;
  v->warm = c->episode_sense->d.warm;
  v->hold = c->episode_sense->d.hold;
  v->warm_ticks = c->episode_sense->warm_ticks;
  v->batch = c->episode_sense->batch;
  return QMPC_OK;
}

}  // extern "C"
