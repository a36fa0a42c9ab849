// qmpc_capi_plant.cpp -- host side of include/qmpc_plant.h (the reduced-order plant; the kernels are in qmpc_plant.hip) and
// of the headers that extend it: qmpc_plant_vary.h, qmpc_terrain.h (qmpc_terrain.hip), qmpc_contact.h (qmpc_contact.hip),
// qmpc_field.h (qmpc_field.hip).
#include <cmath>
#include <vector>

#include "../../include/qmpc_plant.h"
#include "../../include/qmpc_plant_vary.h"  // ... its per-robot parameters and on-device statistics
#include "../../include/qmpc_terrain.h"     // ... its per-robot slopes and stairs
#include "../../include/qmpc_contact.h"     // ... contact decided by the ground
#include "../../include/qmpc_field.h"       // ... height-field terrain from memory
#include "qmpc_host.h"
using namespace qmpc_host;

size_t qmpc_host::carve(QmpcPlantDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_PLANT_ARRAYS(QMPC_CARVE)
  return off;
}

namespace {

// the constants of a launch, from the handle as it stands now
QmpcPlantConst plant_const(const qmpc_ctx* c, double mu, int substeps) {
  QmpcPlantConst K{};
  K.mass = c->mass;
  for (int k = 0; k < 3; ++k) K.ibody[k] = c->ibody[k];
  for (int k = 0; k < 4; ++k) K.geom[k] = (double)c->leg_geom[k];
  K.mu = mu;
  K.substeps = substeps;
  K.h = (1.0 / c->ctrl->freq) / (double)substeps;
  const double l1 = K.geom[0] + K.geom[3], l2 = K.geom[1], l3 = K.geom[2];
  const double base = (l1 * l1 + l2 * l2) + l3 * l3;
  K.r2_lo = base + (2 * l2 * l3) * std::cos(QMPC_PLANT_KNEE_MAX);
  K.r2_hi = base + (2 * l2 * l3) * std::cos(QMPC_PLANT_KNEE_MIN);
  return K;
}

// One launcher per entry of qmpc_plant_pick.h's lists, in the enums' order
typedef hipError_t (*PlantStepLauncher)(const QmpcPlantStepArgs*, int vary, int stats, hipStream_t);
typedef hipError_t (*PlantResetLauncher)(const QmpcPlantResetArgs*, hipStream_t);
#define QMPC_PLANT_ENTRY(NAME, name) qmpc_launch_##name##_step,
const PlantStepLauncher kPlantStep[QMPC_STEP_KINDS] = {QMPC_PLANT_STEP_KINDS(QMPC_PLANT_ENTRY)};
#undef QMPC_PLANT_ENTRY
#define QMPC_PLANT_ENTRY(NAME, name) qmpc_launch_##name##_init,
const PlantResetLauncher kPlantReset[QMPC_RESET_KINDS] = {QMPC_PLANT_RESET_KINDS(QMPC_PLANT_ENTRY)};
#undef QMPC_PLANT_ENTRY

QmpcPlantPick plant_pick(const qmpc_ctx::Plant* k) {
  return qmpc_plant_pick(k->field.z != nullptr, k->contact.flags != 0, k->terrain.rows != nullptr);
}

}  // namespace

int qmpc_host::plant_check(qmpc_ctx* c, int batch) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c) || !plant_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->plant->batch || batch != c->ctrl->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

// The argument block of a step, from the handle as it stands now and the call's three pointers.  Every step kernel is
// given the same block and reads what it knows of.
QmpcPlantStepArgs qmpc_host::plant_step_args(qmpc_ctx* c, int batch, const double* effort, double* state_out, double* motor_out) {
  qmpc_ctx::Plant* k = c->plant.get();
  const QmpcCtrlDev& d = c->ctrl->d;
  QmpcPlantStepArgs A{};
  A.S = k->d;
  A.K = plant_const(c, k->mu, k->substeps);
  A.effort = effort;
  A.contact_state = d.contact_state;
  A.p_des = d.p_des;
  A.v_des = d.v_des;
  A.state_out = state_out;
  A.motor_out = motor_out;
  A.n = batch * 4;
  // nothing bound and the statistics off: the plain instantiation, which is given no QmpcPlantVary to read
  if (k->bound || k->stats_on) A.V = k->vary;
  A.T = k->ground();
  if (k->contact.flags) {
    k->contact.dt = 1.0 / c->ctrl->freq;
    k->contact_dirty = true;
  }
  A.C = k->contact;
  A.Fd = k->field;
  return A;
}

// The plant's reset of the masked robots on whatever ground is bound (qmpc_plant_reset, and the episode manager's).
int qmpc_host::plant_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, const double* init_xyyaw,
                                   hipStream_t stream) {
  const qmpc_ctx::Plant* k = c->plant.get();
  const QmpcPlantPick pick = plant_pick(k);
  // The counters' reset first, on every ground.  With no rows bound it also zeroes support and ground, which the flat
  // reset does not know; the flat init writes none of what it writes, and the terrain's and the field's inits write
  // support and ground after it on the same stream: the same bytes at the end as with the init first.
  if (pick.contact) HIP_TRY(c, qmpc_launch_contact_reset(mask_dev, batch, stream, &k->terrain, &k->contact));
  const QmpcPlantResetArgs A{k->d, plant_const(c, k->mu, k->substeps), mask_dev, init_xyyaw, batch * 4,
                             k->ground(), k->field};
  HIP_TRY(c, kPlantReset[pick.reset](&A, stream));
  return QMPC_OK;
}

extern "C" {

int qmpc_plant_init(qmpc_handle c, int batch, double mu_plant, int substeps, const double* init_xyyaw, void* stream_) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->ctrl->batch || substeps < 1 || !(mu_plant >= 0)) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  qmpc_ctx::Plant* k = made(c->plant);
  HIP_TRY(c, carve_block(k->buf, k->d, c->max_batch));
  if (!k->terrain_buf) {
    // ground[M], support[M] of qmpc_terrain.h, zero until a reset on terrain writes them (first use only)
    DevBuf<double> buf;
    HIP_TRY(c, buf.alloc(2 * (size_t)c->max_batch));
    const hipError_t e = hipMemset(buf, 0, 2 * sizeof(double) * (size_t)c->max_batch);
    if (e != hipSuccess) return fail(c, e, "hipMemset(plant terrain)");
    k->terrain_buf = std::move(buf);
    k->terrain.ground = k->terrain_buf.p;
    k->terrain.support = k->terrain_buf.p + c->max_batch;
  }
  if (!k->contact_buf) {
    // slip[M], drop[M][4] (double), early[M], late[M] (int32) of qmpc_contact.h, zero (first use only)
    const size_t M = (size_t)c->max_batch;
    DevBuf<double> buf;
    HIP_TRY(c, buf.alloc(6 * M));
    const hipError_t e = hipMemset(buf, 0, 6 * sizeof(double) * M);
    if (e != hipSuccess) return fail(c, e, "hipMemset(plant contact)");
    k->contact_buf = std::move(buf);
    k->contact.slip = k->contact_buf.p;
    k->contact.drop = k->contact_buf.p + M;
    k->contact.early = reinterpret_cast<int32_t*>(k->contact_buf.p + 5 * M);
    k->contact.late = k->contact.early + M;
  }
  if (const int rc = order_after_previous(c, stream)) return rc;
  const QmpcPlantResetArgs A{k->d, plant_const(c, mu_plant, substeps), nullptr, init_xyyaw, batch * 4, {}, {}};
  HIP_TRY(c, qmpc_launch_plant_init(&A, stream));
  if (k->contact_dirty) {
    // a plant that stepped with contact on starts again with its counters at zero (no other plant launches this)
    const QmpcTerrainArgs flat{nullptr, k->terrain.ground, k->terrain.support, 0};
    HIP_TRY(c, qmpc_launch_contact_reset(nullptr, c->max_batch, stream, &flat, &k->contact));
    k->contact_dirty = false;
  }
  k->batch = batch;
  k->mu = mu_plant;
  k->substeps = substeps;
  // a new plant is the plain plant: nothing bound (the statistics keep their switch and their values)
  k->vary.mass = k->vary.ibody = k->vary.mu = k->vary.force = k->vary.torque = nullptr;
  k->bound = false;
  k->terrain.rows = nullptr;  // ... and stands on flat ground
  k->terrain.flags = 0;
  k->contact.flags = 0;       // ... with scheduled contact
  k->field = QmpcFieldArgs{};  // ... and no height field
  k->field_flags = 0;
  return QMPC_OK;
}

int qmpc_plant_reset(qmpc_handle c, int batch, const uint8_t* mask_dev, const double* init_xyyaw, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!mask_dev) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  return plant_reset_enqueue(c, batch, mask_dev, init_xyyaw, q.stream);
}

int qmpc_plant_step(qmpc_handle c, int batch, const double* effort, double* state_out, double* motor_out,
                    void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!effort || !state_out || !motor_out) return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  const qmpc_ctx::Plant* k = c->plant.get();
  const QmpcPlantStepArgs A = plant_step_args(c, batch, effort, state_out, motor_out);
  HIP_TRY(c, kPlantStep[plant_pick(k).step](&A, k->bound, k->stats_on, q.stream));
  return QMPC_OK;
}

int qmpc_plant_view_get(qmpc_handle c, qmpc_plant_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c)) return QMPC_ERR_STATE;
  const QmpcPlantDev& d = c->plant->d;
  v->p = d.p;
  v->v = d.v;
  v->q = d.q;
  v->omega = d.omega;
  v->foot = d.foot;
  v->stance = d.stance;
  v->grf = d.grf;
  v->state = d.state;
  v->motor = d.motor;
  v->batch = c->plant->batch;
  v->substeps = c->plant->substeps;
  v->mu_plant = c->plant->mu;
  return QMPC_OK;
}

// ---- include/qmpc_plant_vary.h: per-robot parameters and statistics of the plant ----

int qmpc_plant_set_params(qmpc_handle c, int batch, const qmpc_plant_params* prm) {
  if (const int rc = plant_check(c, batch)) return rc;
  qmpc_ctx::Plant* k = c->plant.get();
  k->vary.mass = prm ? prm->mass : nullptr;
  k->vary.ibody = prm ? prm->ibody : nullptr;
  k->vary.mu = prm ? prm->mu : nullptr;
  k->vary.force = prm ? prm->force : nullptr;
  k->vary.torque = prm ? prm->torque : nullptr;
  k->bound = k->vary.mass || k->vary.ibody || k->vary.mu || k->vary.force || k->vary.torque;
  return QMPC_OK;
}

int qmpc_plant_stats_enable(qmpc_handle c, int on) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c) || !plant_ready(c)) return QMPC_ERR_STATE;
  qmpc_ctx::Plant* k = c->plant.get();
  if (on && !k->stats_buf) {
    // acc[QMPC_PLANT_STATS][M] doubles, then n[M] ints; the initial values come from the host, which synchronises
    DeviceGuard g(c->device);
    const size_t M = (size_t)c->max_batch;
    const size_t bytes = (QMPC_PLANT_STATS * sizeof(double) + sizeof(int)) * M;
    std::vector<char> init(bytes, 0);
    double* a = reinterpret_cast<double*>(init.data());
    for (size_t b = 0; b < M; ++b) {
      a[QMPC_PLANT_STAT_Z_MIN * M + b] = HUGE_VAL;
      a[QMPC_PLANT_STAT_Z_MAX * M + b] = -HUGE_VAL;
    }
    DevBuf<char> buf;  // (the handle's only once it holds the initial values)
    HIP_TRY(c, buf.alloc(bytes));
    const hipError_t e = hipMemcpy(buf, init.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, e, "hipMemcpy(plant statistics)");
    k->stats_buf = std::move(buf);
    k->vary.acc = reinterpret_cast<double*>(k->stats_buf.p);
    k->vary.n = reinterpret_cast<int*>(k->vary.acc + QMPC_PLANT_STATS * M);
    k->vary.acc_stride = c->max_batch;
  }
  k->stats_on = on != 0;
  return QMPC_OK;
}

int qmpc_plant_stats_reset(qmpc_handle c, int batch, const uint8_t* mask_dev, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!c->plant->stats_buf) return QMPC_ERR_STATE;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_plant_stats_reset(&c->plant->vary, mask_dev, batch, q.stream));
  return QMPC_OK;
}

int qmpc_plant_stats_get(qmpc_handle c, qmpc_plant_stats* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c) || !c->plant->stats_buf) return QMPC_ERR_STATE;
  const qmpc_ctx::Plant* k = c->plant.get();
  const size_t M = (size_t)k->vary.acc_stride;
  v->n = k->vary.n;
  v->z_min = k->vary.acc + QMPC_PLANT_STAT_Z_MIN * M;
  v->z_max = k->vary.acc + QMPC_PLANT_STAT_Z_MAX * M;
  v->roll_max = k->vary.acc + QMPC_PLANT_STAT_ROLL_MAX * M;
  v->pitch_max = k->vary.acc + QMPC_PLANT_STAT_PITCH_MAX * M;
  v->vx_sum = k->vary.acc + QMPC_PLANT_STAT_VX_SUM * M;
  v->vy_sum = k->vary.acc + QMPC_PLANT_STAT_VY_SUM * M;
  v->batch = k->batch;
  v->enabled = k->stats_on ? 1 : 0;
  return QMPC_OK;
}

// ---- include/qmpc_terrain.h: per-robot slopes and stairs under the plant ----

int qmpc_plant_set_terrain(qmpc_handle c, int batch, const double* terrain_dev, int flags) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (flags & ~(QMPC_TERRAIN_CLAMP_SWING | QMPC_TERRAIN_REBASE_Z)) return QMPC_ERR_ARG;
  qmpc_ctx::Plant* k = c->plant.get();
  k->terrain.rows = terrain_dev;
  k->terrain.flags = terrain_dev ? flags : 0;
  return QMPC_OK;
}

int qmpc_terrain_view_get(qmpc_handle c, qmpc_terrain_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c)) return QMPC_ERR_STATE;
  const qmpc_ctx::Plant* k = c->plant.get();
  v->ground = k->terrain.ground;
  v->support = k->terrain.support;
  v->terrain = k->terrain.rows;
  v->flags = k->terrain.flags;
  v->batch = k->batch;
  return QMPC_OK;
}

// ---- include/qmpc_contact.h: contact decided by the ground ----

int qmpc_plant_set_contact(qmpc_handle c, int batch, const qmpc_contact_params* prm) {
  if (const int rc = plant_check(c, batch)) return rc;
  qmpc_ctx::Plant* k = c->plant.get();
  if (!prm || prm->flags == 0) {
    k->contact.flags = 0;
    return QMPC_OK;
  }
  if (prm->flags & ~(QMPC_CONTACT_EARLY | QMPC_CONTACT_LATE | QMPC_CONTACT_SLIP)) return QMPC_ERR_ARG;
  for (const double x : {prm->drop_speed, prm->slip_gain, prm->slip_vmax})
    if (!std::isfinite(x) || !(x >= 0)) return QMPC_ERR_ARG;
  k->contact.flags = prm->flags;
  k->contact.drop_speed = prm->drop_speed;
  k->contact.slip_gain = prm->slip_gain;
  k->contact.slip_vmax = prm->slip_vmax;
  return QMPC_OK;
}

int qmpc_contact_view_get(qmpc_handle c, qmpc_contact_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c)) return QMPC_ERR_STATE;
  const qmpc_ctx::Plant* k = c->plant.get();
  v->early = k->contact.early;
  v->late = k->contact.late;
  v->slip = k->contact.slip;
  v->drop = k->contact.drop;
  v->params.flags = k->contact.flags;
  v->params.drop_speed = k->contact.drop_speed;
  v->params.slip_gain = k->contact.slip_gain;
  v->params.slip_vmax = k->contact.slip_vmax;
  v->batch = k->batch;
  return QMPC_OK;
}

// ---- include/qmpc_field.h: height-field terrain from memory ----

int qmpc_plant_set_field(qmpc_handle c, int batch, const qmpc_field_bank* bank, const double* place_dev, int flags) {
  if (const int rc = plant_check(c, batch)) return rc;
  qmpc_ctx::Plant* k = c->plant.get();
  if (!bank) {
    k->field = QmpcFieldArgs{};
    k->field_flags = 0;
    return QMPC_OK;
  }
  if (flags & ~(QMPC_TERRAIN_CLAMP_SWING | QMPC_TERRAIN_REBASE_Z)) return QMPC_ERR_ARG;
  if (!bank->z || !place_dev || bank->nx < 2 || bank->ny < 2 || bank->count < 1) return QMPC_ERR_ARG;
  if (!std::isfinite(bank->cell) || !(bank->cell > 0)) return QMPC_ERR_ARG;
  k->field = QmpcFieldArgs{bank->z, place_dev, bank->cell, bank->nx, bank->ny, bank->count};
  k->field_flags = flags;
  return QMPC_OK;
}

int qmpc_field_view_get(qmpc_handle c, qmpc_field_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c)) return QMPC_ERR_STATE;
  const qmpc_ctx::Plant* k = c->plant.get();
  v->bank.z = k->field.z;
  v->bank.nx = k->field.nx;
  v->bank.ny = k->field.ny;
  v->bank.count = k->field.count;
  v->bank.cell = k->field.cell;
  v->place = k->field.place;
  v->flags = k->field_flags;
  v->batch = k->batch;
  return QMPC_OK;
}

}  // extern "C"
