// qmpc_host.h -- what the host-side translation units of the C ABI share (host only, not installed):
//   qmpc_capi.cpp         the handle and the solve (qmpc.h, qmpc_expert.h, qmpc_debug.h)
//   qmpc_capi_ctrl.cpp    the batched controller, the fleet run and the loop run (qmpc_ctrl.h, qmpc_fleet.h, qmpc_loop.h,
//                         qmpc_ground_run.h)
//   qmpc_capi_plant.cpp   the plant and its extensions (qmpc_plant.h, qmpc_plant_vary.h, qmpc_terrain.h, qmpc_contact.h,
//                         qmpc_field.h)
//   qmpc_capi_stages.cpp  sensors, actuators, episodes (qmpc_sense.h, qmpc_act.h, qmpc_episode.h, qmpc_episode_sense.h)
// The handle, the preamble of an entry point, and the functions one unit defines for another.  Everything here is hidden:
// the library exports the C functions of include/*.h and nothing else.
#ifndef QMPC_HOST_H
#define QMPC_HOST_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <utility>

#include "../../include/qmpc.h"
#include "../../include/qmpc_ctrl.h"
#include "../../include/qmpc_fleet.h"
#include "../../include/qmpc_loop.h"
#include "qmpc_device.h"
#include "qmpc_plan.h"  // the solve's launch plan (host-only)
// the device-side argument blocks the handle keeps.  Each launcher is declared once, in the header its defining file
// includes too: these, qmpc_span.h, and qmpc_launch.h for the rest
#include "qmpc_glue.h"
#include "qmpc_plant.h"
#include "qmpc_sense.h"
#include "qmpc_episode.h"
#include "qmpc_episode_sense.h"
#include "qmpc_act.h"

#pragma GCC visibility push(hidden)

namespace qmpc_host {

// A hipMalloc block and its element count, freed with its owner -- the owner goes with the handle's device current
// (qmpc_destroy).  Move-only; reads as the pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {  // (the block held so far goes with o)
    std::swap(p, o.p), std::swap(n, o.n);
    return *this;
  }
  ~DevBuf() {
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t count) {  // (of an empty owner)
    const hipError_t e = hipMalloc(&p, sizeof(T) * count);
    n = e == hipSuccess ? count : 0;
    return e;
  }
  operator T*() const { return p; }
};

}  // namespace qmpc_host

using qmpc_host::DevBuf;

// (hidden: the library exports the C functions of include/*.h and nothing of this type)
struct __attribute__((visibility("hidden"))) qmpc_ctx {
  int device = 0;
  int max_batch = 0, max_horizon = 0;
  bool is_setup = false;
  int horizon = 0;
  double dt = 0, mu = 0, f_max = 0;
  double mass = 9.0;                       // RobotState.h:23
  double ibody[3] = {.07f, 0.26f, 0.242f}; // RobotState.cpp:38 (float literals)
  double gravity = -9.8f;                  // SolverMPC.cpp:318
  int max_iter = 1000;
  double tol = 1e-9;
  float leg_geom[4] = {0.062f, 0.209f, 0.195f, 0.004f};  // MiniCheetah.h:31-37 (abad, hip, knee, knee Y offset)
  DevBuf<double> d_tables;  // coef[3][H] then ctab[9][H + 1][H + 1] (zero last row and column: the kernels' identity padding reads them)
  DevBuf<int> d_lists;      // [4][max_batch] robot ids handed to classes 4, 2 and 3, and to the large-problem producer
  DevBuf<int> d_counts;     // [3 sets][QMPC_COUNTERS] (layout in qmpc_device.h); sets 0 / 1 ping-ponged between calls, set 2: calls captured into a graph
  // decoupled path (sweep kernel -> work items -> engine kernel) of the 128- and 192-row classes: [0] class 2, [1] class 3
  int split = 1;               // qmpc_set_split: 0 off, 1 automatic (by batch size), 2 always; QMPC_NO_SPLIT=1 in the environment: 0 at creation
  DevBuf<double> d_wk_hinv[3];
  DevBuf<double> d_wk_xu[3];
  DevBuf<QmpcWorkHdr> d_wk_hdr[3];  // [2]: the large problems (192 < n_r <= 432)
  DevBuf<int> d_wk_order[3];
  DevBuf<double> d_wk_ovf[3];  // engine kernels' overflow event pools (one slice per resident workgroup)  // [QMPC_ORDER_BUCKETS][max_batch] item indices, hardest robots first
  int wk_cap[3] = {0, 0, 0};    // work items per class: a bounded pool, min(max_batch, QMPC_ITEMS_*) -- ensure_pools
  DevBuf<int> d_fb_lists;   // [3][max_batch] robots the engine kernels hand back (128-row, 192-row, large problems)
  int dense = 1;               // qmpc_set_dense: the 64-row class at five workgroups per CU -- 0 never, 1 automatic (by the handle's size), 2 whenever the chain is that class alone
  int chunks = 0;              // qmpc_set_chunks (test hook): run the item classes in at least this many chunks (0 / 1: as few as the pools allow)
  int dbg_engine_events = 0;   // test hook: events the engine may hold per robot (0 = the compiled capacity)
  PlanCounters ctr;  // the host-side call counters (call_no, hint_call, so_call, prio_call): plan_solve moves them
  // order hint (qmpc_set_order_hint): 0 off, 1 automatic -- a call whose first class is launched over more robots than it has
  // resident workgroups takes them in the order of the previous call's iteration counts (same batch size), longest first
  int order_hint = 1;
  DevBuf<int> d_hint_iters;  // [max_batch] iteration counts the one-kernel classes left in the previous call, then d_hint_max, d_cu_slots
  // size order (qmpc_set_size_order, default on): no hint usable (first call, another batch size, hint off) -> the first class of a
  // chain, launched over several rounds, takes the robots that fit it largest first by their contact tables; the permutation is
  // built inside the launch (qmpc_kernels.hip: size_order_build)
  int size_order = 1;
  DevBuf<unsigned long long> d_so_order;  // [max_batch] (call number << 32 | robot)
  DevBuf<unsigned long long> d_prio_cu;  // [2048] one-round launches without a hint: one word per CU (qmpc_device.h: prio_cu)
  int hint_batch = 0;           // batch size of the call that wrote d_hint_iters (0: none yet)
  int* d_hint_max = nullptr;    // (a view into d_hint_iters' block) [3] largest iteration count of the last calls (slots rotated by hint_call: read / fold / clear)
  int* d_cu_slots = nullptr;    // (a view into d_hint_iters' block)
  int bal_debug = 0;  // qmpc_set_debug_balance
  int max_stance = 0;          // caller's bound on stance foot-steps per robot (0 = unknown)
  int min_stance = 0;          // ... and lower bound (0 = unknown)
  int admm_mode = 0, admm_max_iter = 10000;  // JCQP alternate, see qmpc_settings_jcqp
  double admm_rho = 1e-7, admm_sigma = 1e-8, admm_alpha = 1.5, admm_term = 0.1;
  DevBuf<double> d_evpool;  // largest size class: global event pool (allocated on first use)
  DevBuf<double> d_ovpool;  // the other classes: overflow event pool, ov_nslice slices, recycled within a call (one flag per slice)
  DevBuf<int> d_ovflags;    // one per slice allocated (min(max_batch, 2048)): 0 = free
  int ov_nslice = 0;           // slices in use (all of them unless qmpc_set_debug_overflow_slices says fewer)
  int ov_spin = 1 << 22;       // probes of a robot that finds every slice taken before it gives up (test hook: qmpc_set_debug_overflow_slices)
  bool device_error = false;   // a HIP call of this handle failed since the last successful solve (fail()): see solve_impl
  DevBuf<int> d_evflags;
  int ev_nslot = 0;
  bool dbg_pool_busy = false;  // test hook: every slice of the 192-row class's pool looks taken (qmpc_set_debug_pool_busy)
  int32_t* ws = nullptr;  // warm-start buffer (device), see qmpc_set_warm_start
  int ws_shift = 1;
  int ws_min_iters = 0;   // qmpc_set_warm_start_min_iters: only robots with at least this many iterations in the previous call start warm
  double* dbg_H = nullptr;
  double* dbg_g = nullptr;
  double* dbg_aux = nullptr;
  long long* dbg_clk = nullptr;
  // staging for qmpc_solve_host
  DevBuf<char> d_stage;
  // the handle's device state (tables, work lists, counters) is ordered by ONE stream at a
  // time: a call that arrives on a different stream is made to wait for the previous one
  hipStream_t last_stream = nullptr;
  bool has_last = false;
  hipEvent_t order_ev = nullptr;
  // host-pointer entry point: its own stream, one pinned (device-visible) staging block
  hipStream_t host_stream = nullptr;
  hipEvent_t host_ev = nullptr;
  void* h_pin = nullptr;
  size_t pin_bytes = 0;
  double tab_dt = -1.0;  // (dt, horizon, model) the tables in d_tables were built for
  int tab_h = -1, tab_model = -1;
  int model = 0;         // QMPC_MODEL_*
  std::string err;
  // batched locomotion controller (qmpc_ctrl.h): device state for max_batch robots, made by qmpc_ctrl_init
  struct Ctrl {
    QmpcCtrlDev d{};
    DevBuf<char> buf;
    int batch = 0;       // robots initialised
    long long ticks = 0; // T: qmpc_ctrl_tick calls since qmpc_ctrl_init
    int schedule = QMPC_CTRL_LOCKSTEP;  // qmpc_ctrl_set_schedule
    int robot_mode = 0;                 // qmpc_ctrl_set_robot_mode (GaitCtrller::_robotMode)
    bool started = false;               // a tick or a reset has been enqueued since qmpc_ctrl_init: the schedule is fixed
    double freq = 0;                    // qmpc_ctrl_init's: the plant's dt is 1 / freq in double
    qmpc_fleet_info fleet{};            // how qmpc_fleet_run's ticks were served since qmpc_ctrl_init (qmpc_fleet.h)
    qmpc_loop_info loop{};              // ... and qmpc_loop_run's (qmpc_loop.h)
    bool ground_run = false;            // qmpc_ground_run_enable: both run calls serve rows and a field fused
  };
  std::unique_ptr<Ctrl> ctrl;
  // reduced-order plant (qmpc_plant.h): device state for max_batch robots, made by qmpc_plant_init
  struct Plant {
    QmpcPlantDev d{};
    DevBuf<char> buf;
    int batch = 0;  // robots initialised
    double mu = 0;
    int substeps = 1;
    // qmpc_plant_vary.h: the caller's arrays as bound (all null: none), the statistics' allocation and switch
    QmpcPlantVary vary{};
    bool bound = false;
    DevBuf<char> stats_buf;
    bool stats_on = false;
    // qmpc_terrain.h: the caller's rows as bound (null: flat ground) and the flags; ground[max_batch], support[max_batch]
    QmpcTerrainArgs terrain{};
    DevBuf<double> terrain_buf;
    // qmpc_contact.h: the flags and scalars as set (flags 0: off); slip[max_batch], drop[max_batch][4], early[max_batch],
    // late[max_batch] in one allocation; whether a contact step has written them since they were last all zero
    QmpcContactArgs contact{};
    DevBuf<double> contact_buf;
    bool contact_dirty = false;
    // qmpc_field.h: the caller's bank and placements as bound (z null: no field) and the binding's QMPC_TERRAIN_* flags
    QmpcFieldArgs field{};
    int field_flags = 0;
    // what a launcher is given for the terrain: the rows as bound (or none) under both bindings' flags (field_flags is 0
    // while no field is bound: without one this is `terrain` as it stands)
    QmpcTerrainArgs ground() const {
      QmpcTerrainArgs t = terrain;
      t.flags |= field_flags;
      return t;
    }
  };
  std::unique_ptr<Plant> plant;
  // sensor model (qmpc_sense.h): the counters n[max_batch], epoch[max_batch] in one allocation made by qmpc_sense_init,
  // the seed, and the caller's arrays as bound (all null: the ideal sensor)
  struct Sense {
    DevBuf<int> buf;
    int batch = 0;  // robots initialised
    uint64_t seed = 0;
    QmpcSenseArgs a{};
    bool bound = false;
  };
  std::unique_ptr<Sense> sense;
  // actuator stage (qmpc_act.h): head, age and the accumulators for max_batch robots in one allocation and the ring in
  // another, both made by qmpc_act_init; the config as given and the caller's arrays as bound (all null: the config's)
  struct Act {
    QmpcActArgs a{};
    DevBuf<char> buf;
    DevBuf<double> ring;
    int batch = 0;  // robots initialised
  };
  std::unique_ptr<Act> act;
  // episode manager (qmpc_episode.h): the per-robot state and the two log words in one allocation made by
  // qmpc_episode_init, the seed, and the rule and the caller's arrays as set (is_set: qmpc_episode_set has been called)
  struct Episode {
    QmpcEpisodeDev d{};
    DevBuf<char> buf;
    int batch = 0;  // robots initialised
    uint64_t seed = 0;
    qmpc_episode_rule rule{};
    qmpc_episode_bind bind{};
    bool is_set = false;
  };
  std::unique_ptr<Episode> episode;
  // episodes on the sensor path (qmpc_episode_sense.h): warm[max_batch], hold[max_batch] and the union the plant's reset is
  // given in one allocation made by qmpc_episode_sense_init, and the warm-up a robot gets when the manager resets it
  struct EpisodeSense {
    QmpcEpisodeSenseDev d{};
    DevBuf<char> buf;
    int batch = 0;  // robots initialised
    int warm_ticks = 0;
  };
  std::unique_ptr<EpisodeSense> episode_sense;
  // (the device arrays and the sub-states free themselves)
  ~qmpc_ctx() {
    if (h_pin) hipHostFree(h_pin);
    if (order_ev) hipEventDestroy(order_ev);
    if (host_ev) hipEventDestroy(host_ev);
    if (host_stream) hipStreamDestroy(host_stream);
  }
};

namespace qmpc_host {

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() { hipSetDevice(prev); }
};

inline int fail(qmpc_ctx* c, hipError_t e, const char* what) {
  c->err = std::string(what) + ": " + hipGetErrorString(e);
  c->device_error = true;  // (the next solve re-arms the device state a failed launch chain may have left behind)
  return QMPC_ERR_DEVICE;
}

#define HIP_TRY(ctx, call)                              \
  do {                                                  \
    hipError_t e__ = (call);                            \
    if (e__ != hipSuccess) return fail(ctx, e__, #call); \
  } while (0)

// One stream at a time orders the handle's device state.  A call on a different stream than the
// previous one waits (on the device, no host block) for everything the previous stream was given.
// (a stream that is being captured into a graph: the work becomes graph nodes; the legacy null stream cannot capture)
inline bool is_capturing(hipStream_t stream) {
  if (!stream) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

inline int order_after_previous(qmpc_ctx* c, hipStream_t stream) {
  // (captured calls: ordering against earlier work of the handle on OTHER streams is the caller's business -- an event
  //  recorded outside the capture cannot be waited for inside it)
  if (is_capturing(stream)) return QMPC_OK;
  if (c->has_last && c->last_stream != stream) {
    if (!c->order_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->order_ev, c->last_stream));
    HIP_TRY(c, hipStreamWaitEvent(stream, c->order_ev, 0));
  }
  c->last_stream = stream;
  c->has_last = true;
  return QMPC_OK;
}

// The preamble of an entry point that enqueues, after its checks: the handle's device current for as long as this lives,
// the caller's stream, ordered after whatever stream served the handle before.  rc != QMPC_OK: enqueue nothing
struct Enqueue {
  DeviceGuard g;
  hipStream_t stream;
  int rc;
  Enqueue(qmpc_ctx* c, void* stream_) : g(c->device), stream((hipStream_t)stream_), rc(order_after_previous(c, stream)) {}
};

// Mini Cheetah _abadLocation (MiniCheetah.h:25-26,105): the Kalman filter's hip location
inline constexpr float kAbadLocation[3] = {0.19f, 0.049f, 0.f};

// A sub-state of the handle (qmpc_ctx::Ctrl, ::Plant, ...): made on first use; made and initialised
template <class S>
S* made(std::unique_ptr<S>& s) {
  if (!s) s.reset(new S());
  return s.get();
}
template <class S>
bool ready(const std::unique_ptr<S>& s) {
  return s && s->batch;
}
inline bool ctrl_ready(const qmpc_ctx* c) { return ready(c->ctrl); }
inline bool plant_ready(const qmpc_ctx* c) { return ready(c->plant); }

// One array of an X-macro list (QMPC_CTRL_ARRAYS, QMPC_PLANT_ARRAYS, ...) laid out in an allocation: 256-byte aligned,
// per_robot elements for each of M robots (base == nullptr: only count).  A list's carve() is defined by the unit of the
// subsystem that owns it.
template <class T>
void carve_array(T*& member, char* base, size_t& off, int per_robot, int M) {
  off = (off + 255) & ~(size_t)255;
  member = base ? reinterpret_cast<T*>(base + off) : nullptr;
  off += sizeof(T) * (size_t)per_robot * (size_t)M;
}
#define QMPC_CARVE(T, name, per_robot) carve_array(d.name, base, off, per_robot, M);
size_t carve(QmpcCtrlDev& d, char* base, int M);          // qmpc_capi_ctrl.cpp
size_t carve(QmpcPlantDev& d, char* base, int M);         // qmpc_capi_plant.cpp
size_t carve(QmpcActDev& d, char* base, int M);           // qmpc_capi_stages.cpp
size_t carve(QmpcEpisodeDev& d, char* base, int M);       // ...
size_t carve(QmpcEpisodeSenseDev& d, char* base, int M);  // ...

// d's arrays as views into buf, which is allocated on first use (a later init of the same handle reuses the block)
template <class Dev>
hipError_t carve_block(DevBuf<char>& buf, Dev& d, int M) {
  if (!buf) {
    const hipError_t e = buf.alloc(carve(d, nullptr, M));
    if (e != hipSuccess) return e;
  }
  carve(d, buf, M);
  return hipSuccess;
}

// ---- what one unit defines for another ----

// qmpc_capi.cpp.  fill_ints: small device arrays are (re)set by a kernel, never by a memset node (see its definition).
// solve_impl: one solve, the record (`in`) or the controller command (`cmd`), optionally over a device-resident due list
hipError_t fill_ints(int* p, int n, int v, hipStream_t stream);
int solve_impl(qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_command* cmd, const qmpc_outputs* out,
               float* f_ff, void* stream_, const int* due_list = nullptr, int* due_count = nullptr);

// qmpc_capi_plant.cpp.  plant_check: controller and plant initialised, both for this batch (c may be null).
// plant_step_args: the argument block of a step, from the handle as it stands now and the call's three pointers
int plant_check(qmpc_ctx* c, int batch);
QmpcPlantStepArgs plant_step_args(qmpc_ctx* c, int batch, const double* effort, double* state_out, double* motor_out);

// The resets of the masked robots, as the episode managers chain them behind their decision.  For all of these the
// caller has made its checks, holds the DeviceGuard and has ordered the stream (an Enqueue in scope).
int ctrl_reset_counter0(qmpc_ctx::Ctrl* k);                                                 // qmpc_capi_ctrl.cpp
int ctrl_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, hipStream_t stream);  // ...
int plant_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, const double* init_xyyaw,
                        hipStream_t stream);                                                // qmpc_capi_plant.cpp

// qmpc_capi_stages.cpp.  What an episode decision reads of the handle's other state (the manager is initialised): the
// decision kernels' and the loop kernel's (qmpc_capi_ctrl.cpp: qmpc_loop_run)
QmpcEpisodeIn episode_inputs(const qmpc_ctx* c);

}  // namespace qmpc_host

#pragma GCC visibility pop

#endif
