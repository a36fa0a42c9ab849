// qmpc_capi.cpp -- host side of the C ABI declared in include/qmpc.h.
//
// Owns the per-handle device state that the reference keeps in file-scope
// globals (src/MPC_Ctrl/convexMPC_interface.cpp:13-20, SolverMPC.cpp:18-57):
// problem constants, the batch-constant coefficient tables, the size-class
// work lists, and staging buffers for the host-pointer entry point.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/qmpc.h"
#include "../../include/qmpc_debug.h"   // test / profiling hooks (same library)
#include "../../include/qmpc_expert.h"  // tuning knobs whose default is the measured optimum, warm start
#include "../../include/qmpc_ctrl.h"    // batched locomotion controller (same library)
#include "../../include/qmpc_plant.h"   // reduced-order plant for it (same library)
#include "../../include/qmpc_plant_vary.h"  // ... its per-robot parameters and on-device statistics
#include "../../include/qmpc_terrain.h"  // ... its per-robot slopes and stairs
#include "../../include/qmpc_contact.h"  // ... contact decided by the ground
#include "../../include/qmpc_field.h"    // ... height-field terrain from memory
#include "../../include/qmpc_sense.h"   // sensor model between the plant and the controller's sensor path
#include "../../include/qmpc_episode.h"  // episodes on the device: termination, respawn, result log
#include "../../include/qmpc_episode_sense.h"  // ... on the sensor path: per-robot warm-up after a reset
#include "../../include/qmpc_act.h"     // actuators between the controller's effort and the plant
#include "../../include/qmpc_fleet.h"   // the closed loop of controller and plant, many ticks in one call
#include "qmpc_device.h"
#include "qmpc_glue.h"    // each launcher is declared once, in the header its defining file includes too:
#include "qmpc_launch.h"  // qmpc_glue.h, qmpc_plant.h, qmpc_sense.h, qmpc_episode.h, qmpc_episode_sense.h, qmpc_act.h, and qmpc_launch.h for the rest
#include "qmpc_plan.h"  // the solve's launch plan (host-only)
#include "qmpc_plant.h"
#include "qmpc_sense.h"
#include "qmpc_episode.h"
#include "qmpc_episode_sense.h"
#include "qmpc_act.h"
#include "qmpc_span.h"  // the fleet run's plan (host-only) and the span kernel's launcher
static_assert(kLongHorizon == QMPC_LONG_HORIZON, "qmpc_plan.h and qmpc.h disagree");

extern "C" size_t qmpc_smem_bytes(int rb) {
  switch (rb) {
    case 1: return qmpc_c1_smem();
    case 2: return qmpc_c2_smem();
    case 3: return qmpc_c3_smem();
    case 4: return qmpc_c4_smem();
    case 6: return qmpc_c6_smem();
  }
  return 0;
}
extern "C" int qmpc_resident_blocks(int rb) {
  switch (rb) {
    case 1: return qmpc_c1_resident();
    case 2: return qmpc_c2_resident();
    case 3: return qmpc_c3_resident();
    case 4: return qmpc_c4_resident();
    case 6: return qmpc_c6_resident();
  }
  return 0;
}
static hipError_t qmpc_prepare(void) {
  hipError_t e;
  if ((e = qmpc_c1_prepare()) != hipSuccess) return e;
  if ((e = qmpc_c4_prepare()) != hipSuccess) return e;
  if ((e = qmpc_c6_prepare()) != hipSuccess) return e;
  if ((e = qmpc_c2_prepare()) != hipSuccess) return e;
  if ((e = qmpc_c3_prepare()) != hipSuccess) return e;
  if ((e = qmpc_big_prepare()) != hipSuccess) return e;
  return qmpc_engine_prepare();
}
static hipError_t qmpc_launch_sweep(int rb, const QmpcParams* P, int grid, hipStream_t stream) {
  return rb == 2 ? qmpc_c2_launch_sweep(P, grid, stream) : (rb == 3 ? qmpc_c3_launch_sweep(P, grid, stream) : hipErrorInvalidValue);
}
static int qmpc_resident_sweep(int rb) { return rb == 2 ? qmpc_c2_resident_sweep() : (rb == 3 ? qmpc_c3_resident_sweep() : 0); }
static hipError_t qmpc_launch(int rb, const QmpcParams* P, int grid, hipStream_t stream) {
  switch (rb) {
    case 1: return qmpc_c1_launch(P, grid, stream);
    case 2: return qmpc_c2_launch(P, grid, stream);
    case 3: return qmpc_c3_launch(P, grid, stream);
    case 4: return qmpc_c4_launch(P, grid, stream);
    case 6: return qmpc_c6_launch(P, grid, stream);
  }
  return hipErrorInvalidValue;
}

// Small device arrays are (re)set by this kernel, never by hipMemsetAsync: a memset node captured into a hipGraph writes
// garbage on replay with this runtime (ROCm 7.2: the counters came back as {512, 24111, 1, 24106, ...}; measured with
// tools/dbg/graph_probe.py), a kernel node replays correctly
__global__ void qmpc_fill_ints_kernel(int* p, int n, int v) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) p[k] = v;
}
static hipError_t fill_ints(int* p, int n, int v, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_fill_ints_kernel, dim3((n + 255) / 256 < 64 ? (n + 255) / 256 : 64), dim3(256), 0, stream, p, n, v);
  return hipGetLastError();
}

namespace {

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

}  // namespace

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

namespace {

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() { hipSetDevice(prev); }
};

int fail(qmpc_ctx* c, hipError_t e, const char* what) {
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
bool is_capturing(hipStream_t stream) {
  if (!stream) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

int order_after_previous(qmpc_ctx* c, hipStream_t stream) {
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

// The solve record (qmpc_inputs), described once: f(array, bytes per robot at horizon h, per robot?) for each of its
// arrays in declaration order.  weights / alpha / x_drag with stride 0 are one row shared by the batch.  `in` may be a
// copy whose pointers f rebinds.
template <class Record, class F>
void for_each_record_array(Record& in, size_t h, F&& f) {
  f(in.p, 4 * 3, true);
  f(in.v, 4 * 3, true);
  f(in.q, 4 * 4, true);
  f(in.w, 4 * 3, true);
  f(in.r, 4 * 12, true);
  f(in.yaw, 4, true);
  f(in.traj, 4 * 12 * h, true);
  f(in.gait, 4 * h, true);
  f(in.weights, 4 * 12, in.weights_stride != 0);
  f(in.alpha, 4, in.alpha_stride != 0);
  f(in.x_drag, 4, in.x_drag_stride != 0);
}
constexpr int kRecordArrays = 11;

// every array of the record given (need_x_drag = false: x_drag may be missing)
bool record_ok(const qmpc_inputs& in, bool need_x_drag = true) {
  int missing = 0;
  for_each_record_array(in, 0, [&](const void* p, size_t, bool) { missing += !p; });
  return missing == (need_x_drag || in.x_drag ? 0 : 1);
}

// the kernels' view of the record
void bind_record(QmpcParams& P, const qmpc_inputs& in) {
  P.p = in.p; P.v = in.v; P.q = in.q; P.w = in.w; P.r = in.r; P.yaw = in.yaw;
  P.traj = in.traj; P.gait = in.gait; P.weights = in.weights; P.alpha = in.alpha; P.x_drag = in.x_drag;
  P.weights_stride = in.weights_stride;
  P.alpha_stride = in.alpha_stride;
  P.x_drag_stride = in.x_drag_stride;
}

// Mini Cheetah _abadLocation (MiniCheetah.h:25-26,105): the Kalman filter's hip location
const float kAbadLocation[3] = {0.19f, 0.049f, 0.f};

}  // namespace

namespace {
int ensure_pools(qmpc_ctx* c);

// an allocation of n elements, zeroed
template <class T>
hipError_t alloc_zeroed(DevBuf<T>& b, size_t n) {
  const hipError_t e = b.alloc(n);
  return e == hipSuccess ? hipMemset(b, 0, sizeof(T) * n) : e;
}

// qmpc_create's device side: every array a handle has from the start, the kernels' attributes, the first launch
hipError_t create_device_state(qmpc_ctx* c) {
#define HIP_OK(call)                        \
  do {                                      \
    const hipError_t e__ = (call);          \
    if (e__ != hipSuccess) return e__;      \
  } while (0)
  const size_t H = (size_t)c->max_horizon, B = (size_t)c->max_batch;
  HIP_OK(c->d_tables.alloc(3 * H + 9 * (H + 1) * (H + 1)));
  HIP_OK(c->d_lists.alloc(4 * B));  // ([3]: the large problems, horizons > 16)
  HIP_OK(alloc_zeroed(c->d_counts, 3 * QMPC_COUNTERS));
  HIP_OK(c->d_fb_lists.alloc(3 * B));
  HIP_OK(alloc_zeroed(c->d_hint_iters, B + 4 + 2048));  // [max_batch] hint iterations, [4] d_hint_max, [2048] d_cu_slots
  c->d_hint_max = c->d_hint_iters + B;
  c->d_cu_slots = c->d_hint_max + 4;  // [2048] the 96-row class's per-CU placement words (zero whenever no kernel runs)
  HIP_OK(alloc_zeroed(c->d_prio_cu, 2048));
  HIP_OK(alloc_zeroed(c->d_so_order, 2 * B));  // near copy, far copy (call numbers start at 1)
  // a robot whose on-chip event pool fills up continues here.  The slices are RECYCLED within a call (one flag per slice,
  // taken with a compare-and-swap, released when its robot is done): ov_nslice bounds the robots that hold one AT THE SAME
  // TIME, not the robots of a call; a robot that finds every slice taken waits (ov_spin probes), then falls back to the
  // Schur-form engine.  Every flag is 0 between calls; after a call that ended in a device error they are re-armed
  // (solve_impl) -- a flag left at 1 would otherwise be lost for the life of the handle
  // (2048 slices of 192 KiB: what a call of 8192 robots needs when the 64-row class runs five per CU ahead of larger
  //  classes -- qmpc_plan.h: plan_solve)
  c->ov_nslice = c->max_batch < 2048 ? c->max_batch : 2048;
  HIP_OK(c->d_ovpool.alloc((size_t)c->ov_nslice * QMPC_OV_SLICE));
  HIP_OK(alloc_zeroed(c->d_ovflags, (size_t)c->ov_nslice));
  HIP_OK(qmpc_prepare());
  // the runtime loads a translation unit's code object at the first launch of one of its kernels (2 MiB of device
  // memory): this file's small kernel (fill) is first launched HERE, not inside some later solve call
  HIP_OK(fill_ints(c->d_hint_max, 4, 0, nullptr));
  return hipStreamSynchronize(nullptr);
#undef HIP_OK
}
}  // namespace

extern "C" {

int qmpc_abi_version(void) { return 23; }  // 23: the batched locomotion controller (qmpc_ctrl.h) added; no signature changed
int qmpc_max_horizon(void) { return QMPC_MAX_HORIZON; }

const char* qmpc_last_error(qmpc_handle h) { return h ? h->err.c_str() : "null handle"; }

int qmpc_create(int device_id, int max_batch, int max_horizon, qmpc_handle* out) {
  if (!out || max_batch <= 0 || max_horizon <= 0 || max_horizon > QMPC_MAX_HORIZON)
    return QMPC_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev)
    return QMPC_ERR_DEVICE;
  qmpc_ctx* c = new qmpc_ctx();
  c->device = device_id;
  c->max_batch = max_batch;
  c->max_horizon = max_horizon;
  const char* ns = std::getenv("QMPC_NO_SPLIT");
  c->split = (ns && ns[0] == '1') ? 0 : 1;
  DeviceGuard g(device_id);
  if (create_device_state(c) != hipSuccess) {
    qmpc_destroy(c);
    return QMPC_ERR_DEVICE;
  }
  *out = c;
  return QMPC_OK;
}

int qmpc_destroy(qmpc_handle h) {
  if (!h) return QMPC_ERR_ARG;
  DeviceGuard g(h->device);
  delete h;
  return QMPC_OK;
}

int qmpc_setup(qmpc_handle c, double dt, int horizon, double mu, double f_max) {
  if (!c) return QMPC_ERR_ARG;
  // (a NaN f_max would switch every fz <= f_max row off without a status bit: no comparison with it is ever true)
  if (horizon <= 0 || horizon > c->max_horizon || !(mu > 0) || !(dt > 0) || f_max != f_max) return QMPC_ERR_ARG;
  // struct problem_setup stores floats (convexMPC_interface.h:13-19)
  c->dt = (double)(float)dt;
  c->mu = (double)(float)mu;
  c->f_max = (double)(float)f_max;
  c->horizon = horizon;
  const int h = horizon;
  if (12 * h > 128 && !c->d_evpool) {
    // the 192-row class keeps its rank-1 events in global memory: one 400 KiB slice (QMPC_EV_SLICE3) per workgroup in
    // flight (256 CUs x 1 workgroup); 1024 flag-guarded slices, so that a slice's previous tenant has usually finished
    // (a workgroup whose predecessor on its slice is still running waits for it).  Allocated here, where the
    // horizon that makes the class reachable is announced -- never inside a solve call (a hipMalloc there
    // synchronises the device and cannot be captured into a graph)
    DeviceGuard g0(c->device);
    const int nslot = c->max_batch < 1024 ? c->max_batch : 1024;
    HIP_TRY(c, c->d_evpool.alloc((size_t)nslot * QMPC_EV_SLICE3));
    HIP_TRY(c, alloc_zeroed(c->d_evflags, (size_t)nslot));
    c->ev_nslot = nslot;
  }
  // the tables depend on (dt, horizon) only: the reference's caller repeats setup_problem with the
  // same values before every solve (ConvexMPCLocomotion.cpp:630), which costs nothing here
  if (c->is_setup && c->tab_dt == c->dt && c->tab_h == h && c->tab_model == c->model) return ensure_pools(c);
  // coefficient tables (see qmpc_device.h); A_ct^3 = 0 makes
  // Adt^d Bdt = dt B + c_d A B + e_d A^2 B exact.
  const int hs = h + 1;  // row stride of the C_pq tables: row h and column h stay zero
  std::vector<double> t(3 * h + 9 * hs * hs, 0.0);
  double* coef = t.data();
  double* ctab = t.data() + 3 * h;
  const double d1 = c->dt;
  for (int d = 0; d < h; ++d) {
    coef[0 * h + d] = d1;
    const double dp = d + 1.0;
    if (c->model == QMPC_MODEL_SPARSE) {
      // SparseCMPC: A_d^d B_d = (I + d dt A) B dt = dt B + d dt^2 A B  (A^2 = 0; no drag term)
      coef[1 * h + d] = (double)d * d1 * d1;
      coef[2 * h + d] = 0.0;
    } else {
      coef[1 * h + d] = (2.0 * d + 1.0) * d1 * d1 / 2.0;
      coef[2 * h + d] = (dp * dp * dp - (double)d * d * d) * d1 * d1 * d1 / 6.0;
    }
  }
  for (int p = 0; p < 3; ++p)
    for (int q = 0; q < 3; ++q)
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < h; ++j) {
          double s = 0.0;
          for (int k = (i > j ? i : j); k < h; ++k) s += coef[p * h + (k - i)] * coef[q * h + (k - j)];
          ctab[((p * 3 + q) * hs + i) * hs + j] = s;
        }
  DeviceGuard g(c->device);
  // solves still in flight read the old tables: wait for the stream that orders this handle
  if (c->has_last) HIP_TRY(c, hipStreamSynchronize(c->last_stream));
  HIP_TRY(c, hipMemcpy(c->d_tables, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
  c->tab_dt = c->dt;
  c->tab_h = h;
  c->tab_model = c->model;
  c->is_setup = true;
  // every pool a solve at this horizon can need is allocated now: no solve call allocates (a hipMalloc synchronises
  // the device and cannot be captured into a graph)
  return ensure_pools(c);
}

int qmpc_set_robot(qmpc_handle c, double mass, const double ibody_diag[3], double gravity) {
  if (!c || !ibody_diag || !(mass > 0)) return QMPC_ERR_ARG;
  for (int k = 0; k < 3; ++k)
    if (!(ibody_diag[k] > 0)) return QMPC_ERR_ARG;
  c->mass = mass;
  for (int k = 0; k < 3; ++k) c->ibody[k] = ibody_diag[k];
  c->gravity = gravity;
  return QMPC_OK;
}

int qmpc_settings(qmpc_handle c, int max_iter, double tol) {
  if (!c || max_iter <= 0 || !(tol >= 0)) return QMPC_ERR_ARG;
  c->max_iter = max_iter;
  c->tol = tol;
  return QMPC_OK;
}

int qmpc_set_max_stance(qmpc_handle c, int max_stance_footsteps) {
  if (!c || max_stance_footsteps < 0) return QMPC_ERR_ARG;
  c->max_stance = max_stance_footsteps;
  return ensure_pools(c);  // (a wider hint can make a larger class reachable)
}

int qmpc_set_min_stance(qmpc_handle c, int min_stance_footsteps) {
  if (!c || min_stance_footsteps < 0) return QMPC_ERR_ARG;
  c->min_stance = min_stance_footsteps;
  return ensure_pools(c);
}

int qmpc_set_model(qmpc_handle c, int model) {
  if (!c || (model != QMPC_MODEL_DENSE && model != QMPC_MODEL_SPARSE)) return QMPC_ERR_ARG;
  if (model != c->model) {
    c->model = model;
    if (c->is_setup) return qmpc_setup(c, c->dt, c->horizon, c->mu, c->f_max);  // rebuild the tables
  }
  return QMPC_OK;
}

int qmpc_settings_jcqp(qmpc_handle c, int use_jcqp, int max_iter, double rho, double sigma, double solver_alpha,
                       double terminate) {
  if (!c || use_jcqp < 0 || use_jcqp > 2) return QMPC_ERR_ARG;
  if (use_jcqp && (max_iter <= 0 || !(rho > 0) || !(sigma >= 0) || !(solver_alpha > 0) || !(terminate >= 0)))
    return QMPC_ERR_ARG;
  c->admm_mode = use_jcqp;
  if (use_jcqp) {
    c->admm_max_iter = max_iter;
    c->admm_rho = rho;
    c->admm_sigma = sigma;
    c->admm_alpha = solver_alpha;
    c->admm_term = terminate;
  }
  return ensure_pools(c);  // (the alternate's launch plan can reach the large-problem pool where the exact solve's does not)
}

int qmpc_set_warm_start(qmpc_handle c, int32_t* ws_dev, int shift_steps) {
  if (!c || shift_steps < 0) return QMPC_ERR_ARG;
  c->ws = ws_dev;
  c->ws_shift = shift_steps;
  return QMPC_OK;
}

int qmpc_set_warm_start_min_iters(qmpc_handle c, int min_iters) {
  if (!c || min_iters < 0) return QMPC_ERR_ARG;
  if (min_iters > 0 && !c->order_hint) return QMPC_ERR_STATE;  // the selection reads the counts the order hint keeps
  c->ws_min_iters = min_iters;
  return QMPC_OK;
}

int qmpc_set_debug(qmpc_handle c, double* H_dev, double* g_dev) {
  if (!c) return QMPC_ERR_ARG;
  c->dbg_H = H_dev;
  c->dbg_g = g_dev;
  return QMPC_OK;
}

int qmpc_set_debug_overflow_spin(qmpc_handle c, int probes) {
  if (!c) return QMPC_ERR_ARG;
  c->ov_spin = probes < 0 ? (1 << 22) : probes;
  return QMPC_OK;
}

int qmpc_set_debug_overflow_slices(qmpc_handle c, int n) {
  if (!c) return QMPC_ERR_ARG;
  const int allocated = (int)c->d_ovflags.n;
  if (n > allocated) return QMPC_ERR_ARG;  // more slices than allocated
  c->ov_nslice = n < 0 ? allocated : n;
  return QMPC_OK;
}

int qmpc_set_split(qmpc_handle c, int on) {
  if (!c) return QMPC_ERR_ARG;
  if (on < 0 || on > 2) return QMPC_ERR_ARG;
  c->split = on;
  return ensure_pools(c);
}

int qmpc_set_dense(qmpc_handle c, int mode) {
  if (!c || mode < 0 || mode > 2) return QMPC_ERR_ARG;
  c->dense = mode;
  return QMPC_OK;
}

int qmpc_set_debug_balance(qmpc_handle c, int mode) {
  if (!c || mode < 0 || mode > 2) return QMPC_ERR_ARG;
  c->bal_debug = mode;
  return QMPC_OK;
}

int qmpc_debug_keys(qmpc_handle c, int batch, const qmpc_inputs* in, int32_t* nst_dev, float* score_dev, float* demand_dev,
                    void* stream_) {
  if (!c || !in || !nst_dev || !score_dev || !demand_dev) return QMPC_ERR_ARG;
  if (!c->is_setup) return QMPC_ERR_STATE;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  if (!record_ok(*in, false) || ((uintptr_t)in->gait & 3u)) return QMPC_ERR_ARG;  // (the key pass reads no x_drag)
  DeviceGuard g(c->device);
  QmpcParams P;
  std::memset(&P, 0, sizeof(P));
  bind_record(P, *in);
  P.batch = batch; P.horizon = c->horizon;
  P.dt = c->dt;
  P.mu_inv = (double)(1.f / (float)c->mu);
  P.mass = c->mass;
  P.gravity = c->gravity;
  HIP_TRY(c, qmpc_launch_keys(&P, nst_dev, score_dev, demand_dev, (hipStream_t)stream_));
  return QMPC_OK;
}

int qmpc_set_size_order(qmpc_handle c, int on) {
  if (!c || on < 0 || on > 1) return QMPC_ERR_ARG;
  c->size_order = on;
  return QMPC_OK;
}

int qmpc_set_order_hint(qmpc_handle c, int mode) {
  if (!c || mode < 0 || mode > 1) return QMPC_ERR_ARG;
  c->order_hint = mode;
  c->hint_batch = 0;
  return QMPC_OK;
}

int qmpc_set_chunks(qmpc_handle c, int n) {
  if (!c || n < 0 || n > 64) return QMPC_ERR_ARG;
  c->chunks = n;
  return QMPC_OK;
}

int qmpc_set_debug_engine_events(qmpc_handle c, int n) {
  if (!c || n < 0) return QMPC_ERR_ARG;
  c->dbg_engine_events = n;
  return QMPC_OK;
}

int qmpc_reserve(qmpc_handle c) {
  if (!c) return QMPC_ERR_ARG;
  if (!c->is_setup) return QMPC_ERR_STATE;
  DeviceGuard g(c->device);
  return ensure_pools(c);  // (qmpc_setup and the hint setters have done this already: kept for callers of earlier versions)
}

int qmpc_set_debug_pool_busy(qmpc_handle c, int on) {
  if (!c) return QMPC_ERR_ARG;
  c->dbg_pool_busy = on != 0;
  return QMPC_OK;
}

int qmpc_set_debug_aux(qmpc_handle c, double* aux_dev) {
  if (!c) return QMPC_ERR_ARG;
  c->dbg_aux = aux_dev;
  return QMPC_OK;
}

int qmpc_debug_ld(qmpc_handle) { return QMPC_DBG_LD; }

// test hook: a work item of the decoupled path after a solve -- which: 0 = 128-row class, 1 = 192-row class, 2 = large
// problems; hinv_host: ld x ld doubles (ld = 128 / 192 / 448), xu_host: ld doubles, hdr4: {rid, n, nst, status0}
int qmpc_debug_read_item(qmpc_handle c, int which, int item, double* hinv_host, double* xu_host, int* hdr4) {
  if (!c || which < 0 || which > 2 || c->wk_cap[which] <= 0 || item < 0 || item >= c->wk_cap[which]) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  const size_t ld = kItems[which].ld;
  HIP_TRY(c, hipDeviceSynchronize());
  if (hinv_host) HIP_TRY(c, hipMemcpy(hinv_host, c->d_wk_hinv[which] + (size_t)item * ld * ld, sizeof(double) * ld * ld, hipMemcpyDeviceToHost));
  if (xu_host) HIP_TRY(c, hipMemcpy(xu_host, c->d_wk_xu[which] + (size_t)item * ld, sizeof(double) * ld, hipMemcpyDeviceToHost));
  if (hdr4) HIP_TRY(c, hipMemcpy(hdr4, c->d_wk_hdr[which] + item, sizeof(int) * 4, hipMemcpyDeviceToHost));
  return QMPC_OK;
}

int qmpc_debug_read_counts(qmpc_handle c, int* host768) {
  if (!c || !host768) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(host768, c->d_counts, sizeof(int) * 3 * QMPC_COUNTERS, hipMemcpyDeviceToHost));
  return QMPC_OK;
}

int qmpc_set_debug_clock(qmpc_handle c, long long* clk_dev) {
  if (!c) return QMPC_ERR_ARG;
  c->dbg_clk = clk_dev;
  return QMPC_OK;
}

}  // extern "C"

namespace {

bool command_ok(const qmpc_command* cmd) {
  return cmd->position && cmd->v_world && cmd->omega_world && cmd->orientation && cmd->rpy && cmd->r_body &&
         cmd->p_foot && cmd->vel_des && cmd->yaw_des_true && cmd->rpy_comp && cmd->gait_offsets &&
         cmd->gait_durations && cmd->gait_iteration && cmd->world_position_desired && cmd->x_comp_integral &&
         !(cmd->gait_type && !cmd->stand_traj);  // a standing robot needs its stand_traj row
}

// the handle's settings as the launch plan reads them (qmpc_plan.h): for the solve and for the allocation of the pools
PlanSettings plan_settings(const qmpc_ctx* c) {
  PlanSettings s;
  s.horizon = c->horizon; s.max_batch = c->max_batch; s.max_stance = c->max_stance; s.min_stance = c->min_stance;
  s.split = c->split; s.dense = c->dense; s.chunks = c->chunks; s.admm_mode = c->admm_mode;
  s.order_hint = c->order_hint; s.size_order = c->size_order; s.hint_batch = c->hint_batch;
  for (int sk = 0; sk < 3; ++sk) s.wk_cap[sk] = c->wk_cap[sk];
  s.has_ws = c->ws != nullptr; s.has_evflags = c->d_evflags.p != nullptr;
  return s;
}

// the kernels' occupancy numbers (cached by the kernels' translation units after the first question)
PlanResident plan_resident() {
  PlanResident r;
  for (const int cls : {1, 2, 3, 4, 6}) r.blocks[cls] = qmpc_resident_blocks(cls);
  for (const int cls : {2, 3}) r.sweep[cls] = qmpc_resident_sweep(cls);
  for (const int cls : {2, 3, 5}) r.engine[cls] = qmpc_engine_resident(cls);
  return r;
}

// one pool of work items (qmpc_plan.h: kItems)
int ensure_items(qmpc_ctx* c, int sk) {
  if (c->wk_cap[sk] > 0) return QMPC_OK;  // (set last: a pool counts as present only when ALL its arrays are)
  const size_t ld = kItems[sk].ld;
  const size_t cap = (size_t)(c->max_batch < kItems[sk].limit ? c->max_batch : kItems[sk].limit);
  // (the engine grid never exceeds the resident workgroups: slice = blockIdx.x)
  size_t wgs = (size_t)qmpc_engine_resident(kItems[sk].cls);
  if (wgs == 0 || wgs > cap) wgs = cap;
  // all or nothing: an allocation that fails half-way (the pools are up to 1.5 GiB) must not leave a pool that LOOKS
  // present -- the next solve would divide by wk_cap == 0 or launch on null arrays.  So: into locals, which free what they
  // got when one of them fails, and into the handle by move when all of them succeeded
  hipError_t e;
  {
    DevBuf<double> hinv, xu, ovf;
    DevBuf<QmpcWorkHdr> hdr;
    DevBuf<int> order;
    e = hinv.alloc(cap * ld * ld);
    if (e == hipSuccess) e = xu.alloc(cap * ld);
    if (e == hipSuccess) e = hdr.alloc(cap);
    if (e == hipSuccess) e = order.alloc(QMPC_ORDER_BUCKETS * cap);
    if (e == hipSuccess) e = ovf.alloc(wgs * QMPC_ENGINE_OVF_EVENTS * kItems[sk].ev_doubles);
    if (e == hipSuccess) {
      c->d_wk_hinv[sk] = std::move(hinv); c->d_wk_xu[sk] = std::move(xu); c->d_wk_hdr[sk] = std::move(hdr);
      c->d_wk_order[sk] = std::move(order); c->d_wk_ovf[sk] = std::move(ovf);
      c->wk_cap[sk] = (int)cap;
      return QMPC_OK;
    }
  }
  (void)hipGetLastError();
  return fail(c, e, "work-item pool allocation");
}

// Every pool the current setup, stance hints and split mode can reach, allocated NOW (qmpc_setup, the hint setters,
// qmpc_set_split, qmpc_reserve call this): a solve call never allocates.  The pools are bounded by QMPC_ITEMS_*,
// not by max_batch: a call with more robots than items runs the class in consecutive chunks.
int ensure_pools(qmpc_ctx* c) {
  if (!c->is_setup) return QMPC_OK;
  DeviceGuard g(c->device);
  const unsigned pools = plan_pools(plan_settings(c));  // (the union of the plans a solve on this handle can make)
  for (int sk = 0; sk < 3; ++sk)
    if (pools >> sk & 1u)
      if (const int rc = ensure_items(c, sk)) return rc;
  return QMPC_OK;
}

// everything that can refuse a solve call, BEFORE the call counter moves: the counter sets ping-pong between calls and
// each call's first kernel zeroes the NEXT call's set, so a call that took a set without launching would leave the
// following call on counters nobody cleared.  (batch == 0: nothing to solve, whatever else the call says)
int check_solve_call(qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_command* cmd, const qmpc_outputs* out,
                     const int* due_list, const int* due_count) {
  if (!c || (!in && !cmd) || !out) return QMPC_ERR_ARG;
  if ((due_list != nullptr) != (due_count != nullptr) || (due_list && !cmd)) return QMPC_ERR_ARG;
  if (!c->is_setup) return QMPC_ERR_STATE;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  if (!out->grf || !out->status) return QMPC_ERR_ARG;
  if (in) {
    if (!record_ok(*in)) return QMPC_ERR_ARG;
    if ((in->weights_stride != 0 && in->weights_stride != 12) || (in->alpha_stride & ~1) ||
        (in->x_drag_stride & ~1))
      return QMPC_ERR_ARG;
  } else if (!command_ok(cmd)) {
    return QMPC_ERR_ARG;
  }
  const unsigned pools = plan_pools(plan_classes(plan_settings(c), in ? c->admm_mode : 0, c->ws != nullptr));
  for (int sk = 0; sk < 3; ++sk)
    if ((pools >> sk & 1u) && c->wk_cap[sk] <= 0) {
      c->err = sk == 2 ? "large-problem pool missing (qmpc_setup / qmpc_reserve allocate it)"
                       : "work-item pool missing (qmpc_setup / qmpc_reserve allocate it)";
      return QMPC_ERR_STATE;
    }
  return QMPC_OK;
}

// the kernel parameter block of a call, but for what differs from launch to launch (lists, counters, work items, order)
QmpcParams bind_params(const qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_command* cmd,
                       const qmpc_outputs* out, float* f_ff, bool capturing) {
  QmpcParams P;
  std::memset(&P, 0, sizeof(P));
  const int h = c->horizon;
  if (in) {
    bind_record(P, *in);
  } else {
    P.c_position = cmd->position; P.c_v_world = cmd->v_world; P.c_omega_world = cmd->omega_world;
    P.c_orientation = cmd->orientation; P.c_rpy = cmd->rpy; P.c_r_body = cmd->r_body; P.c_p_foot = cmd->p_foot;
    P.c_vel_des = cmd->vel_des; P.c_yaw_des_true = cmd->yaw_des_true; P.c_rpy_comp = cmd->rpy_comp;
    P.c_stand_traj = cmd->stand_traj; P.c_rp_des = cmd->rp_des; P.c_gait_type = cmd->gait_type;
    P.c_gait_offsets = cmd->gait_offsets; P.c_gait_durations = cmd->gait_durations;
    P.c_gait_iteration = cmd->gait_iteration; P.c_wpd = cmd->world_position_desired;
    P.c_xci = cmd->x_comp_integral; P.c_body_height = cmd->body_height; P.c_omni_mode = cmd->omni_mode;
    P.f_ff = f_ff;
  }
  P.grf = out->grf; P.soln = out->soln; P.status = out->status; P.iters = out->iters;
  P.batch = batch; P.horizon = h;
  P.dt = c->dt;
  // fpt mu = 1.f/setup->mu  (SolverMPC.cpp:366), float arithmetic
  const float mi = 1.f / (float)c->mu;
  P.mu_inv = (double)mi;
  P.inv_fr_norm = 1.0 / std::sqrt(P.mu_inv * P.mu_inv + 1.0);
  P.f_max = c->f_max; P.mass = c->mass; P.inv_mass = 1.0 / c->mass; P.gravity = c->gravity; P.model = c->model;
  for (int k = 0; k < 3; ++k) P.ibody[k] = c->ibody[k], P.inv_ibody[k] = 1.0 / c->ibody[k];
  P.coef = c->d_tables; P.ctab = c->d_tables + 3 * h;
  P.max_iter = c->max_iter; P.tol = c->tol;
  P.ws = c->ws; P.ws_shift = c->ws_shift;
  // selective warm start: the selection reads the previous call's iteration counts, which exist only while the order hint is on,
  // the call is eager (not captured) and the previous call had this batch size; without them NOBODY qualifies (every robot
  // starts cold) -- eager and captured calls, first and later calls behave alike
  P.ws_min_iters = (c->ws_min_iters > 0 && !(c->order_hint && !capturing && c->hint_batch == batch)) ? 0x7fffffff : c->ws_min_iters;
  if (c->admm_mode && in) {  // (record mode only: the command mode always solves exactly)
    P.admm_mode = c->admm_mode; P.admm_max_iter = c->admm_max_iter;
    P.admm_rho = c->admm_rho; P.admm_sigma = c->admm_sigma; P.admm_alpha = c->admm_alpha; P.admm_term = c->admm_term;
  }
  P.dbg_H = c->dbg_H; P.dbg_g = c->dbg_g; P.dbg_aux = c->dbg_aux; P.dbg_clk = c->dbg_clk;
  P.hint_iters = (c->order_hint && !capturing) ? c->d_hint_iters : nullptr;
  // (selective warm start without usable counts -- hint off, captured call: P.hint_iters stays null, which the kernel reads as
  //  "nobody qualifies", and the call -- and every replay of it -- leaves d_hint_iters alone: a later eager call of the batch
  //  size in hint_batch never selects or orders by counts that an unrelated call wrote)
  P.cu_slots = c->d_cu_slots; P.bal_debug = c->bal_debug;
  P.ovpool = c->d_ovpool; P.ov_nslice = c->ov_nslice; P.ov_flags = c->d_ovflags; P.ov_spin = c->ov_spin;
  P.evpool = c->d_evpool; P.evflags = c->d_evflags; P.ev_nslot = c->ev_nslot;
  P.ev_spin = c->dbg_pool_busy ? 4 : (1 << 16);
  return P;
}

// The plan's launches, in order, on the caller's stream.  Every launch gets a COPY of the bound parameter block with its
// own lists, counters, work items and ordering fields resolved to the handle's arrays: nothing is shared between
// launches, so nothing has to be reset after one.
int enqueue(qmpc_ctx* c, const QmpcParams& bound, const SolvePlan& sp, const int* due_list, int* due_count,
            hipStream_t stream) {
  int* const cnt = c->d_counts + QMPC_COUNTERS * sp.set;  // this call's counters
  int* const cnt_next = sp.set == 2 ? nullptr : c->d_counts + QMPC_COUNTERS * (sp.set ^ 1);  // the next eager call's
  const auto counter = [&](int i) { return i == kNoCounter ? nullptr : (i == kDueCounter ? due_count : cnt + i); };
  const auto list = [&](const ListRef& r) -> const int* {
    switch (r.kind) {
      case LIST_SLOT: return c->d_lists + (size_t)r.idx * c->max_batch;
      case LIST_DUE: return due_list;
      case LIST_HANDBACK: return c->d_fb_lists + (size_t)r.idx * c->max_batch;
      default: return nullptr;
    }
  };
  for (const Launch& L : sp.launches) {
    if (L.kind <= FILL_PRIO) {  // (FILL_EVFLAGS: no kernel of this handle is in flight on another stream -- ordered by solve_impl)
      if (L.kind == FILL_COUNTERS) HIP_TRY(c, fill_ints(cnt, QMPC_COUNTERS, 0, stream));
      else if (L.kind == FILL_EVFLAGS) HIP_TRY(c, fill_ints(c->d_evflags, c->ev_nslot, c->dbg_pool_busy ? 1 : 0, stream));
      else HIP_TRY(c, fill_ints(reinterpret_cast<int*>(c->d_prio_cu.p), 2 * 2048, 0, stream));
      continue;
    }
    QmpcParams P = bound;
    P.ov_count = cnt + QMPC_CNT_OV;  // slices of the overflow pool handed out in this call
    P.list = list(L.list); P.count = counter(L.count); P.qhead = counter(L.qhead);
    P.next_list = L.next.kind == LIST_SLOT ? c->d_lists + (size_t)L.next.idx * c->max_batch : nullptr;
    P.next_count = counter(L.next_count);
    P.clear_counts = L.clear_counts ? cnt_next : nullptr;
    P.status_or = L.status_or; P.rid0 = L.rid0; P.list_hi = L.list_hi;
    if (L.kind != SOLVE) {  // the work items of pool sk, the counter group of the chunk
      const int sk = L.sk;
      int* const grp = cnt + QMPC_CNT_GRP(sk, L.grp);
      P.wk_hinv = c->d_wk_hinv[sk]; P.wk_xu = c->d_wk_xu[sk]; P.wk_hdr = c->d_wk_hdr[sk];
      P.wk_order = c->d_wk_order[sk]; P.wk_ovf = c->d_wk_ovf[sk];
      P.wk_ld = kItems[sk].ld; P.wk_cap = c->wk_cap[sk];
      P.wk_kev = c->dbg_engine_events > 0 ? c->dbg_engine_events : (1 << 20);
      P.fb_list = c->d_fb_lists + (size_t)sk * c->max_batch; P.fb_count = cnt + QMPC_CNT_FB + sk;
      P.wk_count = grp; P.wk_qhead = grp + 1; P.wk_bucket = grp + 8;
      P.wk_zero = L.wk_zero ? cnt + QMPC_CNT_GRP(sk, L.grp ^ 1) : nullptr;
    }
    if (L.hint_max_w != kNoCounter) {
      P.hint_max_r = c->d_hint_max + L.hint_max_r; P.hint_max_w = c->d_hint_max + L.hint_max_w;
      P.hint_max_z = c->d_hint_max + L.hint_max_z; P.hint_hard = L.hint_hard;
    }
    if (L.so_tag) {
      P.so_order = c->d_so_order; P.so_far = c->d_so_order + c->max_batch;
      P.so_hint = L.so_keys_from_hint ? c->d_hint_iters : nullptr;
      P.so_tag = L.so_tag; P.so_first = L.so_first; P.so_nseg = L.so_nseg; P.so_maxfit = L.so_maxfit;
    }
    if (L.prio_tag) P.prio_cu = c->d_prio_cu, P.prio_tag = L.prio_tag;
    switch (L.kind) {
      case SOLVE: HIP_TRY(c, qmpc_launch(L.cls, &P, L.grid, stream)); break;
      case SWEEP: HIP_TRY(c, qmpc_launch_sweep(L.cls, &P, L.grid, stream)); break;
      case BIG_PRODUCER: HIP_TRY(c, qmpc_big_launch(&P, L.grid, stream)); break;
      case ENGINE: HIP_TRY(c, qmpc_engine_launch(L.cls, &P, L.grid, stream)); break;
      default: HIP_TRY(c, qmpc_admm_big_launch(&P, L.grid, stream)); break;
    }
  }
  return QMPC_OK;
}

// one solve: inputs either as the record (`in`) or as the controller command (`cmd`, record built in stage 0).
// due_list / due_count (internal, device-resident, command mode only; nullptr: every robot of the batch): the dense list
// of the robots this call solves and its length, both written on the device by work enqueued before the call (the
// batched controller's per-robot schedule).  A robot that is not listed is not scheduled at all: the first class of
// the chain maps its workgroups to robots through the list and those beyond the device-side count leave at once, as
// the later classes do with theirs, so the robot runs no QP, reaches no later list, no engine and no overflow slice, and
// none of its outputs or command rows is written.
// Check, bind, plan (qmpc_plan.h: a value, no device involved), enqueue.
int solve_impl(qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_command* cmd, const qmpc_outputs* out,
               float* f_ff, void* stream_, const int* due_list = nullptr, int* due_count = nullptr) {
  if (const int rc = check_solve_call(c, batch, in, cmd, out, due_list, due_count)) return rc;
  if (batch == 0) return QMPC_OK;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  hipStream_t stream = q.stream;
  const bool capturing = is_capturing(stream);
  if (c->device_error && !capturing) {
    // the previous call (or set-up step) of this handle failed on the device: whatever its kernels left in the
    // recycled-slice flags and the per-CU placement words is void.  Re-armed with the fill kernel (no memset node: they
    // replay wrongly when captured, and this path must not differ from the normal one in kind)
    if (c->d_ovflags && c->ov_nslice > 0) HIP_TRY(c, fill_ints(c->d_ovflags, (int)c->d_ovflags.n, 0, stream));
    c->device_error = false;
  }
  const QmpcParams P = bind_params(c, batch, in, cmd, out, f_ff, capturing);
  const PlanCall call{batch, capturing, cmd != nullptr, due_list != nullptr, (unsigned)((uintptr_t)P.gait & 7u), P.admm_mode};
  const SolvePlan sp = plan_solve(plan_settings(c), call, plan_resident(), c->ctr);
  if (const int rc = enqueue(c, P, sp, due_list, due_count, stream)) return rc;
  if (sp.leaves_hint) c->hint_batch = batch;
  return QMPC_OK;
}

}  // namespace

extern "C" {

int qmpc_solve(qmpc_handle c, int batch, const qmpc_inputs* in, const qmpc_outputs* out, void* stream) {
  if (!in) return QMPC_ERR_ARG;
  return solve_impl(c, batch, in, nullptr, out, nullptr, stream);
}

int qmpc_solve_commands(qmpc_handle c, int batch, const qmpc_command* cmd, const qmpc_outputs* out, float* f_ff,
                        void* stream) {
  if (!cmd) return QMPC_ERR_ARG;
  return solve_impl(c, batch, nullptr, cmd, out, f_ff, stream);
}

int qmpc_pack(qmpc_handle c, int batch, const qmpc_command* cmd, const qmpc_record* rec, void* stream_) {
  if (!c || !cmd || !rec) return QMPC_ERR_ARG;
  if (!c->is_setup) return QMPC_ERR_STATE;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  if (!command_ok(cmd)) return QMPC_ERR_ARG;
  if (!rec->p || !rec->v || !rec->q || !rec->w || !rec->r || !rec->yaw || !rec->traj || !rec->gait || !rec->x_drag)
    return QMPC_ERR_ARG;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_pack(cmd, rec, batch, c->horizon, (float)c->dt, q.stream));
  return QMPC_OK;
}

int qmpc_forces_to_body(qmpc_handle c, int batch, const float* r_body, const float* grf, float* f_ff, void* stream_) {
  if (!c || !r_body || !grf || !f_ff) return QMPC_ERR_ARG;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_f2b(r_body, grf, f_ff, batch, q.stream));
  return QMPC_OK;
}

}  // extern "C"

namespace {

// host-pointer solve in two halves, so that one host thread can keep several devices busy:
// enqueue (gather into the pinned block, copies / launch on the handle's own stream) and finish
// (wait for the event, scatter the results into the caller's arrays)
struct HostJob {
  size_t B = 0, h = 0;
  size_t o_grf = 0, o_soln = 0, o_st = 0, o_it = 0;
  qmpc_outputs out{};
  bool active = false;
};

int host_enqueue(qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_outputs* out, HostJob& job) {
  if (!c || !in || !out) return QMPC_ERR_ARG;
  if (!c->is_setup) return QMPC_ERR_STATE;
  if (batch <= 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (!record_ok(*in) || !out->grf || !out->status) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  const size_t B = (size_t)batch, h = (size_t)c->horizon;
  // ONE pinned host block holds the whole record and the results:  [ inputs | outputs ].
  //   * small batches (the single-robot shim): the kernel reads and writes the pinned block in
  //     place over PCIe (hipHostMalloc memory is device-visible and coherent) -- no copy
  //     commands at all, one launch and one event wait;
  //   * large batches: ONE H2D copy of the input part into a device mirror, ONE D2H copy of the
  //     output part back (PCIe bandwidth, not latency, matters there).
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 63) & ~(size_t)63;
    return o;
  };
  struct Part {
    size_t off, bytes;
  } rec[kRecordArrays];
  int n = 0;
  for_each_record_array(*in, h, [&](const void*, size_t bytes, bool per_robot) {
    const size_t all = per_robot ? bytes * B : bytes;
    rec[n++] = Part{carve(all), all};
  });
  const size_t in_bytes = (off + 255) & ~(size_t)255;
  off = in_bytes;
  const size_t o_grf = carve(4 * 12 * B), o_soln = carve(out->soln ? 8 * 12 * h * B : 0), o_st = carve(4 * B),
               o_it = carve(out->iters ? 4 * B : 0);
  const size_t total = off, out_bytes = total - in_bytes;
  if (total > c->pin_bytes) {
    if (c->h_pin) hipHostFree(c->h_pin);
    c->h_pin = nullptr;
    c->pin_bytes = 0;
    HIP_TRY(c, hipHostMalloc(&c->h_pin, total, hipHostMallocDefault));
    c->pin_bytes = total;
  }
  if (!c->host_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->host_stream, hipStreamNonBlocking));
  if (!c->host_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->host_ev, hipEventDisableTiming));
  const bool in_place = batch <= 64;
  if (!in_place && total > c->d_stage.n) {
    c->d_stage = DevBuf<char>();  // (the smaller block goes first)
    HIP_TRY(c, c->d_stage.alloc(total));
  }
  char* hb = (char*)c->h_pin;
  hipStream_t s = c->host_stream;
  char* base = in_place ? hb : c->d_stage.p;
  // gather the record into the pinned block; the solve reads it at `base`
  qmpc_inputs din = *in;
  n = 0;
  for_each_record_array(din, h, [&](auto& p, size_t, bool) {
    std::memcpy(hb + rec[n].off, p, rec[n].bytes);
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + rec[n++].off);
  });
  if (!in_place) {
    if (const int rc = order_after_previous(c, s)) return rc;  // the mirror may still be read by an earlier call
    HIP_TRY(c, hipMemcpyAsync(base, hb, in_bytes, hipMemcpyHostToDevice, s));
  }
  qmpc_outputs dout;
  dout.grf = (float*)(base + o_grf);
  dout.soln = out->soln ? (double*)(base + o_soln) : nullptr;
  dout.status = (int32_t*)(base + o_st);
  dout.iters = out->iters ? (int32_t*)(base + o_it) : nullptr;
  const int rc = qmpc_solve(c, batch, &din, &dout, s);
  if (rc != QMPC_OK) return rc;
  if (!in_place) HIP_TRY(c, hipMemcpyAsync(hb + in_bytes, base + in_bytes, out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipEventRecord(c->host_ev, s));
  job.B = B; job.h = h;
  job.o_grf = o_grf; job.o_soln = o_soln; job.o_st = o_st; job.o_it = o_it;
  job.out = *out;
  job.active = true;
  return QMPC_OK;
}

int host_finish(qmpc_ctx* c, HostJob& job) {
  if (!job.active) return QMPC_OK;
  job.active = false;
  DeviceGuard g(c->device);
  // latency path: poll the event for a short while before handing the thread to the OS
  hipError_t q = hipErrorNotReady;
  for (int spin = 0; spin < 20000 && q == hipErrorNotReady; ++spin) q = hipEventQuery(c->host_ev);
  if (q == hipErrorNotReady) q = hipEventSynchronize(c->host_ev);
  if (q != hipSuccess) return fail(c, q, "qmpc_solve_host wait");
  const char* hb = (const char*)c->h_pin;
  const size_t B = job.B, h = job.h;
  std::memcpy(job.out.grf, hb + job.o_grf, 4 * 12 * B);
  if (job.out.soln) std::memcpy(job.out.soln, hb + job.o_soln, 8 * 12 * h * B);
  std::memcpy(job.out.status, hb + job.o_st, 4 * B);
  if (job.out.iters) std::memcpy(job.out.iters, hb + job.o_it, 4 * B);
  return QMPC_OK;
}

}  // namespace

extern "C" {

int qmpc_set_leg_geometry(qmpc_handle c, double abad, double hip, double knee, double knee_y) {
  if (!c || !(abad >= 0) || !(hip > 0) || !(knee > 0)) return QMPC_ERR_ARG;
  c->leg_geom[0] = (float)abad;
  c->leg_geom[1] = (float)hip;
  c->leg_geom[2] = (float)knee;
  c->leg_geom[3] = (float)knee_y;
  return QMPC_OK;
}

int qmpc_leg_kinematics(qmpc_handle c, int batch, const float* q, const float* qd, float* J, float* p, float* v,
                        void* stream) {
  if (!c || !q || !J || !p || (v && !qd)) return QMPC_ERR_ARG;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  DeviceGuard g(c->device);
  HIP_TRY(c, qmpc_launch_leg_kin(c->leg_geom, q, qd, J, p, v, batch, (hipStream_t)stream));
  return QMPC_OK;
}

int qmpc_leg_torques(qmpc_handle c, int batch, const qmpc_leg_command* cmd, float* tau, float* q_des, void* stream) {
  if (!c || !cmd || !tau) return QMPC_ERR_ARG;
  if (!cmd->kp_cart || !cmd->kd_cart || !cmd->p_des || !cmd->v_des || !cmd->q || !cmd->qd || !cmd->J || !cmd->p ||
      !cmd->v)
    return QMPC_ERR_ARG;
  if (batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  DeviceGuard g(c->device);
  HIP_TRY(c, qmpc_launch_leg_cmd(c->leg_geom, cmd, tau, q_des, batch, (hipStream_t)stream));
  return QMPC_OK;
}

int qmpc_swing_trajectory(qmpc_handle c, int n_feet, const float* p0, const float* pf, const float* height,
                          const float* phase, const float* swing_time, float* p, float* v, float* a, void* stream) {
  if (!c || !p0 || !pf || !height || !phase || !swing_time || !p || !v || !a) return QMPC_ERR_ARG;
  if (n_feet < 0 || n_feet > 4 * c->max_batch) return QMPC_ERR_ARG;
  if (n_feet == 0) return QMPC_OK;
  DeviceGuard g(c->device);
  HIP_TRY(c, qmpc_launch_swing(p0, pf, height, phase, swing_time, p, v, a, n_feet, (hipStream_t)stream));
  return QMPC_OK;
}

int qmpc_kf_init(qmpc_handle c, int batch, float* xhat, float* P, void* stream) {
  if (!c || !xhat || !P || batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  DeviceGuard g(c->device);
  HIP_TRY(c, qmpc_launch_kf_init(xhat, P, batch, (hipStream_t)stream));
  return QMPC_OK;
}

int qmpc_kf_step(qmpc_handle c, int batch, const qmpc_kf_state* st, void* stream) {
  if (!c || !st || batch < 0 || batch > c->max_batch) return QMPC_ERR_ARG;
  if (!st->xhat || !st->P || !st->r_body || !st->a_world || !st->omega_body || !st->contact_phase || !st->leg_p ||
      !st->leg_v || !st->position || !st->v_world)
    return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  DeviceGuard g(c->device);
  HIP_TRY(c, qmpc_launch_kf(st, kAbadLocation, batch, (hipStream_t)stream));
  return QMPC_OK;
}

int qmpc_solve_host(qmpc_handle c, int batch, const qmpc_inputs* in, const qmpc_outputs* out) {
  HostJob job;
  const int rc = host_enqueue(c, batch, in, out, job);
  if (rc != QMPC_OK) return rc;
  return host_finish(c, job);
}

int qmpc_solve_sharded(const qmpc_handle* handles, int n_handles, int batch, const qmpc_inputs* in,
                       const qmpc_outputs* out) {
  if (!handles || n_handles <= 0 || n_handles > 64 || !in || !out || batch < 0) return QMPC_ERR_ARG;
  for (int k = 0; k < n_handles; ++k)
    if (!handles[k]) return QMPC_ERR_ARG;
  if (batch == 0) return QMPC_OK;
  if (!record_ok(*in) || !out->grf || !out->status) return QMPC_ERR_ARG;
  const int h = handles[0]->horizon;
  for (int k = 1; k < n_handles; ++k)
    if (handles[k]->horizon != h) return QMPC_ERR_STATE;  // every device must be set up for the same problem
  const int per = (batch + n_handles - 1) / n_handles;  // contiguous shards
  HostJob jobs[64];
  int rc_all = QMPC_OK;
  // enqueue on every device first (each call returns as soon as its copies / launches are queued) ...
  for (int k = 0; k < n_handles; ++k) {
    const int lo = k * per, hi = (lo + per < batch) ? lo + per : batch;
    if (lo >= hi) break;
    const size_t o = (size_t)lo;
    qmpc_inputs si = *in;
    for_each_record_array(si, (size_t)h, [&](auto& p, size_t bytes, bool per_robot) {
      p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<const char*>(p) +
                                                                  (per_robot ? bytes * o : 0));
    });
    qmpc_outputs so;
    so.grf = out->grf + 12 * o;
    so.soln = out->soln ? out->soln + (size_t)12 * h * o : nullptr;
    so.status = out->status + o;
    so.iters = out->iters ? out->iters + o : nullptr;
    const int rc = host_enqueue(handles[k], hi - lo, &si, &so, jobs[k]);
    if (rc != QMPC_OK && rc_all == QMPC_OK) rc_all = rc;
  }
  // ... then collect: the devices run concurrently, one host thread drives them all
  for (int k = 0; k < n_handles; ++k) {
    const int rc = host_finish(handles[k], jobs[k]);
    if (rc != QMPC_OK && rc_all == QMPC_OK) rc_all = rc;
  }
  return rc_all;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Batched locomotion controller (include/qmpc_ctrl.h).  The kernels are in qmpc_glue.hip.
namespace {

// One array of an X-macro list (QMPC_CTRL_ARRAYS, QMPC_PLANT_ARRAYS) laid out in an allocation: 256-byte aligned,
// per_robot elements for each of M robots (base == nullptr: only count)
template <class T>
void carve_array(T*& member, char* base, size_t& off, int per_robot, int M) {
  off = (off + 255) & ~(size_t)255;
  member = base ? reinterpret_cast<T*>(base + off) : nullptr;
  off += sizeof(T) * (size_t)per_robot * (size_t)M;
}
#define QMPC_CARVE(T, name, per_robot) carve_array(d.name, base, off, per_robot, M);
size_t carve(QmpcCtrlDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_CTRL_ARRAYS(QMPC_CARVE)
  return off;
}
size_t carve(QmpcPlantDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_PLANT_ARRAYS(QMPC_CARVE)
  return off;
}
size_t carve(QmpcEpisodeDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_EPISODE_ARRAYS(QMPC_CARVE)
  carve_array(d.log_words, base, off, 2, 1);
  return off;
}
size_t carve(QmpcEpisodeSenseDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_EPISODE_SENSE_ARRAYS(QMPC_CARVE)
  return off;
}
size_t carve(QmpcActDev& d, char* base, int M) {
  size_t off = 0;
  QMPC_ACT_ARRAYS(QMPC_CARVE)
  return off;
}
#undef QMPC_CARVE

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

bool ctrl_ready(const qmpc_ctx* c) { return c->ctrl && c->ctrl->batch; }
bool plant_ready(const qmpc_ctx* c) { return c->plant && c->plant->batch; }

int ctrl_check(qmpc_ctx* c, int batch) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->ctrl->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

// Where a reset robot's counter restarts (qmpc_ctrl_reset, and both episode managers'): in lockstep at T mod 13 (the
// batch keeps solving on the same ticks), with the per-robot schedule at 0, as init_controller leaves it.  A reset
// starts the controller (qmpc_ctrl_set_schedule's window closes).
int ctrl_reset_counter0(qmpc_ctx::Ctrl* k) {
  k->started = true;
  return k->schedule == QMPC_CTRL_PER_ROBOT ? 0 : (int)(k->ticks % 13);
}

// The controller's reset of the masked robots (qmpc_ctrl_reset, and the episode manager's).  The caller holds the
// DeviceGuard and has ordered the stream.
int ctrl_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, hipStream_t stream) {
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  const int counter0 = ctrl_reset_counter0(k);
  HIP_TRY(c, qmpc_launch_ctrl_init(&k->d, mask_dev, counter0, batch, stream));
  return QMPC_OK;
}

// The solve of an MPC tick, behind the locomotion stage that wrote the command rows (and, with the per-robot schedule, the
// list of due robots): the per-tick path's and the fleet run's.  The caller holds the DeviceGuard and has ordered the stream.
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
// leg commands.  The caller holds the DeviceGuard and has ordered the stream.
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
  if (!c->ctrl) c->ctrl.reset(new qmpc_ctx::Ctrl());
  qmpc_ctx::Ctrl* k = c->ctrl.get();
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
// Reduced-order plant (include/qmpc_plant.h).  The kernels are in qmpc_plant.hip.
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

int plant_check(qmpc_ctx* c, int batch) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c) || !plant_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->plant->batch || batch != c->ctrl->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
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

// The argument block of a step, from the handle as it stands now and the call's three pointers.  Every step kernel is
// given the same block and reads what it knows of.
QmpcPlantStepArgs plant_step_args(qmpc_ctx* c, int batch, const double* effort, double* state_out, double* motor_out) {
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

// The plant's reset of the masked robots on whatever ground is bound (qmpc_plant_reset, and the episode manager's).  The
// caller holds the DeviceGuard and has ordered the stream.
int plant_reset_enqueue(qmpc_ctx* c, int batch, const uint8_t* mask_dev, const double* init_xyyaw, hipStream_t stream) {
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

}  // namespace

extern "C" {

int qmpc_plant_init(qmpc_handle c, int batch, double mu_plant, int substeps, const double* init_xyyaw, void* stream_) {
  if (!c) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  if (batch != c->ctrl->batch || substeps < 1 || !(mu_plant >= 0)) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (!c->plant) c->plant.reset(new qmpc_ctx::Plant());
  qmpc_ctx::Plant* k = c->plant.get();
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

// ---------------------------------------------------------------------------------------------------
// Fleet run (include/qmpc_fleet.h): qmpc_ctrl_tick_state -> qmpc_plant_step, `ticks` times, with everything between two
// solves in one launch.  The plan is qmpc_span.h's, the kernel qmpc_span.hip's.
extern "C" {

int qmpc_fleet_run(qmpc_handle c, int batch, int ticks, double* effort, double* state, double* motor, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (ticks < 1 || !effort || !state || !motor) return QMPC_ERR_ARG;
  qmpc_ctx::Ctrl* k = c->ctrl.get();
  qmpc_ctx::Plant* pl = c->plant.get();
  const int reason = (pl->terrain.rows ? QMPC_FLEET_TERRAIN : 0) | (pl->contact.flags ? QMPC_FLEET_CONTACT : 0) |
                     (pl->field.z ? QMPC_FLEET_FIELD : 0);
  // (the counts follow what has been enqueued: a call refused here, or one that stops half way, counts no tick it did not
  //  enqueue)
  if (reason) {
    // what the span kernel does not cover: the per-tick calls themselves, so the launches are theirs exactly
    for (int i = 0; i < ticks; ++i) {
      if (const int rc = qmpc_ctrl_tick_state(c, batch, state, motor, effort, stream_)) return rc;
      k->fleet.reason = reason;  // (the call has enqueued something: it is the last call now)
      if (const int rc = qmpc_plant_step(c, batch, effort, state, motor, stream_)) return rc;
      ++k->fleet.ticks;
      ++k->fleet.fallback_ticks;
    }
    return QMPC_OK;
  }
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  k->started = true;
  k->fleet.reason = 0;
  const bool per_robot = k->schedule == QMPC_CTRL_PER_ROBOT;
  const QmpcPlantStepArgs P = plant_step_args(c, batch, effort, state, motor);
  QmpcSpanArgs A{};
  A.C = k->d;
  A.g = QmpcLegGeom{c->leg_geom[0], c->leg_geom[1], c->leg_geom[2], c->leg_geom[3]};
  A.S = P.S;
  A.K = P.K;
  A.effort = effort;
  A.state = state;
  A.motor = motor;
  A.n = P.n;
  A.V = P.V;
  A.build_list = per_robot ? 1 : 0;
  for (const SpanLaunch& l : plan_spans(k->ticks, ticks, per_robot)) {
    // (a kernel, not a memset node: see fill_ints)
    if (l.reset_due) HIP_TRY(c, fill_ints(k->d.due_count, 1, 0, q.stream));
    HIP_TRY(c, qmpc_launch_span(&A, k->robot_mode, pl->bound, pl->stats_on, l.first_at_c, l.ticks, l.last_after_l, q.stream));
    // T follows the locomotion stages as they are enqueued, in front of the solve that can still fail (ctrl_after_prework)
    k->ticks += l.locos;
    k->fleet.ticks += l.locos;
    k->fleet.fused_ticks += l.locos;
    ++k->fleet.fused_launches;
    if (l.solve)
      if (const int rc = ctrl_solve_enqueue(c, batch, q.stream)) return rc;
  }
  return QMPC_OK;
}

int qmpc_fleet_run_info(qmpc_handle c, qmpc_fleet_info* out) {
  if (!c || !out) return QMPC_ERR_ARG;
  if (!ctrl_ready(c)) return QMPC_ERR_STATE;
  *out = c->ctrl->fleet;
  return QMPC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Sensor model (include/qmpc_sense.h).  The kernels are in qmpc_sense.hip.
namespace {

int sense_check(qmpc_ctx* c, int batch) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!c->sense || !c->sense->batch) return QMPC_ERR_STATE;
  if (batch != c->sense->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

void sense_unbind(QmpcSenseArgs& a) {
  a.acc_bias = a.gyro_bias = a.acc_sigma = a.gyro_sigma = a.q_sigma = a.qd_sigma = nullptr;
}

}  // namespace

extern "C" {

int qmpc_sense_init(qmpc_handle c, int batch, uint64_t seed, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (!c->sense) c->sense.reset(new qmpc_ctx::Sense());
  qmpc_ctx::Sense* k = c->sense.get();
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
  if (!plant_ready(c) || !c->sense || !c->sense->batch) return QMPC_ERR_STATE;
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

int act_check(qmpc_ctx* c, int batch) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!c->act || !c->act->batch) return QMPC_ERR_STATE;
  if (batch != c->act->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

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
  if (!c->act) c->act.reset(new qmpc_ctx::Act());
  qmpc_ctx::Act* k = c->act.get();
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
  if (!ctrl_ready(c) || !plant_ready(c) || !c->act || !c->act->batch) return QMPC_ERR_STATE;
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
namespace {

int episode_check(qmpc_ctx* c, int batch) {
  if (const int rc = plant_check(c, batch)) return rc;
  if (!c->episode || !c->episode->batch) return QMPC_ERR_STATE;
  if (batch != c->episode->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

// what a decision kernel reads of the handle's other state
QmpcEpisodeIn episode_inputs(const qmpc_ctx* c) {
  const qmpc_ctx::Plant* pl = c->plant.get();
  // the plant writes ground[b] on terrain, on a field and with contact on (there 0 without rows); the flat plant never does
  const bool ground = pl->terrain.rows || pl->field.z || pl->contact.flags;
  return QmpcEpisodeIn{pl->d.p, pl->d.q, c->ctrl->d.safe, ground ? pl->terrain.ground : nullptr,
                       (uint32_t)(c->episode->seed & 0xFFFFFFFFu), (uint32_t)(c->episode->seed >> 32)};
}

const int kEpisodeCauses = QMPC_EP_UNSAFE | QMPC_EP_NONFINITE | QMPC_EP_TILT | QMPC_EP_HEIGHT | QMPC_EP_RANGE | QMPC_EP_TIMEOUT;

}  // namespace

extern "C" {

int qmpc_episode_init(qmpc_handle c, int batch, uint64_t seed, void* stream_) {
  if (const int rc = plant_check(c, batch)) return rc;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (!c->episode) c->episode.reset(new qmpc_ctx::Episode());
  qmpc_ctx::Episode* k = c->episode.get();
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
  if (!ctrl_ready(c) || !plant_ready(c) || !c->episode || !c->episode->batch) return QMPC_ERR_STATE;
  const Enqueue q(c, stream_);
  if (q.rc) return q.rc;
  HIP_TRY(c, qmpc_launch_episode_log_clear(&c->episode->d, q.stream));
  return QMPC_OK;
}

int qmpc_episode_view_get(qmpc_handle c, qmpc_episode_view* v) {
  if (!c || !v) return QMPC_ERR_ARG;
  if (!plant_ready(c) || !c->episode || !c->episode->batch) return QMPC_ERR_STATE;
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
  if (!own) return QMPC_OK;
  if (!c->episode_sense || !c->episode_sense->batch) return QMPC_ERR_STATE;
  if (batch != c->episode_sense->batch) return QMPC_ERR_ARG;
  return QMPC_OK;
}

}  // namespace

extern "C" {

int qmpc_episode_sense_init(qmpc_handle c, int batch, int warm_ticks, void* stream_) {
  if (const int rc = episode_sense_check(c, batch, false)) return rc;
  if (warm_ticks < 0) return QMPC_ERR_ARG;
  DeviceGuard g(c->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (!c->episode_sense) c->episode_sense.reset(new qmpc_ctx::EpisodeSense());
  qmpc_ctx::EpisodeSense* k = c->episode_sense.get();
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
  if (!plant_ready(c) || !c->episode_sense || !c->episode_sense->batch) return QMPC_ERR_STATE;
  v->warm = c->episode_sense->d.warm;
  v->hold = c->episode_sense->d.hold;
  v->warm_ticks = c->episode_sense->warm_ticks;
  v->batch = c->episode_sense->batch;
  return QMPC_OK;
}

}  // extern "C"
