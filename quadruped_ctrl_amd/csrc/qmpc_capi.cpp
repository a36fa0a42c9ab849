// qmpc_capi.cpp -- host side of the C ABI declared in include/qmpc.h (the handle and the solve; the headers that stand on
// them are served by qmpc_capi_ctrl.cpp, qmpc_capi_plant.cpp and qmpc_capi_stages.cpp, see qmpc_host.h).
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
#include <type_traits>
#include <vector>

#include "../../include/qmpc.h"
#include "../../include/qmpc_debug.h"   // test / profiling hooks (same library)
#include "../../include/qmpc_expert.h"  // tuning knobs whose default is the measured optimum, warm start
#include "qmpc_host.h"    // the handle; the controller, the plant and the stages around them have their own units
#include "qmpc_launch.h"  // the launchers that have no per-unit header of their own
using namespace qmpc_host;
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
hipError_t qmpc_host::fill_ints(int* p, int n, int v, hipStream_t stream) {
  hipLaunchKernelGGL(qmpc_fill_ints_kernel, dim3((n + 255) / 256 < 64 ? (n + 255) / 256 : 64), dim3(256), 0, stream, p, n, v);
  return hipGetLastError();
}

namespace {

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

}  // namespace

// one solve: inputs either as the record (`in`) or as the controller command (`cmd`, record built in stage 0).
// due_list / due_count (internal, device-resident, command mode only; nullptr: every robot of the batch): the dense list
// of the robots this call solves and its length, both written on the device by work enqueued before the call (the
// batched controller's per-robot schedule).  A robot that is not listed is not scheduled at all: the first class of
// the chain maps its workgroups to robots through the list and those beyond the device-side count leave at once, as
// the later classes do with theirs, so the robot runs no QP, reaches no later list, no engine and no overflow slice, and
// none of its outputs or command rows is written.
// Check, bind, plan (qmpc_plan.h: a value, no device involved), enqueue.
int qmpc_host::solve_impl(qmpc_ctx* c, int batch, const qmpc_inputs* in, const qmpc_command* cmd, const qmpc_outputs* out,
                          float* f_ff, void* stream_, const int* due_list, int* due_count) {
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
