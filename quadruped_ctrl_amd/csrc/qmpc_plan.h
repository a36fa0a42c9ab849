// qmpc_plan.h -- the launch plan of one solve as a VALUE: which kernels a call enqueues, in which order, over which
// grid, on which lists and counters.  Host-only integer logic over the handle's settings (PlanSettings), the call's shape
// (PlanCall) and the kernels' occupancy numbers (PlanResident): no HIP, no handle, no device pointer -- lists and counters
// are named symbolically and qmpc_capi.cpp (enqueue) resolves them.  tests/plan_dump.cpp compiles this header alone.
#ifndef QMPC_PLAN_H
#define QMPC_PLAN_H

#include <vector>

#include "qmpc_device.h"

// the handle fields the decisions read (qmpc_capi.cpp: plan_settings fills it, for the solve and for ensure_pools)
struct PlanSettings {
  int horizon = 0, max_batch = 0;
  int max_stance = 0, min_stance = 0;  // qmpc_set_max_stance / qmpc_set_min_stance (0 = unknown)
  int split = 1, dense = 1, chunks = 0, order_hint = 1, size_order = 1;  // the setters of the same names
  int hint_batch = 0;                  // batch size of the call that left the order hint's counts (0: none)
  int admm_mode = 0;                   // qmpc_settings_jcqp
  int wk_cap[3] = {0, 0, 0};           // work items per pool (0: not allocated)
  bool has_ws = false, has_evflags = false;  // a warm-start buffer is set / the 192-row class's event pool exists
};
// one call
struct PlanCall {
  int batch = 0;
  bool capturing = false, command_mode = false, has_due_list = false;
  unsigned gait_align = 0;   // the record's gait pointer & 7 (record mode)
  int record_mode_admm = 0;  // the JCQP alternate this call runs: the handle's admm_mode in record mode, 0 in command mode
};
// qmpc_resident_blocks / qmpc_resident_sweep / qmpc_engine_resident, indexed by kernel class
struct PlanResident {
  int blocks[7] = {0, 0, 0, 0, 0, 0, 0};  // [1] [2] [3] [4] [6]
  int sweep[4] = {0, 0, 0, 0};            // [2] [3]
  int engine[6] = {0, 0, 0, 0, 0, 0};     // [2] [3] [5]
};
// the handle's host-side call counters, in and out
struct PlanCounters {
  unsigned call_no = 0, hint_call = 0, so_call = 0, prio_call = 0;
};

// Which size classes a solve launches, and which of them through work items (the decoupled path): ONE rule, used by
// the solve and by the allocation of the pools.
//   chain 1 -> 4 -> 2 -> 3 (64 / 96 / 128 / 192 padded rows), n_r = 3 * stance foot-steps; classes k0 .. k1 - 1 are
//   launched; long_h: the large-problem stage behind the 192-row class (192 < n_r <= 432, horizons above 16)
struct ClassPlan {
  int k0 = 0, k1 = 0;
  bool long_h = false;
  bool split[4] = {false, false, false, false};
};
constexpr int kChain[4] = {1, 4, 2, 3};
constexpr int kRows[4] = {64, 96, 128, 192};
constexpr int kLongHorizon = 16;  // QMPC_LONG_HORIZON of include/qmpc.h (qmpc_capi.cpp asserts it)

// the pools of work items, sk 0 = 128-row class, 1 = 192-row class, 2 = large problems: kernel class of the producer and
// the engine (5: the large-problem engine), leading dimension of an item, doubles per overflow event of the engine, items
struct ItemPool {
  int cls, ld, ev_doubles, limit;
};
constexpr ItemPool kItems[3] = {{2, 128, 128 + 64, QMPC_ITEMS_C2}, {3, 192, 192 + 128, QMPC_ITEMS_C3},
                                {5, QMPC_BIG_LD, QMPC_BIG_LD + 192, QMPC_ITEMS_BIG}};
constexpr int item_pool_of_class(int cls) { return cls == 2 ? 0 : 1; }  // (the split classes: 2 and 3)

inline ClassPlan plan_classes(const PlanSettings& c, int admm_mode, bool warm) {
  ClassPlan pl;
  const bool full_problem = (admm_mode == 1), exact_cold = !admm_mode && !warm;
  const int h = c.horizon;
  const int nmax = 12 * h;
  int nclass = 4;
  for (int k = 0; k < 4; ++k)
    if (nmax <= kRows[k]) { nclass = k + 1; break; }
  // a caller that knows its gaits can bound the reduced size (qmpc_set_max_stance):
  // larger classes are then not even launched; violators are flagged WS_FULL
  pl.k1 = nclass;
  if (c.max_stance > 0 && !full_problem) {  // (use_jcqp = 1: every foot-step is a variable block, n_r = 12 h for all robots)
    const int nb = 3 * c.max_stance;
    int hc = 4;
    for (int k = 0; k < 4; ++k)
      if (nb <= kRows[k]) { hc = k + 1; break; }
    if (hc < pl.k1) pl.k1 = hc;
  }
  // ... and with a lower bound the classes that are too small for every robot are skipped
  while (pl.k0 + 1 < pl.k1 && 3 * (full_problem ? 4 * h : c.min_stance) > kRows[pl.k0]) ++pl.k0;
  if (h > kLongHorizon) {
    // long horizons (up to K_MAX_GAIT_SEGMENTS = 36): the 192-row class alone has the threads (12 h tracking-error
    // entries, one per thread) and the LDS (h x h coefficient tables) to assemble them -- it takes every robot; one with
    // more than 64 stance foot-steps goes on to the large-problem path
    pl.k0 = 3;
    pl.k1 = 4;
    // (the large-problem stage: skipped when the caller's size hint, qmpc_set_max_stance, rules such robots out -- a
    //  violator is reported like any other; use_jcqp = 1 makes every robot a large problem, 12 h variables)
    pl.long_h = full_problem || !(c.max_stance > 0 && 3 * c.max_stance <= 192);
  }
  // decoupled path (128- and 192-row classes, exact solve, cold start): sweep kernel -> work items -> engine kernel ->
  // (rarely) the monolithic kernel on the robots the engine handed back.  Automatic: a small batch is latency-bound --
  // one workgroup per CU either way -- and the one-kernel path has one launch and no trip through L2 on it: measured
  // break-even ~300 robots in the 128-row class, below 128 in the 192-row class.  Decided by the HANDLE's size, not
  // the call's: a robot's result does not depend on the batch it is solved in -- the two paths agree to ~1e-14
  // relative, not bit for bit
  for (int k = pl.k0; k < pl.k1; ++k) {
    const bool big = c.split == 2 || c.max_batch >= (kChain[k] == 2 ? 384 : 128);
    pl.split[k] = c.split && big && (kChain[k] == 2 || kChain[k] == 3) && exact_cold;
  }
  return pl;
}

// the pools a class plan goes through, bit sk
inline unsigned plan_pools(const ClassPlan& pl) {
  unsigned m = pl.long_h ? 4u : 0u;
  for (int k = pl.k0; k < pl.k1; ++k)
    if (pl.split[k]) m |= 1u << item_pool_of_class(kChain[k]);
  return m;
}
// ... and the UNION over the plans a solve on this handle can make (what ensure_pools allocates): the exact solve, and --
// when the JCQP alternate is selected -- its own plan (use_jcqp = 1 makes every robot of a long horizon a large problem
// whatever the stance hint says)
inline unsigned plan_pools(const PlanSettings& s) {
  return plan_pools(plan_classes(s, 0, false)) | (s.admm_mode ? plan_pools(plan_classes(s, s.admm_mode, false)) : 0u);
}

enum LaunchKind { FILL_COUNTERS, FILL_EVFLAGS, FILL_PRIO, SOLVE, SWEEP, BIG_PRODUCER, ENGINE, ADMM_BIG };
// a list of robots, by name: slot 0..3 of the handle's lists (classes 4, 2, 3, the large problems), the caller's due list,
// the hand-back list of item pool sk
enum ListKind { LIST_NONE, LIST_SLOT, LIST_DUE, LIST_HANDBACK };
struct ListRef {
  ListKind kind = LIST_NONE;
  int idx = 0;
};
constexpr int kNoCounter = -1;   // counters are indices into the call's set ...
constexpr int kDueCounter = -2;  // ... but for the due list's length, which the caller owns

struct Launch {
  LaunchKind kind = SOLVE;
  int cls = 0;   // kernel class: 1, 2, 3, 4, 6; 5: the large-problem producer, engine and ADMM (fills: 0)
  int grid = 0;  // workgroups (fills: 0, enqueue knows the arrays' lengths)
  ListRef list, next;  // consumed / fed
  int count = kNoCounter, qhead = kNoCounter, next_count = kNoCounter;
  bool clear_counts = false;  // the first kernel of an eager call zeroes the NEXT call's counter set
  int status_or = 0;
  // item launches (sweep, producer, engine, ADMM): pool, chunk [rid0, list_hi), counter group of the chunk, and whether the
  // engine zeroes the next chunk's group.  The hand-back launch: sk too (its list), list_hi unbounded
  int sk = -1, rid0 = 0, list_hi = 0, grp = 0;
  bool wk_zero = false;
  // the first class of a call: order hint, size order, per-CU priority staging (0 / kNoCounter: off)
  int hint_hard = 0, hint_max_r = kNoCounter, hint_max_w = kNoCounter, hint_max_z = kNoCounter;  // slots of d_hint_max
  int so_first = 0, so_nseg = 0, so_maxfit = 0;
  unsigned so_tag = 0;   // != 0: the size order is on
  bool so_keys_from_hint = false;
  unsigned prio_tag = 0;  // != 0: the staging is on
};

struct SolvePlan {
  int set = 0;  // counter set: 0 / 1 ping-ponged between eager calls, 2: captured calls and due-list calls
  bool leaves_hint = false;  // the call leaves iteration counts for the next one: hint_batch becomes its batch
  std::vector<Launch> launches;
};

namespace plan_detail {

constexpr int kHintHard = 5;  // single-round launches: iterations in the previous call from which a robot may keep the highest issue priority
constexpr int kSoFirstPct = 0, kSoFirstPctHint = 50;  // the unsorted head beyond the first round, % of a round: keys from the records / from the hint
constexpr int kSoMinDiv = 8;  // at least a round / kSoMinDiv robots to order (measured 2 / 4 / 8 on batches of 1.1 ... 2.5 rounds: no loss anywhere, +4 ... +13 % at 1.4 rounds)
constexpr int kSoTailRounds = 5;  // a launch of many rounds orders its last five only

inline int at_most(int grid, int resident) { return resident > 0 && resident < grid ? resident : grid; }

// one item class of the decoupled path (sk 0 / 1: sweep kernel of the class; sk 2: the large-problem producer): the
// robots [0, batch) -- or the entries of `base.list` -- in consecutive chunks of at most wk_cap[sk], every chunk a
// producer launch and an engine launch, the pool reused from chunk to chunk.  base: list, count and what the sweep feeds
inline void plan_items(SolvePlan& sp, const PlanSettings& s, const PlanCall& call, const PlanResident& res, int sk,
                       const Launch& base, bool& first) {
  const int batch = call.batch, cls = kItems[sk].cls;
  const bool admm = sk == 2 && call.record_mode_admm, listed = base.list.kind != LIST_NONE;
  int nch = (batch + s.wk_cap[sk] - 1) / s.wk_cap[sk];
  if (s.chunks > nch) nch = s.chunks < batch ? s.chunks : batch;
  const int per = (batch + nch - 1) / nch;  // (<= wk_cap[sk])
  for (int ch = 0; ch < nch; ++ch) {
    const int lo = ch * per, hi = (lo + per < batch) ? lo + per : batch;
    if (lo >= hi) break;
    Launch a = base;
    a.kind = sk == 2 ? BIG_PRODUCER : SWEEP;
    a.cls = cls;
    a.sk = sk; a.rid0 = lo; a.list_hi = hi; a.grp = ch & 1;
    a.qhead = listed ? QMPC_CNT_GRP(sk, a.grp) + 2 : kNoCounter;
    a.clear_counts = first && sp.set != 2;
    first = false;
    // (the large-problem producer has the 192-row class's footprint)
    a.grid = (listed || sk == 2) ? at_most(hi - lo, sk == 2 ? res.blocks[3] : res.sweep[cls]) : hi - lo;
    sp.launches.push_back(a);
    Launch b;  // the engine: one robot per workgroup, the chunk's items as a queue
    b.kind = admm ? ADMM_BIG : ENGINE;
    b.cls = cls;
    b.sk = sk; b.rid0 = lo; b.list_hi = hi; b.grp = a.grp;
    b.wk_zero = ch + 1 < nch;
    // JCQP alternate on the large problems: the producer left M^-1 and the gradient; the ADMM kernel consumes the items
    b.grid = admm ? ((hi - lo) < 2048 ? (hi - lo) : 2048) : at_most(hi - lo, res.engine[cls]);
    sp.launches.push_back(b);
  }
  if (admm) return;  // (the ADMM hands nothing back)
  // robots handed back (event capacity exceeded, lost definiteness): the monolithic kernel, list-consuming.  The
  // large problems have no class to fall back to: the 192-row class's stage 0 REPORTS them (QMPC_ST_WS_FULL)
  Launch f;
  f.cls = sk == 0 ? 2 : 3;
  f.sk = sk;
  f.list = {LIST_HANDBACK, sk}; f.count = QMPC_CNT_FB + sk; f.qhead = QMPC_CNT_FBQ + sk;
  f.list_hi = 0x7fffffff;
  f.status_or = sk == 2 ? 0 : QMPC_DEV_ST_FALLBACK;
  if (f.cls == 3 && s.has_evflags) sp.launches.push_back(Launch{FILL_EVFLAGS});
  f.grid = at_most(batch, res.blocks[f.cls]);
  sp.launches.push_back(f);
}

}  // namespace plan_detail

// The plan of one call.  Everything that can refuse the call has been checked (qmpc_capi.cpp: check_solve_call); the
// counters move here and the caller writes them back to the handle before the first launch.
inline SolvePlan plan_solve(const PlanSettings& s, const PlanCall& call, const PlanResident& res, PlanCounters& ctr) {
  using namespace plan_detail;
  SolvePlan sp;
  sp.launches.reserve(16);
  const int batch = call.batch, admm = call.record_mode_admm;
  const bool due = call.has_due_list;
  const ClassPlan pl = plan_classes(s, admm, s.has_ws);
  if (call.capturing || due) {
    // (a due-list call too: its first launch is a list consumer, and those do not clear the next call's set)
    // a call captured into a hipGraph is replayed with the SAME kernel arguments every time: it cannot take part in
    // the ping-pong (its set would be dirty from the previous replay).  Captured calls use a set of their own, cleared
    // by a small kernel node in front of the call's kernels; the eager calls' two sets are not touched
    sp.set = 2;
    sp.launches.push_back(Launch{FILL_COUNTERS});
  } else {
    sp.set = (int)(ctr.call_no++ & 1u);
  }
  // order hint, size order and priority staging apply to the first class of an eager exact call, launched over the
  // whole batch
  const bool orderable = !due && !call.capturing && !admm;
  bool first = true;  // the next kernel is the first of the call: it carries clear_counts

  // size classes by padded rows: 64 (kernel class 1), 96 (class 4), 128 (class 2), 192 (class 3);
  // n_r = 3 * stance foot-steps.  The first class is launched over the whole batch; a robot that
  // does not fit appends itself to the list of the next one.
  for (int k = pl.k0; k < pl.k1; ++k) {
    const bool head = k == pl.k0, listed = !head || due;
    Launch L;
    if (head && due) {  // the first class takes the caller's list instead of the whole batch
      L.list = {LIST_DUE, 0}; L.count = kDueCounter; L.qhead = QMPC_CNT_DUEQ;
    } else if (listed) {
      L.list = {LIST_SLOT, k - 1}; L.count = k - 1; L.qhead = 4 + (k - 1);
    }
    if (pl.long_h && kChain[k] == 3) {  // robots beyond 192 rows go on to the large-problem producer
      L.next = {LIST_SLOT, 3}; L.next_count = QMPC_CNT_BIGLIST;
    } else if (k + 1 < pl.k1) {
      L.next = {LIST_SLOT, k}; L.next_count = k;
    }
    if (pl.split[k]) {
      plan_items(sp, s, call, res, item_pool_of_class(kChain[k]), L, first);
      continue;
    }
    // the first class of the chain: one workgroup per robot; the later ones: one per resident slot, the list
    // is consumed as a queue (no workgroup is dispatched only to find its list entry missing)
    if (kChain[k] == 3 && s.has_evflags) sp.launches.push_back(Launch{FILL_EVFLAGS});
    L.clear_counts = first && sp.set != 2;
    first = false;
    // The 64-row class on a handle made for large batches: its five-workgroups-per-CU instantiation (same arithmetic,
    // bit-identical results: tests).  Alone in the chain (the stance hint says every robot fits it; qmpc_set_dense(2): on any
    // handle): a launch of several rounds is bound by instruction issue, and the fifth wave per SIMD fills what four leave
    // (trot: +3.5 % at 2048 robots, +8 % at 4096, +14 % from 8192 on: 3.76e7 -> 4.30e7 QP/s at 16384; mixed gaits +3 / +7 /
    // +11 %: tools/dense_threshold.py); one round of workgroups (batch 1024) is bound by its slowest robot and loses 1 - 11 %
    // to the 96-VGPR code.  With larger classes behind it (configs[4]: random contact tables): their robots iterate longer,
    // and 16 events in LDS instead of 28 send about one in eight of them to the overflow pool; the launch still gains
    // (configs[4] 492 -> 482 us per 8192 robots, +2 %) as long as every one of them finds a slice there -- which, the slices
    // being RECYCLED within a call (a flag per slice, released when its robot finishes: the need is bounded by the robots in
    // flight), holds for any batch size.  Never ahead of the large-problem stage.  By the HANDLE's size, never the call's
    int kcls = kChain[k];
    if (kcls == 1 && !pl.long_h && ((s.dense == 1 && s.max_batch >= 2048) || (s.dense == 2 && pl.k1 - pl.k0 == 1))) kcls = 6;
    const int round = res.blocks[kcls];  // resident workgroups: one round of the launch
    // (a due list in front of a 64-row class: qmpc_solve_due_kernel, one workgroup per list place -- the grid is the batch, and
    //  the workgroups beyond the device-side count leave at once; in front of any other class: that class's list consumer)
    L.grid = (listed && !(head && due && (kcls == 1 || kcls == 6))) ? at_most(batch, res.blocks[kChain[k]]) : batch;
    L.cls = kcls;
    // order hint: the first class of the chain, launched over more robots than it has resident workgroups (several rounds:
    // the launch ends with whichever hard robot started last), takes the robots in the order of their iteration counts in the
    // previous call -- the same robots one MPC cycle earlier -- longest first.  Results do not depend on the order.
    // A launch of ONE round (the order cannot matter) uses the counts differently: the robots the previous call found hard
    // keep the highest issue priority through their sweep (qmpc_device.h: hint_hard) -- batch 1024, trot: 2.42e7 -> 2.75e7 QP/s.
    // (Only there: in a launch of many rounds it costs 3 %, measured at 16384 robots.)
    bool use_hint_keys = false;
    if (head && orderable && s.order_hint) {
      if (batch > round) {
        // the permutation is built inside the launch (below), keys = the previous call's counts
        use_hint_keys = s.hint_batch == batch;
      } else if (2 * batch > round) {  // (workgroups share CUs: below that priority has nobody to act on)
        // the largest count of the previous one-round call / of this one / cleared for the next: three slots in rotation
        const unsigned hc = ctr.hint_call++;
        L.hint_max_r = (int)((hc + 2) % 3);
        L.hint_max_w = (int)(hc % 3);
        L.hint_max_z = (int)((hc + 1) % 3);
        if (s.hint_batch == batch) L.hint_hard = kHintHard;
      }
    }
    // the proxies of the size order and of the priority staging read the record: record mode, contact tables aligned
    const bool by_record = s.size_order && !call.command_mode;
    // size order: no usable hint, several rounds, contact tables in memory (record mode) and 8-byte aligned.  The first round keeps
    // robot = workgroup index (its workgroups start before anything can be known); the builders (the first workgroups, one
    // segment of the rest each) need a few microseconds, for which the workgroups that follow robots only handed on may have to wait
    // (measured: no loss on configs[4], where a third of the first round is handed on)
    if (head && orderable && (use_hint_keys || (by_record && (call.gait_align & 7u) == 0)) && round > 0 && batch > round) {
      // (the unsorted head beyond the first round: none by size -- measured 0 / 15 / 30 / 50 % of a round: 0 is best or equal
      //  everywhere, +2.6 % on configs[2] --, half a round by the hint's counts: 0 / 25 / 50 %: 3.92e7 / 3.96e7 / 4.05e7 on
      //  configs[2] with exact counts, equal elsewhere -- robots of one COUNT side by side run their engine phases together)
      const int hd = (int)((long long)round * (use_hint_keys ? kSoFirstPctHint : kSoFirstPct) / 100);
      const int half = (batch - round) / 2 < hd ? (batch - round) / 2 : hd;
      int so_first = (round + half + 7) & ~7;
      // (a launch of many rounds: only its last five are ordered -- a robot lasts three or four rounds at most, so nothing that
      //  starts earlier can end the launch, and every reader pays a memory round trip for its entry: trot, 16384 robots, -3.9 %
      //  with everything ordered)
      if (batch - kSoTailRounds * round > so_first) so_first = (batch - kSoTailRounds * round + 7) & ~7;
      const int n = batch - so_first;
      // strided segments of at most 4096 robots (QMPC_SO_SEG of qmpc_kernels.hip: the builder's LDS scratch)
      // (a multiple of 8, and so_first too: place b of segment j has b % 8 == j % 8 -- readers and builder on one XCD)
      // (QMPC_SO_HEAD = 16 places of the first round per segment on top: 17 nseg workgroups in front of so_first)
      const int nseg = 8 * ((n + 8 * 4080 - 1) / (8 * 4080));
      // (next to nothing to order: the builders and the sixteen first-round places per segment cost more than the order gives)
      if (kSoMinDiv * n >= round && 17 * nseg <= round) {
        L.so_first = so_first;
        L.so_nseg = nseg;
        if (++ctr.so_call == 0) ++ctr.so_call;  // (0 is what fresh memory holds)
        L.so_tag = ctr.so_call;
        L.so_maxfit = kRows[k] / 3;
        L.so_keys_from_hint = use_hint_keys;
      }
    }
    // ONE round, full CUs, no usable hint: the sweep's issue priority is staged per CU by the robots' scores (one atomic maximum on
    // the CU's word: qmpc_kernels.hip, stage 0)
    // (only where the CUs are full: at three workgroups per CU -- 768 robots on 1024 slots -- the staging costs 3 %)
    if (head && orderable && by_record && (call.gait_align & 3u) == 0 && L.hint_hard <= 0 && round > 0 && batch <= round &&
        8 * batch > 7 * round) {
      if (++ctr.prio_call == 0) {  // (the call number wrapped: the words start again)
        sp.launches.push_back(Launch{FILL_PRIO});
        ++ctr.prio_call;
      }
      L.prio_tag = ctr.prio_call;
    }
    sp.launches.push_back(L);
  }
  sp.leaves_hint = s.order_hint && orderable;  // (a due list leaves counts for its robots only)
  if (pl.long_h) {
    // ---- the large problems (192 < n_r <= 432: all feet down beyond 16 segments, a trot beyond 32): H in global memory,
    // block sweep, the seven-block engine; what that engine cannot hold is REPORTED.  Normally the list is empty: launches
    // that find nothing to do
    Launch L;
    L.list = {LIST_SLOT, 3}; L.count = QMPC_CNT_BIGLIST;
    plan_items(sp, s, call, res, 2, L, first);
  }
  return sp;
}

#endif
