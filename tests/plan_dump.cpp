// plan_dump.cpp -- prints the launch plans of fixed scenarios as JSON (tests/test_plan_cpu.py compares them with values
// derived by hand).  Includes qmpc_plan.h alone: the plan needs no HIP and no device.
#include <cstdio>

#include "../quadruped_ctrl_amd/csrc/qmpc_plan.h"

namespace {

const char* kKind[] = {"FILL_COUNTERS", "FILL_EVFLAGS", "FILL_PRIO", "SOLVE", "SWEEP", "BIG_PRODUCER", "ENGINE", "ADMM_BIG"};

void print_list(const char* key, const ListRef& r) {
  static const char* names[] = {"none", "slot", "due", "fb"};
  if (r.kind == LIST_SLOT || r.kind == LIST_HANDBACK) std::printf("\"%s\": \"%s%d\", ", key, names[r.kind], r.idx);
  else std::printf("\"%s\": \"%s\", ", key, names[r.kind]);
}

// a handle as qmpc_create / qmpc_setup / ensure_pools leave it: the event pool of the 192-row class from 12 h > 128 on,
// the item pools the settings can reach at min(max_batch, limit) items
struct Handle {
  const char* block;
  PlanSettings s;
  PlanCounters ctr;
  Handle(const char* name, int max_batch, int h, int max_stance, int min_stance, int admm = 0, int chunks = 0) : block(name) {
    s.max_batch = max_batch; s.horizon = h; s.max_stance = max_stance; s.min_stance = min_stance;
    s.admm_mode = admm; s.chunks = chunks;
    s.has_evflags = 12 * h > 128;
    for (int sk = 0; sk < 3; ++sk)
      if (plan_pools(s) >> sk & 1u) s.wk_cap[sk] = max_batch < kItems[sk].limit ? max_batch : kItems[sk].limit;
  }
};

bool first_scenario = true;

void solve(Handle& hd, const char* name, int batch, bool command = false, bool due = false, bool capturing = false) {
  PlanResident res;
  res.blocks[1] = 1024; res.blocks[6] = 1280; res.blocks[4] = 512; res.blocks[2] = res.blocks[3] = 256;
  res.sweep[2] = res.sweep[3] = 256;
  res.engine[2] = 512; res.engine[3] = res.engine[5] = 256;
  PlanCall call;
  call.batch = batch; call.command_mode = command; call.has_due_list = due; call.capturing = capturing;
  call.record_mode_admm = command ? 0 : hd.s.admm_mode;
  const SolvePlan sp = plan_solve(hd.s, call, res, hd.ctr);
  if (sp.leaves_hint) hd.s.hint_batch = batch;
  std::printf("%s\n{\"name\": \"%s\", \"block\": \"%s\", \"pools\": %u, \"set\": %d, \"leaves_hint\": %d, ", first_scenario ? "" : ",",
              name, hd.block, plan_pools(hd.s), sp.set, (int)sp.leaves_hint);
  first_scenario = false;
  std::printf("\"counters\": [%u, %u, %u, %u], \"launches\": [", hd.ctr.call_no, hd.ctr.hint_call, hd.ctr.so_call, hd.ctr.prio_call);
  for (size_t i = 0; i < sp.launches.size(); ++i) {
    const Launch& L = sp.launches[i];
    std::printf("%s\n  {\"kind\": \"%s\", \"cls\": %d, \"grid\": %d, ", i ? "," : "", kKind[L.kind], L.cls, L.grid);
    print_list("list", L.list);
    print_list("next", L.next);
    std::printf("\"count\": %d, \"qhead\": %d, \"next_count\": %d, \"clear_counts\": %d, \"status_or\": %d, ", L.count, L.qhead,
                L.next_count, (int)L.clear_counts, L.status_or);
    std::printf("\"sk\": %d, \"rid0\": %d, \"list_hi\": %d, \"grp\": %d, \"wk_zero\": %d, ", L.sk, L.rid0, L.list_hi, L.grp, (int)L.wk_zero);
    std::printf("\"hint_hard\": %d, \"hint_max\": [%d, %d, %d], ", L.hint_hard, L.hint_max_r, L.hint_max_w, L.hint_max_z);
    std::printf("\"so_first\": %d, \"so_nseg\": %d, \"so_tag\": %u, \"so_maxfit\": %d, \"so_keys_from_hint\": %d, \"prio_tag\": %u}",
                L.so_first, L.so_nseg, L.so_tag, L.so_maxfit, (int)L.so_keys_from_hint, L.prio_tag);
  }
  std::printf("]}");
}

}  // namespace

int main() {
  std::printf("[");
  {  // 1: one round of the 64-row class, twice
    Handle a("1024_h10_s20", 1024, 10, 20, 20);
    solve(a, "s1_call1", 1024);
    solve(a, "s1_call2", 1024);
  }
  {  // 2: many rounds of the dense 64-row class
    Handle b("16384_h10_s20", 16384, 10, 20, 20);
    solve(b, "s2_call1", 16384);
    solve(b, "s2_call2", 16384);
    solve(b, "s2_b2048_call1", 2048);
    solve(b, "s2_b2048_call2", 2048);
  }
  {  // 3: the controller's per-robot tick
    Handle c("256_h14", 256, 14, 0, 0);
    solve(c, "s3_due_tick", 256, true, true);
  }
  {  // 4: scenario 1 captured / with the priority tag about to wrap / at three workgroups per CU
    Handle a("1024_h10_s20", 1024, 10, 20, 20);
    solve(a, "s4_captured", 1024, false, false, true);
    Handle w("1024_h10_s20", 1024, 10, 20, 20);
    w.ctr.prio_call = 0xffffffffu;
    solve(w, "s4_prio_wrap", 1024);
    Handle t("1024_h10_s20", 1024, 10, 20, 20);
    solve(t, "s4_batch768", 768);
  }
  {
    Handle d("8192_h10", 8192, 10, 0, 0);
    solve(d, "s4_mixed8192", 8192);
  }
  {
    Handle e("512_h10_s40_chunks3", 512, 10, 40, 40, 0, 3);
    solve(e, "s4_chunks3", 300);
  }
  {
    Handle f("1024_h20_jcqp1", 1024, 20, 0, 0, 1);
    solve(f, "s4_jcqp_h20", 1024);
    solve(f, "s4_jcqp_h20_commands", 1024, true);
  }
  {
    Handle g("256_h20_s64", 256, 20, 64, 0);
    solve(g, "s4_h20_exact_s64", 256);
  }
  std::printf("\n]\n");
  return 0;
}
