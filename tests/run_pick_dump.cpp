// run_pick_dump.cpp -- prints which kernel serves a call of the fleet run or the loop run, and the call's reason bits, for
// all 64 combinations of (ground-run switch, rows bound, contact flags set, field bound, actuators, episodes) as JSON
// (tests/test_ground_run_cpu.py compares them with the rule of include/qmpc_ground_run.h, written out there).  Includes
// qmpc_run_pick.h alone: the choice needs no HIP, no device and no handle.
#include <cstdio>

#include "../quadruped_ctrl_amd/csrc/qmpc_run_pick.h"

int main() {
  const char* kKernel[] = {"span", "loop", "loop_terrain", "loop_field", "per_tick"};
  static_assert(sizeof kKernel / sizeof *kKernel == QMPC_RUN_KERNELS, "one name per kernel");
  std::printf("[");
  for (int i = 0; i < 64; ++i) {
    const bool on = i & 32, rows = i & 16, contact = i & 8, field = i & 4, act = i & 2, ep = i & 1;
    const QmpcRunPick p = qmpc_run_pick(on, rows, contact, field, act, ep);
    std::printf("%s\n{\"switch\": %d, \"rows\": %d, \"contact\": %d, \"field\": %d, \"actuators\": %d, \"episodes\": %d, "
                "\"kernel\": \"%s\", \"reason\": %d}",
                i ? "," : "", (int)on, (int)rows, (int)contact, (int)field, (int)act, (int)ep, kKernel[p.kernel], p.reason);
  }
  std::printf("\n]\n");
  return 0;
}
