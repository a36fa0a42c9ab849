// span_dump.cpp -- prints the plans of qmpc_fleet_run calls as JSON (tests/test_fleet_run_cpu.py compares them with the rule
// stated in Python).  Includes qmpc_span.h alone: the plan needs no HIP and no device.
//   span_dump T_MAX ticks [ticks ...]   ->  one plan per (schedule, T in 0 .. T_MAX, ticks)
#include <cstdio>
#include <cstdlib>

#include "../quadruped_ctrl_amd/csrc/qmpc_span.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int t_max = std::atoi(argv[1]);
  std::printf("[");
  bool first = true;
  for (int per_robot = 0; per_robot < 2; ++per_robot)
    for (int T = 0; T <= t_max; ++T)
      for (int a = 2; a < argc; ++a) {
        const int ticks = std::atoi(argv[a]);
        std::printf("%s\n{\"per_robot\": %d, \"T\": %d, \"ticks\": %d, \"launches\": [", first ? "" : ",", per_robot, T, ticks);
        first = false;
        const std::vector<SpanLaunch> plan = plan_spans(T, ticks, per_robot != 0);
        for (size_t i = 0; i < plan.size(); ++i) {
          const SpanLaunch& l = plan[i];
          std::printf("%s[%d, %d, %d, %d, %d, %d]", i ? ", " : "", l.first_at_c, l.ticks, l.last_after_l, l.locos,
                      (int)l.reset_due, (int)l.solve);
        }
        std::printf("]}");
      }
  std::printf("\n]\n");
  return 0;
}
