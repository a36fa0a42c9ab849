// plant_pick_dump.cpp -- prints which kernel steps and which resets the plant for all eight combinations of (field bound,
// contact flags set, rows bound) as JSON (tests/test_plant_varied_cpu.py compares them with a table derived from the
// public headers).  Includes qmpc_plant_pick.h alone: the choice needs no HIP and no device.
#include <cstdio>

#include "../quadruped_ctrl_amd/csrc/qmpc_plant_pick.h"

namespace {

#define NAME_OF(NAME, name) #name,
const char* kStep[] = {QMPC_PLANT_STEP_KINDS(NAME_OF)};
const char* kReset[] = {QMPC_PLANT_RESET_KINDS(NAME_OF)};
#undef NAME_OF

}  // namespace

int main() {
  static_assert(sizeof kStep / sizeof *kStep == QMPC_STEP_KINDS && sizeof kReset / sizeof *kReset == QMPC_RESET_KINDS,
                "one name per kind");
  std::printf("[");
  for (int i = 0; i < 8; ++i) {
    const bool field = i & 4, contact = i & 2, rows = i & 1;
    const QmpcPlantPick p = qmpc_plant_pick(field, contact, rows);
    std::printf("%s\n{\"field\": %d, \"contact\": %d, \"rows\": %d, \"step\": \"%s\", \"reset\": \"%s\", \"counters\": %d}",
                i ? "," : "", (int)field, (int)contact, (int)rows, kStep[p.step], kReset[p.reset], (int)p.contact);
  }
  std::printf("\n]\n");
  return 0;
}
