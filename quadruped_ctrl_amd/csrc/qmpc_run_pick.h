// qmpc_run_pick.h -- which kernel serves a call of the fleet run or the loop run and what its `reason` says, as a pure
// function of the handle's ground-run switch (include/qmpc_ground_run.h), what is bound to the plant and the call's
// options.  No HIP, no handle: tests/run_pick_dump.cpp includes this header alone and prints the choice for every
// combination.  qmpc_capi_ctrl.cpp calls it from both entry points.
#ifndef QMPC_RUN_PICK_H
#define QMPC_RUN_PICK_H

enum QmpcRunKernel {
  QMPC_RUN_SPAN,          // qmpc_span.hip: the flat plant, no option
  QMPC_RUN_LOOP,          // qmpc_loop.hip: the flat plant with the actuator stage and / or the episode step
  QMPC_RUN_LOOP_TERRAIN,  // qmpc_loop.hip with QMPC_LOOP_GROUND=1: terrain rows, any options (none: the fleet run's)
  QMPC_RUN_LOOP_FIELD,    // qmpc_loop.hip with QMPC_LOOP_GROUND=2: a height-field bank on any rows, any options
  QMPC_RUN_PER_TICK,      // the fallback: the per-tick calls themselves
  QMPC_RUN_KERNELS
};

// The bits of `reason` (the values of both public headers' enums: qmpc_capi_ctrl.cpp asserts it)
enum { QMPC_RUN_REASON_TERRAIN = 1, QMPC_RUN_REASON_CONTACT = 2, QMPC_RUN_REASON_FIELD = 4 };

struct QmpcRunPick {
  QmpcRunKernel kernel;
  int reason;  // not 0: kernel is QMPC_RUN_PER_TICK, and the other way round
};

// ground_run: the handle's switch; rows: terrain rows are bound (include/qmpc_terrain.h); contact: the contact flags are
// not 0 (include/qmpc_contact.h); field: a height-field bank is bound (include/qmpc_field.h); actuators, episodes: the
// loop run's options (the fleet run: both false).
// Switch off: every bound ground is a reason and the call falls back, as it always did.  Switch on: the fused kernels
// cover rows and a bank with scheduled contact, in every <MODE, VARY, STATS> instantiation (all sixteen compile without
// scratch), so the only reason left is contact decided by the ground -- alone: what the fused kernels would cover under
// it is not named.
inline QmpcRunPick qmpc_run_pick(bool ground_run, bool rows, bool contact, bool field, bool actuators, bool episodes) {
  QmpcRunPick p;
  p.reason = ground_run ? (contact ? QMPC_RUN_REASON_CONTACT : 0)
                        : (rows ? QMPC_RUN_REASON_TERRAIN : 0) | (contact ? QMPC_RUN_REASON_CONTACT : 0) |
                              (field ? QMPC_RUN_REASON_FIELD : 0);
  p.kernel = p.reason ? QMPC_RUN_PER_TICK
             : field  ? QMPC_RUN_LOOP_FIELD
             : rows   ? QMPC_RUN_LOOP_TERRAIN
             : (actuators || episodes) ? QMPC_RUN_LOOP : QMPC_RUN_SPAN;
  return p;
}

#endif
