// qmpc_span.h -- the plan of one qmpc_fleet_run call (include/qmpc_fleet.h) as a VALUE, and the span kernel's launcher.
//
// A closed-loop tick is the stage sequence  E (estimators + leg data)  L (safety + locomotion)  [solve]  C (leg command)
// P (plant step).  Nothing but the solve couples two robots, so everything between two solves -- a SPAN -- runs in one
// launch of qmpc_span.hip's kernel: it starts with C, P of the tick that has just solved, runs E, L, C, P of every
// following tick, and ends behind E, L of the next tick that solves.  A call begins and ends on a whole tick (effort,
// state and motor are as the last P left them), so the first span of a call starts at E and the last one stops behind P.
//
// The first part is host-only integer logic in the manner of qmpc_plan.h: no HIP, no handle, no device pointer;
// tests/span_dump.cpp compiles it alone.  The second part (HIP only) is what qmpc_span.hip defines and qmpc_capi_ctrl.cpp calls.
#ifndef QMPC_SPAN_H
#define QMPC_SPAN_H

#include <vector>

// One launch of the span kernel, in the kernel's own three arguments, and what the host does behind it.
//   first_at_c   the first tick of the launch starts at C (its E, L ran in the previous launch, its solve in between)
//   ticks        ticks the launch touches, 1 .. 14 in lockstep (C, P of one tick, twelve whole ticks, E, L of the next)
//   last_after_l the last tick of the launch stops behind L: a solve follows (then `solve` is set)
//   locos        L stages in the launch = ticks the controller's T advances by when the launch is enqueued
//   reset_due    per-robot schedule: the due list's count is set to 0 in front of the launch (the span's E does not do
//                it: another workgroup's L could append before the reset lands)
struct SpanLaunch {
  int first_at_c = 0, ticks = 0, last_after_l = 0;
  int locos = 0;
  bool reset_due = false, solve = false;
};

constexpr int kSpanMpcPeriod = 13;  // iterationsBetweenMPC: a lockstep solve follows L where the incremented T is a multiple

// The launches of a call of `ticks` whole ticks on a controller that has enqueued T ticks so far.
// Lockstep: tick k (0-based) of the call solves where (T + k + 1) % 13 == 0.  Per-robot schedule: every tick solves (over
// the due list, which may be empty), so every launch but the last is C, P of one tick and E, L of the next.
inline std::vector<SpanLaunch> plan_spans(long long T, int ticks, bool per_robot) {
  std::vector<SpanLaunch> plan;
  int cur = 0;       // the tick the next launch starts in
  bool mid = false;  // ... behind its solve, at C
  while (cur < ticks) {
    int s = mid ? cur + 1 : cur;  // the next tick that solves, from the first one whose L is still to run
    while (s < ticks && !(per_robot || (T + s + 1) % kSpanMpcPeriod == 0)) ++s;
    SpanLaunch l;
    l.first_at_c = mid ? 1 : 0;
    l.solve = s < ticks;
    l.last_after_l = l.solve ? 1 : 0;
    l.ticks = (l.solve ? s + 1 : ticks) - cur;
    l.locos = l.ticks - (mid ? 1 : 0);
    l.reset_due = per_robot && l.locos > 0;
    plan.push_back(l);
    if (!l.solve) break;
    cur = s;
    mid = true;
  }
  return plan;
}

#if defined(__HIPCC__)
#include "qmpc_glue.h"
#include "qmpc_plant.h"

// The arguments of a span launch, filled in one place (qmpc_capi_ctrl.cpp: qmpc_fleet_run).  The plant's part is the flat
// step's (QmpcPlantStepArgs without terrain, contact and field); effort, state and motor are the caller's rows, read AND
// written by the launch.  n = batch * 4 lanes.
struct QmpcSpanArgs {
  QmpcCtrlDev C;
  QmpcLegGeom g;
  QmpcPlantDev S;
  QmpcPlantConst K;
  double *effort, *state, *motor;
  int n;
  QmpcPlantVary V;
  int build_list;  // per-robot schedule: L appends the due robots to C.due_list
};

// robot_mode 0 / 1, vary and stats as in qmpc_launch_plant_step; first_at_c, ticks, last_after_l: SpanLaunch's
extern "C" hipError_t qmpc_launch_span(const QmpcSpanArgs* A, int robot_mode, int vary, int stats, int first_at_c,
                                       int ticks, int last_after_l, hipStream_t stream);
#endif

#endif
