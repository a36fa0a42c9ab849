"""GPU suite (-m gpu): robot mode 0 of the batched controller over whole gait cycles and through every clamp of its
locomotion stage (csrc/qmpc_glue.hip: qmpc_ctrl_loco_kernel<0>, then qmpc_ctrl_legcmd_kernel and the pack step).

The other bit-exact mode-0 runs stop after 40 ticks; a gait cycle is 182 ticks and the shortest swing 52.  The cases of
tests/ctrl_cycle_cases.py run 380 ticks -- both cycle wraps, every swing from its own lift-off to its own touch-down in
every reachable gait -- and, in the hard case, drive rpy_int, vel_des and pf_rel into their clamps, yaw_des_true through
its re-anchor and the gait commands through two changes mid-swing.  tests/test_ctrl_cycle_cpu.py shows on the CPU that
the restatement reaches all of that on these inputs, and that the 40-tick case reaches none of it.

The comparison is the one of tests/test_gpu_controller.py and tests/test_gpu_ctrl_state.py, by the helpers they share
(teacher_forced, teacher_forced_state): every robot on every tick, EXACT_I32 and EXACT_F32 bit for bit, sw_pf within
LAND_ULPS = 8 ulps of max(1, |Pf|) and equal where the yaw rate is 0, wpd / xci bit for bit, effort == legcmd(f_ff) bit for
bit.  In the two calm tests f_ff is held on each of the 29 MPC ticks to oracle.pack_commands -> solve_batch ->
forces_to_body within the suite's per-robot bound max(1e-4, 1.5 x the reference's float-order spread), a robot on which
the reference stopped at its nWSR cap being compared with the same pipeline run to convergence, and status & 47 == 0.

Wall times on an MI355X (pytest --durations, one run, this file first in the process): test_two_cycles_state_path 4.0 s
(it also pays the process's first use of the device and of the oracle), test_two_cycles_imu_path 1.7 s,
test_hard_branches_state_path 1.0 s; the yardstick, test_gpu_ctrl_state.py::test_teacher_forced_tick_parity_state (the
same per-tick work, 257 robots x 40 ticks, unchanged by this file), 2.3 s in the same run.  The reference stopped at its
nWSR cap on none of the 2 x 29 x 24 solves of the calm tests (largest nWSR 70).
"""
import numpy as np
import pytest

import ctrl_cycle_cases as CC
from ctrl_gpu import teacher_forced, teacher_forced_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calm():
    return CC.calm_case()


class _Watch:
    """each_tick of the helpers: the coverage trace of the restatement as the device's read-outs drove it, and on MPC ticks
    of a run compared with the oracle the library's status bits."""

    def __init__(self, status):
        self.trace, self.status, self.n_mpc = CC.Trace(), status, 0

    def __call__(self, t, c, m, e):
        self.trace.add(m, e)
        if (t + 1) % 13 == 0:
            self.n_mpc += 1
            if self.status:
                assert (c.read("status")[:, 0] & 47 == 0).all(), t


def test_two_cycles_state_path(calm):
    """The calm case through tick_state: 24 robots, 380 ticks, 29 MPC ticks against the oracle."""
    w = _Watch(status=True)
    teacher_forced_state(calm["B"], calm["ticks"], calm["seed"], 10 ** 9, gaits_at=calm["gaits_at"], vel_at=calm["vel_at"],
                          capped="converged", stream=(calm["state"], calm["motor"]), each_tick=w)
    assert w.n_mpc == 29
    CC.assert_calm_coverage(CC.coverage(w.trace))


def test_two_cycles_imu_path(calm):
    """The same robots through tick on make_tick_stream: the Kalman filter sees contact_phase over whole cycles, and the
    restatement is fed the device's own estimator read-out."""
    w = _Watch(status=True)
    c, m, eff = teacher_forced(calm["B"], calm["ticks"], calm["seed"], 10 ** 9, gaits_at=calm["gaits_at"],
                                vel_at=calm["vel_at"], capped="converged", stream=(calm["imu"], calm["motor"]), each_tick=w)
    assert w.n_mpc == 29 and c.view()["ticks"] == calm["ticks"]
    assert np.isfinite(eff).all() and (c.read("safe") == 1).all()
    c.close()
    CC.assert_calm_coverage(CC.coverage(w.trace))


def test_hard_branches_state_path():
    """The hard case through tick_state: 48 robots, 380 ticks.  Its commands are outside what the reference's solver is
    known to handle (tests/test_gpu_ctrl_state.py records it stopping at its cap on milder ones), so f_ff is taken over
    from the device, as test_safety_latch_and_abs_binding does, and not compared with the oracle; the locomotion stage,
    the pack step's wpd / xci, stance legs carrying exactly f_ff and swing legs nothing, and the effort stay bit-exact.
    The coverage counters are recomputed from the restatement as the device's read-outs drove it, and asserted as on the
    CPU: a device that steers the run away from a branch cannot pass.
    LAND_ULPS stays 8 for every robot: the re-anchor robots turn at 8 rad/s, so coordinateRotation's angle reaches 1.04 rad
    (gait 11, durations 10; 0.62 rad in trotRunning), far from the small angles the bound was argued for; measured on an MI355X, the largest
    landing-point distance of the run is 1.00 ulp (0.25 in the calm case)."""
    case = CC.hard_case()
    w = _Watch(status=False)
    teacher_forced_state(case["B"], case["ticks"], case["seed"], 10 ** 9, gaits_at=case["gaits_at"], vel_at=case["vel_at"],
                          mpc="forced", stream=(case["state"], case["motor"]), each_tick=w)
    cov = CC.coverage(w.trace)
    print({k: cov[k] for k in CC.COUNTERS}, "complete swings", cov["complete_swings"])
    CC.assert_hard_coverage(cov)
