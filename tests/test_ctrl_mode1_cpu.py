"""CPU suite for robot mode 1 of the batched locomotion controller (qmpc_ctrl_set_robot_mode, include/qmpc_ctrl.h).

The restatement (tests/ctrl_model_mode1.py) and the kernel (qmpc_glue.hip: qmpc_ctrl_loco_kernel<1>) come from one reading
of ConvexMPCLocomotion.cpp:173-233, so this file also pins facts derived from those lines by hand, independently of both:
  * the horizon claim: every tick that solves has horizonLength 10 and is not a phase-0 tick;
  * the gait the phase-0 branch selects for settled velocity commands, integer by integer;
  * the solve's table: rows 0 .. 9 of the robot's n-row table, and the identity the controller's internal route to the
    solve rests on -- those ten rows are themselves the table of a 10-segment offset / duration gait.
"""
import ctypes as C

import numpy as np

from quadruped_ctrl_amd import binding

import ctrl_model as M
import ctrl_model_mode1 as M1
from c_headers import binding_agrees_with_ctrl_arrays, ctrl_arrays
from ctrl_model import calm_est
from ctrl_model_mode1 import NSEGS, sweep_vel

f32, f64 = np.float32, np.float64


def test_set_robot_mode_exported_and_declared():
    import __graft_entry__ as g
    g.build()
    lib = C.CDLL(binding.LIB_PATH)
    assert hasattr(lib, "qmpc_ctrl_set_robot_mode")
    assert "qmpc_ctrl_set_robot_mode" in binding.CTRL_EXPORTS
    assert binding.CTRL_SIGNATURES["qmpc_ctrl_set_robot_mode"] == [C.c_void_p, C.c_int]
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    assert lib.qmpc_ctrl_set_robot_mode(None, 1) == 1           # a null handle: QMPC_ERR_ARG, no device needed
    assert hasattr(binding.BatchedController, "set_robot_mode")


def test_new_rows_are_in_the_array_list_and_the_binding():
    binding_agrees_with_ctrl_arrays()                           # int rows == CTRL_INT_ARRAYS
    arrays = ctrl_arrays()
    assert arrays["nseg"] == ("int", 1) and arrays["gait_phase"] == ("float", 1)
    assert arrays["mpc_offsets"] == ("int", 4) and arrays["mpc_durations"] == ("int", 4)
    assert {"nseg", "mpc_offsets", "mpc_durations"} <= set(binding.CTRL_INT_ARRAYS)
    assert "gait_phase" not in binding.CTRL_INT_ARRAYS


# ---- the horizon claim, on the model alone
def test_every_solving_tick_has_horizon_ten():
    B, ticks, seg = 72, 3200, 800
    m = M1.CtrlModelMode1(B)
    m.set_gait(np.where(np.arange(B) % 5 == 0, 29, 9))          # (omni robots among them; the gait number selects nothing else)
    est = calm_est(B, np.random.default_rng(7))
    seen = [set() for _ in range(B)]
    restarts = np.zeros(B, int)
    solves = np.zeros(B, int)
    cases = set()
    for t in range(ticks):
        if t % seg == 0:
            m.set_vel(sweep_vel(B, t // seg))
        before = m.counter.copy()
        m.loco(est)
        due = m.due
        # a tick that solves: horizonLength 10, not a phase-0 tick, current_gait 9 (the stand trajectory is never taken)
        assert (m.horizon[due] == 10).all(), t
        assert not (m.phase0 & due).any(), t
        assert (m.current_gait[due] == 9).all(), t
        assert (before[due] % 13 == 12).all(), t
        # a restart leaves the counter at 1; a phase-0 tick without one follows a tick whose counter was a multiple of
        # 13 n, so it leaves 2 (mod 13 n) -- neither is a multiple of 13
        assert (m.counter[m.restarted] == 1).all(), t
        if t > 0:
            nr = m.phase0 & ~m.restarted
            assert ((m.counter[nr] - 2) % (13 * m.nseg[nr]) == 0).all(), t
        restarts += m.restarted & (before > 0)
        solves += due
        for b in range(B):
            seen[b].add(int(m.nseg[b]))
        for b in np.flatnonzero(m.phase0):
            cases.add((int(m.nseg[b]), tuple(m.offsets[b]), int(m.durations[b, 0]), int(m.current_gait[b])))
        # the horizon is not 10 only on phase-0 ticks, which never solve
        assert (m.horizon[~m.phase0] == 10).all()
    # coverage, asserted: an input that exercises nothing fails
    assert set().union(*seen) == NSEGS
    assert (restarts >= 1).all(), restarts.min()
    assert (solves >= ticks // 13 - 3 * 4).all() and solves.min() > 200
    kinds = {(n, g) for n, _, _, g in cases}
    assert {(10, 4), (10, 9), (16, 9), (14, 9), (13, 9), (12, 9), (11, 9)} <= kinds
    assert any(n == 16 and off == (0, 8, 4, 12) and d == 12 for n, off, d, _ in cases)         # walking
    assert any(n == 16 and off[2] not in (4,) and d < 12 for n, off, d, _ in cases)             # walk-to-trot


# ---- hand-derived cases (from :175-227 by hand; float32 filter, double vBody)
SETTLE_X = (0.32, 0.8, 1.75, 1.5, 1.48, 0.0, 0.0)
SETTLE_YAW = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5)
_settled = {}


def _settle(x, yaw=0.0):
    """The robot commanded (x, 0, yaw) after 1600 ticks (16 time constants of the x filter, 7 or more gait cycles): one
    model run for all the cases, one robot each -> (a view of that robot, its filtered x velocity as a double)."""
    if not _settled:
        B = len(SETTLE_X)
        m = M1.CtrlModelMode1(B)
        m.set_vel(np.stack([SETTLE_X, np.zeros(B), SETTLE_YAW], 1))
        est = calm_est(B, np.random.default_rng(1))
        for _ in range(1600):
            m.loco(est)
        _settled["m"] = m
    m = _settled["m"]
    b = [i for i in range(len(SETTLE_X)) if (SETTLE_X[i], SETTLE_YAW[i]) == (x, yaw)][0]

    class Row:
        nseg, offsets, durations = m.nseg[b:b + 1], m.offsets[b:b + 1], m.durations[b:b + 1]
        vel_des, swing_state = m.vel_des[b:b + 1], m.swing_state[b:b + 1]
    return Row, float(f64(m.vel_des[b, 0]))


def _margin(products):
    """Distance of each double product from the nearest integer: float rounding of the filtered velocity (relative
    1e-5 at most, see the settled values) cannot flip a truncation that is 0.05 away from one."""
    return min(abs(p - round(p)) for p in products)


def test_hand_derived_settled_gaits():
    # 0.32: walk-to-trot, h = 16; offsets (0, 8, int(16 * 0.4), int(16 * 0.9)) = (0, 8, 6, 14); durations int(16 * 0.6) = 9
    m, v = _settle(0.32)
    assert abs(v - 0.32) < 1e-4 and _margin([16 * 1.25 * v, 16 * (1.25 * v + 0.5), 16 * (1 - 1.25 * v)]) >= 0.05
    assert m.nseg[0] == 16 and tuple(m.offsets[0]) == (0, 8, 6, 14) and tuple(m.durations[0]) == (9,) * 4
    # 0.8: trot, h = 14
    m, v = _settle(0.8)
    assert 0.4 + 0.05 < v < 1.4 - 0.05
    assert m.nseg[0] == 14 and tuple(m.offsets[0]) == (0, 7, 7, 0) and tuple(m.durations[0]) == (7,) * 4
    # 1.75: h = int(42 - 35) = 7, raised to 10 (any value below 10 is: the margin that matters is to 10)
    m, v = _settle(1.75)
    assert -20.0 * v + 42.0 < 10 - 0.05
    assert m.nseg[0] == 10 and tuple(m.offsets[0]) == (0, 5, 5, 0) and tuple(m.durations[0]) == (5,) * 4
    # 1.5: h = int(42 - 30) = 12.  The product is an integer at the command itself, so this case cannot have the 0.05
    # margin; it holds because the float32 filter approaches the command from below and stalls below it (x * 0.99f +
    # 1.5f * 0.01f stops moving once the step is under half an ulp): v < 1.5, so 42 - 20 v > 12.  1.48 is its neighbour
    # with the margin (42 - 29.6 = 12.4).
    m, v = _settle(1.5)
    assert v < 1.5 and -20.0 * v + 42.0 > 12.0 and abs(v - 1.5) < 1e-4
    assert m.nseg[0] == 12 and tuple(m.offsets[0]) == (0, 6, 6, 0) and tuple(m.durations[0]) == (6,) * 4
    m, v = _settle(1.48)
    assert _margin([-20.0 * v + 42.0]) >= 0.05
    assert m.nseg[0] == 12 and tuple(m.offsets[0]) == (0, 6, 6, 0) and tuple(m.durations[0]) == (6,) * 4
    # command 0, yaw command 0: standing, all feet down on 10 segments, gaitNumber 4 on the phase-0 ticks
    m, v = _settle(0.0)
    assert v == 0.0 and m.nseg[0] == 10 and tuple(m.offsets[0]) == (0, 0, 0, 0) and tuple(m.durations[0]) == (10,) * 4
    assert (M1.mpc_rows(m.offsets[0], m.durations[0], 3, 10) == 1).all() and (m.swing_state == 0).all()
    assert M1.aio_select(0.0, 0.0, 0.0)[3] == 4 and M1.aio_select(0.0, 0.0, 0.5)[3] == 9
    # yaw command 0.5 alone: the 10-segment trot
    m, v = _settle(0.0, yaw=0.5)
    assert m.vel_des[0, 2] > 0.4
    assert m.nseg[0] == 10 and tuple(m.offsets[0]) == (0, 5, 5, 0) and tuple(m.durations[0]) == (5,) * 4
    # the abs of :180 is the float overload: a yaw rate of 0.009 stands, 0.011 trots (int abs(int) would stand at both)
    assert M1.aio_select(0.0, 0.0, 0.009)[3] == 4 and M1.aio_select(0.0, 0.0, 0.011)[2] == (5,) * 4
    # vBody is sqrt(x * x) + y * y, not a norm: x = 0.3, y = 0.4 gives 0.46 (trot, 14), where the norm 0.5 would too, but
    # x = 0, y = 0.5 gives 0.25 (walk-to-trot, 16) where the norm 0.5 gives the trot
    assert M1.aio_select(0.0, 0.5, 0.0)[0] == 16 and M1.aio_select(0.3, 0.4, 0.0)[0] == 14
    # the fast trot never exceeds 13 segments: vBody > 1.4 gives h < 14; x is clipped to 2.0, y to 0.6
    assert M1.aio_select(1.4001, 0.0, 0.0)[0] == 13 and M1.aio_select(2.0, 0.6, 0.0)[0] == 10


# ---- the table the solve reads
def test_table_rule():
    """Rows 0 .. 9 of the n-row table are table[i][j] = (((i + iteration + 1) % n - offset_j) mod n) < duration_j."""
    gaits = {11: ((0, 5, 5, 0), (5,) * 4), 13: ((0, 6, 6, 0), (6,) * 4), 16: ((0, 8, 4, 12), (12,) * 4)}
    for n, (off, dur) in gaits.items():
        for it in range(n):
            rows = M1.mpc_rows(off, dur, it, n)
            assert np.array_equal(rows, M.mpc_table(off, dur, it, n=n)[:40]), (n, it)
            direct = [1 if ((i + it + 1) % n - off[j]) % n < dur[j] else 0 for i in range(10) for j in range(4)]
            assert list(rows) == direct, (n, it)
    off, dur = gaits[16]
    differs = [it for it in range(10) if not np.array_equal(M1.mpc_rows(off, dur, it, 16), M.mpc_table(off, dur, it, n=10)[:40])]
    assert differs, "the 16-segment walk read as a 10-segment gait of the same offsets must differ"


def window_gait(iteration, off, dur, n):
    """qmpc_ctrl_window_gait (qmpc_glue.hip), restated: the 10-segment (offset', duration') whose table at `iteration`
    equals rows 0 .. 9 of the n-segment gait's."""
    place = [0] * 10
    for i in range(10):
        it = (i + iteration + 1) % n
        pr = it - off
        if pr < 0:
            pr += n
        if pr < dur:
            place[(i + iteration + 1) % 10] = 1
    start = [p for p in range(10) if place[p] and not place[p - 1]]
    return (start[0] if start else 0), sum(place)


def test_ten_rows_of_any_table_are_a_ten_segment_gait():
    """The controller hands the solve's command stage (n_segments = horizon = 10, unchanged) a 10-segment gait per leg
    with the same ten rows.  Exhaustive over n = 10 .. 16, every offset 0 .. n (the walk-to-trot case reaches
    offset == n at vBody = 0.4), every duration 0 .. n and every iteration."""
    for n in range(10, 17):
        for off in range(n + 1):
            for dur in range(n + 1):
                for it in range(n):
                    o10, d10 = window_gait(it, off, dur, n)
                    want = M.mpc_table((off,) * 4, (dur,) * 4, it, n=n)[0:40:4]
                    got = M.mpc_table((o10,) * 4, (d10,) * 4, it, n=10)[0:40:4]
                    assert np.array_equal(want, got), (n, off, dur, it)
