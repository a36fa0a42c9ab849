"""GPU suite (-m gpu) for the two estimators at the head of an IMU-path tick, tick by tick: the orientation estimator
(csrc/qmpc_glue.hip: qmpc_ctrl_orientation -- first-visit yaw removal, quatProduct, quatToRPY, quaternionToRotationMatrix)
and the Kalman filter (qmpc_kf_kernel) as the controller feeds it.

The teacher-forced suites (test_gpu_controller.py and the files that follow it) start AFTER the estimators: they hand the
GPU's own orientation, rpy, rBody, position and v_world to the restatement, so a wrong estimator passes them by
construction; the free-running test bounds a calm stream loosely.  Here the estimators' outputs themselves are compared
with tests/ctrl_model.py and oracle/glue_oracle.c, on the cases of tests/est_cases.py (tests/test_est_cases_cpu.py shows
on the CPU that the cases reach what they claim and that each pinned decision moves the restatement's bits on them):
  * what has no transcendental in it -- the quaternion product, rBody, the rBody^T products, the whole filter -- BIT FOR BIT,
    NaN equal to NaN at equal places;
  * rpy, one asinf / atan2f away from identical float arguments, within LAND_ULPS ulps of max(1, |angle|) (the project's
    rule for such a value, inside the suite's 1e-5 rad);
  * the first visit's _ori_ini_inv, behind atan2f and then sinf / cosf, within 1e-5 per component and on the same branch
    of rotationMatrixToQuaternion; the restatement continues from the GPU's (teacher forcing, as for the landing points).
"""
import numpy as np
import pytest

from oracle import glue as G

import ctrl_model as M
import est_cases as E
from ctrl_gpu import EXACT_F32, EXACT_I32, LAND_ULPS, PID, make_ctrl, to_dev

pytestmark = pytest.mark.gpu

f32 = np.float32
ORI_EXACT = ("orientation", "r_body", "omega_body", "omega_world", "a_world")


def _first_visit(c, m, imu_row, rows=None):
    """After the GPU's first visit on imu_row: its _ori_ini_inv against the restatement's (1e-5 per component, the same
    branch), then handed to the restatement m.  -> the worst distance."""
    o = np.stack([imu_row[:, 6], imu_row[:, 3], imu_row[:, 4], imu_row[:, 5]], 1).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = M.yaw_inverse_quat(M.quat_to_rpy(o)[:, 2])
    got = c.read("ori_ini_inv")
    assert (c.read("first_visit") == 0).all()
    rows = np.arange(len(o)) if rows is None else rows
    d = np.abs(got[rows].astype(np.float64) - ref[rows]).max()
    assert d <= 1e-5, d
    car = E.carrier(ref[rows])
    assert np.array_equal(E.carrier(got[rows]), car)
    assert (got[rows][np.arange(len(rows)), car] > 0).all()          # 0.25 S is positive: the other component has the sign
    assert np.array_equal(np.sign(got[rows][:, [0, 3]]), np.sign(ref[rows][:, [0, 3]]))   # (a zero's own sign aside)
    assert (got[rows][:, 1:3] == 0).all()
    m.ori_ini_inv[:] = got
    m.first_visit[:] = 0
    return d


def _check_rpy(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    u = E.ulps(got, ref)
    if np.isfinite(u).any():
        assert np.nanmax(u) <= LAND_ULPS, (what, np.nanmax(u))


def test_orientation_stage_on_hard_attitudes():
    """257 robots, 8 visits (qmpc_ctrl_prework each) of est_cases.hard_attitudes: roll over the whole circle, pitch up to
    and at +-pi/2 (the asin clamp at 0.99999; m < -1, where asin is NaN), negated and not normalised quaternions, first
    visits on every side of the branch boundary |yaw| = 2 pi / 3.

    Measured on an MI355X: _ori_ini_inv within 1.19e-07 of the restatement; rpy against an fp64 evaluation of the same
    float arguments within 1.12 ulps on the GPU and 1.36 ulps in the restatement."""
    imu, motor = E.hard_attitudes()
    V, B = imu.shape[:2]
    c = make_ctrl(B)
    m = M.CtrlModel(B, 500.0, PID)
    worst = {"gpu": 0.0, "restatement": 0.0}
    for v in range(V):
        c.prework(to_dev(c, imu[v]), to_dev(c, motor[v]))
        if v == 0:
            d = _first_visit(c, m, imu[0])
            print(f"ori_ini_inv: worst distance to the restatement {d:.3e}")
        with np.errstate(all="ignore"):
            e = m.estimate(imu[v], motor[v])
        for k in ORI_EXACT:
            g = c.read(k)
            assert E.same_bits(g, e[k]), (v, k, np.nanmax(np.abs(g - e[k])))
        got = c.read("rpy")
        _check_rpy(got, e["rpy"], v)
        r64 = E.rpy64(e["orientation"])
        assert np.array_equal(np.isnan(got), np.isnan(r64)), v
        worst["gpu"] = max(worst["gpu"], np.nanmax(E.ulps(got, r64)))
        worst["restatement"] = max(worst["restatement"], np.nanmax(E.ulps(e["rpy"], r64)))
        # the promises of the case hold on the GPU's read-out too
        clamp = np.arcsin(np.float64(f32(0.99999)))
        assert (np.isnan(got[:, 1]) & np.isfinite(got[:, 0])).any() and (E.ulps(got[:, 1], clamp) <= LAND_ULPS).sum() >= 10
        assert np.nanmax(got[:, 1]) <= f32(clamp) + LAND_ULPS * np.finfo(f32).eps      # nobody beyond the clamp
    print(f"rpy against fp64 on the same float arguments: GPU {worst['gpu']:.2f} ulps, "
          f"restatement {worst['restatement']:.2f} ulps")
    assert (c.read("counter") == 0).all() and c.view()["ticks"] == 0
    c.close()


def test_kalman_filter_inside_the_tick():
    """32 robots on the IMU path, every gait number of command_gaits (standing, trotting, walking among them), the calm
    stream, est_cases.TICK_COUNT ticks (1.5 times the restatement's first covariance reset after tick 100): every tick the
    filter's state before it, the contact phase the previous tick left and the tick's rBody, aWorld, omegaBody and
    previous leg data go through oracle.glue.kf_step -- state, covariance, position and both velocities equal the GPU's
    bit for bit.  Swing legs (contact phase 0: trust 0, factor 101) and a late covariance reset are met on the way."""
    B, ticks = E.TICK_B, E.TICK_COUNT
    imu, motor, gait, vel = E.tick_inputs(ticks)
    c = make_ctrl(B)
    c.set_gait(to_dev(c, gait))
    c.set_vel(to_dev(c, vel))
    imu_d, motor_d = to_dev(c, imu), to_dev(c, motor)
    swing_fed, late_reset = False, np.zeros(B, bool)
    for t in range(ticks):
        x, P, phase = c.read("xhat"), c.read("P"), c.read("contact_phase")
        c.tick(imu_d[t], motor_d[t])
        fed = {k: c.read(k) for k in ("r_body", "a_world", "omega_body", "kf_p", "kf_v")}
        pos, vw, vb = G.kf_step(x, P, fed["r_body"], fed["a_world"], fed["omega_body"], phase, fed["kf_p"], fed["kf_v"])
        for k, ref in (("xhat", x), ("P", P), ("position", pos), ("v_world", vw), ("v_body", vb)):
            g = c.read(k)
            assert np.array_equal(g, ref), (t, k, np.abs(g - ref).max())
        swing_fed |= bool((phase == 0).any())
        if t > 100:
            late_reset |= E.is_reset(P)
    assert swing_fed and late_reset.any()
    assert np.isfinite(x).all() and np.isfinite(P).all()
    assert (c.read("safe") == 1).all() and (c.read("counter") == ticks).all()
    print(f"{ticks} ticks: {late_reset.sum()} of {B} robots reset their covariance after tick 100")
    c.close()


def test_non_finite_imu_row_is_contained():
    """16 robots, 30 ticks (two MPC ticks); from tick 3 robot 5's quaternion has a NaN component and robot 9's
    accelerometer an infinite axis.  The two follow the restatement's own estimator run -- orientation and rBody bit for
    bit, rpy under the rule above, NaN at the same places, the safety latch equal: a NaN rpy does NOT latch
    (abs(NaN) >= 0.5 is false, SafetyChecker.cpp:21-22), and quatToRPY's std::min(m, .99999) returns a NaN m
    (orientation_tools.h:199).  Every other robot is bit-identical to the run without the bad values."""
    B, ticks = E.BAD_B, E.BAD_TICKS
    imu, bad, motor = E.non_finite_rows()
    two = np.array([E.BAD_QUAT, E.BAD_ACC])
    rest = np.setdiff1d(np.arange(B), two)
    a, b = make_ctrl(B), make_ctrl(B)
    m = M.CtrlModel(B, 500.0, PID)
    gait, vel = M.command_gaits(B, 0, 10 ** 9), M.command_vel(B, 62)
    for c in (a, b):
        c.set_gait(to_dev(c, gait))
        c.set_vel(to_dev(c, vel))
    m.set_gait(gait)
    m.set_vel(vel)
    for t in range(ticks):
        ea = a.tick(to_dev(a, bad[t]), to_dev(a, motor[t])).cpu().numpy()
        eb = b.tick(to_dev(b, imu[t]), to_dev(b, motor[t])).cpu().numpy()
        if t == 0:
            _first_visit(a, m, bad[0])
        with np.errstate(all="ignore"):
            e = m.estimate(bad[t], motor[t])
            m.loco(e)
        for k in ("orientation", "r_body"):
            assert E.same_bits(a.read(k)[two], e[k][two]), (t, k)
        _check_rpy(a.read("rpy")[two], e["rpy"][two], t)
        assert np.array_equal(a.read("safe")[two, 0], m.safe[two]), (t, a.read("rpy")[two], e["rpy"][two])
        assert np.array_equal(ea[rest], eb[rest]), t
        for k in EXACT_F32 + EXACT_I32:
            assert np.array_equal(a.read(k)[rest], b.read(k)[rest]), (t, k)
        assert np.isfinite(eb).all()
    # the bad values did arrive, and did what the reference does with them
    assert np.isnan(a.read("rpy")[E.BAD_QUAT]).all() and np.isnan(a.read("orientation")[E.BAD_QUAT]).all()
    assert not np.isfinite(a.read("a_world")[E.BAD_ACC]).all() and np.isfinite(a.read("rpy")[E.BAD_ACC]).all()
    assert a.read("safe")[E.BAD_QUAT, 0] == 1 and (b.read("safe") == 1).all()
    a.close()
    b.close()
