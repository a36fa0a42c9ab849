"""GPU suite (-m gpu) for the batched controller's ticks driven by simulator ground truth (qmpc_ctrl_prework_state /
qmpc_ctrl_tick_state, include/qmpc_ctrl.h; BatchedController.prework_state / tick_state).

The estimator stage is compared with tests/ctrl_model_state.py (the cheater estimators restated in numpy float32): bit
for bit where no transcendental is involved -- the quaternion, rBody, the three rBody^T products, position and the
velocities -- and within the suite's 1e-5 rad for rpy (the device's atan2f / asinf).  Everything after the estimators is
the existing tick, so it is checked with the existing restatements (tests/ctrl_model.py, tests/ctrl_model_mode1.py)
teacher-forced on the GPU's own estimator read-out (tests/ctrl_gpu.py: teacher_forced_state, mode1_state), under the rules
of tests/test_gpu_controller.py and tests/test_gpu_ctrl_mode1.py; the remaining tests compare two runs of the library bit for bit.
"""
import numpy as np
import pytest

from quadruped_ctrl_amd import workloads as W

import ctrl_model as M
from ctrl_gpu import EXACT_F32, EXACT_I32, PID, make_ctrl, mode1_state, teacher_forced_state, to_dev
from ctrl_model import command_gaits, command_vel
from ctrl_model_state import ACC, OMEGA, ORI, POS, VBODY, estimate_state

pytestmark = pytest.mark.gpu

f32 = np.float32
EST_EXACT = ("orientation", "r_body", "omega_body", "omega_world", "a_world", "position", "v_world", "v_body")
LEG = ("q", "qd", "leg_J", "leg_p", "leg_v")


def test_estimator_stage_bit_for_bit():
    """257 robots (1028 threads: the last block is partial), one prework_state: the whole circle of yaw, rolls up to
    0.45 rad, pitches up to 0.3 rad."""
    B = 257
    state, motor = W.make_state_stream(B, 1, 101)
    state, motor = state[0], motor[0]
    rng = np.random.default_rng(102)
    rpy = np.stack([0.45 * np.cos(np.arange(B) * 0.37), rng.uniform(-0.3, 0.3, B), np.linspace(-3.14, 3.14, B)], 1)
    rpy[1:3] = [[0.45, 0.3, 1.0], [0, 0, 0]]              # (robots 0 and 256 sit at the two ends of the circle)
    state[:, ORI] = W._quat_from_rpy(rpy)
    c, ref = make_ctrl(B), make_ctrl(B)
    c.prework_state(to_dev(c, state), to_dev(c, motor))
    imu, _ = W.make_tick_stream(B, 1, 101)
    ref.prework(to_dev(ref, imu[0]), to_dev(ref, motor))
    m = M.CtrlModel(B, 500.0, PID)
    e = estimate_state(m, state, motor)
    assert np.abs(e["rpy"][:, 0]).max() > 0.44 and np.ptp(e["rpy"][:, 2]) > 6.2
    for k in EST_EXACT:
        g = c.read(k)
        assert np.array_equal(g, e[k]), (k, np.abs(g - e[k]).max())
    assert np.array_equal(c.read("position"), state[:, POS].astype(f32))
    d = np.abs(c.read("rpy") - e["rpy"]).max()
    assert d < 1e-5, d
    for k in LEG:
        assert np.array_equal(c.read(k), ref.read(k)), k
    assert (c.read("counter") == 0).all() and (c.read("first_run") == 1).all() and c.view()["ticks"] == 0
    c.close()
    ref.close()


def test_one_code_path_for_the_orientation():
    """The IMU path's orientation read-out fed back as a state quaternion gives the IMU path's derived quantities bit for
    bit: both estimators call the same quaternionToRotationMatrix / quatToRPY / rBody^T code."""
    B = 64
    imu, motor = W.make_tick_stream(B, 1, 111)
    a, b = make_ctrl(B), make_ctrl(B)
    a.prework(to_dev(a, imu[0]), to_dev(a, motor[0]))
    state = np.zeros((B, 16))
    state[:, ORI] = a.read("orientation").astype(np.float64)
    state[:, OMEGA] = imu[0][:, 7:10]
    state[:, ACC] = imu[0][:, 0:3]
    state[:, POS] = [0, 0, 0.29]
    b.prework_state(to_dev(b, state), to_dev(b, motor[0]))
    for k in ("orientation", "rpy", "r_body", "omega_world", "a_world"):
        assert np.array_equal(a.read(k), b.read(k)), k
    assert np.abs(a.read("rpy")[:, 2]).max() < 1e-6      # (the IMU path re-based yaw on this first visit)
    a.close()
    b.close()


def test_filter_is_left_alone():
    B = 32
    c = make_ctrl(B)
    keys = ("xhat", "P", "first_visit", "ori_ini_inv", "kf_p", "kf_v")
    before = {k: c.read(k) for k in keys}
    assert (before["first_visit"] == 1).all() and (before["P"][:, 0] == 100).all()
    state, motor = W.make_state_stream(B, 20, 121)
    c.set_vel(to_dev(c, command_vel(B, 122)))
    for t in range(20):
        eff = c.tick_state(to_dev(c, state[t]), to_dev(c, motor[t]))
    assert np.isfinite(eff.cpu().numpy()).all() and c.view()["ticks"] == 20
    for k in keys:
        assert np.array_equal(c.read(k), before[k]), k
    c.close()


def test_teacher_forced_tick_parity_state():
    """tests/ctrl_gpu.py: teacher_forced with tick_state: robot mode 0, lockstep, 257 robots, 40 ticks (three
    MPC ticks), every gait number and omni variant, switched at tick 20.

    The stream is make_state_stream's with every robot's yaw re-based on its tick-0 yaw (ctrl_model_state.rebase_yaw).
    Why: the reference's controller starts with _yaw_des_true = 0 and re-anchors it only beyond 5 rad
    (ConvexMPCLocomotion.cpp:106), and the cheater estimator, unlike the sensor path's, does not re-base yaw.  With the
    raw stream (yaw uniform on the circle) the walking-gait robots with |yaw| > 2.1 rad get a yaw error of radians into
    the MPC, and the REFERENCE's qpOASES stops at its cap of 100 working-set recalculations (SolverMPC.cpp:527-541) on
    them -- measured on an MI355X: 20 of 257 robots at tick 12, every one with reference nWSR = 100 -- and returns an
    iterate that is not the minimiser, i.e. nothing to compare with (the library is within 6.1e-6 of the same pipeline
    run to convergence on 19 of them; on the 20th, gait 31 at yaw -2.72, it reports status 24 -- fallback route, working
    set full -- and zero forces).  The whole circle of yaw is covered where no solver is involved:
    test_estimator_stage_bit_for_bit, and the raw stream in every other test of this file.  Nobody is dropped here, and
    the test asserts that the reference converged on every robot it compares with."""
    teacher_forced_state(257, 40, 257, 20)


def test_mode1_per_robot_schedule_state():
    """Robot mode 1 on state ticks, 64 robots, 400 ticks, teacher-forced against CtrlModelMode1 as
    tests/test_gpu_ctrl_mode1.py does it (without the oracle solves): x commands over [0, 2] m/s."""
    seen, n_solves = mode1_state(64, 400, 131)
    assert len(seen) >= 3, seen
    assert n_solves > 64 * (400 // 13 - 6)


def test_safety_latch_state():
    """Robot 2's state quaternion has roll 0.7 rad from tick 5: it latches on that tick and outputs zeros from then on;
    robot 1 at roll 0.45 rad keeps running."""
    B, ticks = 6, 30
    c = make_ctrl(B)
    state, motor = W.make_state_stream(B, ticks, 3, roll=(1, 0.45, 0))
    s2, _ = W.make_state_stream(B, ticks, 3, roll=(2, 0.7, 5))
    state[:, 2] = s2[:, 2]
    for t in range(ticks):
        eff = c.tick_state(to_dev(c, state[t]), to_dev(c, motor[t])).cpu().numpy()
        safe, rpy = c.read("safe")[:, 0], c.read("rpy")
        assert safe[1] == 1 and 0.4 < abs(rpy[1, 0]) < 0.5, (t, rpy[1])
        assert safe[2] == (1 if t < 5 else 0), t
        if t >= 5:
            assert 0.5 < abs(rpy[2, 0]) < 1.0 and (eff[2] == 0).all(), (t, rpy[2])
        assert (np.delete(safe, 2) == 1).all(), t
        assert np.abs(eff[[0, 1, 3, 4, 5]]).max(1).min() > 0, t
    c.close()


def test_reset_state_per_robot():
    """Half the robots reset before tick 17 (per-robot schedule): the others are bit-identical to the run without the
    reset; the reset ones restart at counter 0 and first solve 13 ticks later."""
    B, at, ticks = 32, 17, 32
    state, motor = W.make_state_stream(B, ticks, 141)
    a, b = make_ctrl(B, schedule="per_robot"), make_ctrl(B, schedule="per_robot")
    g, v = command_gaits(B, 0, 10 ** 9), command_vel(B, 142)
    mask = np.arange(B) % 2 == 0
    for c in (a, b):
        c.set_gait(to_dev(c, g))
        c.set_vel(to_dev(c, v))
    for t in range(ticks):
        if t == at:
            a.reset(to_dev(a, mask))
            assert (a.read("counter")[mask, 0] == 0).all() and (a.read("counter")[~mask, 0] == at).all()
            a.set_gait(to_dev(a, g))
            a.set_vel(to_dev(a, v))
        x, y = to_dev(a, state[t]), to_dev(a, motor[t])
        ea, eb = a.tick_state(x, y).cpu().numpy(), b.tick_state(x, y).cpu().numpy()
        assert np.array_equal(ea[~mask], eb[~mask]), t
        due = a.read("due")[:, 0]
        if t >= at:
            assert (a.read("counter")[mask, 0] == t - at + 1).all(), t
            assert (due[mask] == (1 if t - at + 1 == 13 else 0)).all(), t       # the 13th tick after the reset
        assert (due[~mask] == (1 if (t + 1) % 13 == 0 else 0)).all(), t
    for k in EXACT_F32 + EXACT_I32 + ("f_ff", "wpd", "xci", "grf", "status", "position", "v_world"):
        assert np.array_equal(a.read(k)[~mask], b.read(k)[~mask]), k
    assert np.abs(a.read("f_ff")[mask]).max() > 1.0 and (a.read("safe") == 1).all()
    a.close()
    b.close()


def test_graph_capture_replay_matches_eager_state():
    """13 captured tick_state calls replayed twice equal 39 eager ticks of a second controller, bit for bit."""
    import torch
    B = 64
    eager, cap = make_ctrl(B), make_ctrl(B)
    dev = eager.device
    state, motor = W.make_state_stream(B, 39, 151)
    for c in (eager, cap):
        c.set_gait(to_dev(c, command_gaits(B, 0, 10 ** 9)))
        c.set_vel(to_dev(c, command_vel(B, 152)))
    for t in range(13):          # first run and one MPC, eager on both
        x, y = to_dev(eager, state[t]), to_dev(eager, motor[t])
        eager.tick_state(x, y)
        cap.tick_state(x, y)
    torch.cuda.synchronize()
    bs = torch.zeros((13, B, 16), dtype=torch.float64, device=dev)
    bm = torch.zeros((13, B, 24), dtype=torch.float64, device=dev)
    be = torch.zeros((13, B, 12), dtype=torch.float64, device=dev)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for k in range(13):
                cap.tick_state(bs[k], bm[k], be[k])
    torch.cuda.current_stream().wait_stream(s)
    for r in range(2):
        lo = 13 * (r + 1)
        bs.copy_(torch.from_numpy(state[lo:lo + 13]))
        bm.copy_(torch.from_numpy(motor[lo:lo + 13]))
        graph.replay()
        torch.cuda.synchronize()
        for k in range(13):
            ee = eager.tick_state(to_dev(eager, state[lo + k]), to_dev(eager, motor[lo + k]))
            torch.cuda.synchronize()
            assert torch.equal(ee, be[k]), (r, k)
    for k in ("f_ff", "p_des", "counter", "xhat", "wpd", "xci", "safe"):
        assert np.array_equal(eager.read(k), cap.read(k)), k
    assert (eager.read("counter") == 39).all() and np.abs(eager.read("f_ff")).max() > 1.0
    eager.close()
    cap.close()


def test_state_argument_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, QmpcError
    c = BatchedController(0, max_batch=8)
    lib, h = c.lib, c.mpc.h
    x = torch.zeros((8, 16), dtype=torch.float64, device=c.device)
    x[:, 0] = 1.0
    y = torch.zeros((8, 24), dtype=torch.float64, device=c.device)
    e = torch.zeros((8, 12), dtype=torch.float64, device=c.device)
    # before init: QMPC_ERR_STATE
    assert lib.qmpc_ctrl_tick_state(h, 8, x.data_ptr(), y.data_ptr(), e.data_ptr(), None) == 3
    assert lib.qmpc_ctrl_prework_state(h, 8, x.data_ptr(), y.data_ptr(), None) == 3
    with pytest.raises(QmpcError):
        c.tick_state(x, y)
    c.init(8, 500.0, PID)
    assert lib.qmpc_ctrl_tick_state(h, 8, None, y.data_ptr(), e.data_ptr(), None) == 1
    assert lib.qmpc_ctrl_tick_state(h, 8, x.data_ptr(), None, e.data_ptr(), None) == 1
    assert lib.qmpc_ctrl_tick_state(h, 8, x.data_ptr(), y.data_ptr(), None, None) == 1
    assert lib.qmpc_ctrl_tick_state(h, 7, x.data_ptr(), y.data_ptr(), e.data_ptr(), None) == 1   # not the initialised batch
    assert lib.qmpc_ctrl_prework_state(h, 8, None, y.data_ptr(), None) == 1
    assert lib.qmpc_ctrl_prework_state(h, 8, x.data_ptr(), None, None) == 1
    assert lib.qmpc_ctrl_prework_state(h, 7, x.data_ptr(), y.data_ptr(), None) == 1
    assert c.view()["ticks"] == 0                                   # nothing above counted as a tick
    for call in (c.tick_state, c.prework_state):
        with pytest.raises(QmpcError):
            call(x.float(), y)                                      # float32
        with pytest.raises(QmpcError):
            call(x[:, :10].contiguous(), y)                         # [B,10]: the IMU layout
        with pytest.raises(QmpcError):
            call(x.cpu(), y)                                        # a CPU tensor
    # the schedule can still be chosen after a prework_state, not after a tick_state
    c.prework_state(x, y)
    assert lib.qmpc_ctrl_set_schedule(h, 1) == 0
    c.tick_state(x, y, e)
    assert lib.qmpc_ctrl_set_schedule(h, 0) == 3 and c.view()["ticks"] == 1
    c.close()
