"""GPU suite (-m gpu) for the batched locomotion controller (include/qmpc_ctrl.h, quadruped_ctrl_amd.BatchedController)
against the numpy restatement in tests/ctrl_model.py and the oracle pipeline.

Teacher forcing: the restatement consumes the GPU's own estimator outputs (orientation, rpy, rBody, omegaWorld, Kalman
filter position / velocity, leg p / v / J) every tick, so the controller arithmetic is compared on identical inputs.
  * Discrete state (contact / swing flags, firstSwing, firstRun, counters, gait selection and iteration, current_gait,
    the safety latch) must be EXACT.
  * Everything the controller computes without a transcendental must be BIT-EXACT: the clamped joint angles, the
    filtered command, yaw_des_true, rpy_int / rpy_comp, stand_traj, pFoot, pfx_rel / pfy_rel (double promotion and the
    double sqrt included), world_position_desired and x_comp_integral after the solve, the swing trajectories and
    pDes / vDes, and the effort.
  * The landing point Pf goes through coordinateRotation(Z, -yaw_rate * stance_time / 2), i.e. through sin / cos,
    whose device and host implementations may differ by an ulp.  It is bounded by LAND_ULPS ulps of max(1, |Pf|)
    (|Pf| is metres: with |pYawCorrected| < 0.3 m a 1-ulp sin / cos difference moves Pf by < 1e-7 m), and the
    restatement then continues from the GPU's Pf, so that nothing downstream is compared under a tolerance.
MPC coupling: on every MPC tick f_ff matches oracle.pack_commands -> qpOASES -> forces_to_body within the suite's
per-robot bound max(1e-4, 1.5 x the reference's own float-order spread) (test_gpu_parity.py); stance legs carry
exactly f_ff, swing legs zero; effort equals oracle.glue.leg_command of the GPU's commands.
Free running (both sides run their own estimator): the estimator's atan2 / asin / sin / cos differ by an ulp, and the
first Kalman filter steps from P = 100 I amplify that to ~1e-4 m (test_gpu_glue.py::test_estimator_to_mpc_chain_on_device
explains the gain), so position / velocity are bounded by 1e-3 m / 1e-2 m/s and rpy by 1e-5 rad, as in that test.
"""
import numpy as np
import pytest

from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W

import ctrl_model as M
from ctrl_gpu import PID, gpu_est, make_ctrl, teacher_forced
from ctrl_model import command_gaits, command_vel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [1, 257, 4096])
def test_teacher_forced_tick_parity(B):
    c, m, eff = teacher_forced(B, 40, seed=B, check_mpc=B <= 257)
    assert np.isfinite(eff).all()
    assert (c.read("safe") == 1).all()
    c.close()


def test_mpc_coupling_large_batch():
    """The oracle check of f_ff on every MPC tick at 1024 robots, all gait numbers and omni variants."""
    c, m, eff = teacher_forced(1024, 27, seed=5)
    c.close()


@pytest.mark.parametrize("prework", [False, True])
def test_free_running_parity(prework):
    """Both sides run their own estimator.  prework=True: the reference's call sequence init_controller -> pre_work ->
    torque_calculator..., i.e. qmpc_ctrl_prework once before the ticks (estimators and leg data, no control step)."""
    import torch
    B, ticks = 64, 130
    c = make_ctrl(B)
    m = M.CtrlModel(B, 500.0, PID)
    imu, motor = W.make_tick_stream(B, ticks + 1, 11)
    vel = command_vel(B, 12)
    g = command_gaits(B, 0, 10 ** 9)
    c.set_vel(torch.from_numpy(vel).to(c.device))
    c.set_gait(torch.from_numpy(g).to(c.device))
    m.set_vel(vel)
    m.set_gait(g)
    worst = {}
    if prework:
        c.prework(torch.from_numpy(imu[0]).to(c.device), torch.from_numpy(motor[0]).to(c.device))
        e = m.estimate(imu[0], motor[0])
        assert (c.read("counter") == 0).all() and (c.read("first_run") == 1).all() and c.view()["ticks"] == 0
        assert np.abs(c.read("rpy") - e["rpy"]).max() < 1e-5
        assert np.abs(c.read("position") - e["position"]).max() < 1e-3
        assert np.abs(c.read("leg_p") - e["leg_p"]).max() < 1e-6   # (sinf / cosf: an ulp)
    for t in range(1, ticks + 1):
        eff = c.tick(torch.from_numpy(imu[t]).to(c.device), torch.from_numpy(motor[t]).to(c.device)).cpu().numpy()
        e = m.estimate(imu[t], motor[t])
        m.loco(e)
        if t % 13 == 0:
            rec, wpd, xci = O.pack_commands(m.command(e), float(m.dt_mpc))
            m.wpd[:], m.xci[:] = wpd, xci
            rec.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)
            soln, _, rc = O.solve_batch(rec)
            m.f_ff[:] = O.forces_to_body(e["r_body"], soln[:, :12].astype(np.float32))
        m.legcmd(e, m.f_ff)
        for k in ("counter", "first_swing", "iteration", "safe", "current_gait"):
            assert np.array_equal(c.read(k).reshape(getattr(m, k).shape), getattr(m, k)), (t, k)
        assert np.array_equal(c.read("swing_state") > 0, m.swing_state > 0), t
        for k, tol in (("rpy", 1e-5), ("position", 1e-3), ("v_world", 1e-2)):
            d = np.abs(c.read(k) - e[k]).max()
            worst[k] = max(worst.get(k, 0.0), d)
            assert d < tol, (t, k, d)
        assert np.isfinite(eff).all()
    print("free-running max deviations:", worst)
    c.close()


def test_safety_latch_and_abs_binding():
    """abs(float) in checkSafeOrientation is the float overload (qmpc_glue.hip): robot 1 rolled to 0.45 rad stays live,
    robot 2 rolled to 0.7 rad from tick 5 latches (int abs(int) would let it run), robot 4 rolled to 1.2 rad from tick 9
    latches; robot 3 with its front-right hip at 0.5 rad (> 0.174533) from tick 7 latches, and its clamped hip angle is
    what the joint PD reads.  A latched robot's effort is zero from that tick on."""
    import torch
    B, ticks = 6, 30
    c = make_ctrl(B)
    dev = c.device
    imu, motor = W.make_tick_stream(B, ticks, 3, roll=(1, 0.45, 0))
    for rb, val, t0 in ((2, 0.7, 5), (4, 1.2, 9)):
        imu_r, _ = W.make_tick_stream(B, ticks, 3, roll=(rb, val, t0))
        imu[:, rb] = imu_r[:, rb]
    motor[7:, 3, 1] = 0.5
    m = M.CtrlModel(B, 500.0, PID)
    for t in range(ticks):
        eff = c.tick(torch.from_numpy(imu[t]).to(dev), torch.from_numpy(motor[t]).to(dev)).cpu().numpy()
        e = gpu_est(c)
        e["leg_q"] = motor[t][:, :12].astype(np.float32)
        m.loco(e, pf_override=c.read("sw_pf"))
        if (t + 1) % 13 == 0:
            rec, wpd, xci = O.pack_commands(m.command(e), float(m.dt_mpc))
            m.wpd[:], m.xci[:] = wpd, xci
            m.f_ff[:] = c.read("f_ff")
        assert np.array_equal(eff, m.legcmd(e, m.f_ff)), t
        assert np.array_equal(c.read("safe")[:, 0], m.safe), t
        safe = c.read("safe")[:, 0]
        rpy = c.read("rpy")
        assert safe[1] == 1 and 0.4 < abs(rpy[1, 0]) < 0.5, (t, rpy[1])
        assert safe[2] == (1 if t < 5 else 0), t
        if t >= 5:
            assert 0.5 < abs(rpy[2, 0]) < 1.0, (t, rpy[2])
        assert safe[4] == (1 if t < 9 else 0), t
        assert safe[3] == (1 if t < 7 else 0), t
        assert safe[0] == 1 and safe[5] == 1
        for b in (2, 3, 4):
            if not safe[b]:
                assert (eff[b] == 0).all()
        if t >= 7:
            assert c.read("q")[3, 1] == np.float32(0.174533)
        assert np.abs(eff[[0, 1, 5]]).max() > 0
    c.close()


def test_view_tensors_alias_the_state():
    """view(): zero-copy device tensors at the pointers qmpc_ctrl_view_get returns, equal to the state they name,
    and still current after further ticks (no snapshot)."""
    import ctypes as C
    import torch
    from quadruped_ctrl_amd.binding import CTRL_VIEW_WIDTH, CtrlView
    B = 33
    c = make_ctrl(B)
    imu, motor = W.make_tick_stream(B, 20, 41)
    c.set_gait(torch.from_numpy(command_gaits(B, 0, 10 ** 9)).to(c.device))
    c.set_vel(torch.from_numpy(command_vel(B, 42)).to(c.device))
    for t in range(14):
        c.tick(torch.from_numpy(imu[t]).to(c.device), torch.from_numpy(motor[t]).to(c.device))
    v = c.view()
    raw = CtrlView()
    assert c.lib.qmpc_ctrl_view_get(c.mpc.h, C.byref(raw)) == 0
    names = dict(leg_q="q")
    for rnd in range(2):
        torch.cuda.synchronize()
        for k, n in CTRL_VIEW_WIDTH.items():
            assert v[k].is_cuda and tuple(v[k].shape) == (B, n), k
            assert v[k].data_ptr() == getattr(raw, k), k
            assert np.array_equal(v[k].cpu().numpy(), c.read(names.get(k, k)).reshape(B, n)), (rnd, k)
        assert v["batch"] == B and v["ticks"] == 14    # (an int taken when view() was called)
        if rnd == 0:   # one more tick: the same tensors now show its state
            c.tick(torch.from_numpy(imu[14]).to(c.device), torch.from_numpy(motor[14]).to(c.device))
    assert c.view()["ticks"] == 15 and (v["counter"] == 15).all()
    del v
    c.close()


def test_reset_leaves_other_robots_bit_identical():
    import torch
    B, ticks, at = 40, 33, 17
    a, b = make_ctrl(B), make_ctrl(B)
    imu, motor = W.make_tick_stream(B, ticks, 21)
    g = torch.from_numpy(command_gaits(B, 0, 10 ** 9)).to(a.device)
    v = torch.from_numpy(command_vel(B, 22)).to(a.device)
    for c in (a, b):
        c.set_gait(g)
        c.set_vel(v)
    mask = np.zeros(B, bool)
    mask[[3, 30]] = True
    for t in range(ticks):
        x, y = torch.from_numpy(imu[t]).to(a.device), torch.from_numpy(motor[t]).to(a.device)
        if t == at:
            a.reset(torch.from_numpy(mask).to(a.device))
            assert (a.read("counter")[mask, 0] == at % 13).all()
            assert (a.read("gait_num")[mask, 0] == 0).all()
            a.set_gait(g)
            a.set_vel(v)
        ea, eb = a.tick(x, y).cpu().numpy(), b.tick(x, y).cpu().numpy()
        assert np.array_equal(ea[~mask], eb[~mask]), t
    for k in ("f_ff", "p_des", "sw_p", "xhat", "counter", "wpd", "xci"):
        assert np.array_equal(a.read(k)[~mask], b.read(k)[~mask]), k
    # the reset robots run (their counters stay congruent to T mod 13: lockstep) and are not latched
    assert ((a.read("counter")[:, 0] - ticks) % 13 == 0).all()
    assert (a.read("safe") == 1).all()
    a.close()
    b.close()


def test_graph_capture_replay_matches_eager():
    """One captured 13-tick block replayed 3 times equals 39 eager ticks, bit for bit (single stream)."""
    import torch
    B = 300
    eager, cap = make_ctrl(B), make_ctrl(B)
    dev = eager.device
    n = 13 * 4
    imu, motor = W.make_tick_stream(B, n, 31)
    g = torch.from_numpy(command_gaits(B, 0, 10 ** 9)).to(dev)
    v = torch.from_numpy(command_vel(B, 32)).to(dev)
    for c in (eager, cap):
        c.set_gait(g)
        c.set_vel(v)
    # the first 13 ticks eager on both (first visit, first run, one MPC)
    for t in range(13):
        x, y = torch.from_numpy(imu[t]).to(dev), torch.from_numpy(motor[t]).to(dev)
        eager.tick(x, y)
        cap.tick(x, y)
    torch.cuda.synchronize()
    bi = torch.zeros((13, B, 10), dtype=torch.float64, device=dev)
    bm = torch.zeros((13, B, 24), dtype=torch.float64, device=dev)
    be = torch.zeros((13, B, 12), dtype=torch.float64, device=dev)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for k in range(13):
                cap.tick(bi[k], bm[k], be[k])
    torch.cuda.current_stream().wait_stream(s)
    # (capture advanced the handle's tick count by 13: a multiple of 13, so T mod 13 is what replays see too)
    for r in range(3):
        lo = 13 * (r + 1)
        bi.copy_(torch.from_numpy(imu[lo:lo + 13]))
        bm.copy_(torch.from_numpy(motor[lo:lo + 13]))
        graph.replay()
        torch.cuda.synchronize()
        for k in range(13):
            x, y = torch.from_numpy(imu[lo + k]).to(dev), torch.from_numpy(motor[lo + k]).to(dev)
            ee = eager.tick(x, y)
            torch.cuda.synchronize()
            assert torch.equal(ee, be[k]), (r, k)
    for k in ("f_ff", "p_des", "counter", "xhat", "wpd", "xci", "safe"):
        assert np.array_equal(eager.read(k), cap.read(k)), k
    eager.close()
    cap.close()


def test_controller_argument_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, QmpcError
    c = BatchedController(0, max_batch=8)
    lib, h = c.lib, c.mpc.h
    x = torch.zeros((8, 10), dtype=torch.float64, device=c.device)
    y = torch.zeros((8, 24), dtype=torch.float64, device=c.device)
    e = torch.zeros((8, 12), dtype=torch.float64, device=c.device)
    # before init
    assert lib.qmpc_ctrl_tick(h, 8, x.data_ptr(), y.data_ptr(), e.data_ptr(), None) == 3
    with pytest.raises(QmpcError):
        c.tick(x, y)
    import ctypes as C
    from quadruped_ctrl_amd.binding import CtrlView
    assert lib.qmpc_ctrl_view_get(h, C.byref(CtrlView())) == 3
    pid = (C.c_double * 4)(0, 0, 1, 0.1)
    assert lib.qmpc_ctrl_init(h, 9, 500.0, pid, None) == 1          # batch > max_batch
    assert lib.qmpc_ctrl_init(h, 8, 500.0, None, None) == 1         # null pid
    assert lib.qmpc_ctrl_init(h, 8, 0.0, pid, None) == 1            # freq
    assert lib.qmpc_ctrl_init(None, 8, 500.0, pid, None) == 1
    c.init(8, 500.0, (0, 0, 1, 0.1))
    assert lib.qmpc_ctrl_tick(h, 8, None, y.data_ptr(), e.data_ptr(), None) == 1
    assert lib.qmpc_ctrl_tick(h, 8, x.data_ptr(), None, e.data_ptr(), None) == 1
    assert lib.qmpc_ctrl_tick(h, 8, x.data_ptr(), y.data_ptr(), None, None) == 1
    assert lib.qmpc_ctrl_tick(h, 7, x.data_ptr(), y.data_ptr(), e.data_ptr(), None) == 1   # not the initialised batch
    assert lib.qmpc_ctrl_reset(h, 8, None, None) == 1
    assert lib.qmpc_ctrl_set_gait(h, 8, None, None) == 1
    assert lib.qmpc_ctrl_set_vel(h, 8, None, None) == 1
    assert lib.qmpc_ctrl_prework(h, 8, None, None, None) == 1
    with pytest.raises(QmpcError):
        c.tick(x[:, :9].contiguous(), y)
    v = CtrlView()
    assert lib.qmpc_ctrl_view_get(h, C.byref(v)) == 0 and v.batch == 8 and v.ticks == 0
    c.close()


def test_calm_stream_1024_robots_1300_ticks():
    """The README use: 1024 robots, 1300 ticks (100 MPC cycles) of the calm synthetic stream, mixed reference gaits:
    finite efforts, no latch."""
    import torch
    from quadruped_ctrl_amd.binding import BatchedController
    B = 1024
    ctrl = BatchedController(0, max_batch=B)
    ctrl.init(B, freq=500.0, pid=PID)
    ctrl.set_gait(torch.from_numpy(command_gaits(B, 0, 10 ** 9)).cuda())
    ctrl.set_vel(torch.from_numpy(command_vel(B, 7)).cuda())
    imu, motor = W.make_tick_stream(B, 1300, 7)
    imu, motor = torch.from_numpy(imu).cuda(), torch.from_numpy(motor).cuda()
    for t in range(1300):
        eff = ctrl.tick(imu[t], motor[t])
    torch.cuda.synchronize()
    v = ctrl.view()
    assert torch.isfinite(eff).all() and v["ticks"] == 1300
    assert (v["safe"] == 1).all() and (v["counter"] == 1300).all()
    assert torch.isfinite(v["f_ff"]).all() and v["f_ff"].abs().max().item() > 1.0
    del v
    ctrl.close()
