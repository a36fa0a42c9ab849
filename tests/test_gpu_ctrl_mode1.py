"""GPU suite (-m gpu) for robot mode 1 of the batched locomotion controller (qmpc_ctrl_set_robot_mode): the `aio` gait
of ConvexMPCLocomotion.cpp:173-233 against the restatement in tests/ctrl_model_mode1.py and the oracle pipeline.

Model parity is teacher-forced exactly as tests/test_gpu_controller.py does it for mode 0, with the same rule per
quantity (ctrl_gpu's EXACT_I32 / EXACT_F32 lists bit for bit, the landing point within its LAND_ULPS, the effort bit for bit),
plus the mode's own state: nseg, the phase, due.  Every robot is compared on every tick, latched ones included.
Forces: on every tick the due robots' records are rebuilt from the restatement -- horizon 10, rows 0 .. 9 of the robot's
n-row table -- solved with the oracle pipeline and compared under the suite's per-robot bound (solve_gpu.bound_for)
max(1e-4, 1.5 x the reference's float-order spread of that robot).  No allow-list.
The other tests compare two runs of the library bit for bit (ctrl_gpu's run_ticks / same_ticks).
"""
import numpy as np
import pytest

from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W

import ctrl_model as M
import ctrl_model_mode1 as M1
from ctrl_gpu import EXACT_F32, EXACT_I32, LAND_ULPS, PID, STATE, converged, gpu_est, make_ctrl, run_ticks, same_ticks
from ctrl_model import command_vel
from ctrl_model_mode1 import NSEGS, sweep_vel
from solve_gpu import bound_for

pytestmark = pytest.mark.gpu

MODE1_STATE = ("nseg", "gait_phase", "due", "grf", "status")


def _gaits1(B):
    """The caller's gait number in mode 1 keeps the omni flag and the :137 test: trot, omni trot, standing, omni standing."""
    return np.array([9, 29, 4, 24, 0, 30], np.int32)[np.arange(B) % 6]


def test_model_parity_and_forces():
    """256 robots, 1500 ticks: velocity commands over all six cases (ctrl_model_mode1.sweep_vel), changed at ticks
    500 and 1000; omni robots; robot 5 rolls over at tick 700 and latches (compared like the others: zero effort).

    The reference's qpOASES call stops after 100 working-set recalculations (SolverMPC.cpp:527-541) and then returns an
    iterate that is not the minimiser; tests/test_gpu_parity.py drops such robots from its comparison (`capped`).  Here
    nobody is dropped: a solve on which the oracle pipeline reports nWSR >= 100 is compared, under the same bound, with
    the same pipeline run to convergence (ctrl_gpu.converged: the oracle's float assembly and swing elimination, qpOASES
    with nWSR 5000).  Measured on an MI355X: 2 of the run's 29433 solves are such -- the rolled-over robot 5 in the
    16-segment walk at ticks 1356 and 1369, which need 105 and 111 recalculations; the capped iterate is 1.4e-2 away from
    the minimiser there, the library 1e-6."""
    import torch
    B, ticks, seg = 256, 1500, 500
    c = make_ctrl(B, schedule="per_robot", mode=1)
    m = M1.CtrlModelMode1(B, 500.0, PID)
    dev = c.device
    imu, motor = W.make_tick_stream(B, ticks, 91, roll=(5, 0.7, 700))
    g = _gaits1(B)
    c.set_gait(torch.from_numpy(g).to(dev))
    m.set_gait(g)
    assert (c.read("nseg") == 14).all() and (c.read("gait_phase") == 0).all()      # the aio constructor, _phase = 0
    seen, restarts, n_solves, worst = set(), np.zeros(B, int), 0, 0.0
    over_total, n_capped, violations = 0, 0, []   # violations: (tick, robot, error, bound), asserted empty after the run
    for t in range(ticks):
        if t % seg == 0:
            vel = sweep_vel(B, t // seg)
            c.set_vel(torch.from_numpy(vel).to(dev))
            m.set_vel(vel)
        before = m.counter.copy()
        eff = c.tick(torch.from_numpy(imu[t]).to(dev), torch.from_numpy(motor[t]).to(dev)).cpu().numpy()
        e = gpu_est(c)
        e["leg_q"] = motor[t][:, :12].astype(np.float32)
        gpu_pf = c.read("sw_pf")
        out = m.loco(e, pf_override=gpu_pf)
        scale = np.maximum(1.0, np.abs(out["pf"]))
        land = np.abs(gpu_pf - out["pf"]) / (np.finfo(np.float32).eps * scale)
        assert land.max() <= LAND_ULPS, (t, land.max())
        zero_yr = m.vel_des[:, 2] == 0
        assert np.array_equal(gpu_pf[zero_yr], out["pf"][zero_yr]), t
        for k in EXACT_I32 + ("nseg",):
            assert np.array_equal(c.read(k).reshape(getattr(m, k).shape), getattr(m, k)), (t, k)
        assert np.array_equal(c.read("due")[:, 0] != 0, m.due), t
        for k in EXACT_F32 + ("gait_phase",):
            g_ = c.read(k).reshape(getattr(m, k).shape)
            assert np.array_equal(g_, getattr(m, k)), (t, k, np.abs(g_ - getattr(m, k)).max())
        due = np.flatnonzero(m.due)
        # every solve: horizon 10, never on a phase-0 tick, never the stand trajectory
        assert (m.horizon[due] == 10).all() and not m.phase0[due].any() and (m.current_gait[due] == 9).all(), t
        f_gpu = c.read("f_ff")
        if len(due):
            n_solves += len(due)
            cmd, tables = m.command_mode1(e, due)
            # what the library handed its solve: a 10-segment gait with the same ten rows
            mo, md, it = c.read("mpc_offsets"), c.read("mpc_durations"), c.read("iteration")[:, 0]
            for k, b in enumerate(due):
                assert np.array_equal(M.mpc_table(mo[b], md[b], int(it[b]), n=10), tables[k]), (t, b)
            rec, wpd, xci = O.pack_commands(cmd, float(m.dt_mpc))
            rec["gait"] = tables
            m.wpd[due], m.xci[due] = wpd, xci
            rec.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)
            soln, nwsr, rc = O.solve_batch(rec)
            assert (rc == 0).all(), t
            for k in np.flatnonzero(nwsr >= 100):
                soln[k] = converged(rec, int(k))
                n_capped += 1
                print(f"tick {t} robot {due[k]}: the reference stopped at its nWSR cap; compared with the converged solve")
            f_ref = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(np.float32))
            err = np.abs(f_gpu[due].astype(np.float64) - f_ref).max(1) / np.maximum(np.abs(f_ref).max(1), 1.0)
            worst = max(worst, float(err.max()))
            if (err >= 1e-4).any():
                over_total += int((err >= 1e-4).sum())
                bnd = bound_for(rec, err=err)
                st = c.read("status")[due, 0]
                for k in np.flatnonzero(err >= 1e-4):
                    print(f"tick {t} robot {due[k]}: f_ff error {err[k]:.3e}, bound {bnd[k]:.3e}, status {st[k]}, "
                          f"nseg {m.nseg[due[k]]}, safe {m.safe[due[k]]}, rpy {e['rpy'][due[k]]}")
                violations += [(t, int(due[k]), float(err[k]), float(bnd[k])) for k in np.flatnonzero(err > bnd)]
            assert (c.read("status")[due, 0] & 47 == 0).all(), t
            m.f_ff[due] = f_gpu[due]
        idle = ~m.due
        assert np.array_equal(f_gpu[idle], m.f_ff[idle]), t              # nobody else's forces moved
        for k in ("wpd", "xci"):
            assert np.array_equal(c.read(k).reshape(getattr(m, k).shape), getattr(m, k)), (t, k)
        eff_m = m.legcmd(e, m.f_ff)
        assert np.array_equal(eff, eff_m), (t, np.abs(eff - eff_m).max())
        if t >= 700:
            assert m.safe[5] == 0 and (eff[5] == 0).all(), t
        seen |= set(int(x) for x in m.nseg)
        restarts += m.restarted & (before > 0)
    print(f"mode 1 parity: {n_solves} solves, worst relative f_ff error {worst:.3e}, {over_total} over the flat 1e-4, "
          f"{n_capped} compared with the converged reference")
    assert seen == NSEGS
    assert (restarts >= 1).all()
    assert n_solves > B * (ticks // 13 - 12)
    assert (np.delete(m.safe, 5) == 1).all() and np.isfinite(eff).all()
    c.close()
    assert not violations, violations


def _apply1(c, B, vel):
    import torch
    c.set_gait(torch.from_numpy(_gaits1(B)).to(c.device))
    c.set_vel(torch.from_numpy(vel).to(c.device))


def _run1(c, B, imu, motor, t0, ticks, resets=None, vel_at=None):
    """Ticks t0 .. t0 + ticks - 1 on a mode-1 controller -> (effort, per-tick snapshots).  vel_at: {tick: vel}; a reset
    zeroes gait and velocity command, so both are applied again after it."""
    import torch
    dev = c.device
    eff, snaps, vel = [], [], None
    for t in range(t0, t0 + ticks):
        if resets and t in resets:
            c.reset(torch.from_numpy(resets[t]).to(dev))
        cur = max(k for k in vel_at if k <= t)
        if t == t0 or t in vel_at or (resets and t in resets):
            _apply1(c, B, vel_at[cur])
        eff.append(c.tick(torch.from_numpy(imu[t]).to(dev), torch.from_numpy(motor[t]).to(dev)).cpu().numpy())
        snaps.append({k: c.read(k) for k in STATE + MODE1_STATE})
    return np.array(eff), snaps


def _same1(a, b, rows, what, a_off=0, b_off=0, ticks=None):
    same_ticks(a[0], a[1], b[0], b[1], rows, what, a_off=a_off, b_off=b_off, ticks=ticks)
    n = ticks if ticks is not None else min(len(a[0]) - a_off, len(b[0]) - b_off)
    for i in range(n):
        for k in MODE1_STATE + ("counter",):
            assert np.array_equal(a[1][a_off + i][k][rows], b[1][b_off + i][k][rows]), (what, i, k)


def test_mode0_untouched():
    """set_robot_mode(0) called explicitly: a per-robot-schedule run is bit-identical to the same run without the call
    (test_gpu_ctrl_schedule.py's mixed gaits and velocities)."""
    B, ticks = 257, 40
    imu, motor = W.make_tick_stream(B, ticks, 51)
    vel = command_vel(B, 52)
    out = []
    for mode in (None, 0):
        c = make_ctrl(B, schedule="per_robot", mode=mode)
        out.append(run_ticks(c, B, imu, motor, vel, 0, ticks, extra=("due", "grf", "status", "nseg")))
        assert c.mpc.horizon == 14
        c.close()
    same_ticks(*out[0], *out[1], np.ones(B, bool), "explicit mode 0 vs default")
    for a, b in zip(out[0][1], out[1][1]):
        for k in ("counter", "due", "grf", "status", "nseg"):
            assert np.array_equal(a[k], b[k]), k
    assert np.abs(out[0][1][-1]["f_ff"]).max() > 1.0


def test_reset_mid_run():
    """Every third robot reset before tick 230 (after restarts and solves): from then on it is the robot of a controller
    freshly initialised in mode 1 at that moment; the others are those of the run without the reset."""
    B, at, ticks = 96, 230, 60
    n = at + ticks
    imu, motor = W.make_tick_stream(B, n, 93)
    vel_at = {0: sweep_vel(B, 0), 120: sweep_vel(B, 1)}
    mask = np.arange(B) % 3 == 0
    c = make_ctrl(B, schedule="per_robot", mode=1)
    r = _run1(c, B, imu, motor, 0, n, resets={at: mask}, vel_at=vel_at)
    c.close()
    c = make_ctrl(B, schedule="per_robot", mode=1)
    p = _run1(c, B, imu, motor, 0, n, vel_at=vel_at)
    c.close()
    c = make_ctrl(B, schedule="per_robot", mode=1)
    f = _run1(c, B, imu, motor, at, ticks, vel_at={at: vel_at[120]})
    c.close()
    _same1(r, f, mask, "reset robots vs fresh mode-1 controller", a_off=at, ticks=ticks)
    _same1(r, p, ~mask, "other robots vs no reset")
    assert (r[1][at]["counter"][mask, 0] == 1).all()
    assert len(np.unique(r[1][-1]["nseg"])) >= 3 and (r[1][-1]["safe"] == 1).all()
    assert np.abs(r[1][-1]["f_ff"][mask]).max() > 1.0              # the reset robots have solved again


def test_graph_of_five_ticks_across_a_restart():
    """A captured graph of 5 mode-1 ticks, replayed 12 times, equals 60 eager ticks bit for bit; the velocity command
    changes before the capture, so counters restart inside the replayed window."""
    import torch
    B, K, R, pre = 150, 5, 12, 215
    n = pre + K * R
    imu, motor = W.make_tick_stream(B, n, 95)
    eager, cap = make_ctrl(B, schedule="per_robot", mode=1), make_ctrl(B, schedule="per_robot", mode=1)
    dev = eager.device
    for t in range(pre):
        x, y = torch.from_numpy(imu[t]).to(dev), torch.from_numpy(motor[t]).to(dev)
        for c in (eager, cap):
            if t in (0, 150):
                _apply1(c, B, sweep_vel(B, 0 if t == 0 else 1))
            c.tick(x, y)
    torch.cuda.synchronize()
    bi = torch.zeros((K, B, 10), dtype=torch.float64, device=dev)
    bm = torch.zeros((K, B, 24), dtype=torch.float64, device=dev)
    be = torch.zeros((K, B, 12), dtype=torch.float64, device=dev)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for k in range(K):
                cap.tick(bi[k], bm[k], be[k])
    torch.cuda.current_stream().wait_stream(s)
    restarts = solved = 0
    for r in range(R):
        lo = pre + K * r
        bi.copy_(torch.from_numpy(imu[lo:lo + K]))
        bm.copy_(torch.from_numpy(motor[lo:lo + K]))
        graph.replay()
        torch.cuda.synchronize()
        for k in range(K):
            x, y = torch.from_numpy(imu[lo + k]).to(dev), torch.from_numpy(motor[lo + k]).to(dev)
            before = eager.read("counter")[:, 0]
            ee = eager.tick(x, y)
            torch.cuda.synchronize()
            assert torch.equal(ee, be[k]), (r, k)
            restarts += int(((eager.read("counter")[:, 0] == 1) & (before > 1)).sum())
            solved += int(eager.read("due").sum())
    assert restarts > 0 and solved > B
    for k in STATE + MODE1_STATE + ("xhat", "offsets", "durations", "mpc_offsets", "mpc_durations"):
        assert np.array_equal(eager.read(k), cap.read(k)), k
    assert (eager.read("safe") == 1).all()
    eager.close()
    cap.close()


def test_set_robot_mode_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, QmpcError
    B = 8
    c = BatchedController(0, max_batch=B)
    lib, h = c.lib, c.mpc.h
    assert lib.qmpc_ctrl_set_robot_mode(h, 1) == 3              # before init: QMPC_ERR_STATE
    c.init(B, 500.0, PID)
    assert lib.qmpc_ctrl_set_robot_mode(h, 1) == 3              # lockstep: QMPC_ERR_STATE, and the message says why
    assert b"lockstep" in lib.qmpc_last_error(h)
    with pytest.raises(QmpcError):
        c.set_robot_mode(1)
    assert lib.qmpc_ctrl_set_robot_mode(h, 0) == 0              # mode 0 runs under either schedule
    c.set_schedule("per_robot")
    assert lib.qmpc_ctrl_set_robot_mode(h, 2) == 1              # QMPC_ERR_ARG
    assert lib.qmpc_ctrl_set_robot_mode(h, -1) == 1
    x = torch.zeros((B, 10), dtype=torch.float64, device=c.device)
    x[:, 6] = 1.0
    y = torch.zeros((B, 24), dtype=torch.float64, device=c.device)
    c.prework(x, y)                                             # pre_work may come first, as in the reference's protocol
    c.set_robot_mode(1)
    assert c.mpc.horizon == 10
    assert lib.qmpc_ctrl_set_schedule(h, 0) == 3                # lockstep is refused while mode 1 is selected
    c.set_robot_mode(0)
    c.set_robot_mode(1)
    c.tick(x, y)
    assert (c.read("nseg") == 10).all() and (c.read("current_gait") == 4).all()   # command 0: the standing case
    assert lib.qmpc_ctrl_set_robot_mode(h, 0) == 3              # after the first tick: QMPC_ERR_STATE
    assert lib.qmpc_ctrl_set_robot_mode(h, 1) == 3
    c.init(B, 500.0, PID)                                       # init returns to mode 0 (and lockstep)
    assert c.mpc.horizon == 14
    c.tick(x, y)
    assert (c.read("nseg") == 14).all() and (c.read("durations") == 7).all()      # gait number 0: the 14-segment trot
    c.init(B, 500.0, PID)
    c.set_schedule("per_robot")
    m = torch.zeros(B, dtype=torch.bool, device=c.device)
    c.reset(m)
    assert lib.qmpc_ctrl_set_robot_mode(h, 1) == 3              # after a reset: QMPC_ERR_STATE
    c.close()
