"""CPU suite: the parametrised references of tests/test_gpu_constants.py, pinned at the second constants without a GPU,
and the conditions its streams and poses have to meet there.

  * oracle/kron_model.assemble (mass, ibody, gravity, dt, the closed form the kernel shares) against a brute-force fp64
    condensation written from the reference's ct_ss_mats -> c2qp -> qH, qg (SolverMPC.cpp:64-125, 226-267, 296-399);
  * oracle.glue's forward and inverse kinematics at the second geometry against tests/ctrl_model.py's fp64 FK (fk64);
  * tests/plant_model.py's closed forms (tests/test_plant_cpu.py) with the second body, geometry, frequency and friction;
  * tests/ctrl_model.py at 400 Hz and 1000 Hz: no latch, stance / swing edges, the swing time.
"""
import numpy as np
import pytest

from oracle import glue as G
from oracle import kron_model as K
from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W

import ctrl_model as M
import plant_cases as PC
import plant_model as PM
from ctrl_model import fk64
from second_robot import F_MAX2, GEOM2_F, GRAVITY2, IBODY2, MASS2, PLANT2, SOLVE2


PID = (0.0, 0.0, 3.0, 0.3)


# ---- the condensation ------------------------------------------------------------------------------------------------

def brute_force(b, i):
    """(H, g) of robot i, fp64: continuous-time matrices, their exact discretisation, the stacked prediction matrices
    and the dense products.  The 25 x 25 augmented matrix [[A, B], [0, 0]] dt is nilpotent of index 4 (A^3 = 0), so its
    exponential is its Taylor series to third order."""
    h = b["horizon"]
    dt = np.float64(np.float32(b["dt"]))                      # problem_setup stores a float
    mass = np.float64(b.get("mass", 9.0))
    ib = np.asarray(b["ibody"], np.float64) if "ibody" in b else np.array([.07, .26, .242], np.float32).astype(np.float64)
    grav = np.float64(b["gravity"]) if "gravity" in b else np.float64(np.float32(-9.8))
    yaw = np.float64(b["yaw"][i])
    c, s = np.cos(yaw), np.sin(yaw)
    Ryaw = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    I_inv = np.linalg.inv(Ryaw @ np.diag(ib) @ Ryaw.T)
    A = np.zeros((13, 13))
    A[3, 9] = A[4, 10] = A[5, 11] = 1.0
    A[11, 9] = np.float64(b["x_drag"][i])
    A[11, 12] = 1.0
    A[0:3, 6:9] = Ryaw.T
    Bc = np.zeros((13, 12))
    r = np.asarray(b["r"][i], np.float64).reshape(3, 4)
    for f in range(4):
        x, y, z = r[:, f]
        Bc[6:9, 3 * f:3 * f + 3] = I_inv @ np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        Bc[9:12, 3 * f:3 * f + 3] = np.eye(3) / mass
    Mx = np.zeros((25, 25))
    Mx[:13, :13], Mx[:13, 13:] = A * dt, Bc * dt
    E = np.eye(25) + Mx + Mx @ Mx / 2 + Mx @ Mx @ Mx / 6
    assert not (Mx @ Mx @ Mx @ Mx).any()
    Adt, Bdt = E[:13, :13], E[:13, 13:]
    pw = [np.eye(13)]
    for _ in range(h):
        pw.append(Adt @ pw[-1])
    A_qp = np.vstack(pw[1:])
    B_qp = np.zeros((13 * h, 12 * h))
    for a in range(h):
        for c_ in range(a + 1):
            B_qp[13 * a:13 * a + 13, 12 * c_:12 * c_ + 12] = pw[a - c_] @ Bdt
    w13 = np.concatenate([b["weights"][i].astype(np.float64), [0.0]])
    S = np.diag(np.tile(w13, h))
    x0 = np.concatenate([K.quat_to_rpy(b["q"][i]), b["p"][i], b["w"][i], b["v"][i], [grav]]).astype(np.float64)
    xd = np.concatenate([b["traj"][i].astype(np.float64).reshape(h, 12), np.zeros((h, 1))], 1).reshape(-1)
    H = 2 * (B_qp.T @ S @ B_qp + np.float64(b["alpha"][i]) * np.eye(12 * h))
    g = 2 * B_qp.T @ S @ (A_qp @ x0 - xd)
    return H, g


def _agree(b, robots):
    for i in robots:
        H, g = K.assemble(b, i)
        Hb, gb = brute_force(b, i)
        eh, eg = np.abs(H - Hb).max() / np.abs(Hb).max(), np.abs(g - gb).max() / np.abs(gb).max()
        assert eh < 1e-12 and eg < 1e-12, (i, eh, eg)


def _drag(b):
    rng = np.random.default_rng(11)
    b["x_drag"] = rng.normal(0, 0.7, b["batch"]).astype(np.float32)
    return b


BATCHES = [lambda: W.make_config(2, batch=16), lambda: _drag(W.make_config(4, batch=16)), lambda: _drag(W.make_trot(8, 16))]


@pytest.mark.parametrize("mk", BATCHES, ids=["config2", "config4-drag", "trot16-drag"])
def test_fp64_model_is_the_brute_force_condensation(mk):
    b = mk()
    robots = range(0, b["batch"], b["batch"] // 4)
    _agree(b, robots)
    for dt, mu in SOLVE2:
        _agree(dict(b, dt=dt, mu=mu, f_max=F_MAX2, mass=MASS2, ibody=IBODY2, gravity=GRAVITY2), robots)
    # and the parameters arrive: the second body's H and g are not the first's
    H1, g1 = K.assemble(b, 0)
    H2, g2 = K.assemble(dict(b, mass=MASS2, ibody=IBODY2, gravity=GRAVITY2), 0)
    assert np.abs(H2 - H1).max() > 1e-3 * np.abs(H1).max() and np.abs(g2 - g1).max() > 1e-3 * np.abs(g1).max()
    H3, g3 = K.assemble(dict(b, gravity=GRAVITY2), 0)
    assert np.array_equal(H3, H1) and np.abs(g3 - g1).max() > 1e-6 * np.abs(g1).max()


def test_constraint_rows_take_mu_and_f_max_from_the_batch():
    """oracle.assemble / oracle.reduce build the friction and force rows from b["mu"], b["f_max"]: the solver checks of
    the GPU file rely on it."""
    b = W.make_config(2, batch=4)
    for mu, fm in ((SOLVE2[0][1], F_MAX2), (SOLVE2[1][1], F_MAX2)):
        H, g, A, lb, ub, _ = O.assemble(dict(b, mu=mu, f_max=fm), 0)
        _, _, _, Ar, lr, ur = O.reduce(H, g, A, lb, ub)
        vals = np.unique(np.abs(Ar[Ar != 0]))
        assert np.float64(np.float32(1.0) / np.float32(mu)) in vals or np.float64(np.float32(mu)) in vals, vals
        assert ur[np.isfinite(ur) & (ur < 1e4)].max() == np.float64(np.float32(fm))


# ---- kinematics ------------------------------------------------------------------------------------------------------

def test_fk_and_ik_at_the_second_geometry():
    """tests/test_glue_cpu.py's two checks with GEOM2, at its tolerances."""
    s = W.make_leg_states(64)
    g64 = GEOM2_F.astype(np.float64)
    J, p, v = G.leg_update(s["q"], s["qd"], GEOM2_F)
    for b in range(0, 64, 7):
        for leg in range(4):
            q = s["q"][b, 3 * leg:3 * leg + 3].astype(np.float64)
            assert np.abs(p[b, 3 * leg:3 * leg + 3] - fk64(q, leg, g64)).max() < 2e-6
            Jn = np.zeros((3, 3))
            for k in range(3):
                e = np.zeros(3)
                e[k] = 1e-6
                Jn[:, k] = (fk64(q + e, leg, g64) - fk64(q - e, leg, g64)) / 2e-6
            assert np.abs(J[b, leg].reshape(3, 3) - Jn).max() < 2e-5
            assert np.abs(p[b, 3 * leg:3 * leg + 3] - fk64(q, leg)).max() > 1e-3      # not the default's
    tau, qdes = G.leg_command(dict(s, J=J, p=p, v=v, p_des=p), GEOM2_F)
    _, p2, _ = G.leg_update(qdes, s["qd"], GEOM2_F)
    mirror = p.reshape(64, 4, 3) * np.array([-1.0, 1.0, 1.0], np.float32)
    assert np.abs(p2.reshape(64, 4, 3) - mirror).max() < 2e-5
    assert (qdes.reshape(64, 4, 3)[:, :, 2] <= 0).all()
    _, qdes1 = G.leg_command(dict(s, J=J, p=p, v=v, p_des=p))
    assert np.abs(qdes - qdes1).max() > 1e-2


# ---- the plant's closed forms ----------------------------------------------------------------------------------------

def test_plant_closed_forms_at_the_second_constants():
    """tests/test_plant_cpu.py's closed forms -- free fall, torque-free spin, hover under J^-T, the friction cone, pulling
    and straight legs -- as tests/plant_cases.py states them, with mass 12.5, inertia (0.11, 0.36, 0.41), the second
    geometry, 400 Hz and mu 0.6."""
    PC.free_fall(PLANT2)
    PC.spin(PLANT2)
    pl = PC.hover(PLANT2)
    PC.friction_and_straight_knee(PLANT2)
    # the hover's torques are this geometry's: the default robot's Jacobian at the same feet is another
    R = PM.rot(pl.q)
    r = PM.mulT(R[:, None, :], pl.foot - pl.p[:, None, :]) - PM.HIP
    J1, _ = PM.leg_fk(PM.leg_ik(r))
    J2, _ = PM.leg_fk(PM.leg_ik(r, geom=pl.geom), geom=pl.geom)
    assert np.abs(J1 - J2).max() > 1e-2
    # one step of a general spin follows Euler's equations of THIS inertia: wdot = I^-1 (-(w x I w))
    pl = PC.model(1, PLANT2)
    pl.w[:] = [[1.0, 2.0, -1.5]]
    w = pl.w[0].copy()
    pl.step(np.zeros((1, 12)), *PC.none(1))
    I = np.array(IBODY2)
    assert np.abs(pl.w[0] - (w + (1 / 400.0) * (-np.cross(w, I * w) / I))).max() < 1e-15


def test_plant_parity_case_holds_its_conditions_at_the_second_constants():
    """The case of tests/test_gpu_plant.py::_single_step (tests/plant_cases.py) built for PLANT2 meets that test's own
    conditions on the model alone: the singular robot 256, the cone, the clamp -- and the stand pose is inside the controller's joint limits."""
    for sub in (1, 4):
        B, m, old, new, tau, cs, pd, vd = PC.parity_case(sub, PLANT2)           # (asserts the determinants itself)
        m.step(tau.reshape(B, 12), cs, pd, vd)
        g = m.grf
        on_cone = np.abs(np.hypot(g[..., 0], g[..., 1]) - m.mu * g[..., 2]) < 1e-12
        assert (on_cone & (g[..., 2] > 1)).sum() > 20 and (g[0][new[0]] == 0).all()
        assert sub > 1 or (g[256] == 0).all()
        assert abs(m.motor[5, 2] - PM.KNEE_MIN) < 1e-9 or new[5, 0]
    pl = PC.model(4, PLANT2)
    a = pl.motor[:, :12].reshape(4, 4, 3)
    assert (np.abs(a[..., 0]) < 1.0472).all() and (a[..., 1] > -1.8).all() and (a[..., 1] < 0.174533).all()
    assert (a[..., 2] > -0.174533).all() and (a[..., 2] < 2.79253).all()


# ---- the controller's streams ----------------------------------------------------------------------------------------

def _cpu_run(freq, geom, ticks=40, B=257, switch_at=20):
    m = M.CtrlModel(B, freq, PID, geom=geom)
    imu, motor = W.make_tick_stream(B, ticks, B, dt=1.0 / freq)
    m.set_vel(M.command_vel(B, B + 1))
    sw_hist, gaits, st = [], [], None
    for t in range(ticks):
        if t in (0, switch_at):
            m.set_gait(M.command_gaits(B, t, switch_at))
        e = m.estimate(imu[t], motor[t])
        m.loco(e)
        sw_hist.append(m.swing_state > 0)
        gaits.append(M.split_gait(m.gait_num)[0].copy())
        st = m.swing_time.copy()
    return m, np.array(sw_hist), np.array(gaits), st


@pytest.mark.parametrize("freq,geom", [(400.0, GEOM2_F), (1000.0, G.GEOM)], ids=["400Hz-geom2", "1000Hz"])
def test_controller_streams_meet_their_conditions(freq, geom):
    """What the 40-tick runs of the GPU file rely on, on the restatement alone (its own estimator): nobody latches; a
    swing -> stance edge occurs under every gait number, a stance -> swing edge under every gait number whose feet lift
    inside the window; and the swing time is 13 (14 - duration) / freq, more than 10 % off the 500 Hz value.

    The window: the gait clock counts ticks, not seconds (phase = counter / 182 at any frequency), so 40 ticks reach
    phase 0.22 of every gait.  Pronking (2), trotRunning (5), walking (10) and walking2 (11) are entered at the switch
    of tick 20 with all their feet in stance until phase 0.43 at the earliest, and standing (4) never lifts a foot:
    those five see touch-downs only (the switch puts swinging feet down).  Lift-offs are covered by the other seven."""
    m, sw, gaits, st = _cpu_run(freq, geom)
    assert (m.safe == 1).all()
    down = sw[:-1] & ~sw[1:]
    up = ~sw[:-1] & sw[1:]
    lifts = set()
    for gn in sorted(set(int(x) for x in gaits.reshape(-1))):
        on = (gaits[1:] == gn)[..., None]
        assert (down & on).any(), gn
        if (up & on).any():
            lifts.add(gn)
    assert lifts >= {0, 1, 3, 6, 7, 8, 9}, lifts
    ref = np.float32(0.026) * (14 - m.durations).astype(np.float32)
    moving = ref > 0
    assert np.array_equal(st, np.float32(1.0 / freq) * np.float32(13) * (14 - m.durations).astype(np.float32))
    assert (np.abs(st[moving] / ref[moving] - 1) > 0.1).all() and moving.any()
    if freq == 400.0:
        # 1 / 400 is no float, and qmpc_ctrl_init's order 13 float(1 / freq) still lands on float(0.0325)
        assert float(np.float32(1.0 / freq)) != 1.0 / freq and m.dt_mpc == np.float32(1.0 / freq) * np.float32(13) == np.float32(0.0325)
