"""GPU suite (-m gpu) for the reduced-order plant (include/qmpc_plant.h; BatchedPlant, rollout).

The kernel is compared with tests/plant_model.py (numpy float64, the same expressions in the same order) at 1e-10
relative to max(1, |x|) per output: about six orders above fp64 rounding of the chain, the device's atan2 / sin / cos /
sqrt included, far below any modelling difference.  The closed-loop walk is held to the CPU loop's recorded statistics
(tests/golden/plant_closed_loop_cpu.json) by plant_loop.envelope(); everything else compares two runs of the library
bit for bit.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from quadruped_ctrl_amd import workloads as W

import plant_loop as L
import plant_model as PM
from plant_cases import DEFAULTS, parity_case as _parity_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
f32 = np.float32
PLANT_KEYS = ("p", "v", "q", "omega", "foot", "grf", "stance", "state", "motor")
assert DEFAULTS["freq"] == L.FREQ


def _pair(B, schedule="lockstep", mode=None, substeps=1, xyyaw=None, max_batch=None, consts=None):
    """consts: a dict like DEFAULTS; its body goes to qmpc_set_robot (gravity -9.81, which the plant does not read) and
    its geometry to qmpc_set_leg_geometry, None leaves the handle as created."""
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant
    k = consts or DEFAULTS
    c = BatchedController(0, max_batch=max_batch or B)
    c.init(B, k["freq"], L.PID)
    if consts is not None:
        c.mpc.set_robot(float(k["mass"]), [float(x) for x in k["ibody"]], -9.81)
        c.mpc.set_leg_geometry(*[float(x) for x in k["geom"]])
    if schedule != "lockstep":
        c.set_schedule(schedule)
    if mode is not None:
        c.set_robot_mode(mode)
    p = BatchedPlant(c)
    p.init(k["mu"], substeps, None if xyyaw is None else torch.from_numpy(np.ascontiguousarray(xyyaw, np.float64)).to(c.device))
    return c, p


def _dev(c, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(c.device)


def _snap(plant):
    import torch
    torch.cuda.synchronize()
    v = plant.view()
    return {k: v[k].cpu().numpy().copy() for k in PLANT_KEYS}


def _close(got, want, what):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: worst error relative to max(1, |x|) {err.max():.3e}")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def _compare(snap, model, what):
    for k, mk in (("state", "state"), ("motor", "motor"), ("p", "p"), ("v", "v"), ("q", "q"), ("omega", "w"),
                  ("foot", "foot"), ("grf", "grf")):
        _close(snap[k], getattr(model, mk), f"{what} {k}")
    assert np.array_equal(snap["stance"] != 0, model.stance), what


@pytest.mark.parametrize("substeps", [1, 4])
def test_single_step_parity(substeps):
    """B = 257 (the last block is partial, 1028 lanes are no multiple of 64): random poses and joint states, every old
    and new stance pattern (both edges, all-swing, all-stance), a saturated cone, pulling legs, a near-straight knee, a
    swing command out of reach and a zero one."""
    _single_step(substeps)


def _start(c, plant, m, cs, pd, vd):
    """The model's state and the controller outputs the plant reads, put on the device: the views alias the state."""
    B = m.B
    pv, cv = plant.view(), c.view()
    for key, val in (("p", m.p), ("v", m.v), ("q", m.q), ("omega", m.w), ("foot", m.foot.reshape(B, 12))):
        pv[key].copy_(_dev(c, val))
    pv["stance"].copy_(_dev(c, m.stance.astype(np.int32)))
    cv["contact_state"].copy_(_dev(c, cs))
    cv["p_des"].copy_(_dev(c, pd.reshape(B, 12)))
    cv["v_des"].copy_(_dev(c, vd.reshape(B, 12)))


def _single_step(substeps, consts=None):
    """The body of test_single_step_parity; consts: see _pair."""
    B, m, old, new, tau, cs, pd, vd = _parity_case(substeps, consts or DEFAULTS)
    c, plant = _pair(B, substeps=substeps, consts=consts)
    _start(c, plant, m, cs, pd, vd)
    state, motor = plant.step(_dev(c, tau.reshape(B, 12)))
    want_state, want_motor = m.step(tau.reshape(B, 12), cs, pd, vd)
    s = _snap(plant)
    s["foot"], s["grf"] = s["foot"].reshape(B, 4, 3), s["grf"].reshape(B, 4, 3)
    _compare(s, m, f"substeps {substeps}")
    assert np.array_equal(state.cpu().numpy(), s["state"]) and np.array_equal(motor.cpu().numpy(), s["motor"])
    # the cases are there: both edges, zero and saturated forces, the clamp
    assert (new & ~old).any() and (old & ~new).any() and (~new).all(1).any() and new.all(1).any()
    g = m.grf
    on_cone = np.abs(np.hypot(g[..., 0], g[..., 1]) - m.mu * g[..., 2]) < 1e-12
    assert (on_cone & (g[..., 2] > 1)).sum() > 20 and (g[0][new[0]] == 0).all()
    assert substeps > 1 or (g[256] == 0).all()      # (with substeps the body has dropped off the singularity by the second)
    assert abs(m.motor[5, 2] - PM.KNEE_MIN) < 1e-9 or new[5, 0]
    c.close()


def _walk_setup(mode, reps):
    gait, vel, xyyaw = L.commands(mode)
    return np.tile(gait, reps), np.tile(vel, (reps, 1)), np.tile(xyyaw, (reps, 1))


def test_teacher_forced_closed_loop():
    """64 robots, 40 ticks (three solves): at every tick the numpy plant is stepped from the device plant's previous
    state with the device's effort and controller view, and compared with the device's step."""
    _closed_loop(64, 40)


def _closed_loop(B, ticks, consts=None):
    """The body of test_teacher_forced_closed_loop; consts: see _pair."""
    k = consts or DEFAULTS
    gait, vel, xyyaw = _walk_setup(0, B // L.N_CMD)
    c, plant = _pair(B, xyyaw=xyyaw, consts=consts)
    c.set_gait(_dev(c, gait))
    c.set_vel(_dev(c, vel))
    m = PM.PlantModel(B, k["freq"], k["mu"], 1, xyyaw, mass=k["mass"], ibody=k["ibody"], geom=k["geom"])
    s = _snap(plant)
    s["foot"], s["grf"] = s["foot"].reshape(B, 4, 3), s["grf"].reshape(B, 4, 3)
    _compare(s, m, "init")
    moved = 0.0
    for t in range(ticks):
        m.load(s)
        eff = c.tick_state(plant.state, plant.motor, plant.effort).cpu().numpy()
        v = c.view()
        cs, pd, vd = (v[k].cpu().numpy() for k in ("contact_state", "p_des", "v_des"))
        plant.step(plant.effort)
        m.step(eff, cs, pd, vd)
        s = _snap(plant)
        s["foot"], s["grf"] = s["foot"].reshape(B, 4, 3), s["grf"].reshape(B, 4, 3)
        _compare(s, m, f"tick {t}")
        moved = max(moved, float(np.abs(eff).max()))
    assert moved > 1.0 and (c.read("safe") == 1).all() and c.view()["ticks"] == ticks
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_closed_loop_walk(mode):
    """The CPU yardstick's commands, four robots per command, 650 ticks, device controller + device plant: every robot
    stays safe, no solve reports an error bit, and per robot the height's extremes, the largest |roll| and |pitch| and
    the last second's mean forward speed lie inside the CPU run's recorded value for that command widened by twice the
    CPU run's own spread of the quantity over its 16 robots (plant_loop.envelope: the only source of the bounds)."""
    from quadruped_ctrl_amd.binding import rollout
    reps = 4
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_closed_loop_cpu.json")))
    rec = gold[f"mode{mode}"]
    gait, vel, xyyaw = _walk_setup(mode, reps)
    assert np.array_equal(rec["vel"], vel[:L.N_CMD]) and np.array_equal(rec["gait"], gait[:L.N_CMD])
    c, plant = _pair(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None, xyyaw=xyyaw)
    c.set_gait(_dev(c, gait))
    c.set_vel(_dev(c, vel))
    r = L.Recorder(B, L.TICKS)
    r.add(plant.state.cpu().numpy(), initial=True)
    for t in range(L.TICKS):
        rollout(c, plant, 1)
        r.add(plant.state.cpu().numpy())
        assert (c.read("status")[:, 0] & 47 == 0).all(), t
    assert (c.read("safe") == 1).all()
    stats, env = r.stats(), L.envelope(rec)
    for k in L.STATS:
        lo, hi = np.tile(env[k][0], reps), np.tile(env[k][1], reps)
        want = np.tile(np.asarray(rec[k]), reps)
        print(f"mode {mode} {k}: largest distance from the CPU run {np.abs(stats[k] - want).max():.3e}, "
              f"allowed {float((hi - want).max()):.3e}")
        assert (stats[k] >= lo).all() and (stats[k] <= hi).all(), (k, stats[k], lo, hi)
    c.close()


@pytest.mark.parametrize("schedule,ticks", [("lockstep", 26), ("per_robot", 5)])
def test_graph_capture_matches_eager(schedule, ticks):
    from quadruped_ctrl_amd.binding import QmpcError, rollout
    B = 64
    gait, vel, xyyaw = _walk_setup(0, 4)
    out = []
    for graph in (False, True):
        c, plant = _pair(B, schedule, xyyaw=xyyaw)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        rollout(c, plant, 13)                                        # an eager start: past the first solve
        if graph and schedule == "lockstep":
            with pytest.raises(QmpcError):
                rollout(c, plant, 5, graph=True)
        res = rollout(c, plant, ticks, graph=graph)
        assert (res["graph"] is not None) == graph
        snap = _snap(plant)
        snap["effort"] = res["effort"].cpu().numpy().copy()
        v = c.view()
        snap.update({"ctrl_" + k: v[k].cpu().numpy().copy() for k in v if k not in ("batch", "ticks")})
        out.append(snap)
        assert v["ticks"] == 13 + ticks
        c.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(out[0]["effort"]).max() > 1.0


def test_reset_masked_robots_only():
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    gait, vel, xyyaw = _walk_setup(0, 4)
    mask = (np.arange(B) % 3 == 0)
    runs = []
    for do_reset in (False, True):
        c, plant = _pair(B, "per_robot", xyyaw=xyyaw)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        first = _snap(plant)
        rollout(c, plant, 20)
        if do_reset:
            plant.reset(_dev(c, mask), _dev(c, xyyaw))
            after = _snap(plant)
            c.reset(_dev(c, mask))
            c.set_gait(_dev(c, gait))
            c.set_vel(_dev(c, vel))
        else:
            before = _snap(plant)
        rollout(c, plant, 15)
        end = _snap(plant)
        end["effort"] = plant.effort.cpu().numpy().copy()
        runs.append(end)
        c.close()
    for k in PLANT_KEYS:
        assert np.array_equal(after[k][mask], first[k][mask]), k         # the initial state, bit for bit
        assert np.array_equal(after[k][~mask], before[k][~mask]), k      # the others: untouched
    assert not np.array_equal(before["p"][mask], first["p"][mask])
    for k in runs[0]:
        assert np.array_equal(runs[0][k][~mask], runs[1][k][~mask]), k   # ... and they go on as if nothing happened
    assert not np.array_equal(runs[0]["state"][mask], runs[1]["state"][mask])


def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant, PlantView, QmpcError
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device=c.device)
    eff, st, mo = d(B, 12), d(B, 16), d(B, 24)
    mask = torch.zeros(B, dtype=torch.uint8, device=c.device)
    v = PlantView()
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == STATE            # before qmpc_ctrl_init
    with pytest.raises(QmpcError):
        BatchedPlant(c).init()
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == STATE   # before plant_init
    assert lib.qmpc_plant_reset(h, B, mask.data_ptr(), None, None) == STATE
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_init(None, B, 0.4, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B + 1, 0.4, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, 0.4, 0, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, -0.1, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, float("nan"), 1, None, None) == ARG
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == STATE                   # a refused init initialises nothing
    assert lib.qmpc_plant_init(h, B, 0.4, 2, None, None) == OK
    assert lib.qmpc_plant_view_get(h, None) == ARG
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == OK and (v.batch, v.substeps, v.mu_plant) == (B, 2, 0.4)
    assert lib.qmpc_plant_step(h, B - 1, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, None, st.data_ptr(), mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), None, mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), None, None) == ARG
    assert lib.qmpc_plant_reset(h, B, None, None, None) == ARG
    assert lib.qmpc_plant_reset(h, B + 1, mask.data_ptr(), None, None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(st).all() and torch.isfinite(mo).all()
    c.close()


def test_plant_touches_no_controller_state():
    """After a closed-loop run and a controller re-init, the controller fed make_state_stream produces the efforts of
    a handle that never had a plant."""
    from quadruped_ctrl_amd.binding import rollout
    B, ticks = 64, 27
    gait, vel, xyyaw = _walk_setup(0, 4)
    state, motor = W.make_state_stream(B, ticks, 64)
    effs = []
    for with_plant in (True, False):
        c, plant = _pair(B, xyyaw=xyyaw) if with_plant else (None, None)
        if not with_plant:
            from quadruped_ctrl_amd.binding import BatchedController
            c = BatchedController(0, max_batch=B)
        else:
            c.set_gait(_dev(c, gait))
            c.set_vel(_dev(c, vel))
            rollout(c, plant, 26)
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        out = []
        for t in range(ticks):
            out.append(c.tick_state(_dev(c, state[t]), _dev(c, motor[t])).cpu().numpy().copy())
            if with_plant and t % 2:
                plant.step(plant.effort)                                 # the plant running beside it changes nothing
        effs.append(np.stack(out))
        c.close()
    assert np.array_equal(effs[0], effs[1]) and np.abs(effs[0]).max() > 1.0
