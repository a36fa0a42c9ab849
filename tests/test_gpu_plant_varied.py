"""GPU suite (-m gpu) for the plant's per-robot parameters and statistics (include/qmpc_plant_vary.h;
BatchedPlant.set_params / enable_stats / reset_stats / stats).

The kernel is compared with tests/plant_model_varied.py at tests/test_gpu_plant.py's tolerance, 1e-10 relative to
max(1, |x|) (fleet_gpu.TOL): the same arithmetic with a handful more fp64 operations per substep.  The walk under the disturbance of
plant_loop_varied.variation() is held to the CPU loop's recorded statistics
(tests/golden/plant_varied_closed_loop_cpu.json) by plant_loop.envelope(); everything else compares two runs of the
library bit for bit.  The shared helpers and the walk (walk, stats_from_accumulators, assert_inside_envelope) are
tests/fleet_gpu.py's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fleet_gpu as G
import plant_loop as L
import plant_loop_varied as LV
import plant_model as PM
import plant_model_varied as PV
from plant_cases import DEFAULTS, parity_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PARAMS = ("mass", "ibody", "mu", "force", "torque")
_pair, _dev, _snap, _close, _compare, _walk_pair = G.pair, G.dev, G.snap, G.close, G.compare, G.walk_pair
_snap3, _stats = G.snap_legs, G.plant_stats


def _values(B, seed):
    """Per-robot mass in [5, 15], inertia scale in [0.5, 2], mu in [0, 1.2] with exact zeros, force within +-50 N,
    torque within +-5 N m."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.0, 1.2, B)
    mu[::5] = 0.0
    return dict(mass=rng.uniform(5.0, 15.0, B), ibody=PM.IBODY[None, :] * rng.uniform(0.5, 2.0, (B, 1)), mu=mu,
                force=rng.uniform(-50.0, 50.0, (B, 3)), torque=rng.uniform(-5.0, 5.0, (B, 3)))


def _bind(c, plant, vals):
    """-> the device tensors bound (None values are not bound)."""
    t = {k: _dev(c, v) for k, v in vals.items() if v is not None}
    plant.set_params(**t)
    return t


def _model(B, substeps, vals, src=None, xyyaw=None):
    mv = PV.VariedPlantModel(B, DEFAULTS["freq"], DEFAULTS["mu"], substeps, xyyaw, mass_b=vals.get("mass"),
                             ibody_b=vals.get("ibody"), mu_b=vals.get("mu"), force=vals.get("force"), torque=vals.get("torque"))
    if src is not None:
        for k in ("p", "v", "q", "w", "foot", "stance"):
            setattr(mv, k, getattr(src, k).copy())
    return mv


@pytest.mark.parametrize("substeps", [1, 4])
def test_single_step_parity_with_all_five_bound(substeps):
    """tests/test_gpu_plant.py's single-step case (B = 257: a partial last block, a lane count that is no multiple of 64;
    every stance pattern, saturated cones, pulling legs, a straight knee) with every robot its own body, floor and push."""
    B, m, old, new, tau, cs, pd, vd = parity_case(substeps)
    vals = _values(B, 1000 + substeps)
    mv = _model(B, substeps, vals, m)
    c, plant = _pair(B, substeps=substeps)
    G.start(c, plant, m, cs, pd, vd)
    keep = _bind(c, plant, vals)
    plant.enable_stats()
    plant.step(_dev(c, tau.reshape(B, 12)))
    mv.step(tau.reshape(B, 12), cs, pd, vd)
    m.step(tau.reshape(B, 12), cs, pd, vd)
    _compare(_snap3(plant, B), mv, f"varied, substeps {substeps}")
    st = _stats(plant)
    for k in PV.STAT_KEYS[1:]:
        _close(st[k], mv.stats[k], f"statistics {k}")
    assert (st["n"] == 1).all()
    # the variation is felt, and the cones are the robots' own: saturated feet, among them floors of mu = 0
    assert np.abs(mv.state - m.state).max() > 1e-3
    g = mv.grf
    on_cone = (np.abs(np.hypot(g[..., 0], g[..., 1]) - vals["mu"][:, None] * g[..., 2]) < 1e-12) & (g[..., 2] > 1)
    assert on_cone.sum() > 20 and (on_cone & (vals["mu"][:, None] == 0)).any()
    del keep
    c.close()


@pytest.mark.parametrize("which", PARAMS + ("all",))
def test_each_pointer_alone_and_all_together(which):
    """B = 8, all four feet standing (robots 240 .. 247 of the single-step case: a saturated cone and pulling legs among
    them): one member bound with the other four NULL, and all five.  A swapped or ignored pointer fails the parity."""
    B0, m0, old, new, tau, cs, pd, vd = parity_case(1)
    idx = np.arange(240, 248)
    B = len(idx)
    assert new[idx].all()
    m = PM.PlantModel(B, DEFAULTS["freq"], DEFAULTS["mu"], 1)
    for k in ("p", "v", "q", "w", "foot", "stance"):
        setattr(m, k, getattr(m0, k)[idx].copy())
    tau, cs, pd, vd = tau[idx], cs[idx], pd[idx], vd[idx]
    full = _values(B, 77)
    full["mu"] = np.array([0.0, 0.05, 0.1, 0.15, 0.9, 1.0, 1.1, 1.2])
    vals = full if which == "all" else {which: full[which]}
    mv = _model(B, 1, vals, m)
    c, plant = _pair(B)
    G.start(c, plant, m, cs, pd, vd)
    keep = _bind(c, plant, vals)
    plant.step(_dev(c, tau.reshape(B, 12)))
    mv.step(tau.reshape(B, 12), cs, pd, vd)
    m.step(tau.reshape(B, 12), cs, pd, vd)
    _compare(_snap3(plant, B), mv, which)
    # this member alone moves the model by far more than the tolerance: the parity above could not pass without it
    assert np.abs(mv.state - m.state).max() > 1e-6, which
    del keep
    c.close()


def _neutral(B):
    return dict(mass=np.full(B, PM.MASS), ibody=np.tile(PM.IBODY, (B, 1)), mu=np.full(B, DEFAULTS["mu"]),
                force=np.zeros((B, 3)), torque=np.zeros((B, 3)))


def test_neutral_values_change_no_bit_and_init_unbinds():
    from quadruped_ctrl_amd.binding import rollout
    B = 64

    def same(a, b, what):
        sa, sb = _snap(a), _snap(b)
        for k in G.PLANT_KEYS:
            assert np.array_equal(sa[k], sb[k]), (what, k)
        assert np.array_equal(a.effort.cpu().numpy(), b.effort.cpu().numpy()), what

    ca, pa, (gait, vel, xyyaw) = _walk_pair(B)
    cb, pb, _ = _walk_pair(B)
    keep = _bind(ca, pa, _neutral(B))
    pa.enable_stats()
    for n in (13, 7):
        rollout(ca, pa, n)
        rollout(cb, pb, n)
        same(pa, pb, f"neutral, {n}")
    pa.set_params(None)                                     # unbound (the statistics stay on): still the same
    rollout(ca, pa, 20)
    rollout(cb, pb, 20)
    same(pa, pb, "unbound")
    assert np.abs(pa.effort.cpu().numpy()).max() > 1.0 and (_stats(pa)["n"] == 40).all()
    # a binding that matters ...
    heavy = _bind(ca, pa, dict(mass=np.full(B, 2 * PM.MASS)))
    rollout(ca, pa, 3)
    rollout(cb, pb, 3)
    assert not np.array_equal(_snap(pa)["p"], _snap(pb)["p"])
    # ... is gone after qmpc_plant_init: both pairs start again and agree
    for c, p in ((ca, pa), (cb, pb)):
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        p.init(DEFAULTS["mu"], 1, _dev(c, xyyaw))
        rollout(c, p, 14)
    same(pa, pb, "after init")
    del keep, heavy
    ca.close()
    cb.close()


def test_teacher_forced_closed_loop_under_variation():
    """64 robots, 40 ticks (three solves), plant_loop_varied.variation() with the push moved to ticks 10 .. 29 and a yaw
    moment of 2 N m beside it, both rewritten in place on the stream every tick: at every tick the numpy plant is stepped
    from the device plant's previous state and compared with the device's step; the statistics with the model's."""
    B, ticks = 64, 40
    var = LV.variation(B, push_ticks=(10, 30))
    sign = np.sign(var["push"][:, 1])
    twist = np.stack([np.zeros(B), np.zeros(B), 2.0 * sign], 1)
    torque = lambda t: twist if 10 <= t < 30 else np.zeros((B, 3))
    c, plant, (gait, vel, xyyaw) = _walk_pair(B)
    vals = dict(mass=var["mass"], ibody=var["ibody"], mu=var["mu"], force=var["force"](0), torque=torque(0))
    dev = _bind(c, plant, vals)
    plant.enable_stats()
    m = _model(B, 1, vals, xyyaw=xyyaw)
    s = _snap3(plant, B)
    _compare(s, m, "init")
    moved = 0.0
    for t in range(ticks):
        m.load(s)
        m.force, m.torque = var["force"](t), torque(t)
        dev["force"].copy_(_dev(c, m.force))
        dev["torque"].copy_(_dev(c, m.torque))
        eff = c.tick_state(plant.state, plant.motor, plant.effort).cpu().numpy()
        v = c.view()
        cs, pd, vd = (v[k].cpu().numpy() for k in ("contact_state", "p_des", "v_des"))
        plant.step(plant.effort)
        m.step(eff, cs, pd, vd)
        s = _snap3(plant, B)
        _compare(s, m, f"tick {t}")
        moved = max(moved, float(np.abs(eff).max()))
    st = _stats(plant)
    assert (st["n"] == ticks).all() and (m.stats["n"] == ticks).all()
    for k in PV.STAT_KEYS[1:]:
        _close(st[k], m.stats[k], f"statistics {k}")
    assert moved > 1.0 and (c.read("safe") == 1).all()
    assert np.abs(st["vy_sum"]).max() > 0.1            # the shove moved them sideways
    c.close()


def test_bad_values_stay_inside_their_robot():
    """NaN force on robot 3, mass 0 on robot 7, negative mu on robot 11: after 5 ticks every other robot's plant state and
    statistics are those of a run without the three, bit for bit."""
    from quadruped_ctrl_amd.binding import rollout
    B, bad = 16, [3, 7, 11]
    good = np.setdiff1d(np.arange(B), bad)
    out = []
    for spoil in (False, True):
        c, plant, _ = _walk_pair(B)
        vals = _values(B, 5)
        vals["mu"][bad] = 0.5
        if spoil:
            vals["force"][3, 1] = np.nan
            vals["mass"][7] = 0.0
            vals["mu"][11] = -0.3
        keep = _bind(c, plant, vals)
        plant.enable_stats()
        rollout(c, plant, 5)
        out.append((_snap(plant), _stats(plant)))
        del keep
        c.close()
    for part in (0, 1):
        for k in out[0][part]:
            assert np.array_equal(out[0][part][k][good], out[1][part][k][good]), k
    assert not np.isfinite(out[1][0]["state"][3]).all() and np.isfinite(out[1][0]["state"][good]).all()
    assert np.isfinite(out[0][0]["state"]).all()


def test_statistics_reset_masked_robots_only():
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    mask = np.arange(B) % 3 == 0
    ends = []
    for do_reset in (False, True):
        c, plant, _ = _walk_pair(B, "per_robot")
        plant.enable_stats()
        first = _stats(plant)
        rollout(c, plant, 20)
        before = _stats(plant)
        if do_reset:
            plant.reset_stats(_dev(c, mask))
            after = _stats(plant)
        rollout(c, plant, 10)
        ends.append(_stats(plant))
        c.close()
    init = PV.stats_initial(B)
    for k in PV.STAT_KEYS:
        assert np.array_equal(first[k], init[k]), k                       # what the first enable left
        assert np.array_equal(after[k][mask], init[k][mask]), k           # the initial values again
        assert np.array_equal(after[k][~mask], before[k][~mask]), k       # the others: untouched
        assert np.array_equal(ends[0][k][~mask], ends[1][k][~mask]), k    # ... and they go on as if nothing happened
    assert (before["n"] == 20).all() and (ends[1]["n"][mask] == 10).all() and (ends[1]["n"][~mask] == 30).all()
    assert (ends[1]["z_max"][mask] < ends[0]["z_max"][mask]).any()        # (the start's 0.29 is forgotten)
    # NULL: all robots; a disabled plant keeps the values and stops counting
    c, plant, _ = _walk_pair(B)
    plant.enable_stats()
    rollout(c, plant, 3)
    plant.enable_stats(False)
    rollout(c, plant, 2)
    s = plant.stats()
    assert s["enabled"] is False and (_stats(plant)["n"] == 3).all()
    plant.reset_stats()
    got = _stats(plant)
    for k in PV.STAT_KEYS:
        assert np.array_equal(got[k], init[k]), k
    c.close()


def test_graph_replays_read_the_rewritten_force():
    """Lockstep, 13 eager ticks, then a 26-tick block captured with parameters bound and statistics on, replayed twice
    with the force tensor rewritten between the replays: bit for bit an eager run doing the same."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    var = LV.variation(B)
    out = []
    for graph in (False, True):
        c, plant, _ = _walk_pair(B)
        dev = _bind(c, plant, dict(mass=var["mass"], ibody=var["ibody"], mu=var["mu"], force=np.zeros((B, 3)),
                                   torque=var["torque"]))
        plant.enable_stats()
        rollout(c, plant, 13)
        res = rollout(c, plant, 26, graph=graph)
        mid = _snap(plant)
        dev["force"].copy_(_dev(c, var["push"]))
        if graph:
            res["graph"].replay()
        else:
            rollout(c, plant, 26)
        snap = _snap(plant)
        snap["effort"] = plant.effort.cpu().numpy().copy()
        snap.update({"stats_" + k: v for k, v in _stats(plant).items()})
        snap.update({"mid_" + k: v for k, v in mid.items()})
        out.append(snap)
        del dev
        c.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert (out[1]["stats_n"] == 65).all() and np.abs(out[1]["effort"]).max() > 1.0
    # the second replay felt the push: 30 N on 7 .. 13 kg for 52 ms is 0.12 .. 0.22 m/s where nothing resists
    assert np.abs(out[1]["v"][:, 1] - out[1]["mid_v"][:, 1]).max() > 0.02


@pytest.mark.parametrize("mode", [0, 1])
def test_the_fleet_survives(mode):
    """The CPU yardstick's commands, four robots per command, 650 ticks, under plant_loop_varied.variation(): payloads of
    0.8 .. 1.4 times the MPC's 9 kg, floors of mu 0.3 .. 0.8 under an MPC planning on 0.4, a 30 N shove for 50 ticks.
    The statistics are read from the device twice, at tick 150 and at the end.  Every robot stays safe, no solve
    reports an error bit, and the five statistics lie inside plant_loop.envelope() of the CPU run on the same plant."""
    from quadruped_ctrl_amd.binding import rollout
    reps = 4
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_varied_closed_loop_cpu.json")))
    rec = gold[f"mode{mode}"]
    var = LV.variation(B)
    for k in ("mass", "ibody", "mu", "push"):
        assert np.array_equal(np.asarray(gold["variation"][k]), var[k][:L.N_CMD]), k
    c, plant, (gait, vel, xyyaw) = _walk_pair(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None)
    assert np.array_equal(rec["vel"], vel[:L.N_CMD]) and np.array_equal(rec["gait"], gait[:L.N_CMD])
    dev = _bind(c, plant, dict(mass=var["mass"], ibody=var["ibody"], mu=var["mu"], force=var["force"](0), torque=var["torque"]))
    plant.enable_stats()
    t0, t1 = var["push_ticks"]

    def tick(t):
        if t in (t0, t1):
            dev["force"].copy_(_dev(c, var["force"](t)))
        rollout(c, plant, 1)

    start, at150, end = G.walk(c, plant, tick, L.TICKS, lambda t: mode == 1 or (t + 1) % 13 == 0)
    G.assert_inside_envelope(G.stats_from_accumulators(start, at150, end), rec, reps, f"mode {mode}")
    del dev
    c.close()


def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, PlantParams, PlantStats
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    mass = torch.full((B,), 9.0, dtype=torch.float64, device=c.device)
    prm, v = PlantParams(mass=mass.data_ptr()), PlantStats()
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_set_params(h, B, C.byref(prm)) == STATE             # before qmpc_plant_init
    assert lib.qmpc_plant_stats_enable(h, 1) == STATE
    assert lib.qmpc_plant_stats_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_stats_reset(h, B, None, None) == STATE
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_plant_stats_get(h, C.byref(v)) == STATE                   # before the first enable
    assert lib.qmpc_plant_stats_reset(h, B, None, None) == STATE
    assert lib.qmpc_plant_set_params(None, B, C.byref(prm)) == ARG
    assert lib.qmpc_plant_set_params(h, B + 1, C.byref(prm)) == ARG
    assert lib.qmpc_plant_set_params(h, B, C.byref(prm)) == OK
    assert lib.qmpc_plant_set_params(h, B, None) == OK                        # unbinds
    assert lib.qmpc_plant_stats_enable(h, 1) == OK
    assert lib.qmpc_plant_stats_get(h, None) == ARG
    assert lib.qmpc_plant_stats_reset(h, B - 1, None, None) == ARG
    assert lib.qmpc_plant_stats_reset(h, B, None, None) == OK
    assert lib.qmpc_plant_stats_get(h, C.byref(v)) == OK and (v.batch, v.enabled) == (B, 1)
    assert lib.qmpc_plant_stats_enable(h, 0) == OK
    assert lib.qmpc_plant_stats_get(h, C.byref(v)) == OK and (v.batch, v.enabled) == (B, 0)
    torch.cuda.synchronize()
    c.close()
