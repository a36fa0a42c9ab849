"""GPU suite (-m gpu) for the plant's per-robot terrain (include/qmpc_terrain.h; BatchedPlant.set_terrain / terrain).

The kernels of csrc/qmpc_terrain.hip are compared with tests/plant_model_terrain.py at tests/test_gpu_plant.py's
tolerance, 1e-10 relative to max(1, |x|): the same arithmetic with a few dozen more fp64 operations per step, and a floor()
whose argument the case keeps 1e-6 tread depths away from an integer (about ten orders above its rounding).  The walk on
plant_loop_terrain.terrain() is held to the CPU loops' recorded statistics
(tests/golden/plant_terrain_closed_loop_cpu.json) by plant_loop.envelope(); everything else compares two runs of the
library bit for bit.  The shared helpers (snap3, compare_terrain, walk_pair, stand_on, ...) and the walk are
tests/fleet_gpu.py's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fleet_gpu as G
import plant_loop as L
import plant_loop_terrain as LT
import plant_model as PM
import plant_model_terrain as PT
import plant_model_varied as PV
import terrain_cases as TC
from plant_cases import DEFAULTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_pair, _dev, _snap, _close, _same = G.pair, G.dev, G.snap, G.close, G.same
_snap3, _stats, _compare_terrain, _all, _walk_pair, _stand_on = (G.snap3, G.plant_stats, G.compare_terrain, G.all_robots,
                                                                  G.walk_pair, G.stand_on)


# ---- 1. single-step parity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("vary,stats", [(False, False), (False, True), (True, False), (True, True)])
def test_single_step_parity(substeps, vary, stats):
    """tests/terrain_cases.py: B = 37 (148 lanes: a partial last wave, an odd number of quads), slope and stairs together
    under every robot, both flags, touch-down edges on several treads, swing feet commanded below the surface, in all
    four <VARY, STATS> instantiations.  The case's own promises are asserted on the model (TC.check)."""
    B = TC.B
    case = TC.parity_case(substeps)
    m0, rows, old, new, tau, cs, pd, vd = case
    vals = TC.values(1000 + substeps) if vary else None
    m = TC.model(substeps, rows, vals, src=m0)
    c, plant = _pair(B, substeps=substeps)
    G.start(c, plant, m0, cs, pd, vd)
    dev = _dev(c, rows)
    plant.set_terrain(dev, clamp_swing=True, rebase_z=True)
    plant.terrain()["support"].copy_(_dev(c, m0.support))
    keep = {k: _dev(c, v) for k, v in (vals or {}).items()}
    if vary:
        plant.set_params(**keep)
    if stats:
        plant.enable_stats()
        plant.reset_stats()
    plant.step(_dev(c, tau.reshape(B, 12)))
    m.step(tau.reshape(B, 12), cs, pd, vd)
    TC.check(case, m)
    s = _snap3(plant, B)
    _compare_terrain(s, m, f"substeps {substeps} vary {vary} stats {stats}")
    # the view's p is world truth, the state row's column 6 is the height above the stance feet
    assert np.array_equal(s["state"][:, 6], s["p"][:, 2] - s["support"]) and np.abs(s["support"]).max() > 0.01
    assert np.array_equal(s["state"][:, 4:6], s["p"][:, :2])
    if stats:
        st = _stats(plant)
        for k in PV.STAT_KEYS[1:]:
            _close(st[k], m.stats[k], f"statistics {k}")
        assert (st["n"] == 1).all() and np.array_equal(st["z_min"], s["state"][:, 6])     # re-based
    del dev, keep
    c.close()


# ---- 2. the case cannot pass without the feature -------------------------------------------------------------------------

def test_every_column_and_flag_moves_the_model():
    """On the model alone (the parity above holds the kernels to it): against the case's result, each column of the rows
    zeroed or shifted, and each flag dropped, moves the state or the feet by more than 1e-6 -- four orders above the
    parity's tolerance.  The plane's columns z0, gx, gy also move it when they alone are non-zero; the flight's columns
    need one another by definition (k = 0 unless count > 0 and run > 0), which is asserted too."""
    B = TC.B
    m0, rows, old, new, tau, cs, pd, vd = TC.parity_case(1)

    def run(r, flags=(True, True)):
        m = TC.model(1, r, None, flags, src=m0)
        m.step(tau.reshape(B, 12), cs, pd, vd)
        return np.concatenate([m.state, m.foot.reshape(B, 12), m.motor, m.support[:, None], m.ground[:, None]], 1)

    base = run(rows)
    for j, name in enumerate(PT.COLUMNS):
        r = rows.copy()
        r[:, j] = r[:, j] + 0.5 if name in ("s0", "psi") else 0.0
        moved = np.abs(run(r) - base).max()
        print(f"column {name}: moves the result by {moved:.3e}")
        assert moved > 1e-6, name
    for k, flags in enumerate(((False, True), (True, False))):
        moved = np.abs(run(rows, flags) - base).max()
        print(f"flag {1 << k} dropped: moves the result by {moved:.3e}")
        assert moved > 1e-6, flags
    flat = run(np.zeros((B, 8)))
    for j, name in enumerate(PT.COLUMNS):
        r = np.zeros((B, 8))
        r[:, j] = rows[:, j] if name != "count" else 4.0
        moved = np.abs(run(r) - flat).max()
        assert (moved > 1e-6) == (name in ("z0", "gx", "gy")), (name, moved)


# ---- 3. neutrality -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
@pytest.mark.parametrize("extras", [False, True])
def test_zero_rows_change_no_bit(schedule, extras):
    """26 closed-loop ticks (tick_state -> step) with all-zero rows bound under flags = 0, then 26 more under rebase_z,
    against the unbound plant: no bit differs -- with nothing else bound, and with per-robot parameters and statistics."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    ca, pa, (gait, vel, xyyaw) = _walk_pair(B, schedule)
    cb, pb, _ = _walk_pair(B, schedule)
    keep = []
    if extras:
        var = _payloads(B)
        for c, p in ((ca, pa), (cb, pb)):
            t = {k: _dev(c, v) for k, v in var.items()}
            p.set_params(**t)
            p.enable_stats()
            p.reset_stats()
            keep.append(t)
    rows = _stand_on(ca, pa, np.zeros((B, 8)), xyyaw)              # (the reset on zero terrain is the flat reset)
    _same(pa, pb, "after reset")
    assert pa.terrain()["bound"] and not pb.terrain()["bound"]
    rollout(ca, pa, 26)
    rollout(cb, pb, 26)
    _same(pa, pb, "zero rows, no flags")
    pa.set_terrain(rows, rebase_z=True)
    rollout(ca, pa, 26)
    rollout(cb, pb, 26)
    _same(pa, pb, "zero rows, rebase_z")
    assert np.abs(pa.effort.cpu().numpy()).max() > 1.0
    if extras:
        sa, sb = _stats(pa), _stats(pb)
        for k in PV.STAT_KEYS:
            assert np.array_equal(sa[k], sb[k]), k
        assert (sa["n"] == 52).all()
    del keep, rows
    ca.close()
    cb.close()


def _payloads(B):
    """Per-robot payloads, floors and a constant push (plant_loop_varied's kind, any values do here)."""
    rng = np.random.default_rng(11)
    return dict(mass=rng.uniform(7.0, 12.0, B), ibody=PM.IBODY[None, :] * rng.uniform(0.8, 1.3, (B, 1)),
                mu=rng.uniform(0.3, 0.8, B), force=rng.uniform(-5.0, 5.0, (B, 3)), torque=rng.uniform(-0.5, 0.5, (B, 3)))


def test_init_unbinds_and_reset_keeps_the_binding():
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    ca, pa, (gait, vel, xyyaw) = _walk_pair(B)
    cb, pb, _ = _walk_pair(B)
    rows = _stand_on(ca, pa, LT.terrain(B), xyyaw, clamp_swing=True, rebase_z=True)
    assert pa.terrain()["bound"] and pa.terrain()["flags"] == 3
    rollout(ca, pa, 13)
    pa.reset(_all(ca, B), _dev(ca, xyyaw))                         # keeps the binding: the robots stand on their terrain
    t = pa.terrain()
    assert t["bound"] and np.abs(t["ground"].cpu().numpy()).max() > 0.01
    s = _snap3(pa, B)
    assert np.array_equal(s["p"][:, 2], 0.29 + s["ground"]) and np.abs(s["foot"][..., 2]).max() > 0.01
    rollout(ca, pa, 3)
    rollout(cb, pb, 3)
    assert not np.array_equal(_snap(pa)["p"], _snap(pb)["p"])
    # qmpc_plant_init unbinds: both pairs start again and agree bit for bit
    for c, p in ((ca, pa), (cb, pb)):
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        p.init(DEFAULTS["mu"], 1, _dev(c, xyyaw))
        rollout(c, p, 14)
    assert not pa.terrain()["bound"] and pa.terrain()["flags"] == 0
    _same(pa, pb, "after init")
    del rows
    ca.close()
    cb.close()


# ---- 4. reset on terrain, masked -------------------------------------------------------------------------------------------

def test_masked_reset_places_the_robots_on_their_terrain():
    """B = 37 on slopes and stairs with both flags, five ticks of history, then a reset of every third robot to new
    places: the masked robots are where the model's reset puts them, the others keep every bit."""
    from quadruped_ctrl_amd.binding import rollout
    B = 37
    rng = np.random.default_rng(4)
    k = np.arange(B) % L.N_CMD
    gait, vel, xyyaw = (a[k] for a in L.commands(0))
    c, plant = _pair(B, xyyaw=xyyaw)
    c.set_gait(_dev(c, gait))
    c.set_vel(_dev(c, vel))
    rows = TC.rows_for(np.concatenate([xyyaw[:, :2], np.zeros((B, 1))], 1), rng)
    dev = _stand_on(c, plant, rows, xyyaw, clamp_swing=True, rebase_z=True)
    m = PT.TerrainPlantModel(B, L.FREQ, DEFAULTS["mu"], 1, xyyaw)
    m.set_terrain(rows, clamp_swing=True, rebase_z=True)
    m.reset(np.ones(B, bool), xyyaw)
    _compare_terrain(_snap3(plant, B), m, "reset of all")
    rollout(c, plant, 5)
    before = _snap3(plant, B)
    mask = np.arange(B) % 3 == 0
    place = xyyaw + rng.uniform(-0.3, 0.3, (B, 3))
    plant.reset(_dev(c, mask), _dev(c, place))
    after = _snap3(plant, B)
    m.reset(mask, place)
    for key, mk in (("state", "state"), ("motor", "motor"), ("p", "p"), ("v", "v"), ("q", "q"), ("omega", "w"),
                    ("foot", "foot"), ("grf", "grf"), ("ground", "ground"), ("support", "support")):
        _close(after[key][mask], getattr(m, mk)[mask], f"masked reset {key}")
        assert np.array_equal(after[key][~mask], before[key][~mask]), key
    assert (after["stance"][mask] == 1).all() and np.array_equal(after["stance"][~mask], before["stance"][~mask])
    hz = m.height(after["foot"][..., 0], after["foot"][..., 1])
    assert np.abs(after["foot"][..., 2] - hz)[mask].max() < 1e-12 and np.abs(after["p"][mask, 2] - 0.29 - after["ground"][mask]).max() < 1e-12
    assert np.abs(after["ground"][mask]).max() > 0.01 and not np.array_equal(before["p"][~mask], m.p[~mask])
    del dev
    c.close()


# ---- 5. a captured graph reads the rows, not a copy ------------------------------------------------------------------------

def test_graph_replay_reads_the_rewritten_rows():
    """Lockstep, flat rows bound, a 13-tick block captured (and replayed once), the rows rewritten on the stream to
    plant_loop_terrain.terrain(), the graph replayed: bit for bit an eager run doing the same, and not the run whose rows
    stay flat."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    out = {}
    for name, graph, rewrite in (("eager", False, True), ("graph", True, True), ("flat", False, False)):
        c, plant, (gait, vel, xyyaw) = _walk_pair(B)
        dev = _stand_on(c, plant, np.zeros((B, 8)), xyyaw, clamp_swing=True, rebase_z=True)
        plant.enable_stats()
        plant.reset_stats()
        res = rollout(c, plant, 13, graph=graph)
        if rewrite:
            dev.copy_(_dev(c, LT.terrain(B)))
        if graph:
            res["graph"].replay()
        else:
            rollout(c, plant, 13)
        snap = _snap3(plant, B)
        snap["effort"] = plant.effort.cpu().numpy().copy()
        snap.update({"stats_" + k: v for k, v in _stats(plant).items()})
        out[name] = snap
        del dev, res
        c.close()
    for k in out["eager"]:
        assert np.array_equal(out["eager"][k], out["graph"][k]), k
    assert (out["graph"]["stats_n"] == 26).all() and np.abs(out["graph"]["effort"]).max() > 1.0
    assert np.abs(out["graph"]["ground"]).max() > 0.01 and not np.array_equal(out["graph"]["state"], out["flat"]["state"])


# ---- 6. bad values ---------------------------------------------------------------------------------------------------------

def test_bad_values_stay_inside_their_robot():
    """A NaN slope on robot 3, run = 0 with count = 4 on robot 7, rise = inf on robot 11: after a reset and 5 ticks every
    other robot's plant state, terrain views and statistics are those of a run without the three, bit for bit."""
    from quadruped_ctrl_amd.binding import rollout
    B, bad = 16, [3, 7, 11]
    good = np.setdiff1d(np.arange(B), bad)
    out = []
    for spoil in (False, True):
        c, plant, (gait, vel, xyyaw) = _walk_pair(B)
        rows = LT.terrain(B)
        rows[7] = rows[4]                                   # (a flight under robot 7 too)
        if spoil:
            rows[3, 1] = np.nan
            rows[7, 4] = 0.0
            rows[11, 3], rows[11, 4], rows[11, 5] = np.inf, 0.1, 4.0
        dev = _stand_on(c, plant, rows, xyyaw, clamp_swing=True, rebase_z=True)
        plant.enable_stats()
        plant.reset_stats()
        rollout(c, plant, 5)
        out.append((_snap3(plant, B), _stats(plant)))
        del dev
        c.close()
    for part in (0, 1):
        for k in out[0][part]:
            assert np.array_equal(out[0][part][k][good], out[1][part][k][good]), k
    assert not np.isfinite(out[1][0]["state"][3]).all() and not np.isfinite(out[1][0]["state"][11]).all()
    assert np.isfinite(out[1][0]["state"][good]).all() and np.isfinite(out[0][0]["state"]).all()
    assert np.isfinite(out[1][0]["state"][7]).all()         # run = 0: no flight, the plane alone


# ---- 7. the fleet walks ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LT.PATHS)
def test_the_fleet_walks_on_terrain(mode, path):
    """The CPU yardstick's commands, four robots per command, on plant_loop_terrain.terrain() with swing feet clamped:
    through tick_state with the re-based height (path "state"), and through the sensors with sense_loop.noise() after
    settle() (path "sensed").  The statistics are read from the device a second before the end and at the end.  Every
    robot stays safe, no solve reports an error bit, and the five statistics lie inside plant_loop.envelope() of the CPU
    run on the same ground."""
    reps = 4
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_terrain_closed_loop_cpu.json")))
    rec = gold[f"mode{mode}"][path]
    ticks = gold["ticks"]
    rows = LT.terrain(B)
    assert np.array_equal(np.asarray(gold["rows"]), rows[:L.N_CMD]) and ticks == LT.TICKS
    c, plant, (gait, vel, xyyaw) = _walk_pair(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None)
    assert np.array_equal(gold[f"mode{mode}"]["vel"], vel[:L.N_CMD]) and np.array_equal(gold[f"mode{mode}"]["gait"], gait[:L.N_CMD])
    dev = _stand_on(c, plant, rows, xyyaw, clamp_swing=True, rebase_z=path == "state")
    plant.enable_stats()
    plant.reset_stats()
    start, mid, end = G.ground_walk(c, plant, path, mode, ticks, gold["seed"], gold["settle"])
    G.assert_inside_envelope(G.stats_from_accumulators(start, mid, end), rec, reps, f"mode {mode} {path}")
    # they climbed: the stance feet of the robots that left an upward flight stand four treads up
    t = plant.terrain()
    sup = t["support"].cpu().numpy()
    left = np.tile(np.asarray(rec["left_flight"]), reps)
    up = left & (rows[:, 3] > 0)
    assert up.any() and np.abs(sup[up] - 4 * rows[up, 3]).max() < 1e-9
    del dev
    c.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, TerrainView
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    rows = torch.zeros((B, 8), dtype=torch.float64, device=c.device)
    v = TerrainView()
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_set_terrain(h, B, rows.data_ptr(), 0) == STATE          # before qmpc_plant_init
    assert lib.qmpc_terrain_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_plant_set_terrain(None, B, rows.data_ptr(), 0) == ARG
    assert lib.qmpc_plant_set_terrain(h, B + 1, rows.data_ptr(), 0) == ARG        # a foreign batch
    assert lib.qmpc_plant_set_terrain(h, B, rows.data_ptr(), 4) == ARG            # unknown flag bits
    assert lib.qmpc_plant_set_terrain(h, B, rows.data_ptr(), -1) == ARG
    assert lib.qmpc_terrain_view_get(h, None) == ARG
    assert lib.qmpc_terrain_view_get(h, C.byref(v)) == OK and (v.terrain, v.flags, v.batch) == (None, 0, B)
    assert lib.qmpc_plant_set_terrain(h, B, rows.data_ptr(), 3) == OK
    assert lib.qmpc_terrain_view_get(h, C.byref(v)) == OK and (v.terrain, v.flags, v.batch) == (rows.data_ptr(), 3, B)
    assert v.ground and v.support
    assert lib.qmpc_plant_set_terrain(h, B, None, 3) == OK                        # unbinds
    assert lib.qmpc_terrain_view_get(h, C.byref(v)) == OK and (v.terrain, v.flags) == (None, 0)
    torch.cuda.synchronize()
    c.close()
