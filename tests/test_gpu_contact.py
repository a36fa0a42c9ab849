"""GPU suite (-m gpu) for contact decided by the ground (include/qmpc_contact.h; BatchedPlant.set_contact / contact).

The kernels of csrc/qmpc_contact.hip are compared with tests/plant_model_contact.py at tests/test_gpu_plant.py's
tolerance, 1e-10 relative to max(1, |x|): the terrain step's arithmetic plus a few dozen fp64 operations, with every
comparison the step branches on kept 1e-6 (relative) away from a tie by the case (about ten orders above its rounding);
the flags and the counters are compared exactly.  The walk on plant_loop_contact.walk_config() is held to the CPU loops'
recorded statistics (tests/golden/plant_contact_closed_loop_cpu.json) by plant_loop.envelope() and the same rule for the
contact counters; everything else compares two runs of the library bit for bit.  The shared helpers (snap4,
compare_contact, start_contact, masked_reset_is_the_models, ...) and the walk are tests/fleet_gpu.py's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import contact_cases as CC
import fleet_gpu as G
import plant_loop as L
import plant_loop_contact as LC
import plant_loop_terrain as LT
import plant_model_contact as PCM
import plant_model_varied as PV
from plant_cases import DEFAULTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_pair, _dev, _snap, _close, _same = G.pair, G.dev, G.snap, G.close, G.same
_snap4, _stats, _all, _walk_pair, _stand_on = G.snap4, G.plant_stats, G.all_robots, G.walk_pair, G.stand_on
_compare_contact, _start_contact = G.compare_contact, G.start_contact
CONTACT_KEYS, ON = G.CONTACT_KEYS, G.ON


# ---- 1. single-step parity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("vary,stats", [(False, False), (False, True), (True, False), (True, True)])
def test_single_step_parity(substeps, vary, stats):
    """tests/contact_cases.py: B = 37, slope and stairs under every robot, all three flags, none of the parameters at its
    default; feet pinned early, kept, released, late in the air, landing, sliding (one over a tread edge), robots with no
    foot pinned -- in all four <VARY, STATS> instantiations.  The case's own promises are asserted on the model."""
    B = CC.B
    case = CC.parity_case(substeps)
    m0, rows, old, new, tau, cs, pd, vd = case
    vals = CC.values(1000 + substeps) if vary else None
    m = CC.stepped(case, substeps, vals)
    CC.check(case, m)
    c, plant = _pair(B, substeps=substeps)
    dev = _start_contact(c, plant, m0, cs, pd, vd, rows, (True, True), (True, True, True), CC.PARAMS)
    keep = {k: _dev(c, v) for k, v in (vals or {}).items()}
    if vary:
        plant.set_params(**keep)
    if stats:
        plant.enable_stats()
        plant.reset_stats()
    v = plant.contact()
    assert v["flags"] == 7 and (v["drop_speed"], v["slip_gain"], v["slip_vmax"]) == tuple(CC.PARAMS.values())
    plant.step(_dev(c, tau.reshape(B, 12)))
    s = _snap4(plant, B)
    _compare_contact(s, m, f"substeps {substeps} vary {vary} stats {stats}")
    assert np.array_equal(s["state"][:, 6], s["p"][:, 2] - s["support"]) and np.abs(s["support"]).max() > 0.01
    if stats:
        st = _stats(plant)
        for k in PV.STAT_KEYS[1:]:
            _close(st[k], m.stats[k], f"statistics {k}")
        assert (st["n"] == 1).all() and np.array_equal(st["z_min"], s["state"][:, 6])
    del dev, keep
    c.close()


@pytest.mark.parametrize("flags,bound", [((False, True, True), True), ((True, False, False), True), ((False, False, True), True),
                                         ((True, True, True), False)])
def test_single_step_parity_other_flags(flags, bound):
    """The branches a dropped flag leaves to the older rule -- touch-down by the schedule without `late`, release by the
    schedule and the terrain's swing clamp without `early`, a saturated foot that stays without `slip` -- and the step
    with no terrain bound (a null rows pointer: height 0, normal (0, 0, 1))."""
    B = CC.B
    case = CC.parity_case(1)
    m0, rows, old, new, tau, cs, pd, vd = case
    if not bound:
        case = (m0, None) + tuple(case[2:])
    m = CC.stepped(case, 1, flags=flags)
    CC.check_ties(m)
    c, plant = _pair(B)
    dev = _start_contact(c, plant, m0, cs, pd, vd, rows if bound else None, (True, True), flags, CC.PARAMS)
    plant.step(_dev(c, tau.reshape(B, 12)))
    s = _snap4(plant, B)
    _compare_contact(s, m, f"flags {flags} bound {bound}")
    tr = m.trace
    assert (tr["pin2"] != tr["s"]).any() == (flags[0] or flags[1])
    if not bound:
        assert np.array_equal(s["ground"], np.zeros(B)) and (s["foot"][..., 2][tr["pin2"] & ~tr["pin0"]] == 0).all()
    del dev
    c.close()


# ---- 2. the parity cannot pass on a kernel that ignores a flag or a parameter ------------------------------------------

def test_every_flag_and_every_parameter_moves_the_model():
    """On the model alone (the parity above holds the kernels to it): each contact flag dropped and each parameter doubled
    moves the case's result by more than 1e-6 -- four orders above the parity's tolerance."""
    for what, moved in CC.sensitivity(1).items():
        print(f"{what}: moves the result by {moved:.3e}")
        assert moved > 1e-6, what


# ---- 3. neutrality -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
@pytest.mark.parametrize("terrain", [False, True])
def test_flags_zero_change_no_bit(schedule, terrain):
    """39 closed-loop ticks: 13 after contact was switched on and off again with set_contact(None) before any step, 26
    more after set_contact() with every flag False -- against the same run without any of the calls: no bit differs,
    and the counters stay zero."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    ca, pa, (gait, vel, xyyaw) = _walk_pair(B, schedule)
    cb, pb, _ = _walk_pair(B, schedule)
    keep = []
    if terrain:
        for c, p in ((ca, pa), (cb, pb)):
            keep.append(_stand_on(c, p, LT.terrain(B), xyyaw, clamp_swing=True, rebase_z=True))
    pa.set_contact(**ON)
    assert pa.contact()["flags"] == 7
    pa.set_contact(None)
    assert pa.contact()["flags"] == 0
    rollout(ca, pa, 13)
    rollout(cb, pb, 13)
    _same(pa, pb, "after set_contact(None)")
    pa.set_contact()
    rollout(ca, pa, 26)
    rollout(cb, pb, 26)
    _same(pa, pb, "flags 0")
    sa, sb = _snap4(pa, B), _snap4(pb, B)
    for k in ("ground", "support") + CONTACT_KEYS:
        assert np.array_equal(sa[k], sb[k]), k
    assert not sa["early"].any() and not sa["slip"].any() and np.abs(pa.effort.cpu().numpy()).max() > 1.0
    # ... and the flags do something on this very run
    pa.set_contact(**ON)
    rollout(ca, pa, 13)
    rollout(cb, pb, 13)
    assert not np.array_equal(_snap(pa)["state"], _snap(pb)["state"]) and _snap4(pa, B)["early"].any()
    del keep
    ca.close()
    cb.close()


def test_init_switches_contact_off_and_reset_keeps_it():
    """reset(mask) keeps contact on and zeroes the masked robots' counters and drop only; init() switches it off, zeroes
    the counters, and the plant is the plain plant again, bit for bit.  The masked reset is the model's on flat ground
    and on terrain (fleet_gpu.masked_reset_is_the_models; tests/test_gpu_field.py runs it on the field)."""
    from quadruped_ctrl_amd.binding import rollout
    for ground in ("flat", "terrain"):
        G.masked_reset_is_the_models(ground)
    B = 64
    ca, pa, (gait, vel, xyyaw) = _walk_pair(B)
    cb, pb, _ = _walk_pair(B)
    rows = _stand_on(ca, pa, LC.rows_for(B, 0.04), xyyaw, clamp_swing=True, rebase_z=True)
    pa.init(0.15, 1, _dev(ca, xyyaw))                       # (a slippery floor: everybody slides)
    pa.set_terrain(rows, clamp_swing=True, rebase_z=True)
    pa.set_contact(**ON)
    pa.reset(_all(ca, B), _dev(ca, xyyaw))
    rollout(ca, pa, 130)
    pa.contact()["drop"].fill_(0.25)                        # (few feet are late at any one tick: every drop is seen to go)
    before = _snap4(pa, B)
    assert before["early"].all() and (before["slip"] > 0).sum() > B // 2 and before["late"].any()
    mask = np.arange(B) % 3 == 0
    pa.reset(_dev(ca, mask), _dev(ca, xyyaw))
    after = _snap4(pa, B)
    assert pa.contact()["flags"] == 7
    for k in CONTACT_KEYS:
        assert not after[k][mask].any() and np.array_equal(after[k][~mask], before[k][~mask]), k
    for k in ("state", "foot", "support", "stance"):
        assert np.array_equal(after[k][~mask], before[k][~mask]), k
    assert (after["stance"][mask] == 1).all()
    rollout(ca, pa, 13)
    assert _snap4(pa, B)["early"][mask].any()
    for c, p in ((ca, pa), (cb, pb)):
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        p.init(DEFAULTS["mu"], 1, _dev(c, xyyaw))
    z = _snap4(pa, B)
    assert pa.contact()["flags"] == 0 and not any(z[k].any() for k in CONTACT_KEYS)
    rollout(ca, pa, 14)
    rollout(cb, pb, 14)
    _same(pa, pb, "after init")
    assert not any(_snap4(pa, B)[k].any() for k in CONTACT_KEYS)
    del rows
    ca.close()
    cb.close()


# ---- 4. graph ----------------------------------------------------------------------------------------------------------

def test_graph_replays_equal_eager_ticks():
    """Lockstep on stairs with all three flags on a slippery floor: a captured 13-tick block (replayed once by the
    capture) and one more replay equal 26 eager ticks bit for bit, counters and statistics included."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    out = {}
    for name, graph in (("eager", False), ("graph", True)):
        c, plant, (gait, vel, xyyaw) = _walk_pair(B)
        plant.init(0.15, 1, _dev(c, xyyaw))
        dev = _stand_on(c, plant, LC.rows_for(B, 0.04), xyyaw, clamp_swing=True, rebase_z=True)
        plant.set_contact(**ON)
        plant.reset(_all(c, B), _dev(c, xyyaw))
        plant.enable_stats()
        plant.reset_stats()
        rollout(c, plant, 117)                              # (into the walk: feet stub and slide by now)
        res = rollout(c, plant, 13, graph=graph)
        if graph:
            res["graph"].replay()
        else:
            rollout(c, plant, 13)
        snap = _snap4(plant, B)
        snap["effort"] = plant.effort.cpu().numpy().copy()
        snap.update({"stats_" + k: v for k, v in _stats(plant).items()})
        out[name] = snap
        del dev, res
        c.close()
    for k in out["eager"]:
        assert np.array_equal(out["eager"][k], out["graph"][k]), k
    g = out["graph"]
    assert (g["stats_n"] == 143).all() and g["early"].any() and g["late"].any() and (g["slip"] > 0).any()


# ---- 5. bad values -----------------------------------------------------------------------------------------------------

def test_bad_values_stay_inside_their_robot():
    """A NaN slope on robot 3, rise = inf on robot 11, and from the third tick on a NaN effort on robot 5 and an infinite
    one on robot 9: every other robot's plant state, terrain and contact views are those of a run without them, bit for
    bit."""
    B, bad = 16, [3, 5, 9, 11]
    good = np.setdiff1d(np.arange(B), bad)
    out = []
    for spoil in (False, True):
        c, plant, (gait, vel, xyyaw) = _walk_pair(B)
        rows = LC.rows_for(B, 0.04)
        if spoil:
            rows[3, 1] = np.nan
            rows[11, 3], rows[11, 4], rows[11, 5] = np.inf, 0.1, 4.0
        dev = _stand_on(c, plant, rows, xyyaw, clamp_swing=True, rebase_z=True)
        plant.set_contact(**ON)
        plant.reset(_all(c, B), _dev(c, xyyaw))
        for t in range(6):
            c.tick_state(plant.state, plant.motor, plant.effort)
            if spoil and t >= 2:
                plant.effort[5, 4] = float("nan")
                plant.effort[9, :] = float("inf")
            plant.step(plant.effort)
        out.append(_snap4(plant, B))
        del dev
        c.close()
    for k in out[0]:
        assert np.array_equal(out[0][k][good], out[1][k][good]), k
    for b in (3, 11):                                       # (a NaN torque gives fn > 0 false: no force, a finite robot)
        assert not np.isfinite(out[1]["state"][b]).all(), b
    assert not np.array_equal(out[0]["state"][[5, 9]], out[1]["state"][[5, 9]])
    assert np.isfinite(out[1]["state"][good]).all() and np.isfinite(out[0]["state"]).all()


# ---- 6. the fleet walks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LC.PATHS)
def test_the_fleet_walks_with_contact_decided_by_the_ground(mode, path):
    """The CPU yardstick's commands, four robots per command, on plant_loop_contact.walk_config(): the top walked stairs
    under all three flags on the top walked floor.  Every robot stays safe, no solve reports an error bit, the five
    statistics lie inside plant_loop.envelope() of the CPU run, and so do the counters by the same rule -- a command's own
    recorded value widened by twice its spread across the 16 commands.  Feet were early, late and slid somewhere."""
    reps = 4
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_contact_closed_loop_cpu.json")))
    rec = gold[f"mode{mode}"][path]
    ticks = gold["ticks"]
    cfg = LC.walk_config()
    rows = LC.rows_for(B, cfg["rise"])
    assert gold["walk"]["config"] == cfg and np.array_equal(np.asarray(gold["walk"]["rows"]), rows[:L.N_CMD]) and ticks == LC.TICKS
    c, plant, (gait, vel, xyyaw) = _walk_pair(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None)
    assert np.array_equal(gold[f"mode{mode}"]["vel"], vel[:L.N_CMD]) and np.array_equal(gold[f"mode{mode}"]["gait"], gait[:L.N_CMD])
    plant.init(cfg["mu"], 1, _dev(c, xyyaw))
    dev = _stand_on(c, plant, rows, xyyaw, clamp_swing=True, rebase_z=path == "state")
    plant.set_contact(early=bool(cfg["flags"] & 1), late=bool(cfg["flags"] & 2), slip=bool(cfg["flags"] & 4))
    plant.reset(_all(c, B), _dev(c, xyyaw))
    plant.enable_stats()
    plant.reset_stats()
    start, mid, end = G.ground_walk(c, plant, path, mode, ticks, gold["seed"], gold["settle"])
    G.assert_inside_envelope(G.stats_from_accumulators(start, mid, end), rec, reps, f"mode {mode} {path}")
    got = _snap4(plant, B)
    for k in ("early", "late", "slip"):
        v = np.asarray(rec[k], np.float64)
        spread = 2.0 * (v.max() - v.min())
        want = np.tile(v, reps)
        print(f"mode {mode} {path} {k}: largest distance from the CPU run {np.abs(got[k] - want).max():.3e}, allowed {spread:.3e}")
        assert got[k].any() and (np.abs(got[k] - want) <= spread).all(), (k, got[k], want, spread)
    del dev
    c.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, ContactParams, ContactView
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    v = ContactView()
    prm = lambda *a: C.byref(ContactParams(*a))
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_set_contact(h, B, prm(7, 1.0, 0.01, 1.0)) == STATE          # before qmpc_plant_init
    assert lib.qmpc_contact_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_plant_set_contact(None, B, prm(7, 1.0, 0.01, 1.0)) == ARG
    assert lib.qmpc_plant_set_contact(h, B + 1, prm(7, 1.0, 0.01, 1.0)) == ARG        # a foreign batch
    assert lib.qmpc_plant_set_contact(h, B, prm(8, 1.0, 0.01, 1.0)) == ARG            # unknown flag bits
    assert lib.qmpc_plant_set_contact(h, B, prm(-1, 1.0, 0.01, 1.0)) == ARG
    for bad in (-1.0, float("nan"), float("inf")):
        for k in range(3):
            a = [1.0, 0.01, 1.0]
            a[k] = bad
            assert lib.qmpc_plant_set_contact(h, B, prm(7, *a)) == ARG, (bad, k)
    assert lib.qmpc_contact_view_get(h, None) == ARG
    assert lib.qmpc_contact_view_get(h, C.byref(v)) == OK and (v.params.flags, v.batch) == (0, B)
    assert lib.qmpc_plant_set_contact(h, B, prm(5, 0.0, 0.0, 0.0)) == OK              # zeros are values
    assert lib.qmpc_contact_view_get(h, C.byref(v)) == OK and v.params.flags == 5 and v.params.drop_speed == 0.0
    assert v.early and v.late and v.slip and v.drop
    assert lib.qmpc_plant_set_contact(h, B, None) == OK                               # off
    assert lib.qmpc_contact_view_get(h, C.byref(v)) == OK and v.params.flags == 0
    assert lib.qmpc_plant_set_contact(h, B, prm(0, -1.0, 0.01, 1.0)) == OK            # flags 0: off, nothing else is read
    # contact stays a call of its own: the terrain's flags know nothing of it
    rows = torch.zeros((B, 8), dtype=torch.float64, device=c.device)
    assert lib.qmpc_plant_set_terrain(h, B, rows.data_ptr(), 4) == ARG
    torch.cuda.synchronize()
    c.close()
