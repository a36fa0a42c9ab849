"""GPU suite (-m gpu) for height-field terrain from memory (include/qmpc_field.h; BatchedPlant.set_field / field).

The kernels of csrc/qmpc_field.hip are compared with tests/plant_model_field.py at tests/test_gpu_plant.py's tolerance,
1e-10 relative to max(1, |x|): the terrain / contact step's arithmetic plus a few dozen fp64 operations, with every
floor() argument kept 1e-6 cells away from an integer and every comparison 1e-6 (relative) away from a tie by the case
(tests/field_cases.py); flags and counters are compared exactly.  The walks at plant_loop_field.RUNGS are held to the CPU
loops' recorded statistics (tests/golden/plant_field_closed_loop_cpu.json) by plant_loop.envelope(); everything else
compares two runs of the library bit for bit.  The shared helpers and the walk are tests/fleet_gpu.py's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import field_cases as FC
import fleet_gpu as G
import plant_loop as L
import plant_loop_field as LF
import plant_loop_terrain as LT
import plant_model_varied as PV
from plant_cases import DEFAULTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_pair, _dev, _snap, _close, _same = G.pair, G.dev, G.snap, G.close, G.same
_stats, _all, _walk_pair = G.plant_stats, G.all_robots, G.walk_pair
_snap4, CONTACT_KEYS, ON = G.snap4, G.CONTACT_KEYS, G.ON


def _start_field(c, plant, case, contact):
    """The case's state on the device; terrain, field and contact bound as field_cases.model binds them -> what must
    stay referenced."""
    m0, rows, z, place, cell, old, new, tau, cs, pd, vd = case
    G.start(c, plant, m0, cs, pd, vd)
    keep = [_dev(c, z), _dev(c, place)]
    if rows is not None:
        keep.append(_dev(c, rows))
        plant.set_terrain(keep[-1], clamp_swing=True, rebase_z=False)
    plant.terrain()["support"].copy_(_dev(c, m0.support))
    plant.set_field(keep[0], keep[1], cell, clamp_swing=rows is None, rebase_z=True)
    if contact:
        plant.set_contact(True, True, True, **FC.PARAMS)
        v = plant.contact()
        for k in CONTACT_KEYS:
            v[k].copy_(_dev(c, getattr(m0, k)))
    return keep


def _run_case(case, substeps, vary, stats, contact, dyadic=False, z=None):
    """One step of the case on the device -> (snapshot, the model after its step)."""
    B = FC.B
    vals = FC.values(1000 + substeps) if vary else None
    m = FC.stepped(case, substeps, vals, contact)
    FC.check(case, m, dyadic)
    if z is not None:
        case = case[:2] + (z,) + case[3:]
    c, plant = _pair(B, substeps=substeps)
    keep = _start_field(c, plant, case, contact)
    var = {k: _dev(c, v) for k, v in (vals or {}).items()}
    if vary:
        plant.set_params(**var)
    if stats:
        plant.enable_stats()
        plant.reset_stats()
    f = plant.field()
    assert f["bound"] and (f["nx"], f["ny"], f["count"], f["cell"]) == (FC.NX, FC.NY, FC.COUNT, case[4]) and f["z"] is keep[0]
    assert f["flags"] == (3 if case[1] is None else 2) and plant.terrain()["flags"] == (0 if case[1] is None else 1)
    plant.step(_dev(c, case[7].reshape(B, 12)))
    s = _snap4(plant, B)
    if stats:
        s["stats"] = _stats(plant)
    del keep, var
    c.close()
    return s, m


def _compare_field(s, m, what, contact):
    (G.compare_contact if contact else G.compare_terrain)(s, m, what)


# ---- 1. single-step parity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("vary,stats", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("contact", [False, True])
def test_single_step_parity(substeps, vary, stats, contact):
    """tests/field_cases.py: B = 37, a bank of 3 maps of 7 x 5 samples on 0.11 m cells over slope and stairs; feet inside
    cells and off each of the four edges, map indices 0, count - 1 and a fractional one, zs negative and 0 -- with
    scheduled contact (flags 0) and with all three contact flags (7), in all four <VARY, STATS> instantiations.  grf is
    the witness of the per-foot normal.  The case's own promises are asserted on the model."""
    case = FC.parity_case(substeps)
    s, m = _run_case(case, substeps, vary, stats, contact)
    _compare_field(s, m, f"substeps {substeps} vary {vary} stats {stats} contact {contact}", contact)
    assert np.array_equal(s["state"][:, 6], s["p"][:, 2] - s["support"]) and np.abs(s["support"]).max() > 0.01
    if stats:
        for k in PV.STAT_KEYS[1:]:
            _close(s["stats"][k], m.stats[k], f"statistics {k}")
        assert (s["stats"]["n"] == 1).all() and np.array_equal(s["stats"]["z_min"], s["state"][:, 6])


@pytest.mark.parametrize("contact", [False, True])
@pytest.mark.parametrize("bound,dyadic", [(False, False), (True, True)])
def test_single_step_parity_field_alone_and_on_grid_lines(contact, bound, dyadic):
    """The field with no terrain rows bound (a null rows pointer: the analytic term is 0, both flags ride on the field's
    binding), and the sub-case whose pinned feet stand exactly on grid lines (cell 2^-3, origins on multiples of 2^-6: u
    and v are integers exactly, in the model and on the device)."""
    case = FC.parity_case(1, bound, dyadic)
    s, m = _run_case(case, 1, False, False, contact, dyadic)
    _compare_field(s, m, f"bound {bound} dyadic {dyadic} contact {contact}", contact)


# ---- 2. the parity cannot pass without the feature ---------------------------------------------------------------------

@pytest.mark.parametrize("contact", [False, True])
def test_a_zero_bank_moves_the_case_far_beyond_the_tolerance(contact):
    """The same case with the bank replaced by zeros ON THE DEVICE: state, foot and grf leave the model (which keeps the
    bank) by more than 1e-4 -- six orders above the parity's tolerance."""
    case = FC.parity_case(1)
    s, m = _run_case(case, 1, False, False, contact, z=np.zeros_like(case[2]))
    for k in ("state", "foot", "grf"):
        moved = float(np.abs(s[k].reshape(FC.B, -1) - getattr(m, k).reshape(FC.B, -1)).max())
        print(f"contact {contact} {k}: a zero bank moves it by {moved:.3e}")
        assert moved > 1e-4, (k, moved)


# ---- 3. neutrality -----------------------------------------------------------------------------------------------------

def _zero_bank(c, B):
    rng = np.random.default_rng(5)
    place = np.stack([rng.integers(0, 2, B).astype(float), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B),
                      rng.uniform(-2, 2, B)], 1)
    return _dev(c, np.zeros((2, 9, 11), f32)), _dev(c, place)


@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
@pytest.mark.parametrize("ground", ["flat", "terrain", "contact", "terrain+contact"])
def test_zero_bank_changes_no_bit(schedule, ground):
    """39 closed-loop ticks (tick_state -> step) with a bank of all-zero samples bound under flags 0 and lively
    placements, against the same plant without the field: no bit of any output differs -- on flat ground, on slopes and
    stairs, and with contact decided by the ground.  The reset on the field is the other reset, bit for bit, too."""
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    ca, pa, (gait, vel, xyyaw) = _walk_pair(B, schedule)
    cb, pb, _ = _walk_pair(B, schedule)
    keep = [_zero_bank(ca, B)]
    pa.set_field(keep[0][0], keep[0][1], 0.07)
    for c, p in ((ca, pa), (cb, pb)):
        if "terrain" in ground:
            keep.append(_dev(c, LT.terrain(B)))
            p.set_terrain(keep[-1], clamp_swing=True, rebase_z=True)
        if "contact" in ground:
            p.set_contact(**ON)
        p.reset(_all(c, B), _dev(c, xyyaw))
    assert pa.field()["bound"] and not pb.field()["bound"]

    def same(what):
        _same(pa, pb, what)
        sa, sb = _snap4(pa, B), _snap4(pb, B)
        for k in ("grf", "ground", "support") + CONTACT_KEYS:
            assert np.array_equal(sa[k], sb[k]), (what, k)
        return sa

    same("reset")
    for n in (13, 26):
        rollout(ca, pa, n)
        rollout(cb, pb, n)
        sa = same(f"{n} ticks")
    assert np.abs(sa["grf"]).max() > 10 and np.abs(pa.effort.cpu().numpy()).max() > 1.0
    assert ("contact" in ground) == bool(sa["early"].any())
    del keep
    ca.close()
    cb.close()


# ---- 4. graph ----------------------------------------------------------------------------------------------------------

def _walk_on_field(B, kind, path="state", mode=0, amp=None, schedule=None):
    """A fleet standing on plant_loop_field.field_for(B, amp) -> (c, plant, what must stay referenced, commands)."""
    c, plant, cmds = _walk_pair(B, schedule or ("per_robot" if mode == 1 else "lockstep"), mode if mode == 1 else None)
    z, place, cell = LF.field_for(B, LF.RUNGS[kind] if amp is None else amp)
    keep = [_dev(c, z), _dev(c, place)]
    plant.set_field(keep[0], keep[1], cell, clamp_swing=True, rebase_z=path == "state")
    fl = LF.contact_flags(kind)
    plant.set_contact(early=bool(fl & 1), late=bool(fl & 2), slip=bool(fl & 4))
    plant.reset(_all(c, B), _dev(c, cmds[2]))
    return c, plant, keep, cmds


def test_graph_replays_equal_eager_ticks_with_the_ground_rewritten_between_them():
    """13 captured ticks of tick_state -> step (replayed once by the capture); then robot 3's place row is rewritten to
    move it to another map and the samples around robot 6's foot are raised, in place; one more replay.  Equal, bit for bit,
    to 13 eager ticks, the same edits, 13 more: the pointers are captured, the values are not."""
    import torch
    from quadruped_ctrl_amd.binding import rollout
    B = 16
    out = {}
    for name, graph in (("eager", False), ("graph", True)):
        c, plant, keep, cmds = _walk_on_field(B, "contact", amp=0.04)
        z2 = torch.cat([keep[0], keep[0].flip(2)]).contiguous()          # a bank of two maps
        plant.set_field(z2, keep[1], LF.CELL, clamp_swing=True, rebase_z=True)
        plant.reset(_all(c, B), _dev(c, cmds[2]))
        rollout(c, plant, 117)                                           # (into the walk)
        res = rollout(c, plant, 13, graph=graph)
        foot = plant.view()["foot"][6].cpu().numpy().reshape(4, 3)
        i, j = np.floor((foot[0, :2] - keep[1][6, 1:3].cpu().numpy()) / LF.CELL).astype(int)
        mid = _snap(plant)["state"].copy()
        keep[1][3, 0] = 1.0
        z2[0, j - 4:j + 5, i - 4:i + 5] += 0.03                          # (0.4 m square: the next swing foot meets it)
        if graph:
            res["graph"].replay()
        else:
            rollout(c, plant, 13)
        snap = _snap4(plant, B)
        snap["effort"], snap["mid"] = plant.effort.cpu().numpy().copy(), mid
        out[name] = snap
        del keep, res, z2
        c.close()
    for k in out["eager"]:
        assert np.array_equal(out["eager"][k], out["graph"][k]), k
    # ... and the edits were felt: the same walk without them ends elsewhere for robots 3 and 6 and nowhere else
    c, plant, keep, cmds = _walk_on_field(B, "contact", amp=0.04)
    z2 = torch.cat([keep[0], keep[0].flip(2)]).contiguous()
    plant.set_field(z2, keep[1], LF.CELL, clamp_swing=True, rebase_z=True)
    plant.reset(_all(c, B), _dev(c, cmds[2]))
    rollout(c, plant, 143)
    plain = _snap4(plant, B)
    c.close()
    differs = (plain["state"] != out["graph"]["state"]).any(1) | (plain["ground"] != out["graph"]["ground"])
    assert differs[3] and differs[6] and not differs[np.setdiff1d(np.arange(B), [3, 6])].any(), np.flatnonzero(differs)


# ---- 5. bad values -----------------------------------------------------------------------------------------------------

def test_bad_values_stay_inside_their_robot():
    """Place rows with NaN, +-inf and 1e300 origins and scales and map indices -5, 1e9 and NaN (the index logic clamps
    them: tests/test_field_cpu.py holds that on the CPU): every other robot's plant state, terrain and contact views are
    those of a run without those rows, bit for bit, and a bad map index alone is a clamped index, not a bad robot."""
    from quadruped_ctrl_amd.binding import rollout
    B = 16
    spoiled = {1: (0.0, np.nan, 0.0, 1.0), 3: (0.0, 0.0, np.inf, 1.0), 4: (0.0, -np.inf, 0.0, 1.0), 6: (0.0, 1e300, -1e300, 1.0),
               8: (0.0, 0.0, 0.0, np.nan), 9: (0.0, 0.0, 0.0, np.inf), 11: (-5.0, None, None, 1.0), 12: (1e9, None, None, 1.0),
               14: (np.nan, None, None, 1.0)}
    good = np.setdiff1d(np.arange(B), list(spoiled))
    out = []
    for spoil in (False, True):
        c, plant, keep, (gait, vel, xyyaw) = _walk_on_field(B, "contact", amp=0.02)
        if spoil:
            place = keep[1].cpu().numpy().copy()
            for b, row in spoiled.items():
                place[b] = [place[b, k] if v is None else v for k, v in enumerate(row)]
            keep[1].copy_(_dev(c, place))
        plant.reset(_all(c, B), _dev(c, xyyaw))
        rollout(c, plant, 13)
        out.append(_snap4(plant, B))
        del keep
        c.close()
    for k in out[0]:
        assert np.array_equal(out[0][k][good], out[1][k][good]), k
    assert np.isfinite(out[0]["state"]).all() and np.isfinite(out[1]["state"][good]).all()
    for b in (11, 12, 14):                                   # one map in the bank: every index clamps to it
        assert np.array_equal(out[0]["state"][b], out[1]["state"][b]), b
    for b in (1, 3, 4, 6):                                   # a NaN origin lands on column 0, a far one on an edge sample:
        assert np.isfinite(out[1]["state"][b]).all(), b      # finite robots on another patch of ground
    assert not np.array_equal(out[0]["foot"][[1, 3, 4, 6]], out[1]["foot"][[1, 3, 4, 6]])
    for b in (8, 9):                                         # a NaN or infinite scale is a NaN or infinite ground
        assert not np.isfinite(out[1]["state"][b]).all(), b


# ---- 6. the fleet walks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", LF.KINDS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LF.PATHS)
def test_the_fleet_walks_on_the_field(kind, mode, path):
    """The CPU yardstick's commands, two robots per command, spread over one random_blocks map at
    plant_loop_field.RUNGS[kind] (amplitude 0 where no rung was walked): every robot stays safe, no solve reports an error
    bit, and the five statistics lie inside plant_loop.envelope() of the CPU run."""
    reps = 2
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_field_closed_loop_cpu.json")))
    rec = gold["walk"][kind][f"mode{mode}"][path]
    ticks = gold["ticks"]
    assert gold["rungs"] == LF.RUNGS and gold["walk"][kind]["amp"] == (LF.RUNGS[kind] or 0.0) and ticks == LF.TICKS
    c, plant, keep, (gait, vel, xyyaw) = _walk_on_field(B, kind, path, mode)
    assert np.array_equal(gold["walk"][kind][f"mode{mode}"]["vel"], vel[:L.N_CMD])
    assert np.array_equal(gold["walk"][kind][f"mode{mode}"]["gait"], gait[:L.N_CMD])
    assert np.array_equal(np.asarray(gold["place"]), keep[1].cpu().numpy()[:L.N_CMD])
    plant.enable_stats()
    plant.reset_stats()
    start, mid, end = G.ground_walk(c, plant, path, mode, ticks, gold["seed"], gold["settle"])
    G.assert_inside_envelope(G.stats_from_accumulators(start, mid, end), rec, reps, f"{kind} mode {mode} {path}")
    got = _snap4(plant, B)
    if LF.RUNGS[kind]:
        assert np.abs(got["support"]).max() > 1e-3            # the ground is felt
    assert bool(got["early"].any()) == (kind == "contact")
    del keep
    c.close()


# ---- 7. reset and errors -----------------------------------------------------------------------------------------------

def test_reset_keeps_the_binding_and_init_unbinds():
    """reset(mask) stands the masked robots on the summed surface -- the field over slope and stairs -- and leaves the
    others alone; init() unbinds, and the plant is the plain plant again, bit for bit.  With contact decided by the ground
    the masked reset is the model's too, counters included (fleet_gpu.masked_reset_is_the_models, which tests/test_gpu_contact.py runs on flat ground and on terrain)."""
    from quadruped_ctrl_amd.binding import rollout
    import plant_model_field as PF
    G.masked_reset_is_the_models("field")
    B = 32
    ca, pa, keep, (gait, vel, xyyaw) = _walk_on_field(B, "scheduled", amp=0.06)
    cb, pb, _ = _walk_pair(B)
    rows = LT.terrain(B)
    keep.append(_dev(ca, rows))
    pa.set_terrain(keep[-1], clamp_swing=True, rebase_z=False)
    rollout(ca, pa, 13)
    before = _snap4(pa, B)
    mask = np.arange(B) % 3 == 0
    pa.reset(_dev(ca, mask), _dev(ca, xyyaw))
    f = pa.field()
    assert f["bound"] and f["flags"] == 3 and (f["nx"], f["ny"], f["count"]) == (LF.N_MAP, LF.N_MAP, 1) and f["batch"] == B
    after = _snap4(pa, B)
    m = PF.FieldPlantModel(B, L.FREQ, DEFAULTS["mu"], 1, xyyaw)
    m.set_terrain(rows, clamp_swing=True)
    z, place, cell = LF.field_for(B, 0.06)
    m.set_field(z, place, cell, clamp_swing=True, rebase_z=True)
    m.reset(np.ones(B, bool), xyyaw)
    for k, mk in (("p", "p"), ("foot", "foot"), ("state", "state"), ("motor", "motor"), ("ground", "ground"), ("support", "support")):
        _close(after[k][mask], getattr(m, mk)[mask], f"reset {k}")
        assert np.array_equal(after[k][~mask], before[k][~mask]), k
    assert np.abs(after["foot"][mask][..., 2] - m.height(m.foot[..., 0], m.foot[..., 1])[mask]).max() < 1e-12
    assert np.abs(m.ground - PF.PT.TerrainPlantModel.height(m, xyyaw[:, 0], xyyaw[:, 1])).max() > 1e-3   # field + terrain
    assert np.array_equal(after["p"][mask][:, 2], 0.29 + after["ground"][mask]) and (after["stance"][mask] == 1).all()
    for c, p in ((ca, pa), (cb, pb)):
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        p.init(DEFAULTS["mu"], 1, _dev(c, xyyaw))
    f = pa.field()
    assert not f["bound"] and f["z"] is None and f["flags"] == 0 and not pa.terrain()["bound"]
    rollout(ca, pa, 14)
    rollout(cb, pb, 14)
    _same(pa, pb, "after init")
    pa.set_field(keep[0], keep[1], LF.CELL)
    assert pa.field()["bound"]
    pa.set_field(None)
    assert not pa.field()["bound"]
    rollout(ca, pa, 13)
    rollout(cb, pb, 13)
    _same(pa, pb, "after set_field(None)")
    del keep
    ca.close()
    cb.close()


def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant, FieldBank, FieldView, QmpcError
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    z = torch.zeros((2, 5, 7), dtype=torch.float32, device=c.device)
    place = torch.zeros((B, 4), dtype=torch.float64, device=c.device)
    bank = lambda zp=None, nx=7, ny=5, count=2, cell=0.1: C.byref(FieldBank(z.data_ptr() if zp is None else zp, nx, ny, count, cell))
    v = FieldView()
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_set_field(h, B, bank(), place.data_ptr(), 0) == STATE           # before qmpc_plant_init
    assert lib.qmpc_field_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_plant_set_field(None, B, bank(), place.data_ptr(), 0) == ARG
    assert lib.qmpc_plant_set_field(h, B + 1, bank(), place.data_ptr(), 0) == ARG          # a foreign batch
    for kw in (dict(nx=1), dict(ny=1), dict(count=0), dict(nx=-7), dict(cell=0.0), dict(cell=-0.1), dict(cell=float("nan")),
               dict(cell=float("inf")), dict(zp=0)):
        assert lib.qmpc_plant_set_field(h, B, bank(**kw), place.data_ptr(), 0) == ARG, kw
    assert lib.qmpc_plant_set_field(h, B, bank(), None, 0) == ARG                          # a null place
    assert lib.qmpc_plant_set_field(h, B, bank(), place.data_ptr(), 4) == ARG              # unknown flag bits
    assert lib.qmpc_plant_set_field(h, B, bank(), place.data_ptr(), -1) == ARG
    assert lib.qmpc_field_view_get(h, None) == ARG
    assert lib.qmpc_field_view_get(h, C.byref(v)) == OK and not v.bank.z and v.batch == B   # nothing of the above was bound
    assert lib.qmpc_plant_set_field(h, B, bank(nx=2, ny=2, count=1), place.data_ptr(), 3) == OK
    assert lib.qmpc_field_view_get(h, C.byref(v)) == OK
    assert (v.bank.z, v.bank.nx, v.bank.ny, v.bank.count, v.bank.cell, v.place, v.flags) == (z.data_ptr(), 2, 2, 1, 0.1, place.data_ptr(), 3)
    assert lib.qmpc_plant_set_field(h, B, None, None, 99) == OK                            # unbind: nothing else is read
    assert lib.qmpc_field_view_get(h, C.byref(v)) == OK and not v.bank.z and v.flags == 0
    # the binding checks what the C call cannot: dtype, layout, device, shape
    plant = BatchedPlant(c)
    with pytest.raises(QmpcError):
        plant.set_field(z, place, 0.1)                                                     # before init()
    plant.init()
    for bad_z in (z.double(), z[:, :, ::2], z[0], z.cpu()):
        with pytest.raises(QmpcError):
            plant.set_field(bad_z, place, 0.1)
    for bad_place in (place.float(), place[:, :3], place[:4], None):
        with pytest.raises(QmpcError):
            plant.set_field(z, bad_place, 0.1)
    with pytest.raises(QmpcError):
        plant.set_field(z, place)                                                          # no cell
    plant.set_field(z, place, 0.1, rebase_z=True)
    assert plant.field()["flags"] == 2 and plant.field()["place"] is place
    torch.cuda.synchronize()
    c.close()
