"""CPU suite for contact decided by the ground (include/qmpc_contact.h): the exported surface, the numpy restatement
tests/plant_model_contact.py at hand-computed points -- the model the GPU suite (tests/test_gpu_contact.py) holds the
kernels to --, the single-step case, the ladders' record and the CPU closed loop that the GPU walk is measured by, and
the compiled contact kernels' registers and scratch."""
import json
import math
import os
import re

import numpy as np
import pytest

import contact_cases as CC
import kernel_resources as KR
import plant_cases as PC
import plant_loop as L
import plant_loop_contact as LC
import plant_model as PM
import plant_model_contact as PCM
import plant_model_terrain as PT
import terrain_cases as TC
from c_headers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GOLD = os.path.join(ROOT, "tests", "golden", "plant_contact_closed_loop_cpu.json")


def _fields(hdr, struct):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
    return re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_contact_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_contact.h")).read()
    want = {"qmpc_plant_set_contact", "qmpc_contact_view_get"}
    assert declared("qmpc_contact.h") == want == set(binding.CONTACT_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    assert _fields(hdr, "qmpc_contact_view") == [n for n, _ in binding.ContactView._fields_]
    assert _fields(hdr, "qmpc_contact_params") == [n for n, _ in binding.ContactParams._fields_]
    assert re.search(r"QMPC_CONTACT_EARLY = 1, QMPC_CONTACT_LATE = 2, QMPC_CONTACT_SLIP = 4", hdr)
    assert (binding.CONTACT_EARLY, binding.CONTACT_LATE, binding.CONTACT_SLIP) == (PCM.EARLY, PCM.LATE, PCM.SLIP) == (1, 2, 4)
    # the older headers still declare exactly what they declared
    assert declared("qmpc_terrain.h") == {"qmpc_plant_set_terrain", "qmpc_terrain_view_get"} == set(binding.TERRAIN_EXPORTS)
    assert declared("qmpc_plant.h") == set(binding.PLANT_EXPORTS) and not want & (declared("qmpc_plant.h") | declared("qmpc_terrain.h"))
    # the binding's defaults are the header's
    import inspect
    d = {k: v.default for k, v in inspect.signature(binding.BatchedPlant.set_contact).parameters.items() if k != "self"}
    assert d == dict(early=False, late=False, slip=False, drop_speed=PCM.DROP_SPEED, slip_gain=PCM.SLIP_GAIN,
                     slip_vmax=PCM.SLIP_VMAX) and (PCM.DROP_SPEED, PCM.SLIP_GAIN, PCM.SLIP_VMAX) == (1.0, 0.01, 1.0)


# ---- the model at hand-computed points ---------------------------------------------------------------------------------

STAIRS = np.array([[0.0, 0.0, 0.0, 0.04, 0.2, 4.0, 0.1, 0.0]])       # the front feet (x = 0.19) stand on the first tread


def _one(rows=None, mu=0.4, **contact):
    m = PCM.ContactPlantModel(1, 500.0, mu, 1)
    m.set_terrain(rows)
    m.set_contact(**contact)
    m.reset(np.ones(1, bool))
    return m


def test_early_touch_down_pins_on_the_tread_and_releases_when_the_command_clears_it():
    """Foot 0 swings over the first tread (height 0.04) while the body falls freely (no torque: 4e-5 m in the first
    tick).  Commanded 5 mm below the tread it is pinned on it, at the commanded xy; it stays there, bit for bit, while
    the command stays below; it is released on the first tick the command is 5 mm above.  Without `early` it goes where
    it is told, through the tread."""
    cs = np.array([[0.0, 1.0, 1.0, 1.0]], f32)
    vd = np.zeros((1, 12), f32)

    def pd(dz):                                            # the stand pose, foot 0 ends dz above the tread (body at 0.29)
        out = PC.STAND.copy()
        out[0, 0], out[0, 2] = 0.01, -(0.29 - 0.04) + dz
        return out.reshape(1, 12).astype(f32)

    for early in (True, False):
        m = _one(STAIRS, early=early, late=True)
        assert np.array_equal(m.foot[0, :, 2], [0.04, 0.04, 0.0, 0.0]) and m.p[0, 2] == 0.29
        m.foot[0, 0, 2], m.stance[0, 0] = 0.08, False      # in the air
        m.step(np.zeros((1, 12)), cs, pd(-0.005), vd)
        want_xy = m.p[0, :2] + (PM.HIP[0, :2] + [f32(0.01), f32(PC.STAND[0, 1])])      # (the command is float32)
        assert np.abs(m.foot[0, 0, :2] - want_xy).max() < 1e-15
        if not early:
            assert not m.stance[0, 0] and abs(m.foot[0, 0, 2] - (0.035 - 9.81 * 0.002 ** 2)) < 1e-8 and m.early[0] == 0
            continue
        assert m.stance[0, 0] and m.foot[0, 0, 2] == 0.04 and m.early[0] == 1 and m.drop[0, 0] == 0
        held = m.foot[0, 0].copy()
        m.step(np.zeros((1, 12)), cs, pd(-0.005), vd)
        assert m.stance[0, 0] and np.array_equal(m.foot[0, 0], held) and m.early[0] == 2
        m.step(np.zeros((1, 12)), cs, pd(+0.005), vd)
        assert not m.stance[0, 0] and m.early[0] == 2 and 0.0445 < m.foot[0, 0, 2] < 0.045
        assert np.array_equal(m.stance[0, 1:], [True, True, True]) and m.late[0] == 0


def test_late_foot_lands_after_the_drop_has_covered_its_height():
    """Foot 1 is scheduled to stand 0.03 m above flat ground, its command is where it is, and the diagonal pair (feet 0
    and 3) carries the body with m g / 2 each, so the body stays put.  With drop_speed 0.9 m/s the foot is lowered 1.8 mm
    per tick and lands on tick ceil(0.03 / 0.0018) = 17, carrying nothing until then."""
    speed, up = 0.9, 0.03
    m = _one(None, late=True, drop_speed=speed)
    m.foot[0, 1, 2], m.stance[0, 1] = up, False
    f = np.zeros((1, 4, 3))
    f[0, [0, 3], 2] = m.mass * PM.GRAVITY / 2
    tau = PC.hold(m, f).reshape(1, 12)
    cs = np.ones((1, 4), f32)
    pd = (PM.mulT(PM.rot(m.q)[:, None, :], m.foot - m.p[:, None, :]) - PM.HIP).reshape(1, 12).astype(f32)
    vd = np.zeros((1, 12), f32)
    n = math.ceil(up / (speed * m.dt))
    assert n == 17
    for t in range(1, n + 1):
        m.step(tau, cs, pd, vd)
        assert (m.grf[0, 1] == 0).all() and abs(m.p[0, 2] - 0.29) < 1e-9
        if t < n:
            assert not m.stance[0, 1] and abs(m.drop[0, 1] - t * speed * m.dt) < 1e-15
            assert abs(m.foot[0, 1, 2] - (up - t * speed * m.dt)) < 1e-7 and m.late[0] == t
    assert m.stance[0, 1] and m.foot[0, 1, 2] == 0.0 and m.drop[0, 1] == 0.0 and m.late[0] == n and m.early[0] == 0
    # without `late` the schedule puts it down at once
    m = _one(None, early=True)
    m.foot[0, 1, 2], m.stance[0, 1] = up, False
    m.step(tau, cs, pd, vd)
    assert m.stance[0, 1] and m.foot[0, 1, 2] == 0.0 and m.late[0] == 0


def test_saturated_foot_slides_against_its_friction_and_an_unsaturated_one_does_not_move():
    mu, fz, gain = 0.4, 20.0, 0.01
    m = _one(None, mu=mu, slip=True, slip_gain=gain)
    f = np.zeros((1, 4, 3))
    f[0, :, 2] = fz
    f[0, 0, 0] = 2 * mu * fz                                # foot 0: twice the cone along +x
    f[0, 1:, 1] = 0.5 * mu * fz                             # the others: half of it
    tau = PC.hold(m, f).reshape(1, 12)
    before = m.foot.copy()
    cs, (_, pd, vd) = np.ones((1, 4), f32), PC.none(1)
    m.step(tau, cs, pd, vd)
    want = m.h * gain * (2 * mu * fz - mu * fz)             # 0.002 * 0.01 * 8 N = 0.16 mm
    assert abs((m.foot[0, 0, 0] - before[0, 0, 0]) + want) < 1e-13 and abs(m.foot[0, 0, 1] - before[0, 0, 1]) < 1e-15
    assert m.foot[0, 0, 2] == 0.0 and np.array_equal(m.foot[0, 1:], before[0, 1:])
    assert abs(m.slip[0] - want) < 1e-13 and abs(m.grf[0, 0, 0] - mu * fz) < 1e-10 and m.stance.all()
    # the speed's cap; and without the flag the foot stays
    m = _one(None, mu=mu, slip=True, slip_gain=gain, slip_vmax=0.05)
    m.step(tau, cs, pd, vd)
    assert abs(m.slip[0] - m.h * 0.05) < 1e-18 and abs((m.foot[0, 0, 0] - before[0, 0, 0]) + m.h * 0.05) < 1e-15
    m = _one(None, mu=mu, early=True, late=True)
    m.step(tau, cs, pd, vd)
    assert np.array_equal(m.foot, before) and m.slip[0] == 0.0


@pytest.mark.parametrize("substeps", [1, 4])
def test_flags_zero_is_the_terrain_plant_bit_for_bit(substeps):
    m0, rows, old, new, tau, cs, pd, vd = TC.parity_case(substeps)
    mt = TC.model(substeps, rows, TC.values(7), src=m0)
    mc = PCM.ContactPlantModel(TC.B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps, rows=rows, clamp_swing=True,
                               rebase_z=True, **{k + ("_b" if k in ("mass", "ibody", "mu") else ""): v
                                                 for k, v in TC.values(7).items()})
    mc.set_contact(drop_speed=3.0, slip_gain=5.0, slip_vmax=7.0)          # every flag False
    for k in ("p", "v", "q", "w", "foot", "stance", "support", "ground"):
        setattr(mc, k, getattr(m0, k).copy())
    for m in (mt, mc):
        m.step(tau.reshape(TC.B, 12), cs, pd, vd)
    for k in ("p", "v", "q", "w", "foot", "grf", "stance", "state", "motor", "support", "ground"):
        assert np.array_equal(getattr(mt, k), getattr(mc, k)), k
    assert not mc.early.any() and not mc.late.any() and not mc.slip.any() and not mc.drop.any()


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("vary", [False, True])
def test_single_step_case_holds_what_it_promises(substeps, vary):
    """tests/contact_cases.py, which the GPU suite compares the kernels on: every branch is taken and no comparison is
    within 1e-6 of a tie."""
    case = CC.parity_case(substeps)
    after = CC.stepped(case, substeps, CC.values(1000 + substeps) if vary else None)
    CC.check(case, after)
    assert np.isfinite(after.state).all() and np.isfinite(after.motor).all()


def test_every_flag_and_every_parameter_moves_the_case():
    for what, moved in CC.sensitivity(1).items():
        assert moved > 1e-6, (what, moved)


# ---- the ladders and the closed loop ------------------------------------------------------------------------------------

def test_rungs_are_the_record():
    gold = json.load(open(GOLD))
    assert gold["rungs"] == LC.RUNGS and gold["ticks"] == LC.TICKS and gold["run"] == LC.RUN
    for name, lad in (("flat", (True,)), ("stairs", LC.STAIRS_LADDER), ("friction", LC.FRICTION_LADDER)):
        rec = gold["ladders"][name]
        assert rec["rungs"] == list(lad)
        walked = [w["rung"] for w in rec["walked"]]
        assert walked == list(lad[:len(walked)]) and all(w["walked"] for w in rec["walked"])   # a ladder ends at its first fall
        assert (walked[-1] if walked else None) == LC.RUNGS[name]
        assert len(walked) + (rec["fell"] is not None) + len(rec["beyond"]) == len(lad)
        if rec["fell"] is not None:
            assert rec["fell"]["rung"] == lad[len(walked)] and not rec["fell"]["walked"]
            assert any(r["fallen"] for r in rec["fell"]["runs"].values())
    assert gold["walk"]["config"] == LC.walk_config()
    assert np.array_equal(gold["walk"]["rows"], LC.rows_for(L.N_CMD, LC.RUNGS["stairs"]))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LC.PATHS)
def test_cpu_closed_loop_with_contact_is_safe_and_is_what_the_fixture_records(mode, path):
    """The reference pipeline keeps every robot safe on walk_config() -- the top walked stairs under all three flags on the
    top walked floor --, with every qpOASES return code 0 and nWSR < 100, and the statistics and the counters are the
    fixture's (1e-6, as the other closed-loop fixtures)."""
    gold = json.load(open(GOLD))
    stats, info = LC.cpu_loop_contact(mode, path)
    rec = gold[f"mode{mode}"]
    gait, vel, xyyaw = L.commands(mode)
    assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
    assert (info["safe"] == 1).all() and (info["rc_bad"] == 0).all() and (info["nwsr_max"] < 100).all(), (mode, path, info)
    for k in L.STATS:
        assert np.abs(stats[k] - np.asarray(rec[path][k])).max() < 1e-6, (mode, path, k)
    assert np.abs(info["travel"] - np.asarray(rec[path]["travel"])).max() < 1e-6
    assert np.array_equal(info["early"], rec[path]["early"]) and np.array_equal(info["late"], rec[path]["late"])
    assert np.abs(info["slip"] - np.asarray(rec[path]["slip"])).max() < 1e-6
    assert info["early"].any() and info["late"].any() and (info["slip"] > 0).any()


# ---- the kernels --------------------------------------------------------------------------------------------------------

# profiles/plant_kernel_resources.txt, qmpc_contact.hip:  VGPRs, AGPRs, SGPR spills, VGPR spills, waves per SIMD
CONTACT_TABLE = {"qmpc_contact_reset_kernel": (10, 0, 0, 0, 8),
                 "qmpc_contact_step_kernelILb0ELb0E": (249, 0, 30, 0, 1), "qmpc_contact_step_kernelILb0ELb1E": (249, 0, 30, 0, 1),
                 "qmpc_contact_step_kernelILb1ELb0E": (256, 11, 59, 0, 1), "qmpc_contact_step_kernelILb1ELb1E": (256, 11, 59, 0, 1)}


@KR.no_hipcc
def test_contact_kernel_resources(tmp_path):
    """The four <VARY, STATS> instantiations of the contact step and the counters' reset compile for gfx950 without
    scratch, without spills to memory and without LDS, and within their rows of profiles/plant_kernel_resources.txt."""
    res = KR.kernel_resources("qmpc_contact.hip", tmp_path)
    assert len(res) == 5 and sum("qmpc_contact_step_kernel" in k for k in res) == 4, sorted(res)
    assert all(v["vgpr_spill"] == 0 for v in res.values()), res
    KR.hold(res, CONTACT_TABLE)
