"""CPU suite for the plant's per-robot terrain (include/qmpc_terrain.h): the exported surface, the numpy restatement
tests/plant_model_terrain.py on what it must reproduce -- the model the GPU suite (tests/test_gpu_terrain.py) holds the
kernels to --, the CPU closed loops on slopes and stairs that the GPU walk is measured by, and the compiled terrain
kernels' registers and scratch."""
import json
import os
import re

import numpy as np
import pytest

import kernel_resources as KR
import plant_cases as PC
import plant_loop as L
import plant_loop_terrain as LT
import plant_model as PM
import plant_model_terrain as PT
import plant_model_varied as PV
import terrain_cases as TC
from c_headers import declared
from plant_cases import none as _none

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MODEL_KEYS = ("p", "v", "q", "w", "foot", "grf", "stance", "state", "motor")


def test_terrain_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_terrain.h")).read()
    want = {"qmpc_plant_set_terrain", "qmpc_terrain_view_get"}
    assert declared("qmpc_terrain.h") == want == set(binding.TERRAIN_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    body = re.search(r"typedef struct \{([^}]*)\} qmpc_terrain_view;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in binding.TerrainView._fields_]
    assert re.search(r"QMPC_TERRAIN_CLAMP_SWING = 1, QMPC_TERRAIN_REBASE_Z = 2", hdr)
    assert (binding.TERRAIN_CLAMP_SWING, binding.TERRAIN_REBASE_Z) == (PT.CLAMP_SWING, PT.REBASE_Z) == (1, 2)
    # the two older headers still declare exactly what they declared
    assert declared("qmpc_plant.h") == {"qmpc_plant_init", "qmpc_plant_reset", "qmpc_plant_step", "qmpc_plant_view_get"} \
        == set(binding.PLANT_EXPORTS)
    assert declared("qmpc_plant_vary.h") == {"qmpc_plant_set_params", "qmpc_plant_stats_enable", "qmpc_plant_stats_reset",
                                          "qmpc_plant_stats_get"} == set(binding.PLANT_VARY_EXPORTS)
    assert not want & (declared("qmpc_plant.h") | declared("qmpc_plant_vary.h"))


@pytest.mark.parametrize("substeps", [1, 4])
def test_zero_rows_without_flags_are_bit_neutral(substeps):
    """An all-zero row under flags = 0: VariedPlantModel bit for bit on the single-step case (every stance pattern,
    saturated cones, pulling legs, a straight knee), with the statistics."""
    B, m, old, new, tau, cs, pd, vd = PC.parity_case(substeps)
    keep = {k: getattr(m, k).copy() for k in ("p", "v", "q", "w", "foot", "stance")}
    mv = PV.VariedPlantModel(B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps)
    mt = PT.TerrainPlantModel(B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps, rows=np.zeros((B, 8)))
    for mm in (mv, mt):
        for k, val in keep.items():
            setattr(mm, k, val.copy())
        mm.step(tau.reshape(B, 12), cs, pd, vd)
    for k in MODEL_KEYS:
        assert np.array_equal(getattr(mv, k), getattr(mt, k)), k
    for k in PV.STAT_KEYS:
        assert np.array_equal(mv.stats[k], mt.stats[k]), k
    assert np.abs(mt.grf).max() > 1 and np.array_equal(mt.ground, np.zeros(B))
    # ... and re-basing on feet that stand at 0 changes nothing either
    mr = PT.TerrainPlantModel(B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps, rows=np.zeros((B, 8)), rebase_z=True)
    for k, val in keep.items():
        setattr(mr, k, val.copy())
    mr.step(tau.reshape(B, 12), cs, pd, vd)
    assert np.array_equal(mr.state, mv.state)


def test_height_at_hand_computed_points():
    """Robot 0: plane 0.5 + 0.1 x - 0.2 y with 3 treads of 0.25 x 0.04 from abscissa 1.0 along +x; robot 1: 4 treads
    down along heading 90 degrees; robot 2: count 0; robot 3: run 0 with count 4 (no flight); robot 4: a plane alone."""
    rows = np.array([[0.5, 0.1, -0.2, 0.04, 0.25, 3, 1.0, 0.0],
                     [0.0, 0.0, 0.0, -0.03, 0.1, 4, -0.2, np.pi / 2],
                     [0.1, 0.0, 0.0, 0.05, 0.2, 0, 0.0, 0.0],
                     [0.1, 0.0, 0.0, 0.05, 0.0, 4, 0.0, 0.0],
                     [-1.0, 0.25, 0.5, 0.0, 0.0, 0, 0.0, 0.0]])
    m = PT.TerrainPlantModel(5, rows=rows)
    # x of robot 0: before the flight, on treads 1, 2 and 3 (the last), beyond it
    for x, k in ((0.0, 0), (0.99, 0), (1.01, 1), (1.3, 2), (1.6, 3), (1.74, 3), (1.76, 3), (5.0, 3)):
        h = m.height(np.full(5, x), np.full(5, 2.0))
        assert abs(h[0] - (0.5 + 0.1 * x - 0.2 * 2.0 + 0.04 * k)) < 1e-15, (x, k)
        assert h[2] == 0.1 and h[3] == 0.1 and abs(h[4] - (-1.0 + 0.25 * x + 1.0)) < 1e-15
    for y, k in ((-0.5, 0), (-0.21, 0), (-0.19, 1), (-0.05, 2), (0.05, 3), (0.15, 4), (0.25, 4), (9.0, 4)):
        h = m.height(np.full(5, 7.0), np.full(5, y))
        assert abs(h[1] - (-0.03 * k)) < 1e-15, (y, k)
    # [B, 4] feet broadcast against [B] rows
    x = np.tile([[0.0, 1.1, 1.3, 9.0]], (5, 1))
    assert np.allclose(m.height(x, np.zeros((5, 4)))[0], [0.5, 0.61 + 0.04, 0.63 + 0.08, 1.4 + 0.12], atol=1e-15)
    n = m.normal()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15 and np.allclose(n[4] * np.sqrt(1 + 0.0625 + 0.25), [-0.25, -0.5, 1])


def test_friction_cone_about_the_contact_normal():
    """On slopes, a tangential demand beyond the cone lands on the cone about n, |t| = mu fn, in the demanded direction
    with the normal part kept; an unsaturated force is left untouched, bit for bit; a pulling leg gets nothing."""
    B = 4
    rows = np.zeros((B, 8))
    rows[:, 1], rows[:, 2] = [0.2, -0.3, 0.0, 0.15], [-0.1, 0.0, 0.25, 0.15]
    mu = np.array([0.0, 0.3, 0.4, 0.9])
    xy = np.array([[0, 0, 0.0], [1, 2, 0.7], [-1, 0.5, -2.0], [0.3, 0.3, 3.0]])
    _, pd, vd = _none(B)
    cs = np.ones((B, 4), f32)

    def plant(mu_b):
        pl = PT.TerrainPlantModel(B, 500.0, 0.4, 1, xy, mu_b=mu_b)
        pl.set_terrain(rows)
        pl.reset(np.ones(B, bool), xy)
        return pl

    pl = plant(mu)
    n = pl.normal()[:, None, :]
    e1 = np.cross(n, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)                  # a unit tangent
    fn = 20.0
    for scale, saturated in ((3.0, True), (0.5, False)):
        f = fn * n + (scale * np.maximum(mu, 0.05)[:, None, None] * fn) * e1 * np.ones((B, 4, 1))
        pl = plant(mu)
        tau = PC.hold(pl, f)
        pl.step(tau.reshape(B, 12), cs, pd, vd)
        g = pl.grf
        gn = (g * n).sum(-1)
        t = g - gn[..., None] * n
        assert np.abs(gn - fn).max() < 1e-10
        if saturated:
            assert np.abs(np.linalg.norm(t, axis=-1) - mu[:, None] * gn).max() < 1e-12
            assert np.abs(np.cross(t[1:], np.broadcast_to(e1, t.shape)[1:])).max() < 1e-10       # in the demanded direction
            assert np.abs(t[0]).max() < 1e-14                                        # mu = 0: along the normal alone
        else:
            free = plant(np.full(B, 100.0))
            free.step(tau.reshape(B, 12), cs, pd, vd)
            assert np.array_equal(g[1:], free.grf[1:]) and np.abs(g[1:] - f[1:]).max() < 1e-10
    pl = plant(mu)
    pl.step(PC.hold(pl, -fn * n * np.ones((B, 4, 1))).reshape(B, 12), cs, pd, vd)
    assert np.array_equal(pl.grf, np.zeros((B, 4, 3)))


def test_reset_stands_on_the_surface_and_support_survives_a_flight_phase():
    B = 16
    xy = L.commands(0)[2]
    rungs = dict(stairs_up=(0.1, 0.04), cross_slope=0.15, stairs_down=(0.1, 0.04), uphill=0.15)
    rows = LT.terrain(B, rungs)
    pl = PT.TerrainPlantModel(B, 500.0, 0.4, 1, xy)
    flat_foot = pl.foot.copy()
    assert np.array_equal(pl.foot[..., 2], np.zeros((B, 4))) and np.array_equal(pl.support, np.zeros(B))
    pl.set_terrain(rows, clamp_swing=True, rebase_z=True)
    mask = np.arange(B) % 3 != 1
    pl.reset(mask, xy)
    h = pl.height(pl.foot[..., 0], pl.foot[..., 1])
    assert np.array_equal(pl.foot[mask][..., 2], h[mask]) and np.array_equal(pl.foot[~mask], flat_foot[~mask])
    assert np.array_equal(pl.foot[..., :2], flat_foot[..., :2])
    assert np.array_equal(pl.p[mask, 2], (0.29 + pl.ground)[mask]) and np.array_equal(pl.ground[mask], pl.height(xy[:, 0], xy[:, 1])[mask])
    assert np.array_equal(pl.ground[~mask], np.zeros(B)[~mask]) and np.array_equal(pl.p[~mask, 2], np.full(B, 0.29)[~mask])
    c = pl.foot[..., 2]
    assert np.array_equal(pl.support[mask], (((c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])) / 4.0)[mask])
    assert np.array_equal(pl.state[mask, 6], (pl.p[:, 2] - pl.support)[mask]) and np.array_equal(pl.q[:, 1:3], np.zeros((B, 2)))
    # the front feet of the stairs' robots already stand on the first tread (0.19 m ahead, the flight starts at 0.10)
    up = np.arange(B) % 4 == 0
    assert np.allclose(c[up & mask][:, :2], 0.04) and np.allclose(c[up & mask][:, 2:], 0.0) and np.abs(c[(np.arange(B) % 4 == 3) & mask]).max() > 0.01
    # a flight phase: no foot in stance, support keeps its value; two feet back down: their mean
    pl.reset(np.ones(B, bool), xy)
    before = pl.support.copy()
    cs, pd, vd = _none(B)
    for _ in range(3):
        pl.step(np.zeros((B, 12)), cs, pd, vd)
        assert np.array_equal(pl.support, before)
    cs2 = cs.copy()
    cs2[:, [0, 3]] = 0.5
    pl.step(np.zeros((B, 12)), cs2, pd, vd)
    hz = pl.height(pl.foot[..., 0], pl.foot[..., 1])
    assert np.array_equal(pl.foot[:, [0, 3], 2], hz[:, [0, 3]])                     # touch-down on the surface
    assert np.array_equal(pl.support, (pl.foot[:, 0, 2] + pl.foot[:, 3, 2]) / 2.0) and not np.array_equal(pl.support, before)
    assert np.array_equal(pl.state[:, 6], pl.p[:, 2] - pl.support) and np.array_equal(pl.ground, pl.height(pl.p[:, 0], pl.p[:, 1]))
    # clamp_swing: the swing feet (commanded to the stand pose of a falling body) are nowhere below the surface
    assert (pl.foot[..., 2] >= hz).all()


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("vary", [False, True])
def test_single_step_case_holds_what_it_promises(substeps, vary):
    """tests/terrain_cases.py, which the GPU suite compares the kernels on: touch-down edges on several treads, swing feet
    lifted onto the surface, saturated cones, and no abscissa within 1e-6 tread depths of an edge -- no case is dropped."""
    case = TC.parity_case(substeps)
    m, rows, old, new, tau, cs, pd, vd = case
    after = TC.model(substeps, rows, TC.values(1000 + substeps) if vary else None, src=m)
    after.step(tau.reshape(TC.B, 12), cs, pd, vd)
    TC.check(case, after)
    assert np.isfinite(after.state).all() and np.isfinite(after.motor).all()
    # the terrain is felt: the same state on flat ground ends elsewhere
    flat = PV.VariedPlantModel(TC.B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps)
    for k in ("p", "v", "q", "w", "foot", "stance"):
        setattr(flat, k, getattr(m, k).copy())
    flat.step(tau.reshape(TC.B, 12), cs, pd, vd)
    assert np.abs(flat.state - after.state).max() > 1e-3


def test_terrain_is_the_stated_ground():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_terrain_closed_loop_cpu.json")))
    rungs = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gold["rungs"].items()}
    assert rungs == LT.RUNGS and gold["ticks"] == LT.TICKS <= 1300
    rows = LT.terrain(32)
    assert np.array_equal(rows[:16], gold["rows"]) and np.array_equal(rows[16:], rows[:16])
    xy = L.commands(0)[2]
    assert np.array_equal(xy, L.commands(1)[2])
    for k in range(16):
        z0, gx, gy, rise, run, count, s0, psi = rows[k]
        r = LT.RUNGS[LT.KINDS[k % 4]]
        if k % 4 in (0, 2) and r is not None:
            assert (run, abs(rise), count) == (r[0], r[1], 4) and (rise > 0) == (k % 4 == 0) and psi == xy[k, 2]
            assert abs(s0 - (xy[k, 0] * np.cos(psi) + xy[k, 1] * np.sin(psi) + 0.10)) < 1e-15 and gx == gy == z0 == 0
        else:
            assert (rise, run, count, s0, psi, z0) == (0, 0, 0, 0, 0, 0)
            assert (gx, gy) == ((0, r or 0) if k % 4 == 1 else (r or 0, 0)) if k % 4 in (1, 3) else (gx, gy) == (0, 0)
    # the reference's own 0.01 m stairs are among the walked rungs, and what fell is on record
    for name in ("stairs_up", "stairs_down"):
        assert [0.2, 0.01] in gold["walked"][name]
    for name, lad in LT.LADDERS.items():
        assert len(gold["walked"][name]) + len(gold["fell"][name]) == len(lad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LT.PATHS)
def test_cpu_closed_loop_on_terrain_is_safe_and_is_what_the_fixture_records(mode, path):
    """The reference pipeline keeps every robot safe on the walked rungs, with every qpOASES return code 0 and nWSR < 100,
    and the statistics are the fixture's (1e-6, as the other closed-loop fixtures)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_terrain_closed_loop_cpu.json")))
    stats, info = LT.cpu_loop_terrain(mode, path)
    rec = gold[f"mode{mode}"]
    gait, vel, xyyaw = L.commands(mode)
    assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
    assert (info["safe"] == 1).all() and (info["rc_bad"] == 0).all() and (info["nwsr_max"] < 100).all(), (mode, path, info)
    assert info["n_solves"] >= 16 * (LT.TICKS // 13 - 5)
    for k in L.STATS:
        print(mode, path, k, np.abs(stats[k] - np.asarray(rec[path][k])).max())
        assert np.abs(stats[k] - np.asarray(rec[path][k])).max() < 1e-6, (mode, path, k)
    assert np.abs(info["travel"] - np.asarray(rec[path]["travel"])).max() < 1e-6
    if path == "state":
        assert (stats["z_min"] > 0.2).all()             # re-based: the height above the stance feet
    # the fastest robots have left their flights, and somebody climbed: the support height moved by whole treads
    rows = info["rows"]
    stairs = rows[:, 5] > 0
    assert (np.abs(info["support"][stairs]) > 0).any() or not stairs.any()
    assert np.array_equal(np.asarray(rec[path]["left_flight"]), info["travel"] > np.where(stairs, LT.START + rows[:, 5] * rows[:, 4], np.inf))


# profiles/plant_kernel_resources.txt, qmpc_terrain.hip:  VGPRs, AGPRs, SGPR spills, VGPR spills, waves per SIMD
TERRAIN_TABLE = {"qmpc_terrain_init_kernel": (100, 0, 0, 0, 4),
                 "qmpc_terrain_step_kernelILb0ELb0E": (247, 0, 17, 0, 2), "qmpc_terrain_step_kernelILb0ELb1E": (247, 0, 17, 0, 2),
                 "qmpc_terrain_step_kernelILb1ELb0E": (255, 10, 31, 0, 1), "qmpc_terrain_step_kernelILb1ELb1E": (255, 10, 31, 0, 1)}


@KR.no_hipcc
def test_terrain_kernel_resources(tmp_path):
    """Every terrain kernel -- the reset on terrain and the four <VARY, STATS> instantiations of the step -- compiles
    for gfx950 without scratch, without spills to memory and without LDS, and within its row of
    profiles/plant_kernel_resources.txt."""
    res = KR.kernel_resources("qmpc_terrain.hip", tmp_path)
    assert len(res) == 5 and sum("qmpc_terrain_step_kernel" in k for k in res) == 4, sorted(res)
    assert all(v["vgpr_spill"] == 0 for v in res.values()), res
    KR.hold(res, TERRAIN_TABLE)
