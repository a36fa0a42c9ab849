"""CPU suite for height-field terrain from memory (include/qmpc_field.h): the exported surface, the index logic of
csrc/qmpc_field_index.h under the sanitizers in a stand-alone host program, the numpy restatement
tests/plant_model_field.py on what it must reproduce -- the model the GPU suite (tests/test_gpu_field.py) holds the kernels
to --, the single-step case, the ladder's record and the CPU closed loops that the GPU walk is measured by, and the compiled
field kernels' scratch."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import field_cases as FC
import kernel_resources as KR
import plant_loop as L
import plant_loop_field as LF
import plant_loop_terrain as LT
import plant_model_contact as PCM
import plant_model_field as PF
import plant_model_terrain as PT
from c_headers import declared, members
from quadruped_ctrl_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLD = os.path.join(ROOT, "tests", "golden", "plant_field_closed_loop_cpu.json")
f32 = np.float32
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
OUT_KEYS = ("p", "v", "q", "w", "foot", "grf", "stance", "state", "motor", "support", "ground", "early", "late", "slip",
            "drop")


def test_field_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_field.h")).read()
    want = {"qmpc_plant_set_field", "qmpc_field_view_get"}
    assert declared("qmpc_field.h") == want == set(binding.FIELD_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    assert members(hdr, "qmpc_field_bank") == [n for n, _ in binding.FieldBank._fields_] == ["z", "nx", "ny", "count", "cell"]
    assert members(hdr, "qmpc_field_view") == [n for n, _ in binding.FieldView._fields_] == ["bank", "place", "flags", "batch"]
    # the older headers still declare exactly what they declared, and no longer call the feature out of scope
    assert declared("qmpc_terrain.h") == set(binding.TERRAIN_EXPORTS) and declared("qmpc_contact.h") == set(binding.CONTACT_EXPORTS)
    for name in ("include/qmpc_terrain.h", "include/qmpc_contact.h", "INTEGRATION.md"):
        text = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, name)).read())
        assert "Still out of scope" in text and not re.search(r"Still out of scope:[^.]*height maps", text), name
    import inspect
    d = {k: v.default for k, v in inspect.signature(binding.BatchedPlant.set_field).parameters.items()
         if k in ("clamp_swing", "rebase_z")}
    assert d == dict(clamp_swing=False, rebase_z=False)


# ---- the index logic, on the CPU under the sanitizers ------------------------------------------------------------------

@no_hipcc
def test_index_logic_keeps_every_tap_inside_the_bank(tmp_path):
    """tests/field_index_dump.cpp: csrc/qmpc_field_index.h alone, host only, built with AddressSanitizer and UBSan and run
    directly.  It feeds u, v and map +-0, every exact grid line and its neighbours, just inside and outside each edge,
    +-1e9, +-1e300, +-inf, NaN and the limits of int, for (nx, ny, count) = (2, 2, 1) and (7, 5, 3), and reads the four
    taps from a heap array of exactly the bank's size.  Every tap lies inside [0, count ny nx), the sanitizers are
    silent, and the indices and weights are the model's."""
    exe = str(tmp_path / "field_index_dump")
    # host code only (-x c++: no device pass), and the sanitizers named for the host side alone
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "field_index_dump.cpp"), "-o", exe],
                   check=True)
    syms = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms              # both runtimes are linked in
    shapes = [(2, 2, 1), (7, 5, 3)]
    run = subprocess.run([exe] + [str(x) for s in shapes for x in s], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr and run.stderr.startswith("checksum"), run.stderr[-2000:]
    t = np.array([line.split() for line in run.stdout.splitlines()], dtype=np.float64)
    assert len(t) > 50000 and t.shape[1] == 17
    for nx, ny, count in shapes:
        r = t[(t[:, 0] == nx) & (t[:, 1] == ny) & (t[:, 2] == count)]
        u, v, mp = r[:, 3], r[:, 4], r[:, 5]
        for bad in (np.isnan, np.isposinf, np.isneginf):
            assert bad(u).any() and bad(v).any() and bad(mp).any()
        assert (np.abs(u) == 1e300).any() and (u == nx - 1).any() and (u == np.nextafter(nx - 1.0, np.inf)).any()
        m, i, j, a, b = r[:, 6], r[:, 7], r[:, 8], r[:, 9], r[:, 10]
        taps = r[:, 13:17]
        assert taps.min() >= 0 and taps.max() < count * ny * nx
        assert (m >= 0).all() and (m <= count - 1).all() and (i >= 0).all() and (i <= nx - 2).all() and (j >= 0).all() and (j <= ny - 2).all()
        assert (a >= 0).all() and (a <= 1).all() and (b >= 0).all() and (b <= 1).all()
        assert np.array_equal(taps, (m * ny * nx + j * nx + i)[:, None] + np.array([0, 1, nx, nx + 1]))
        with np.errstate(invalid="ignore"):
            mi, ma, minx = PF.FieldPlantModel.axis(u, nx)
            mj, mb, miny = PF.FieldPlantModel.axis(v, ny)
            mm = np.where(~(mp >= 0.0), 0.0, mp)
            mm = np.where(mm > count - 1.0, count - 1.0, mm).astype(np.int64)
        assert np.array_equal(mi, i) and np.array_equal(mj, j) and np.array_equal(ma, a) and np.array_equal(mb, b)
        assert np.array_equal(minx, r[:, 11] != 0) and np.array_equal(miny, r[:, 12] != 0) and np.array_equal(mm, m)


# ---- the model ---------------------------------------------------------------------------------------------------------

def _zero_bank_pair(kind, terrain, path):
    """-> (a FieldPlantModel on an all-zero bank of two maps with lively placements, its parent without the field), both
    reset on the same ground."""
    B = L.N_CMD
    _, _, xyyaw = L.commands(0)
    rng = np.random.default_rng(5)
    z = np.zeros((2, 9, 11), f32)
    place = np.stack([rng.integers(0, 2, B).astype(float), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B),
                      rng.uniform(-2, 2, B)], 1)
    rows = LT.terrain(B) if terrain else None
    fl = LF.contact_flags(kind)
    out = []
    for cls in (PF.FieldPlantModel, PCM.ContactPlantModel):
        m = cls(B, L.FREQ, 0.4, 1, xyyaw)
        m.set_terrain(rows, clamp_swing=True, rebase_z=path == "state")
        if cls is PF.FieldPlantModel:
            m.set_field(z, place, 0.07)                     # flags 0
        m.set_contact(early=bool(fl & 1), late=bool(fl & 2), slip=bool(fl & 4))
        m.reset(np.ones(B, bool), xyyaw)
        out.append(m)
    return out


@pytest.mark.parametrize("kind,terrain", [("scheduled", False), ("scheduled", True), ("contact", False), ("contact", True)])
def test_zero_bank_is_the_parent_bit_for_bit(kind, terrain):
    """A 50-tick closed-loop walk on a bank of all-zero samples, any placements: the plant without the field, bit for bit,
    on flat ground, on slopes and stairs, with scheduled contact and with contact on."""
    mf, mp = _zero_bank_pair(kind, terrain, "state")
    for k in OUT_KEYS:
        assert np.array_equal(getattr(mf, k), getattr(mp, k)), ("reset", k)
    for m in (mf, mp):
        LF.cpu_loop_field(0, "state", kind, 0.0, ticks=50, plant=m)
    for k in OUT_KEYS:
        assert np.array_equal(getattr(mf, k), getattr(mp, k)), k
    assert np.abs(mf.grf).max() > 10 and (not terrain or np.abs(mf.ground).max() > 1e-3)
    assert np.signbit(mf.grf).any()


def test_no_bank_is_the_parent():
    m = PF.FieldPlantModel(4)
    assert m.z is None and m.height.__func__ is PF.FieldPlantModel.height
    m.set_terrain(np.zeros((4, 8)))
    assert np.array_equal(m.height(np.ones(4), np.ones(4)), np.zeros(4))
    m.set_field(np.ones((1, 2, 2), f32), np.tile([0.0, 0.0, 0.0, 1.0], (4, 1)), 1.0)
    m.set_field(None)
    assert m.z is None and m.fflags == 0


def test_a_bank_sampled_from_a_plane_is_the_analytic_plane_bit_for_bit():
    """Dyadic numbers, so that every operation is exact: cell 2^-4, origin and slopes multiples of 2^-3, query points with
    few mantissa bits.  height() and the per-foot normal are TerrainPlantModel's on the same plane, bit for bit -- with
    the plane in the bank alone, and split between the bank and the rows."""
    B, cell, nx, ny = 3, 2.0 ** -4, 40, 36
    z0, gx, gy, ox, oy = 0.5, 0.25, -0.125, -1.0, -0.875
    X, Y = ox + cell * np.arange(nx), oy + cell * np.arange(ny)
    plane = z0 + gx * X[None, :] + gy * Y[:, None]
    z = plane.astype(f32)[None]
    assert np.array_equal(z[0].astype(np.float64), plane)
    place = np.tile([0.0, ox, oy, 1.0], (B, 1))
    rows = np.tile([z0, gx, gy, 0, 0, 0, 0, 0.0], (B, 1))
    t = PT.TerrainPlantModel(B, rows=rows)
    x = np.tile([[0.1875, 0.3125, -0.4375, 0.71875]], (B, 1))
    y = np.tile([[0.28125, -0.5, 0.09375, 0.65625]], (B, 1))
    m = PF.FieldPlantModel(B)
    m.set_field(z, place, cell)
    assert np.array_equal(m.height(x, y), t.height(x, y)) and np.array_equal(m.height(x[:, 0], y[:, 0]), t.height(x[:, 0], y[:, 0]))
    h, n = m._bound(m.foot_surface, x, y)
    assert np.array_equal(h, t.height(x, y)) and np.array_equal(n, np.broadcast_to(t.normal()[:, None, :], n.shape))
    # half the plane in the rows, half in the bank (zs = 0.5: still exact)
    half = np.tile([z0 / 2, gx / 2, gy / 2, 0, 0, 0, 0, 0.0], (B, 1))
    m.set_terrain(half)
    m.set_field(z, np.tile([0.0, ox, oy, 0.5], (B, 1)), cell)
    h, n = m.foot_surface(x, y)
    assert np.array_equal(h, t.height(x, y)) and np.array_equal(n, np.broadcast_to(t.normal()[:, None, :], n.shape))
    # off the map the edge sample extends outward and the gradient across that edge is 0
    m.set_terrain(None)
    m.set_field(z, place, cell)
    f, fx, fy = m.sample(np.full(B, ox - 1.0), np.full(B, 0.0))
    assert np.array_equal(f, m.sample(np.full(B, ox), np.full(B, 0.0))[0]) and (fx == 0).all() and (fy == gy).all()
    f, fx, fy = m.sample(np.full(B, 0.0), np.full(B, Y[-1] + 3.0))
    assert np.array_equal(f, m.sample(np.full(B, 0.0), np.full(B, Y[-1]))[0]) and (fy == 0).all() and (fx == gx).all()


def test_heights_are_continuous_across_cell_borders():
    z, cell = FC.bank(), FC.CELL
    B = 4
    m = PF.FieldPlantModel(B)
    m.set_field(z, np.tile([1.0, 0.0, 0.0, 1.3], (B, 1)), cell)
    eps = 1e-9
    for i in range(1, FC.NX - 1):
        for j in range(1, FC.NY - 1):
            x, y = i * cell, j * cell
            y_in = np.full(B, y + 0.37 * cell)
            hx = [m.height(np.full(B, x + d), y_in)[0] for d in (-eps, 0.0, eps)]
            hy = [m.height(np.full(B, x + 0.41 * cell), np.full(B, y + d))[0] for d in (-eps, 0.0, eps)]
            assert max(abs(hx[0] - hx[1]), abs(hx[2] - hx[1]), abs(hy[0] - hy[1]), abs(hy[2] - hy[1])) < 1e-9 * 1.3 * 0.6 / cell + 1e-15
            assert abs(m.height(np.full(B, x), np.full(B, y))[0] - 1.3 * float(z[1, j, i])) < 1e-15       # nodes are samples
    # ... while the slope jumps there (so the normal is per cell)
    fx = [m.sample(np.full(B, 2 * cell + d), np.full(B, 1.5 * cell))[1][0] for d in (-eps, eps)]
    assert abs(fx[0] - fx[1]) > 1e-3


def test_every_column_of_place_and_every_map_moves_the_result():
    case = FC.parity_case(1)
    base = FC.stepped(case, 1)
    m0, rows, z, place, cell = case[:5]
    for col, delta in ((0, None), (1, 0.013), (2, 0.013), (3, 0.21)):
        other = place.copy()
        other[:, col] = (other[:, col] + 1) % FC.COUNT if delta is None else other[:, col] + delta
        got = FC.stepped(case[:3] + (other,) + case[4:], 1)
        assert np.abs(got.state - base.state).max() > 1e-6 and np.abs(got.grf - base.grf).max() > 1e-6, col
    for k in range(FC.COUNT):
        z2 = z.copy()
        z2[k] += f32(0.01) * np.random.default_rng(k).uniform(-1, 1, z[k].shape).astype(f32)
        got = FC.stepped(case, 1, z=z2)
        on = np.floor(np.clip(place[:, 0], 0, FC.COUNT - 1)) == k
        moved = np.maximum(np.abs(got.state - base.state).max(1), np.abs(got.ground - base.ground))
        moved = np.maximum(moved, np.abs(got.foot - base.foot).reshape(FC.B, -1).max(1))
        felt = moved[on & (place[:, 3] != 0)] > 1e-9       # (the ground under the body at the least)
        assert felt.all() and len(felt) >= 10 and (moved[~on] == 0).all() and (moved[place[:, 3] == 0] == 0).all(), k
    z2 = z.copy()
    z2[0, 1, 2] += f32(0.01)                                   # one sample: x fastest
    got = FC.stepped(case, 1, z=z2)
    assert np.abs(got.foot - base.foot).max() > 0


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("contact", [False, True])
@pytest.mark.parametrize("bound,dyadic", [(True, False), (False, False), (True, True)])
def test_single_step_case_holds_what_it_promises(substeps, contact, bound, dyadic):
    """tests/field_cases.py, which the GPU suite compares the kernels on."""
    case = FC.parity_case(substeps, bound, dyadic)
    for vals in (None, FC.values(1000 + substeps)):
        FC.check(case, FC.stepped(case, substeps, vals, contact), dyadic)
    moved = FC.moved_by_the_field(case, substeps, contact)
    assert min(moved.values()) > 1e-4, moved                  # far above the GPU parity's 1e-10


def test_random_blocks_is_the_stated_recipe():
    z = W.random_blocks(3)
    assert z.shape == (256, 256) and z.dtype == f32 and z.flags["C_CONTIGUOUS"] and 0 <= z.min() and z.max() <= 0.06
    assert np.array_equal(z, W.random_blocks(3)) and not np.array_equal(z, W.random_blocks(4))
    blocks = z.reshape(128, 2, 128, 2)
    assert (blocks == blocks[:, :1, :, :1]).all() and len(np.unique(z)) > 16000 and abs(z.mean() - 0.03) < 1e-3
    y = W.random_blocks(3, n=7, block=3, amp=0.2)
    assert y.shape == (7, 7) and y.max() > 0.06 and (y[:3, :3] == y[0, 0]).all() and (y[6, 6] == y[6:, 6:]).all()
    assert not W.random_blocks(3, amp=0.0).any()


# ---- the ladder and the closed loop -------------------------------------------------------------------------------------

def test_rungs_are_the_record():
    gold = json.load(open(GOLD))
    assert gold["rungs"] == LF.RUNGS and gold["ticks"] == LF.TICKS
    assert gold["map"] == dict(n=LF.N_MAP, block=LF.BLOCK, cell=LF.CELL, seed=LF.MAP_SEED)
    assert np.array_equal(gold["place"], LF.field_for(L.N_CMD, 0.0)[1])
    assert LF.LADDER[:3] == (0.02, 0.04, 0.06) and LF.LADDER[3:] == (0.10, 0.15)
    for kind in LF.KINDS:
        rec = gold["ladders"][kind]
        assert rec["rungs"] == list(LF.LADDER)
        walked = [w["rung"] for w in rec["walked"]]
        assert walked == list(LF.LADDER[:len(walked)]) and all(w["walked"] for w in rec["walked"])  # a climb ends at its first fall
        assert (walked[-1] if walked else None) == LF.RUNGS[kind]
        assert len(walked) + (rec["fell"] is not None) + len(rec["beyond"]) == len(LF.LADDER)
        if rec["fell"] is not None:
            assert rec["fell"]["rung"] == LF.LADDER[len(walked)] and not rec["fell"]["walked"]
            assert any(r["fallen"] for r in rec["fell"]["runs"].values())
        assert gold["walk"][kind]["amp"] == (LF.RUNGS[kind] or 0.0)


@pytest.mark.parametrize("kind", LF.KINDS)
def test_the_first_fallen_rung_falls(kind):
    """One run of the record's first fallen rung -- the one that lost a robot first in the record -- loses it again."""
    rec = json.load(open(GOLD))["ladders"][kind]["fell"]
    if rec is None:
        return                                                 # (every rung was walked: nothing fell)
    name, run = next((k, r) for k, r in rec["runs"].items() if r["fallen"])
    mode, path = int(name[4]), name.split("_")[1]
    _, info = LF.cpu_loop_field(mode, path, kind, rec["rung"])
    ok = (info["safe"].reshape(-1) == 1) & (info["rc_bad"] == 0) & (info["nwsr_max"] < 100)
    assert np.array_equal(np.flatnonzero(~ok), run["fallen"])


@pytest.mark.parametrize("kind", LF.KINDS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", LF.PATHS)
def test_cpu_closed_loop_on_the_field_is_safe_and_is_what_the_fixture_records(kind, mode, path):
    """The reference pipeline keeps every robot safe on RUNGS, with every qpOASES return code 0 and nWSR < 100, and the
    statistics and the counters are the fixture's (1e-6, as the other closed-loop fixtures)."""
    gold = json.load(open(GOLD))
    stats, info = LF.cpu_loop_field(mode, path, kind)
    rec = gold["walk"][kind][f"mode{mode}"]
    gait, vel, xyyaw = L.commands(mode)
    assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
    assert (info["safe"] == 1).all() and (info["rc_bad"] == 0).all() and (info["nwsr_max"] < 100).all(), (kind, mode, path, info)
    for k in L.STATS:
        assert np.abs(stats[k] - np.asarray(rec[path][k])).max() < 1e-6, (kind, mode, path, k)
    assert np.abs(info["travel"] - np.asarray(rec[path]["travel"])).max() < 1e-6
    assert np.abs(info["support"] - np.asarray(rec[path]["support"])).max() < 1e-6
    assert np.array_equal(info["early"], rec[path]["early"]) and np.array_equal(info["late"], rec[path]["late"])
    assert np.abs(info["slip"] - np.asarray(rec[path]["slip"])).max() < 1e-6
    if LF.RUNGS[kind]:
        assert np.abs(info["support"]).max() > 1e-3                       # the ground is felt
    if kind == "contact":
        assert info["early"].any() and info["late"].any()


# ---- the kernels --------------------------------------------------------------------------------------------------------

# profiles/plant_kernel_resources.txt, qmpc_field.hip:  VGPRs, AGPRs, SGPR spills, VGPR spills (to AGPRs), waves per SIMD
FIELD_TABLE = {"qmpc_field_init_kernel": (102, 0, 0, 0, 4),
               "qmpc_field_step_kernelILb0ELb0E": (255, 2, 26, 0, 1), "qmpc_field_step_kernelILb0ELb1E": (255, 2, 26, 0, 1),
               "qmpc_field_step_kernelILb1ELb0E": (256, 26, 40, 0, 1), "qmpc_field_step_kernelILb1ELb1E": (256, 26, 40, 0, 1),
               "qmpc_field_contact_step_kernelILb0ELb0E": (255, 4, 31, 0, 1), "qmpc_field_contact_step_kernelILb0ELb1E": (255, 4, 31, 0, 1),
               "qmpc_field_contact_step_kernelILb1ELb0E": (256, 30, 72, 4, 1), "qmpc_field_contact_step_kernelILb1ELb1E": (256, 30, 72, 4, 1)}


@no_hipcc
def test_field_kernel_resources(tmp_path):
    """The reset on the field and the four <VARY, STATS> instantiations of each step compile for gfx950 without scratch
    and without LDS, within their rows of profiles/plant_kernel_resources.txt, and the kernels the plant launched before
    are where they were: no kernel of qmpc_field.hip's in the other files."""
    res = KR.kernel_resources("qmpc_field.hip", tmp_path)
    assert len(res) == 9 and sum("qmpc_field_step_kernel" in k for k in res) == 4 \
        and sum("qmpc_field_contact_step_kernel" in k for k in res) == 4, sorted(res)
    KR.hold(res, FIELD_TABLE)
