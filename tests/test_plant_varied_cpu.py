"""CPU suite for the plant's per-robot parameters and statistics (include/qmpc_plant_vary.h): the exported surface, the
numpy restatement tests/plant_model_varied.py on what it must reproduce -- the model the GPU suite
(tests/test_gpu_plant_varied.py) holds the kernel to --, the CPU closed loop on the varied plant that the GPU walk is
measured by, and the compiled plant kernels' registers and scratch."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kernel_resources as KR
import plant_cases as PC
import plant_loop as L
import plant_loop_varied as LV
import plant_model as PM
import plant_model_varied as PV
from plant_cases import none as _none

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
f32 = np.float32
MODEL_KEYS = ("p", "v", "q", "w", "foot", "grf", "stance", "state", "motor")


def test_vary_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_plant_vary.h")).read()
    decl = set(re.findall(r"^int (qmpc_\w+)\(", hdr, re.M))
    want = {"qmpc_plant_set_params", "qmpc_plant_stats_enable", "qmpc_plant_stats_reset", "qmpc_plant_stats_get"}
    assert decl == want == set(binding.PLANT_VARY_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the structures of the binding follow the header's member order
    for struct, cls in (("qmpc_plant_stats", binding.PlantStats), ("qmpc_plant_params", binding.PlantParams)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+);", body) == [n for n, _ in cls._fields_], struct
    # qmpc_plant.h still declares exactly its four, and none of them moved into the new list
    old = set(re.findall(r"^int (qmpc_\w+)\(", open(os.path.join(ROOT, "include", "qmpc_plant.h")).read(), re.M))
    assert old == {"qmpc_plant_init", "qmpc_plant_reset", "qmpc_plant_step", "qmpc_plant_view_get"} == set(binding.PLANT_EXPORTS)
    assert not old & want


@pytest.mark.parametrize("substeps", [1, 4])
def test_neutral_values_are_bit_neutral(substeps):
    """Mass 9, the handle's inertia, mu = mu_plant, zero force and torque, all five bound: PlantModel bit for bit."""
    B, m, old, new, tau, cs, pd, vd = PC.parity_case(substeps)
    keep = {k: getattr(m, k).copy() for k in ("p", "v", "q", "w", "foot", "stance")}
    mv = PV.VariedPlantModel(B, PC.DEFAULTS["freq"], PC.DEFAULTS["mu"], substeps, mass_b=np.full(B, PM.MASS),
                             ibody_b=np.tile(PM.IBODY, (B, 1)), mu_b=np.full(B, PC.DEFAULTS["mu"]), force=np.zeros((B, 3)),
                             torque=np.zeros((B, 3)))
    for k, val in keep.items():
        setattr(mv, k, val.copy())
    m.step(tau.reshape(B, 12), cs, pd, vd)
    mv.step(tau.reshape(B, 12), cs, pd, vd)
    for k in MODEL_KEYS:
        assert np.array_equal(getattr(m, k), getattr(mv, k)), k
    assert np.abs(m.grf).max() > 1 and (mv.stats["n"] == 1).all() and np.array_equal(mv.stats["z_min"], m.p[:, 2])


def test_closed_forms_of_the_external_wrench():
    B = 3
    mass = np.array([5.0, 9.0, 14.5])
    ib = PM.IBODY[None, :] * np.array([0.5, 1.0, 2.0])[:, None]
    cs, pd, vd = _none(B)
    # an all-swing robot under force = (0, 0, m_b g): vdot = 0 exactly, the height stays
    force = np.zeros((B, 3))
    force[:, 2] = mass * PM.GRAVITY
    pl = PV.VariedPlantModel(B, 500.0, 0.4, 2, mass_b=mass, ibody_b=ib, force=force)
    z0 = pl.p[:, 2].copy()
    for _ in range(10):
        st, _ = pl.step(np.zeros((B, 12)), cs, pd, vd)
    assert np.array_equal(pl.v, np.zeros((B, 3))) and np.array_equal(pl.p[:, 2], z0)
    assert np.array_equal(st[:, 13:16], np.tile([0.0, 0.0, PM.GRAVITY], (B, 1)))    # the accelerometer feels the push
    assert np.array_equal(pl.grf, np.zeros((B, 4, 3)))                               # ... the ground's reactions do not
    # at rest under torque = (0, 0, t): w_z = h t / I_zz,b after one substep
    t = np.array([0.5, -2.0, 3.0])
    torque = np.zeros((B, 3))
    torque[:, 2] = t
    pl = PV.VariedPlantModel(B, 500.0, 0.4, 1, ibody_b=ib, torque=torque, force=force, mass_b=mass)
    pl.step(np.zeros((B, 12)), cs, pd, vd)
    assert np.array_equal(pl.w[:, 2], pl.h * (t / ib[:, 2])) and np.array_equal(pl.w[:, :2], np.zeros((B, 2)))


def test_friction_cone_of_the_robots_own_floor():
    """A saturated stance foot lies on the cone of its own mu_b; mu_b = 0 gives purely vertical forces."""
    B = 4
    mu = np.array([0.0, 0.2, 0.4, 1.1])
    pl = PV.VariedPlantModel(B, 500.0, 0.4, 1, mu_b=mu)
    fz = 20.0
    f = np.zeros((B, 4, 3))
    f[..., 2] = fz
    f[..., 0], f[..., 1] = 3 * fz * 0.6, -3 * fz * 0.8            # tangential demand beyond every cone here
    tau = PC.hold(pl, f)
    _, pd, vd = _none(B)
    pl.step(tau.reshape(B, 12), np.ones((B, 4), f32), pd, vd)
    g = pl.grf
    assert np.abs(g[..., 2] - fz).max() < 1e-11
    assert np.abs(np.hypot(g[..., 0], g[..., 1]) - mu[:, None] * g[..., 2]).max() < 1e-12
    assert np.array_equal(g[0, :, :2], np.zeros((4, 2))) and (np.hypot(g[1:, :, 0], g[1:, :, 1]) > 1).all()
    assert np.abs(g[1:, :, 0] * (-0.8) - g[1:, :, 1] * 0.6).max() < 1e-11     # in the demanded direction


def test_variation_is_the_stated_disturbance():
    v = LV.variation(32)
    assert np.array_equal(v["mass"][:16], 9.0 * np.repeat([0.8, 1.0, 1.2, 1.4], 4)) and np.array_equal(v["mass"][16:], v["mass"][:16])
    assert np.array_equal(v["mu"][:8], [0.3, 0.4, 0.6, 0.8] * 2)
    assert np.array_equal(v["ibody"][4], [0.07, 0.26, 0.242]) and np.array_equal(v["ibody"][12], np.array([0.07, 0.26, 0.242]) * 1.4)
    assert not v["force"](299).any() and not v["force"](350).any() and not v["torque"].any()
    for t in (300, 349):
        assert np.array_equal(v["force"](t)[:4], [[0, -30.0, 0], [0, 30.0, 0]] * 2)


def test_cpu_closed_loop_on_the_varied_plant_is_safe_and_is_what_the_fixture_records():
    """tests/test_plant_cpu.py's yardstick test on the varied plant: the reference pipeline, planning on 9 kg and mu 0.4,
    keeps every robot safe on plant_loop_varied.variation(), and the statistics are the fixture's (1e-6: see there)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_varied_closed_loop_cpu.json")))
    assert gold["ticks"] == L.TICKS == 650 and tuple(gold["pid"]) == L.PID
    var = LV.variation(L.N_CMD)
    for k in ("mass", "ibody", "mu", "push", "torque"):
        assert np.array_equal(gold["variation"][k], var[k]), k
    assert tuple(gold["variation"]["push_ticks"]) == var["push_ticks"] == (300, 350)
    for mode in (0, 1):
        stats, info = LV.cpu_loop_varied(mode)
        rec = gold[f"mode{mode}"]
        gait, vel, xyyaw = L.commands(mode)
        assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
        assert (info["safe"] == 1).all() and info["rc_bad"] == 0 and info["nwsr_max"] < 100, (mode, info)
        assert info["n_solves"] >= 16 * 45
        for k in L.STATS:
            print(mode, k, np.abs(stats[k] - np.asarray(rec[k])).max())
            assert np.abs(stats[k] - np.asarray(rec[k])).max() < 1e-6, (mode, k)
        assert (stats["z_min"] > 0.2).all() and (stats["roll_max"] < 0.15).all() and (stats["pitch_max"] < 0.15).all()
        assert np.abs(stats["vx_mean"] - vel[:, 0]).max() < 0.05


def test_statistics_from_the_accumulators_are_the_recorders():
    """fleet_gpu.stats_from_accumulators -- the one formula every device walk rebuilds its five statistics with -- on the
    CPU loop's own model, in both robot modes: the start state, the model's accumulators copied before the step of tick
    150 and at the end give what plant_loop.Recorder returned for the same run.  The extremes are the same comparisons of
    the same doubles: equal.  vx_mean: the two sides sum at most 650 speeds of a few m/s in a different order,
    650^2 * 1.1e-16 * |v| / 500 is below 1e-12."""
    import fleet_gpu as G
    for mode in (0, 1):
        seen = {}

        def sample(t, plant):
            if t == 0:
                seen["start"], seen["plant"] = np.asarray(plant.state, np.float64).copy(), plant
            if t == L.TICKS - int(L.FREQ):
                seen["mid"] = {k: v.copy() for k, v in plant.stats.items()}

        stats, info = LV.cpu_loop_varied(mode, each_tick=sample)
        assert (seen["mid"]["n"] == 150).all() and (seen["plant"].stats["n"] == L.TICKS).all()
        got = G.stats_from_accumulators(seen["start"], seen["mid"], seen["plant"].stats)
        for k in ("z_min", "z_max", "roll_max", "pitch_max"):
            assert np.array_equal(got[k], stats[k]), (mode, k, np.abs(got[k] - stats[k]).max())
        err = np.abs(got["vx_mean"] - stats["vx_mean"]).max()
        print(f"mode {mode} vx_mean: accumulators against Recorder {err:.3e}")
        assert err <= 1e-12, (mode, err)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_choice_for_every_binding(tmp_path):
    """tests/plant_pick_dump.cpp: csrc/qmpc_plant_pick.h alone, host only.  The step and the reset kernel for all eight
    combinations of (field bound, contact flags set, rows bound) are the public headers' rules: a bound field takes the
    kernels of include/qmpc_field.h whatever else is bound; without one, contact flags take include/qmpc_contact.h's step
    on any ground; without either, rows take include/qmpc_terrain.h's; else the flat plant.  The reset stands the robots
    on the ground -- field, rows or flat -- and ignores contact, whose counters it zeroes exactly when contact is on."""
    exe = str(tmp_path / "plant_pick_dump")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "plant_pick_dump.cpp"), "-o", exe],
                   check=True)
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    #           field contact rows   step             reset
    want = [(0, 0, 0, "plant", "plant"),
            (0, 0, 1, "terrain", "terrain"),
            (0, 1, 0, "contact", "plant"),
            (0, 1, 1, "contact", "terrain"),
            (1, 0, 0, "field", "field"),
            (1, 0, 1, "field", "field"),
            (1, 1, 0, "field_contact", "field"),
            (1, 1, 1, "field_contact", "field")]
    assert [(g["field"], g["contact"], g["rows"], g["step"], g["reset"]) for g in got] == want
    assert [g["counters"] for g in got] == [w[1] for w in want]


# profiles/plant_kernel_resources.txt, qmpc_plant.hip:  VGPRs, AGPRs, SGPR spills, VGPR spills, waves per SIMD
PLANT_TABLE = {"qmpc_plant_init_kernel": (98, 0, 0, 0, 4), "qmpc_plant_stats_reset_kernel": (6, 0, 0, 0, 8),
               "qmpc_plant_step_kernelILb0ELb0E": (221, 0, 15, 0, 2), "qmpc_plant_step_kernelILb0ELb1E": (221, 0, 15, 0, 2),
               "qmpc_plant_step_kernelILb1ELb0E": (243, 0, 41, 0, 2), "qmpc_plant_step_kernelILb1ELb1E": (243, 0, 41, 0, 2)}


@KR.no_hipcc
def test_plant_kernel_resources(tmp_path):
    """Every plant kernel -- init, the statistics' reset and the four <VARY, STATS> instantiations of the step --
    compiles for gfx950 without scratch, spill to memory or LDS, and within its row of profiles/plant_kernel_resources.txt:
    the plain step keeps the 221 VGPRs INTEGRATION.md G records for it."""
    res = KR.kernel_resources("qmpc_plant.hip", tmp_path)
    assert len(res) == 6 and sum("qmpc_plant_step_kernel" in k for k in res) == 4, sorted(res)
    assert all(v["vgpr_spill"] == 0 for v in res.values()), res
    KR.hold(res, PLANT_TABLE)
