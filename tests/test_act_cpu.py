"""CPU suite for the actuator stage (include/qmpc_act.h): the exported surface and the default config, the motor, the
accumulation order and the ring indexing of csrc/qmpc_act_model.h under the sanitizers in a stand-alone host program
against the numpy restatement tests/act_model.py -- the model the GPU suite (tests/test_gpu_act.py) holds the kernel to --,
the recorded CPU closed loop with its ladders (tests/golden/act_closed_loop_cpu.json), and the compiled kernels'
resources."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import act_cases as AC
import act_model as AM
import plant_loop as L
from c_headers import members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
GOLD = os.path.join(ROOT, "tests", "golden", "act_closed_loop_cpu.json")


def test_act_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_act.h")).read()
    decl = set(re.findall(r"^int (qmpc_\w+)\(", hdr, re.M))
    want = {"qmpc_act_config_default", "qmpc_act_init", "qmpc_act_set_params", "qmpc_act_reset", "qmpc_act", "qmpc_act_view_get"}
    assert decl == want == set(binding.ACT_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert list(f.argtypes) == binding.ACT_SIGNATURES[name] and f.restype is C.c_int
        # the arity of the binding's table is the header's
        args = re.search(r"^int %s\(([^)]*)\)" % name, hdr, re.M).group(1)
        assert len(args.split(",")) == len(binding.ACT_SIGNATURES[name]), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the structures of the binding follow the header's member order
    for struct, cls in (("qmpc_act_config", binding.ActConfig), ("qmpc_act_params", binding.ActParams),
                        ("qmpc_act_view", binding.ActView)):
        assert members(hdr, struct) == [n for n, _ in cls._fields_], struct
    assert list(AM.PARAMS) == list(binding.ACT_PARAM_FIELDS) and AM.ACCUMULATORS == binding.ACT_STATS
    assert int(re.search(r"#define QMPC_ACT_MAX_DELAY (\d+)", hdr).group(1)) == AM.MAX_DELAY == binding.ACT_MAX_DELAY == 64
    # none of the new symbols went into an older header or list
    older = (set(binding.EXPORTS) | set(binding.CTRL_EXPORTS) | set(binding.PLANT_EXPORTS) | set(binding.PLANT_VARY_EXPORTS)
             | set(binding.SENSE_EXPORTS) | set(binding.EPISODE_EXPORTS) | set(binding.EPISODE_SENSE_EXPORTS))
    assert not older & want
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "qmpc_act.h":
            assert "qmpc_act" not in open(os.path.join(ROOT, "include", h)).read(), h
    # without a device every entry point refuses a null handle or pointer
    assert lib.qmpc_act_config_default(None) == 1
    assert lib.qmpc_act_init(None, 4, None, None) == 1 and lib.qmpc_act_set_params(None, 4, None) == 1
    assert lib.qmpc_act_reset(None, 4, None, None, 0, None) == 1 and lib.qmpc_act(None, 4, None, None, None) == 1
    assert lib.qmpc_act_view_get(None, None) == 1


def test_default_config_is_the_mini_cheetah():
    """src/Dynamics/MiniCheetah.h:28-46: abad and hip gear 6, knee 9.33, kt 0.05, R 0.173, 24 V, damping 0.01, dry
    friction 0.2, cap 3 N m; ActuatorModel::_frictionEnabled = true; and no latency."""
    from quadruped_ctrl_amd import binding
    cfg = binding.ActConfig()
    assert binding.load_library().qmpc_act_config_default(C.byref(cfg)) == 0
    got = dict(gear=tuple(cfg.gear), **{k: getattr(cfg, k) for k in binding.ACT_CONFIG_FIELDS})
    want = dict(gear=(6.0, 6.0, 9.33), kt=0.05, R=0.173, battery_v=24.0, damping=0.01, dry_friction=0.2, tau_max=3.0,
                friction=1, max_delay=0)
    assert got == want == AM.config() == binding.BatchedActuators.default_config()
    # the header states them
    hdr = open(os.path.join(ROOT, "include", "qmpc_act.h")).read()
    assert "gear 6 / 6 / 9.33, kt 0.05, R 0.173, 24 V, damping 0.01, dry friction 0.2, cap 3 N m" in hdr


# ---- the header on the CPU under the sanitizers ---------------------------------------------------------------------------

def _hex(x):
    return " ".join("%016x" % int(u) for u in np.asarray(x, np.float64).reshape(-1).view(np.uint64))


DT = 1.0 / 500.0
CALLS = 3
RING_CASES = [(D, seed) for D in (0, 1, 5, 64) for seed in (0, 1)]


def _period_cases():
    """-> [(cfg, binding, call)]: friction on and off, every binding of act_cases.BINDINGS, three consecutive periods."""
    return [(dict(friction=fr), names, call) for fr in (1, 0) for names in AC.BINDINGS for call in range(CALLS)]


def _ring_script(D, seed):
    """150 periods of one robot: delays below 0, inside and above max_delay, resets in the middle."""
    rng = np.random.default_rng(100 * D + seed)
    n = 150
    delay = rng.integers(-2, D + 4, n)
    delay[:20] = D                                        # the age is below the delay at the start ...
    reset = rng.random(n) < 0.04
    reset[70] = True
    delay[70:70 + D + 2] = D                              # ... and after the reset in the middle
    return delay.astype(int), reset


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/act_dump.cpp: csrc/qmpc_act_model.h alone, host only, built with AddressSanitizer and UBSan and run directly
    on the case file -> (its P lines as token lists, its R lines as an int array)."""
    d = tmp_path_factory.mktemp("act")
    exe, cases = str(d / "act_dump"), str(d / "cases.txt")
    # host code only (-x c++: no device pass), and the sanitizers named for the host side alone
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "act_dump.cpp"), "-o", exe], check=True)
    syms = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms              # both runtimes are linked in
    prm = AC.params()
    with open(cases, "w") as f:
        for cfg, names, call in _period_cases():
            c = AM.config(**cfg)
            acc = np.random.default_rng(call).uniform(0.0, 5.0, (AC.B, 4)) * (call > 0)   # the accumulators found
            eff, qd = AC.period(call)
            for b in range(AC.B):
                val = lambda k, key: prm[k][b] if k in names else c[key]
                f.write("P %d %d %s %s %s %s\n" % (
                    c["friction"], "strength" in names,
                    _hex(list(c["gear"]) + [c["kt"], c["R"], val("battery_v", "battery_v"), val("tau_max", "tau_max"),
                                            val("damping", "damping"), val("dry_friction", "dry_friction"),
                                            prm["strength"][b], DT]), _hex(acc[b]), _hex(eff[b]), _hex(qd[b])))
        for D, seed in RING_CASES:
            delay, reset = _ring_script(D, seed)
            f.write("R %d %d %s\n" % (D, len(delay), " ".join("%d %d" % (a, r) for a, r in zip(delay, reset))))
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr and run.stderr.startswith("records"), run.stderr[-2000:]
    lines = run.stdout.splitlines()
    p = [ln.split()[1:] for ln in lines if ln.startswith("P ")]
    r = np.array([ln.split()[1:] for ln in lines if ln.startswith("R ")], dtype=np.int64)
    return p, r


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@no_hipcc
def test_model_header_computes_what_the_model_computes(dump):
    """The 37-robot case table under friction on / off, nothing bound, each array bound alone and all bound, three
    periods on accumulators that are not zero: the twelve torques, the two counts and the four accumulators of every
    robot are the model's, bit for bit -- the summation order included.  The table reaches both voltage clamps, both
    torque clamps, both at once, rates of +0, -0 and tiny values of both signs, NaN and inf in the command and the rate."""
    p = dump[0]
    cases = _period_cases()
    assert len(p) == len(cases) * AC.B
    prm = AC.params()
    seen = dict(v_hi=0, v_lo=0, t_hi=0, t_lo=0, both=0, nan_out=0, strength=0)
    at = 0
    for cfg, names, call in cases:
        acc = np.random.default_rng(call).uniform(0.0, 5.0, (AC.B, 4)) * (call > 0)
        eff, qd = AC.period(call)
        m = AM.ActModel(AC.B, DT, cfg)
        m.set_params(**{k: prm[k] for k in names if k != "delay"})
        for k, name in enumerate(("tau_peak", "e_heat", "e_mech", "e_pos")):
            m.acc[name] = acc[:, k].copy()
        tau = m.apply(eff, qd)
        rows = p[at:at + AC.B]
        at += AC.B
        got_tau = np.array([[int(x, 16) for x in r[:12]] for r in rows], np.uint64)
        got_n = np.array([[int(x) for x in r[12:14]] for r in rows])
        got_acc = np.array([[int(x, 16) for x in r[14:18]] for r in rows], np.uint64)
        assert np.array_equal(got_tau, _bits(tau)), (cfg, names, call)
        assert np.array_equal(got_n[:, 0], m.acc["n_vsat"]) and np.array_equal(got_n[:, 1], m.acc["n_tsat"]), (cfg, names, call)
        for k, name in enumerate(("tau_peak", "e_heat", "e_mech", "e_pos")):
            assert np.array_equal(got_acc[:, k], _bits(m.acc[name])), (cfg, names, call, name)
        # what the table reached, by the model's own intermediate values
        g = np.tile(np.asarray(m.cfg["gear"]), 4)[None, :]
        V = (prm["battery_v"] if "battery_v" in names else np.full(AC.B, m.cfg["battery_v"]))[:, None]
        T = (prm["tau_max"] if "tau_max" in names else np.full(AC.B, m.cfg["tau_max"]))[:, None]
        with np.errstate(all="ignore"):
            bemf = ((qd * g) * 0.05) * 2.0
            vdes = ((eff / g) / (0.05 * 1.5)) * 0.173 + bemf
            vact = AM.coerce(vdes, -V, V)
            tam = ((0.05 * 1.5) * (vact - bemf)) / 0.173
        seen["v_hi"] += int((vdes > V).sum())
        seen["v_lo"] += int((vdes < -V).sum())
        seen["t_hi"] += int((tam > T).sum())
        seen["t_lo"] += int((tam < -T).sum())
        seen["both"] += int((((vdes > V) | (vdes < -V)) & ((tam > T) | (tam < -T))).sum())
        seen["nan_out"] += int(np.isnan(tau[AC.NAN_ROBOT]).sum())
        seen["strength"] += "strength" in names
        # sgn(+-0) = 0: with no command and no rate the friction terms vanish; a tiny rate of either sign feels the dry term
        assert (tau[8] == 0).all()
        if cfg["friction"]:
            dry = prm["dry_friction"][7] if "dry_friction" in names else m.cfg["dry_friction"]
            assert (tau[7, 0:2] == 0).all() and (dry == 0 or (tau[7, 2] < 0 and tau[7, 3] > 0))
        else:
            assert (tau[7] == 0).all()
        # the peak ignored the NaN robot's NaNs, and a NaN power counted 0 in e_pos
        assert np.isfinite(m.acc["tau_peak"][np.arange(AC.B) != AC.NAN_ROBOT]).all() and not np.isnan(m.acc["tau_peak"]).any()
        assert not np.isnan(m.acc["e_pos"][AC.NAN_ROBOT]) or np.isinf(eff[AC.NAN_ROBOT]).any()
    assert at == len(p) and all(v > 0 for v in seen.values()), seen


@no_hipcc
def test_model_header_indexes_the_ring_as_the_model_does(dump):
    """max_delay 0, 1, 5 and 64, 150 periods each: delays below 0 and above max_delay, the age below the delay at the start
    and after a reset in the middle, many more periods than rows.  The row, head and age are the model's, the row lies
    inside the ring (the program kept it in a heap array of exactly max_delay + 1 doubles under AddressSanitizer), and
    the value applied is the one stored min(clamp(delay), age) periods earlier."""
    r = dump[1]
    at = 0
    for D, seed in RING_CASES:
        delay, reset = _ring_script(D, seed)
        n = len(delay)
        got = r[at:at + n]
        at += n
        m = AM.ActModel(1, DT, dict(max_delay=D, friction=0))
        since = 0
        for c in range(n):
            if reset[c]:
                m.reset()
                since = 0
            m.set_params(delay=np.array([delay[c]], np.int32))
            head, age = int(m.head[0]), int(m.age[0])
            m.apply(np.full((1, 12), float(c)), np.zeros((1, 12)))
            back = min(min(max(int(delay[c]), 0), D), since)
            assert got[c].tolist() == [int(m.last_row[0]), head, age, c - back], (D, seed, c, got[c])
            assert 0 <= got[c][0] <= D and m.last_cmd[0, 0] == c - back and age == min(since, D)
            since += 1
        assert n > 2 * (D + 1) and (delay < 0).any() and (delay > D).any() and reset[70]
    assert at == len(r)


def test_identity_motor_is_the_rounding_of_its_chain():
    """friction 0, V and tau_max huge, delay 0: the output is the command through the divide and multiply chain -- within
    4 ulp of it, and exactly the model's value (asserted on the GPU)."""
    rng = np.random.default_rng(1)
    eff, qd = rng.uniform(-30, 30, (64, 12)), rng.uniform(-30, 30, (64, 12))
    m = AM.ActModel(64, DT, dict(friction=0, battery_v=1e300, tau_max=1e300))
    out = m.apply(eff, qd)
    assert (m.acc["n_vsat"] == 0).all() and (m.acc["n_tsat"] == 0).all()
    # vdes - bemf cancels to within an ulp of the LARGER of the two voltages: the bound is relative to that
    g = np.tile(np.asarray(m.cfg["gear"]), 4)[None, :]
    scale = np.maximum(np.abs(eff), np.abs(qd * g * 0.05 * 2.0) * (0.05 * 1.5) / 0.173 * g)
    # (eight roundings, each at most an ulp at that magnitude, doubled for a result just below a power of two)
    assert np.abs(out - eff).max() > 0 and (np.abs(out - eff) <= 16 * np.spacing(scale)).all()


# ---- the recorded closed loop ---------------------------------------------------------------------------------------------

def test_recorded_ladders_walk_and_fall_where_the_file_says():
    """tests/golden/act_closed_loop_cpu.json (tests/golden/make_act_closed_loop.py): the default motor keeps 16 of 16
    robots safe in both modes, every walking rung keeps 16 of 16, every falling rung loses at least one, and every
    ladder holds both kinds."""
    import act_loop as AL
    gold = json.load(open(GOLD))
    assert gold["ticks"] == L.TICKS == 650 and tuple(gold["pid"]) == L.PID and gold["freq"] == L.FREQ
    assert gold["config"] == json.loads(json.dumps(AM.config()))
    for mode in (0, 1):
        rec = gold[f"mode{mode}"]
        gait, vel, xyyaw = L.commands(mode)
        assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
        assert set(rec["ladders"]) == set(AL.LADDERS) == {"default", "tau_max", "delay", "battery_v"}
        d = rec["ladders"]["default"]["default"]
        assert d["walks"] and d["safe_count"] == 16 and d["safe"] == [1] * 16 and d["rc_bad"] == 0 and d["nwsr_max"] < 100
        for name, rungs in AL.LADDERS.items():
            rows = rec["ladders"][name]
            assert list(rows) == [r for r, _ in rungs]
            for (rname, actuator), row in zip(rungs, rows.values()):
                assert row["actuator"] == actuator and row["safe_count"] == sum(row["safe"])
                assert set(row["counters"]) == set(AM.ACCUMULATORS) and row["counters"]["n"] == [L.TICKS] * 16
                if row["walks"]:
                    assert row["safe_count"] == 16 and min(row["z_min"]) > 0.15 and max(row["roll_max"]) < 0.5, (mode, rname)
                else:
                    assert row["safe_count"] < 16, (mode, rname)
            if name != "default":
                walks = [row["walks"] for row in rows.values()]
                # a ladder runs from walking to falling: its last walking rung is followed by its first falling one
                assert walks[0] and not walks[-1] and walks == sorted(walks, reverse=True), (mode, name, walks)
        # the limits bite where they should: the cap ladder saturates the torque, the battery ladder the voltage
        lad = rec["ladders"]
        assert sum(lad["tau_max"]["tau_max_1.0"]["counters"]["n_tsat"]) > sum(d["counters"]["n_tsat"])
        assert sum(lad["battery_v"]["battery_v_2.0"]["counters"]["n_vsat"]) > 1000 > sum(d["counters"]["n_vsat"])
        assert min(d["counters"]["e_heat"]) > 0 and min(d["counters"]["tau_peak"]) > 0


@pytest.mark.parametrize("mode", [0, 1])
def test_a_short_rung_is_the_recorded_prefix(mode):
    """One rung (8 ticks of latency) run again for 130 ticks: the state and the accumulators are the file's, exactly, so
    the file cannot drift from the model."""
    import act_loop as AL
    gold = json.load(open(GOLD))
    lname, rname = gold["prefix_rung"]
    actuator = dict(AL.LADDERS[lname])[rname]
    stats, info = AL.cpu_loop_act(mode, ticks=gold["prefix_ticks"], trace=True, **actuator)
    want = gold[f"mode{mode}"]["prefix"]
    assert gold["prefix_ticks"] == 130 and info["rc_bad"] == 0
    assert np.array_equal(info["states"][-1], np.asarray(want["state"], np.float64))
    assert np.array_equal(info["safe"], want["safe"])
    for k in AM.ACCUMULATORS:
        assert np.array_equal(info["counters"][k], np.asarray(want["counters"][k], info["counters"][k].dtype)), k
    assert (info["counters"]["n"] == 130).all() and (info["counters"]["e_heat"] > 0).all()


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@no_hipcc
def test_act_kernel_resources(tmp_path):
    """The actuator kernel and its reset compile for gfx950, with the build's own flags, without scratch, spills or LDS
    (profiles/plant_kernel_resources.txt), and the translation unit is part of the build."""
    import __graft_entry__ as G
    assert "qmpc_act.hip" in G.OTHER_SOURCES
    src = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_act.hip")
    out = subprocess.run([HIPCC] + G.HIPFLAGS + ["-c", src, "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "act.o")],
                         capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    assert len(res) == 2 and all(any(k in n for n in res) for k in ("qmpc_act_kernel", "qmpc_act_reset_kernel")), sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)
