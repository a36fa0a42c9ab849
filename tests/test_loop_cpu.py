"""CPU suite for the loop run (include/qmpc_loop.h): the exported surface and the ABI version, the null-handle refusals,
the compiled resources of the loop kernel (csrc/qmpc_loop.hip), the single texts it shares with the per-tick kernels, and
the accumulation order of its four-lane actuator stage against the per-tick kernel's sixteen-lane order in a stand-alone
host program under the sanitizers (tests/loop_dump.cpp)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import act_cases as AC
import act_model as AM
import kernel_resources as KR
from c_headers import members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
NAMES = {"qmpc_loop_run", "qmpc_loop_run_info"}


def test_loop_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_loop.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = set(re.findall(r"^int (qmpc_\w+)\(", code, re.M))
    assert decl == NAMES == set(binding.LOOP_ENTRY_POINTS) == set(binding.LOOP_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert list(f.argtypes) == binding.LOOP_SIGNATURES[name] and f.restype is C.c_int
        args = re.search(r"^int %s\(([^)]*)\)" % name, code, re.M).group(1)
        assert len(args.split(",")) == len(binding.LOOP_SIGNATURES[name]), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the binding's structures and reason bits follow the header
    assert members(hdr, "qmpc_loop_opts") == [n for n, _ in binding.LoopOpts._fields_] == list(binding.LOOP_OPTS_FIELDS)
    assert members(hdr, "qmpc_loop_info") == [n for n, _ in binding.LoopInfo._fields_] == list(binding.LOOP_INFO_FIELDS)
    assert all(t is C.c_int for _, t in binding.LoopOpts._fields_)
    assert [t for _, t in binding.LoopInfo._fields_] == [C.c_longlong] * 4 + [C.c_int]
    bits = {k.lower(): int(v) for k, v in re.findall(r"QMPC_LOOP_(\w+) = (\d+)", hdr)}
    assert bits == binding.LOOP_REASONS == binding.FLEET_REASONS
    # the new symbols are in no older list and no older header; the new list is none of the twelve *EXPORTS tables
    older = [getattr(binding, n) for n in dir(binding) if n == "EXPORTS" or n.endswith("_EXPORTS")]
    assert len(older) == 12 and not any(NAMES & set(t) for t in older)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "qmpc_loop.h":
            assert "qmpc_loop" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert '#include "qmpc_episode.h"' in hdr
    # the Python surface
    assert hasattr(binding.BatchedController, "loop_info")
    sig = inspect.signature(binding.rollout_loop).parameters
    assert list(sig) == ["ctrl", "plant", "ticks", "graph", "actuators", "episodes", "every", "actuator_stats"]
    assert (sig["graph"].default, sig["actuators"].default, sig["episodes"].default, sig["every"].default,
            sig["actuator_stats"].default) == (False, None, None, 1, False)
    import __graft_entry__ as G
    assert "qmpc_loop.hip" in G.OTHER_SOURCES


def test_null_handle_and_null_pointers_are_refused():
    """Without a device every entry point refuses a null handle (QMPC_ERR_ARG), whatever else it is given."""
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    opts = binding.LoopOpts(1, 1, 1)
    assert lib.qmpc_loop_run(None, 4, 13, None, None, None, None, None) == 1
    assert lib.qmpc_loop_run(None, 4, 13, C.byref(opts), None, None, None, None) == 1
    assert lib.qmpc_loop_run_info(None, None) == 1
    info = binding.LoopInfo()
    assert lib.qmpc_loop_run_info(None, C.byref(info)) == 1


# ---- the kernel ------------------------------------------------------------------------------------------------------------

# The loop kernel's instantiations by <MODE, VARY, STATS> as the mangled name spells them, recorded from this build:
# VGPRs, AGPRs (the compiler's spill space), SGPR spills (to VGPR lanes), VGPR spills (to AGPRs), waves per SIMD
LOOP_TABLE = {"qmpc_loop_kernelILi0ELb0ELb0E": (256, 155, 114, 20, 1), "qmpc_loop_kernelILi0ELb0ELb1E": (256, 188, 126, 20, 1),
              "qmpc_loop_kernelILi0ELb1ELb0E": (256, 173, 173, 20, 1), "qmpc_loop_kernelILi0ELb1ELb1E": (256, 213, 195, 20, 1),
              "qmpc_loop_kernelILi1ELb0ELb0E": (256, 160, 124, 20, 1), "qmpc_loop_kernelILi1ELb0ELb1E": (256, 196, 136, 20, 1),
              "qmpc_loop_kernelILi1ELb1ELb0E": (256, 181, 183, 20, 1), "qmpc_loop_kernelILi1ELb1ELb1E": (256, 219, 228, 38, 1)}


@no_hipcc
def test_loop_kernel_resources(tmp_path):
    """The eight instantiations of the loop kernel (robot mode x VARY x STATS; the actuator stage and the episode step
    are run-time switches) compile for gfx950, with the build's own flags, without scratch and without LDS, at one
    wave per SIMD or more, inside the figures recorded from this build."""
    import __graft_entry__ as G
    res = KR.kernel_resources("qmpc_loop.hip", tmp_path, G.HIPFLAGS)
    assert len(res) == 8 and all(v["sgpr"] <= 106 and v["waves"] >= 1 for v in res.values()), res
    KR.hold(res, LOOP_TABLE)                                   # (scratch == 0 and lds == 0 for every row)


def test_loop_kernel_shares_its_stage_texts():
    """One text for every stage: the loop kernel includes E / C (functions), L, P and the decision (texts) once each,
    calls the shared reset bodies, and holds no copy of the motor's expressions."""
    text = open(os.path.join(CSRC, "qmpc_loop.hip")).read()
    code = re.sub(r"//.*", "", text)
    for inc in ("qmpc_plant_step_body.h", "qmpc_ctrl_loco_body.h", "qmpc_ctrl_stages.h", "qmpc_episode_decide_body.h",
                "qmpc_act_model.h", "qmpc_loop.h"):
        assert code.count('#include "%s"' % inc) == 1, inc
    for fn in ("qmpc_ctrl_est_state_body(", "qmpc_ctrl_legcmd_body(", "qmpc_ctrl_due_append(", "qmpc_act_joint(",
               "qmpc_act_sums_quad(", "qmpc_act_row(", "qmpc_act_next_head(", "qmpc_act_next_age(",
               "qmpc_ctrl_init_robot<true>(", "qmpc_ctrl_set_robot(", "plant_init_lane(", "plant_stats_reset_robot(",
               "qmpc_act_reset_robot("):
        assert code.count(fn) == 1, fn
    assert code.count("qmpc_act_energy(") == 3
    # nothing of qmpc_act_joint's body: no back-EMF, no coerce, no sgn, none of its names
    for word in ("bemf", "vdes", "vact", "k15", "ides", "qmpc_act_coerce", "qmpc_act_sgn", "M.kt *", "/ g", "tau_cmd"):
        assert word not in code, word
    # ... and the per-tick kernels call the same bodies
    for src, fns in (("qmpc_plant.hip", ("plant_init_lane(", "plant_stats_reset_robot(")),
                     ("qmpc_act.hip", ("qmpc_act_reset_robot(",)), ("qmpc_glue.hip", ("qmpc_ctrl_set_robot(",))):
        body = re.sub(r"//.*", "", open(os.path.join(CSRC, src)).read())
        for fn in fns:
            assert body.count(fn) == 1, (src, fn)
    # the span kernel's file is as it was: eight kernels of its own, none of the new stages
    span = open(os.path.join(CSRC, "qmpc_span.hip")).read()
    assert "qmpc_loop" not in span and "qmpc_act" not in span and "episode" not in span
    # the fp contraction is off in the kernel and in the stage body
    assert text.count("#pragma clang fp contract(off)") == 2


# ---- the accumulation order on the CPU under the sanitizers ------------------------------------------------------------------

def _hex(x):
    return " ".join("%016x" % int(u) for u in np.asarray(x, np.float64).reshape(-1).view(np.uint64))


DT = 1.0 / 500.0
CALLS = 3


def _cases():
    """act_cases' hostile periods (NaN, inf, zeros and denormals of both signs, every clamp), friction on and off, nothing
    bound and everything bound, three periods on accumulators that are not zero."""
    return [(fr, names, call) for fr in (1, 0) for names in ((), AM.PARAMS) for call in range(CALLS)]


@no_hipcc
def test_four_lane_order_is_the_sixteen_lane_order(tmp_path):
    """tests/loop_dump.cpp: csrc/qmpc_act_model.h alone, host only, built with AddressSanitizer and UBSan and run directly.
    For every robot-period of the case table the four-lane accumulation (three joints a lane, the twelve terms through
    emulated width-4 shuffles: qmpc_act_sums_quad, the loop kernel's own function) gives in EVERY lane of the quad the
    bits the sixteen-lane order gives: both counts, the peak and the three energies."""
    exe, cases = str(tmp_path / "loop_dump"), str(tmp_path / "cases.txt")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "loop_dump.cpp"), "-o", exe], check=True)
    syms = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms              # both runtimes are linked in
    prm = AC.params()
    n = 0
    with open(cases, "w") as f:
        for fr, names, call in _cases():
            c = AM.config(friction=fr)
            acc = np.random.default_rng(call).uniform(0.0, 5.0, (AC.B, 4)) * (call > 0)   # the accumulators found
            eff, qd = AC.period(call)
            for b in range(AC.B):
                val = lambda k: prm[k][b] if k in names else c[k]
                f.write("P %d %d %s %s %s %s\n" % (
                    c["friction"], "strength" in names,
                    _hex(list(c["gear"]) + [c["kt"], c["R"], val("battery_v"), val("tau_max"), val("damping"),
                                            val("dry_friction"), prm["strength"][b], DT]), _hex(acc[b]), _hex(eff[b]), _hex(qd[b])))
                n += 1
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr and run.stderr.startswith("records %d ok" % n), \
        run.stderr[-2000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) == 5 * n and [ln[0] for ln in lines[:5]] == ["S", "Q", "Q", "Q", "Q"]
    nan_rows = sat_rows = 0
    for k in range(n):
        s = lines[5 * k]
        for lane in range(4):
            q = lines[5 * k + 1 + lane]
            assert q[0] == "Q" and q[1:] == s[1:], (k, lane, s, q)
        energies = np.array([int(t, 16) for t in s[4:]], np.uint64).view(np.float64)
        nan_rows += int(np.isnan(energies).any())
        sat_rows += int(int(s[1]) > 0 and int(s[2]) > 0)
    # the table is hostile: periods whose sums are NaN (robot NAN_ROBOT of every case) and periods that saturate both ways
    assert nan_rows >= len(_cases()) and sat_rows >= len(_cases()), (nan_rows, sat_rows)
    eff, qd = AC.period(0)
    assert np.isnan(eff[AC.NAN_ROBOT]).any() and np.isinf(qd[AC.NAN_ROBOT]).any() and (np.abs(qd[6]) == AC.TINY).any()
