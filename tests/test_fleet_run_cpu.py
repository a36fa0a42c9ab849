"""CPU suite for the fleet run (include/qmpc_fleet.h): the exported surface and the ABI version, the host plan of a call
(csrc/qmpc_span.h, through tests/span_dump.cpp) against the rule stated here, and the compiled resources of the span kernel
(csrc/qmpc_span.hip) and of the per-tick kernels whose bodies it shares (csrc/qmpc_ctrl_stages.h)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import kernel_resources as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")


def test_fleet_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_fleet.h")).read()
    decl = set(re.findall(r"^int (qmpc_\w+)\(", hdr, re.M))
    want = {"qmpc_fleet_run", "qmpc_fleet_run_info"}
    assert decl == want == set(binding.FLEET_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert list(f.argtypes) == binding.FLEET_SIGNATURES[name] and f.restype is C.c_int
        args = re.search(r"^int %s\(([^)]*)\)" % name, hdr, re.M).group(1)
        assert len(args.split(",")) == len(binding.FLEET_SIGNATURES[name]), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the binding's structure and reason bits follow the header
    body = re.search(r"typedef struct \{([^}]*)\} qmpc_fleet_info;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in binding.FleetInfo._fields_] == list(binding.FLEET_INFO_FIELDS)
    bits = {k.lower(): int(v) for k, v in re.findall(r"QMPC_FLEET_(\w+) = (\d+)", hdr)}
    assert bits == binding.FLEET_REASONS
    # none of the new symbols went into an older header or list
    older = (set(binding.EXPORTS) | set(binding.CTRL_EXPORTS) | set(binding.PLANT_EXPORTS) | set(binding.PLANT_VARY_EXPORTS)
             | set(binding.ACT_EXPORTS))
    assert not older & want
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "qmpc_fleet.h":
            assert "qmpc_fleet" not in open(os.path.join(ROOT, "include", h)).read(), h
    # without a device every entry point refuses a null handle or pointer (QMPC_ERR_ARG)
    assert lib.qmpc_fleet_run(None, 4, 13, None, None, None, None) == 1
    assert lib.qmpc_fleet_run_info(None, None) == 1
    assert hasattr(binding.BatchedController, "fleet_info")
    import inspect
    assert inspect.signature(binding.rollout).parameters["fused"].default is False
    import __graft_entry__ as G
    assert "qmpc_span.hip" in G.OTHER_SOURCES


# ---- the plan --------------------------------------------------------------------------------------------------------------

def rule(T, ticks, per_robot):
    """The plan of a call, from the definition of a span: tick k of the call solves behind its L where the incremented
    count is a multiple of 13 (lockstep) or always (per robot); a launch runs from where the last one stopped -- the head
    of tick 0, or C of the tick that has just solved -- up to L of the next tick that solves, or to the call's end."""
    solves = [k for k in range(ticks) if per_robot or (T + k + 1) % 13 == 0]
    plan, start = [], (0, 0)                                    # start: (tick, 1 when the tick's E and L have run)
    for stop in solves + [None]:
        end = ticks - 1 if stop is None else stop
        locos = end - start[0] + 1 - start[1]
        plan.append([start[1], end - start[0] + 1, int(stop is not None), locos, int(per_robot and locos > 0), int(stop is not None)])
        start = (end, 1)
    return plan


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("span") / "span_dump")
    # host only, and the header alone: no HIP language, no device code, no runtime header
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "span_dump.cpp"), "-o", exe],
                   check=True)
    return json.loads(subprocess.run([exe, "25", "1", "12", "13", "14", "40"], check=True, capture_output=True, text=True).stdout)


@no_hipcc
def test_plan_is_the_rule(plans):
    assert len(plans) == 2 * 26 * 5
    for p in plans:
        assert p["launches"] == rule(p["T"], p["ticks"], bool(p["per_robot"])), p


@no_hipcc
def test_plan_by_hand(plans):
    """A few plans written out: [first_at_c, ticks touched, last_after_l, L stages, reset the due count, solve follows]."""
    got = {(p["per_robot"], p["T"], p["ticks"]): p["launches"] for p in plans}
    # T = 5 (mid-period), 40 ticks: solves behind L of ticks 7, 20 and 33 of the call (T + k + 1 = 13, 26, 39)
    assert got[0, 5, 40] == [[0, 8, 1, 8, 0, 1], [1, 14, 1, 13, 0, 1], [1, 14, 1, 13, 0, 1], [1, 7, 0, 6, 0, 0]]
    # a whole period from T = 0: E .. L of tick 12, the solve, C and P of tick 12
    assert got[0, 0, 13] == [[0, 13, 1, 13, 0, 1], [1, 1, 0, 0, 0, 0]]
    # twelve ticks between two solves: one launch, no solve
    assert got[0, 0, 12] == [[0, 12, 0, 12, 0, 0]]
    # one tick that solves (T = 12) and one that does not
    assert got[0, 12, 1] == [[0, 1, 1, 1, 0, 1], [1, 1, 0, 0, 0, 0]]
    assert got[0, 3, 1] == [[0, 1, 0, 1, 0, 0]]
    # per robot: E, L | solve | C, P, E, L | solve | ... | C, P -- one launch and one solve per tick, and the last C, P
    assert got[1, 7, 1] == [[0, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0]]
    assert got[1, 0, 13] == [[0, 1, 1, 1, 1, 1]] + [[1, 2, 1, 1, 1, 1]] * 12 + [[1, 1, 0, 0, 0, 0]]
    for p in plans:                                           # every L once, every call ends behind a P
        assert sum(l[3] for l in p["launches"]) == p["ticks"] and p["launches"][-1][2] == 0, p
        assert all(1 <= l[1] <= 14 for l in p["launches"]) or p["per_robot"], p


# ---- the kernels -----------------------------------------------------------------------------------------------------------

# The span kernel's instantiations by <MODE, VARY, STATS> as the mangled name spells them:
# VGPRs, AGPRs (the compiler's spill space), SGPR spills (to VGPR lanes), VGPR spills (to AGPRs), waves per SIMD
SPAN_TABLE = {"qmpc_span_kernelILi0ELb0ELb0E": (256, 111, 63, 8, 1), "qmpc_span_kernelILi0ELb0ELb1E": (256, 151, 67, 8, 1),
              "qmpc_span_kernelILi0ELb1ELb0E": (256, 147, 117, 8, 1), "qmpc_span_kernelILi0ELb1ELb1E": (256, 183, 135, 8, 1),
              "qmpc_span_kernelILi1ELb0ELb0E": (256, 125, 75, 8, 1), "qmpc_span_kernelILi1ELb0ELb1E": (256, 163, 73, 8, 1),
              "qmpc_span_kernelILi1ELb1ELb0E": (256, 159, 127, 8, 1), "qmpc_span_kernelILi1ELb1ELb1E": (256, 195, 153, 8, 1)}


@no_hipcc
def test_span_kernel_resources(tmp_path):
    """The eight instantiations of the span kernel (robot mode x VARY x STATS) compile for gfx950, with the build's own
    flags, without scratch and without LDS: the issue's condition.  The figures DESIGN.md section 0 and INTEGRATION.md G
    record are held as upper bounds: 256 VGPRs, 106 SGPRs, the AGPRs the compiler spills into (111 for the plain
    lockstep kernel to 195 with everything on), the spills beside them, and -- a whole register file -- exactly one wave
    per SIMD."""
    import __graft_entry__ as G
    res = KR.kernel_resources("qmpc_span.hip", tmp_path, G.HIPFLAGS)
    assert len(res) == 8 and all(v["sgpr"] <= 106 and v["waves"] == 1 for v in res.values()), res
    KR.hold(res, SPAN_TABLE)
    # one text for the stages: the span kernel holds no copy of its own
    text = open(os.path.join(CSRC, "qmpc_span.hip")).read()
    for inc in ("qmpc_plant_step_body.h", "qmpc_ctrl_loco_body.h", "qmpc_ctrl_stages.h"):
        assert text.count('#include "%s"' % inc) == 1, inc
    for fn in ("qmpc_ctrl_est_state_body(", "qmpc_ctrl_legcmd_body(", "qmpc_ctrl_due_append("):
        assert text.count(fn) == 1, fn
    assert "due_count" not in re.sub(r"//.*", "", text)      # the span's E does not reset the fleet-wide word


@no_hipcc
def test_per_tick_kernels_keep_their_resources(tmp_path):
    """The per-tick kernels whose bodies are now shared with the span kernel compile to the parent's figures: the
    estimator 66 VGPRs, the leg command 39, the locomotion kernel 84 in robot mode 0 and 121 in mode 1, at the parent's
    waves per SIMD and SGPRs, none with scratch.  (E and C are functions of qmpc_ctrl_stages.h; L is the text
    qmpc_ctrl_loco_body.h, because as a function it cost the mode-0 kernel 92 VGPRs.  The plant kernels' figures are held
    by tests/test_plant_varied_cpu.py, which is unchanged.)"""
    import __graft_entry__ as G
    res = KR.kernel_resources("qmpc_glue.hip", tmp_path, G.HIPFLAGS)
    pick = lambda part: [v for k, v in res.items() if part in k]
    for part, vgpr, sgpr, waves in (("qmpc_ctrl_est_state_kernel", 66, 29, 7), ("qmpc_ctrl_legcmd_kernel", 39, 30, 8),
                                    ("qmpc_ctrl_loco_kernelILi0E", 84, 92, 5), ("qmpc_ctrl_loco_kernelILi1E", 121, 92, 4)):
        got = pick(part)
        assert len(got) == 1, part
        print(part, got[0])
        assert (got[0]["vgpr"], got[0]["sgpr"], got[0]["waves"], got[0]["scratch"]) == (vgpr, sgpr, waves, 0), (part, got[0])
    # the kernels use the shared bodies and hold no second copy
    glue = open(os.path.join(CSRC, "qmpc_glue.hip")).read()
    for fn in ("qmpc_ctrl_est_state_body(", "qmpc_ctrl_legcmd_body(", "qmpc_ctrl_due_append(", '#include "qmpc_ctrl_loco_body.h"'):
        assert glue.count(fn) == 1, fn
    assert "ConvexMPCLocomotion::run" not in re.sub(r"//.*", "", glue) and "S.swing_rem" not in glue
    stages = open(os.path.join(CSRC, "qmpc_ctrl_stages.h")).read()
    for fn in ("qmpc_ctrl_est_state_body", "qmpc_ctrl_legcmd_body"):
        body = re.search(r"%s\([^)]*\) \{\n(.*?)\n" % fn, stages, re.S).group(1)
        assert body == "#pragma clang fp contract(off)", fn
    loco = open(os.path.join(CSRC, "qmpc_ctrl_loco_body.h")).read()
    assert "S.swing_rem" in loco and not re.search(r"\breturn\b", re.sub(r"//.*", "", loco))
