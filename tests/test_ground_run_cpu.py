"""CPU suite for the ground-run switch (include/qmpc_ground_run.h): the exported surface and the ABI version, the
null-handle refusals, the host's choice of kernel and reason for every combination of switch, bindings and options in a
stand-alone host program (tests/run_pick_dump.cpp), and the compiled resources of the loop kernel's two ground compiles
(csrc/qmpc_loop.hip with QMPC_LOOP_GROUND 1 and 2)."""
import ctypes as C
import itertools
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
NAMES = {"qmpc_ground_run_enable", "qmpc_ground_run_enabled"}


def test_ground_run_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_ground_run.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = set(re.findall(r"^int (qmpc_\w+)\(", code, re.M))
    assert decl == NAMES == set(binding.GROUND_RUN_ENTRY_POINTS) == set(binding.GROUND_RUN_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert list(f.argtypes) == binding.GROUND_RUN_SIGNATURES[name] and f.restype is C.c_int
        args = re.search(r"^int %s\(([^)]*)\)" % name, code, re.M).group(1)
        assert len(args.split(",")) == len(binding.GROUND_RUN_SIGNATURES[name]), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the new symbols are in none of the twelve *EXPORTS tables, and the new tables are none of them
    older = [getattr(binding, n) for n in dir(binding) if n == "EXPORTS" or n.endswith("_EXPORTS")]
    assert len(older) == 12 and not any(NAMES & set(t) for t in older)
    # the header speaks of the two run calls in words: their names stay in their own headers, which keep two declarations
    assert "qmpc_fleet" not in hdr and "qmpc_loop" not in hdr
    for h, want in (("qmpc_fleet.h", {"qmpc_fleet_run", "qmpc_fleet_run_info"}), ("qmpc_loop.h", {"qmpc_loop_run", "qmpc_loop_run_info"})):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "qmpc_ground_run.h" in text, h                       # ... and point to this one by file name
        assert set(re.findall(r"^int (qmpc_\w+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.M)) == want, h
    # the Python surface
    assert callable(binding.BatchedController.set_ground_run) and isinstance(binding.BatchedController.ground_run, property)
    # the two ground compiles are jobs of the build, not files: csrc's sources are the build's list
    import __graft_entry__ as G
    hips = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))}
    assert hips == set(G.OTHER_SOURCES) | {"qmpc_kernels.hip", "convex_mpc_shim.cpp"}, sorted(hips ^ set(G.OTHER_SOURCES))


def test_null_handle_and_null_pointer_are_refused():
    """Without a device both entry points refuse a null handle (QMPC_ERR_ARG), whatever else they are given."""
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    on = C.c_int(7)
    assert lib.qmpc_ground_run_enable(None, 0) == 1 and lib.qmpc_ground_run_enable(None, 1) == 1
    assert lib.qmpc_ground_run_enabled(None, None) == 1 and lib.qmpc_ground_run_enabled(None, C.byref(on)) == 1
    assert on.value == 7


# ---- the host's choice ---------------------------------------------------------------------------------------------------------

TERRAIN, CONTACT, FIELD = 1, 2, 4                                # the reason bits of both run headers


def rule(switch, rows, contact, field, actuators, episodes):
    """include/qmpc_ground_run.h, written out.  Switch off: every bound ground and ground-decided contact is a reason,
    and any reason is the per-tick path -- today's behaviour.  Switch on: the fused kernels cover rows and a field, so
    the only reason left is the contact bit, alone.  Without a reason: a field takes the field compile of the loop
    kernel whatever else is bound, rows without one the terrain compile, with any options or none; the flat plant takes
    the loop kernel where an option is set and the span kernel where none is."""
    if switch:
        reason = CONTACT if contact else 0
    else:
        reason = (TERRAIN if rows else 0) | (CONTACT if contact else 0) | (FIELD if field else 0)
    if reason:
        return "per_tick", reason
    if field:
        return "loop_field", 0
    if rows:
        return "loop_terrain", 0
    return ("loop" if actuators or episodes else "span"), 0


@no_hipcc
def test_kernel_and_reason_for_every_combination(tmp_path):
    """tests/run_pick_dump.cpp: csrc/qmpc_run_pick.h alone, host only.  All 64 combinations of (switch, rows, contact,
    field, actuators, episodes) against rule() above; with the switch off every bound ground gives today's reason bits
    and the per-tick path."""
    from quadruped_ctrl_amd import binding
    assert binding.FLEET_REASONS == binding.LOOP_REASONS == dict(terrain=TERRAIN, contact=CONTACT, field=FIELD)
    exe = str(tmp_path / "run_pick_dump")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "run_pick_dump.cpp"), "-o", exe],
                   check=True)
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    keys = ("switch", "rows", "contact", "field", "actuators", "episodes")
    assert [tuple(g[k] for k in keys) for g in got] == list(itertools.product((0, 1), repeat=6))
    for g in got:
        assert (g["kernel"], g["reason"]) == rule(*(g[k] for k in keys)), g
    # ... spelled out for the switch off: a bound ground is never served fused, and the flat plant is served as it was
    off = [g for g in got if not g["switch"]]
    for g in off:
        bound = g["rows"] or g["contact"] or g["field"]
        assert (g["kernel"] == "per_tick") == bool(bound), g
        assert g["reason"] == g["rows"] * TERRAIN + g["contact"] * CONTACT + g["field"] * FIELD, g
    # ... and for the switch on: every ground with scheduled contact is fused, contact decided by the ground never is
    on = [g for g in got if g["switch"]]
    assert all(g["kernel"] in ("loop_terrain", "loop_field") and g["reason"] == 0
               for g in on if (g["rows"] or g["field"]) and not g["contact"])
    assert all(g["kernel"] == "per_tick" and g["reason"] == CONTACT for g in on if g["contact"])
    # the capi unit asks this function and holds no reason expression of its own
    capi = re.sub(r"//.*", "", open(os.path.join(CSRC, "qmpc_capi_ctrl.cpp")).read())
    assert capi.count("qmpc_run_pick(") == 1 and "QMPC_FLEET_TERRAIN :" not in capi and "QMPC_LOOP_TERRAIN :" not in capi


# ---- the two ground compiles ---------------------------------------------------------------------------------------------------

# The loop kernel's instantiations by <MODE, VARY, STATS> as the mangled name spells them, recorded from this build
# (profiles/plant_kernel_resources.txt): VGPRs, AGPRs (the compiler's spill space), SGPR spills (to VGPR lanes), VGPR spills
# (to AGPRs), scratch bytes per lane, waves per SIMD
GROUND_TABLES = {
    1: {"qmpc_loop_kernelILi0ELb0ELb0E": (256, 162, 114, 38, 0, 1), "qmpc_loop_kernelILi0ELb0ELb1E": (256, 198, 124, 38, 0, 1),
        "qmpc_loop_kernelILi0ELb1ELb0E": (256, 190, 171, 44, 0, 1), "qmpc_loop_kernelILi0ELb1ELb1E": (256, 230, 189, 42, 0, 1),
        "qmpc_loop_kernelILi1ELb0ELb0E": (256, 166, 126, 38, 0, 1), "qmpc_loop_kernelILi1ELb0ELb1E": (256, 204, 138, 38, 0, 1),
        "qmpc_loop_kernelILi1ELb1ELb0E": (256, 198, 207, 42, 0, 1), "qmpc_loop_kernelILi1ELb1ELb1E": (256, 238, 208, 44, 0, 1)},
    2: {"qmpc_loop_kernelILi0ELb0ELb0E": (256, 173, 120, 38, 0, 1), "qmpc_loop_kernelILi0ELb0ELb1E": (256, 213, 130, 40, 0, 1),
        "qmpc_loop_kernelILi0ELb1ELb0E": (256, 208, 179, 46, 0, 1), "qmpc_loop_kernelILi0ELb1ELb1E": (256, 247, 207, 46, 0, 1),
        "qmpc_loop_kernelILi1ELb0ELb0E": (256, 181, 132, 42, 0, 1), "qmpc_loop_kernelILi1ELb0ELb1E": (256, 221, 144, 38, 0, 1),
        "qmpc_loop_kernelILi1ELb1ELb0E": (256, 216, 195, 48, 0, 1), "qmpc_loop_kernelILi1ELb1ELb1E": (256, 255, 214, 48, 0, 1)},
}
COLUMNS = ("vgpr", "agpr", "sgpr_spill", "vgpr_spill", "scratch", "waves")


def hold_with_scratch(res, table):
    """kernel_resources.hold with a stated scratch figure per row: every figure an upper bound -- the scratch too, which is
    0 in every row recorded so far -- the occupancy a lower one, LDS 0, every kernel in the table and the other way
    round."""
    seen = set()
    for part, row in table.items():
        got = [k for k in res if part in k]
        assert len(got) == 1, (part, sorted(res))
        seen.add(got[0])
        v, want = res[got[0]], dict(zip(COLUMNS, row))
        print(got[0], v)
        assert v["lds"] == 0, (got[0], v)
        assert all(v[c] <= want[c] for c in COLUMNS[:-1]) and v["waves"] >= want["waves"], (got[0], v, want)
    assert seen == set(res), sorted(set(res) - seen)


@no_hipcc
@pytest.mark.parametrize("ground", [1, 2], ids=["terrain", "field"])
def test_ground_compile_resources(tmp_path, ground):
    """csrc/qmpc_loop.hip under the build's flags with -DQMPC_LOOP_GROUND: eight kernels (robot mode x VARY x STATS), no
    LDS, one wave per SIMD or more, inside the rows recorded from this build -- which hold no scratch."""
    import __graft_entry__ as G
    res = KR.kernel_resources("qmpc_loop.hip", tmp_path, G.HIPFLAGS + ["-DQMPC_LOOP_GROUND=%d" % ground])
    assert len(res) == 8 and all("qmpc_loop_kernel" in k for k in res), sorted(res)
    assert all(v["lds"] == 0 and v["sgpr"] <= 106 and v["waves"] >= 1 for v in res.values()), res
    hold_with_scratch(res, GROUND_TABLES[ground])


def test_build_compiles_the_loop_kernel_three_times_and_shares_the_reset():
    """The ground compiles are two more jobs on the same source beside the size classes; the launcher's name follows the
    define and is declared once; the ground reset is one function behind both init kernels and the loop kernel's
    stage R."""
    import __graft_entry__ as G
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    # the built library holds all three compiles' launchers, from ONE source file of the build's list
    for name in ("qmpc_launch_loop", "qmpc_launch_loop_terrain", "qmpc_launch_loop_field"):
        assert hasattr(lib, name), name
    assert G.OTHER_SOURCES.count("qmpc_loop.hip") == 1
    strip = lambda f: re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
    loop, hdr = strip("qmpc_loop.hip"), strip("qmpc_loop.h")
    for name in ("qmpc_launch_loop_terrain", "qmpc_launch_loop_field"):
        assert loop.count(name) == 1 and hdr.count(name + "(") == 1, name
    for f in ("qmpc_loop.hip", "qmpc_terrain.hip", "qmpc_field.hip"):
        assert strip(f).count("plant_ground_init_lane<") == 1, f
    dev = strip("qmpc_plant_dev.h")
    body = dev[dev.index("void plant_ground_init_lane("):]
    assert body[body.index("{"):].lstrip("{ \n").startswith("#pragma clang fp contract(off)")
    assert "QMPC_LOOP_GROUND" not in strip("qmpc_span.hip")          # the fleet run on ground is the loop kernel's
