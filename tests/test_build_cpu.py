"""CPU suite: compile-time budgets of the solve kernels (hipcc cross-compiles gfx950 without a GPU).

The occupancy the design relies on is a property of the compiled code, not of the source: four 64-row workgroups
per CU need <= 128 VGPRs and no scratch, two 96-row workgroups (6 waves each) need <= 128 VGPRs too -- at 137 only one
fits and the class is 45 % slower, which no functional test notices."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_kernels.hip")


def _resources(rb, tmp):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", f"-DQMPC_RB={rb}", "-c", SRC,
                          "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, f"k{rb}.o")],
                         capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_register_budgets(tmp_path):
    with ThreadPoolExecutor(2) as ex:
        r1, r4 = ex.map(lambda rb: _resources(rb, str(tmp_path)), (1, 4))
    solve1 = {k: v for k, v in r1.items() if "qmpc_solve_kernel" in k}
    solve4 = {k: v for k, v in r4.items() if "qmpc_solve_kernel" in k}
    assert len(solve1) == 3 and len(solve4) == 6          # record / command / warm (x list-consuming for class 4)
    for k, v in {**solve1, **solve4}.items():
        warm = "ELb1ELb0EEv" in k or "ELb1ELb1EEv" in k    # <RB, CMD, WARM, LISTED>: the optional warm-start instantiations
        # (round 6: the list-consuming COMMAND-mode instantiation of the 96-row class -- qmpc_solve_commands behind a 64-row
        #  first class, at the 128-register limit with 139 scalar registers spilled to VGPR lanes -- parks three dwords in scratch:
        #  two stores and two loads per robot, between the sweep and the engine (the parameter block grew by the size order's
        #  fields); every other instantiation of the two classes: none)
        few_per_robot = k.startswith("_Z17qmpc_solve_kernelILi4ELb1ELb0ELb1E")
        assert v["scratch"] <= (32 if warm else (16 if few_per_robot else 0)), (k, v)
        assert v["vgpr"] <= 128, (k, v)                    # 4 waves per SIMD: 4 (class 1) / 2 (class 4) workgroups per CU


def test_every_source_is_built():
    """build() compiles the files it lists: a .hip or .cpp in csrc/ that it does not list is never linked (its entry
    points would be missing from the library), and a listed file that is gone fails the build."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    csrc = os.path.dirname(SRC)
    present = {f for f in os.listdir(csrc) if f.endswith((".hip", ".cpp"))}
    # (qmpc_kernels.hip: once per size class; convex_mpc_shim.cpp: a library of its own)
    assert present - {"qmpc_kernels.hip", "convex_mpc_shim.cpp"} == set(G.OTHER_SOURCES)
    assert len(set(G.OTHER_SOURCES)) == len(G.OTHER_SOURCES)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_cold_build_from_sources(tmp_path):
    """build() must not depend on binaries that happen to be on disk.  A COLD build -- every
    translation unit of every size class compiled from the sources into an empty directory, linked, the shim linked
    against it -- and the result exports every symbol the headers declare (same check as the in-tree library)."""
    import ctypes as C
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    from quadruped_ctrl_amd import binding
    out = str(tmp_path / "cold")
    os.makedirs(out)
    lib = G.build(out_dir=out)
    assert os.path.dirname(lib) == out and os.path.getsize(lib) > 1 << 20
    objs = sorted(os.listdir(os.path.join(out, "obj")))
    assert [o for o in objs if o.startswith("qmpc_kernels_c")] == [f"qmpc_kernels_c{rb}.o" for rb in (1, 2, 3, 4, 6)]
    dll = C.CDLL(lib)
    # every header's surface, not the solve's alone: a host unit missing from the link shows here
    tables = [t for t in vars(binding) if t == "EXPORTS" or t.endswith("_EXPORTS")]
    assert len(tables) == 12, tables
    names = {n for t in tables for n in getattr(binding, t)} | {"qmpc_debug_ctrl_read"}
    assert set(binding.EXPORTS) < names
    for name in sorted(names):
        assert hasattr(dll, name), name
    shim = C.CDLL(os.path.join(out, "libconvexmpc_shim.so"))
    for name in ("setup_problem", "update_problem_data", "update_problem_data_floats", "update_solver_settings",
                 "get_solution", "_Z13update_x_dragf", "qmpc_shim_last_status"):
        assert hasattr(shim, name), name
