"""CPU suite for the batched controller's MPC schedule (qmpc_ctrl_set_schedule, include/qmpc_ctrl.h): the entry point
is declared, exported and bound, the ABI version has not moved, and the arrays of the per-robot schedule are reachable
by name."""
import ctypes as C
import os
import re

from quadruped_ctrl_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_schedule_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "qmpc_ctrl.h")).read()
    decl = set(re.findall(r"^int (qmpc_[a-z_]+)\s*\(", hdr, re.M))
    assert "qmpc_ctrl_set_schedule" in decl
    assert re.search(r"enum\s*\{\s*QMPC_CTRL_LOCKSTEP\s*=\s*0\s*,\s*QMPC_CTRL_PER_ROBOT\s*=\s*1\s*\}", hdr)
    assert "qmpc_ctrl_set_schedule" in binding.CTRL_EXPORTS
    assert binding.CTRL_SIGNATURES["qmpc_ctrl_set_schedule"] == [C.c_void_p, C.c_int]
    assert binding.CTRL_SCHEDULES == dict(lockstep=0, per_robot=1)
    lib = C.CDLL(binding.LIB_PATH)
    assert hasattr(lib, "qmpc_ctrl_set_schedule")
    # the argument check needs no device: a null handle is refused (QMPC_ERR_ARG)
    lib.qmpc_ctrl_set_schedule.argtypes = [C.c_void_p, C.c_int]
    assert lib.qmpc_ctrl_set_schedule(None, 0) == 1
    assert lib.qmpc_ctrl_set_schedule(None, 1) == 1
    # purely additive: the ABI version stays
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    assert hasattr(binding.BatchedController, "set_schedule")


def test_due_arrays_are_in_the_controller_array_list():
    src = open(os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_glue.h")).read()
    body = re.search(r"#define QMPC_CTRL_ARRAYS\(X\)((?:.*\\\n)*.*)", src).group(1)
    arrays = {n: (t, int(w)) for t, n, w in re.findall(r"X\((\w+), (\w+), (\d+)\)", body)}
    assert arrays["due"] == ("int", 1)
    assert "due" in binding.CTRL_INT_ARRAYS
    # qmpc.h is left alone: the due list is internal, not a field of qmpc_command
    pub = open(os.path.join(ROOT, "include", "qmpc.h")).read()
    assert "due" not in re.search(r"typedef struct \{[^}]*\} qmpc_command;", pub, re.S).group(0)


def test_due_kernel_register_budget(tmp_path):
    """qmpc_solve_due_kernel (the first class over a due list) has the first-class kernel's body: within the 128 VGPRs of
    four waves per SIMD and without scratch, like the other cold instantiations of the 64-row class (test_build_cpu.py)."""
    import shutil
    import subprocess
    import pytest
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_kernels.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-DQMPC_RB=1", "-c", src,
                          "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k1.o")],
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
    due = {k: v for k, v in res.items() if "qmpc_solve_due_kernel" in k}
    assert len(due) == 1
    for k, v in due.items():
        assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)
