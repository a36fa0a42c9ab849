"""What the compiler says a .hip file's kernels need on gfx950 -- TEST SIDE ONLY.

kernel_resources(src, tmp_path) compiles one file with -Rpass-analysis=kernel-resource-usage and returns
{mangled kernel name: {vgpr, agpr, sgpr, sgpr_spill, vgpr_spill, scratch [B/lane], lds [B/block], waves [per SIMD]}}.
hold(res, table) holds the rows of profiles/plant_kernel_resources.txt: every figure an upper bound, the occupancy a
lower one, every kernel of the file in the table and the other way round.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value"]

_PATTERNS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r" AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"),
             ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
             ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))
COLUMNS = ("vgpr", "agpr", "sgpr_spill", "vgpr_spill", "waves")       # of a table's rows; scratch and LDS are 0 in all


def kernel_resources(src, tmp_path, flags=FLAGS):
    out = subprocess.run([HIPCC] + list(flags) + ["-c", os.path.join(CSRC, src), "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "k.o")], capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in _PATTERNS:
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


def hold(res, table):
    """table: {part of a mangled name that picks ONE kernel: (vgpr, agpr, sgpr_spill, vgpr_spill, waves)}."""
    seen = set()
    for part, row in table.items():
        got = [k for k in res if part in k]
        assert len(got) == 1, (part, sorted(res))
        seen.add(got[0])
        v = res[got[0]]
        print(got[0], v)
        want = dict(zip(COLUMNS, row))
        assert v["scratch"] == 0 and v["lds"] == 0, (got[0], v)
        assert all(v[c] <= want[c] for c in COLUMNS[:-1]) and v["waves"] >= want["waves"], (got[0], v, want)
    assert seen == set(res), sorted(set(res) - seen)
