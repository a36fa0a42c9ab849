"""CPU suite: the LDS layout of the E tables (csrc/qmpc_etab.h) against the bank rules of the LDS, and the compiled shape of
stage 2's loads (tools/etab_shape.py).  No GPU.

Bank rules.  tests/etab_banks.cpp includes the header alone and replays, for one wave-instruction, how the LDS services it:

  ds_read_b128    four groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63};
                  bank of byte address a: (a / 4) mod 64
  ds_read2_b64    two accesses, each four groups of 16 contiguous lanes; bank (a / 4) mod 32

Inside a group identical addresses broadcast and every further distinct address on a busy bank costs one more LDS cycle.  The
figure checked is the worst number of distinct addresses on one bank in any group: 1 = free of conflicts.

Cases.  In stage 2 lane l of a wave owns matrix row i = l (+ 64 per further 64-row window of the larger classes) and reads
E[u][v] with u = 3 foot(i) + axis(i) from the robot's stance list (u = 0 on a padding row), v the wave's column: wave c of a 64-row
workgroup walks columns 16 c .. 16 c + 15, v = 3 foot(j) + axis(j) (a column beyond the list reads foot 0).  Contact tables at
h = 10: trot, pacing, bounding and standing at every gait iteration, and random tables (each foot-step in stance with
probability 1/2, as configs[4] draws them).  Every wave, every column it walks, and all twelve v besides.

The layout it replaced (u * 12 + v doubles, two tables 144 doubles apart, ds_read2_b64) must show its three-way conflict in
the same program: the test would have caught it.

Compiled shape, classes 1 and 6, between barrier 2 and the sweep: the E reads are 16-byte loads -- 16 per start axis of `fill`,
48 per copy of the solve -- and ds_read2_b64 does not exceed the parent commit's count there (class 1: 56 and 48 in its two
copies, class 6: 48 and 48, none of them 16-byte loads; counted on the parent's source with the same marker added behind
barrier 2, which changes no instruction.  With the pairs: 8 and 0, 0 and 0).
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import etab_shape  # noqa: E402
from engine_iter_shape import assembly  # noqa: E402
from quadruped_ctrl_amd.gait import mpc_table  # noqa: E402
from quadruped_ctrl_amd.workloads import GAITS_H10  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
H = 10
PARENT_READ2_B64 = {1: 56, 6: 48}   # ds_read2_b64 in a copy of stage 2 in the parent commit's build (its larger copy)
E_LOADS_PER_COPY = 3 * 16           # three start axes of `fill`, CW = 16 elements each


def tables():
    out = [mpc_table(H, *GAITS_H10[g], it) for g in ("trot", "pacing", "bounding", "standing") for it in range(H)]
    rng = np.random.default_rng(20310)
    for _ in range(8):
        g = (rng.random((H, 4)) < 0.5).astype(np.uint8)
        g[0, rng.integers(0, 4)] = 1
        out.append(g.reshape(-1))
    return out


def cases_of(table):
    """-> set of (u of lanes 0..63, v): what the waves of the workgroups that assemble this table read in one instruction."""
    sidx = np.flatnonzero(table)            # foot-step ids 4 k + foot of the stance list
    n = 3 * sidx.size
    out = set()
    for base in range(0, n, 64):            # a wave = 64 consecutive rows
        rows = np.arange(base, base + 64)
        u = np.where(rows < n, 3 * (sidx[np.minimum(rows // 3, sidx.size - 1)] & 3) + rows % 3, 0)
        vs = set(range(12))
        for j in range(64):                 # the columns the four waves of a 64-row workgroup walk
            slot = j // 3
            kj = sidx[slot] if slot < sidx.size else 4 * H
            vs.add(3 * (int(kj) & 3) + j % 3)
        out |= {(tuple(int(x) for x in u), v) for v in vs}
    return out


@pytest.fixture(scope="module")
def banks(tmp_path_factory):
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("etab") / "etab_banks")
    # host only, and the header alone: no HIP language, no device code, no runtime header
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "quadruped_ctrl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "etab_banks.cpp"), "-o", exe], check=True)

    def run(cases):
        text = "".join(" ".join(map(str, u)) + f" {v}\n" for u, v in sorted(cases))
        got = json.loads(subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout)
        assert got["cases"] == len(cases)
        return got

    return run


def test_every_table_is_free_of_conflicts(banks):
    cases = set()
    for t in tables():
        cases |= cases_of(t)
    got = banks(cases)
    print(got)
    assert got["cases"] >= 12 * 30          # (distinct lane maps of the tables, twelve columns each)
    assert got["pairs_b128"] == 1
    assert got["plain_read2_b64"] == 3      # (the layout this one replaced: caught)


def test_trot_alone_shows_the_old_conflict(banks):
    got = banks(cases_of(mpc_table(H, *GAITS_H10["trot"], 0)))
    print(got)
    assert got["pairs_b128"] == 1
    assert got["plain_read2_b64"] == 3
    assert got["plain_read_b64"] == 2       # (rows u and u + 8 on 64 banks)


def test_any_lane_to_row_map_is_free_of_conflicts(banks):
    rng = np.random.default_rng(20311)
    cases = {(tuple(int(x) for x in rng.integers(0, 12, 64)), int(v)) for v in range(12) for _ in range(20)}
    assert banks(cases)["pairs_b128"] == 1


@pytest.mark.parametrize("rb", [1, 6])
def test_stage2_reads_e_as_16_byte_pairs(rb):
    got = etab_shape.count(assembly(rb), rb)
    print(got)
    assert got["stages"]
    for st in got["stages"]:
        assert st["ds_read_b128"] >= E_LOADS_PER_COPY, st
        assert st["ds_read2_b64"] <= PARENT_READ2_B64[rb], st
