"""CPU suite: the launch plan of a solve (csrc/qmpc_plan.h: plan_solve) is a value computed by host-only integer logic, so
it is pinned here without a device.  tests/plan_dump.cpp includes the header alone and prints the plans of fixed
scenarios; the expected plans below were derived by hand from the launch rules (each with the rule beside it), with
these occupancy numbers as inputs: resident workgroups of class 1: 1024, class 6: 1280, class 4: 512, classes 2 / 3: 256;
sweep kernels 2 / 3: 256; engines 2: 512, 3 / 5: 256."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# counter indices of a set (csrc/qmpc_device.h)
CNT_BIGLIST, CNT_FB, CNT_FBQ, CNT_DUEQ = 3, 8, 12, 18
DUE_COUNT = -2          # the due list's length: the caller's, not a counter of the set
FALLBACK = 16           # QMPC_DEV_ST_FALLBACK
UNBOUNDED = 0x7fffffff


def grp(sk, g):
    """first counter of group g of item pool sk (QMPC_CNT_GRP)"""
    return 64 + 32 * (2 * sk + g)


DEFAULT = dict(cls=0, grid=0, list="none", next="none", count=-1, qhead=-1, next_count=-1, clear_counts=0, status_or=0,
               sk=-1, rid0=0, list_hi=0, grp=0, wk_zero=0, hint_hard=0, hint_max=[-1, -1, -1], so_first=0, so_nseg=0,
               so_tag=0, so_maxfit=0, so_keys_from_hint=0, prio_tag=0)


def L(kind, **kw):
    assert set(kw) <= set(DEFAULT)
    return dict(DEFAULT, kind=kind, **kw)


def handback(sk, grid):
    """the monolithic kernel on the robots the engine of pool sk handed back (the large problems have no class to fall
    back to: no status bit)"""
    return L("SOLVE", cls=2 if sk == 0 else 3, grid=grid, list=f"fb{sk}", count=CNT_FB + sk, qhead=CNT_FBQ + sk, sk=sk,
             list_hi=UNBOUNDED, status_or=0 if sk == 2 else FALLBACK)


def size_order(first, tag, from_hint=0):
    """8 segments (at most 32640 robots to order), 64 / 3 = 21 foot-steps fit the 64-row class"""
    return dict(so_first=first, so_nseg=8, so_tag=tag, so_maxfit=21, so_keys_from_hint=from_hint)


# name -> (counter set, leaves the order hint, (call_no, hint_call, so_call, prio_call) after the call, launches)
EXPECTED = {
    # 1. handle 1024, batch 1024, h = 10, stance 20..20 (60 rows: the 64-row class alone; handle < 2048: class 1)
    #    one round (1024 <= 1024 resident), 2 * batch > round: hint_max slots (hc + 2, hc, hc + 1) % 3 with hc = 0; no previous
    #    call: hint_hard 0, so the priority staging applies (8 * 1024 > 7 * 1024): tag 1
    "s1_call1": (0, 1, (1, 1, 0, 1), [L("SOLVE", cls=1, grid=1024, clear_counts=1, hint_max=[2, 0, 1], prio_tag=1)]),
    #    second call of the same batch: set 1, hc = 1, hint_hard 5, hence no staging
    "s1_call2": (1, 1, (2, 2, 0, 1), [L("SOLVE", cls=1, grid=1024, clear_counts=1, hint_hard=5, hint_max=[0, 1, 2])]),
    # 2. handle 16384 (>= 2048: class 6, 1280 resident): 12.8 rounds, the last five ordered: so_first = 16384 - 5 * 1280
    "s2_call1": (0, 1, (1, 0, 1, 0), [L("SOLVE", cls=6, grid=16384, clear_counts=1, **size_order(9984, 1))]),
    #    second call: keys from the hint; the head (1280 + 640) is below the five-round tail
    "s2_call2": (1, 1, (2, 0, 2, 0), [L("SOLVE", cls=6, grid=16384, clear_counts=1, **size_order(9984, 2, 1))]),
    #    batch 2048 after a call of another size: by size, no unsorted head: so_first = 1280
    "s2_b2048_call1": (0, 1, (3, 0, 3, 0), [L("SOLVE", cls=6, grid=2048, clear_counts=1, **size_order(1280, 3))]),
    #    ... and again: by the hint, head min((2048 - 1280) / 2, 640) = 384: (1280 + 384 + 7) & ~7
    "s2_b2048_call2": (1, 1, (4, 0, 4, 0), [L("SOLVE", cls=6, grid=2048, clear_counts=1, **size_order(1664, 4, 1))]),
    # 3. the controller's per-robot tick: handle 256, h = 14 (168 rows: all four classes), command mode, due list.
    #    A due-list call runs on set 2 behind a fill, clears nothing, orders nothing and leaves no hint; class 2 is not split
    #    (256 < 384), class 3 is (256 >= 128): one chunk, then its event flags and the hand-back launch
    "s3_due_tick": (2, 0, (0, 0, 0, 0), [
        L("FILL_COUNTERS"),
        L("SOLVE", cls=1, grid=256, list="due", count=DUE_COUNT, qhead=CNT_DUEQ, next="slot0", next_count=0),
        L("SOLVE", cls=4, grid=256, list="slot0", count=0, qhead=4, next="slot1", next_count=1),
        L("SOLVE", cls=2, grid=256, list="slot1", count=1, qhead=5, next="slot2", next_count=2),
        L("SWEEP", cls=3, grid=256, list="slot2", count=2, qhead=grp(1, 0) + 2, sk=1, list_hi=256),
        L("ENGINE", cls=3, grid=256, sk=1, list_hi=256),
        L("FILL_EVFLAGS"),
        handback(1, 256)]),
    # 4. scenario 1 captured: set 2 behind a fill; no clear_counts, hint, size order or staging; no host counter moves
    "s4_captured": (2, 0, (0, 0, 0, 0), [L("FILL_COUNTERS"), L("SOLVE", cls=1, grid=1024)]),
    #    the staging's call number wraps to 0: the words are cleared and the tag starts again at 1
    "s4_prio_wrap": (0, 1, (1, 1, 0, 1), [L("FILL_PRIO"),
                                          L("SOLVE", cls=1, grid=1024, clear_counts=1, hint_max=[2, 0, 1], prio_tag=1)]),
    #    batch 768 on the 1024 handle: hint_max slots (2 * 768 > 1024), but no staging: 8 * 768 <= 7 * 1024
    "s4_batch768": (0, 1, (1, 1, 0, 0), [L("SOLVE", cls=1, grid=768, clear_counts=1, hint_max=[2, 0, 1])]),
    #    8192 robots, h = 10 (120 rows: classes 1, 4, 2), no stance hints: class 6 ahead of larger classes (handle >= 2048),
    #    6.4 rounds: so_first = 8192 - 5 * 1280; class 4 as a queue over its 512 resident workgroups; class 2 split
    #    (handle >= 384), 4096 items: two chunks on groups 0 / 1, the first engine zeroes the second chunk's group
    "s4_mixed8192": (0, 1, (1, 0, 1, 0), [
        L("SOLVE", cls=6, grid=8192, clear_counts=1, next="slot0", next_count=0, **size_order(1792, 1)),
        L("SOLVE", cls=4, grid=512, list="slot0", count=0, qhead=4, next="slot1", next_count=1),
        L("SWEEP", cls=2, grid=256, list="slot1", count=1, qhead=grp(0, 0) + 2, sk=0, rid0=0, list_hi=4096, grp=0),
        L("ENGINE", cls=2, grid=512, sk=0, rid0=0, list_hi=4096, grp=0, wk_zero=1),
        L("SWEEP", cls=2, grid=256, list="slot1", count=1, qhead=grp(0, 1) + 2, sk=0, rid0=4096, list_hi=8192, grp=1),
        L("ENGINE", cls=2, grid=512, sk=0, rid0=4096, list_hi=8192, grp=1),
        handback(0, 256)]),
    #    qmpc_set_chunks(3), 300 robots, stance 40..40 (120 rows: class 2 alone, split on a 512 handle): three chunks of 100
    #    over the batch itself (no list: one sweep workgroup per robot, no queue head); the first launch clears the counters
    "s4_chunks3": (0, 1, (1, 0, 0, 0), [
        L("SWEEP", cls=2, grid=100, sk=0, rid0=0, list_hi=100, grp=0, clear_counts=1),
        L("ENGINE", cls=2, grid=100, sk=0, rid0=0, list_hi=100, grp=0, wk_zero=1),
        L("SWEEP", cls=2, grid=100, sk=0, rid0=100, list_hi=200, grp=1),
        L("ENGINE", cls=2, grid=100, sk=0, rid0=100, list_hi=200, grp=1, wk_zero=1),
        L("SWEEP", cls=2, grid=100, sk=0, rid0=200, list_hi=300, grp=0),
        L("ENGINE", cls=2, grid=100, sk=0, rid0=200, list_hi=300, grp=0),
        handback(0, 256)]),
    #    h = 20, use_jcqp = 1, 1024 robots: class 3 alone and monolithic (the alternate is never split), every robot goes on
    #    to the large-problem producer (the 192-row class's footprint: 256) and the ADMM, grid min(chunk, 2048); nothing is
    #    handed back; no ordering and no hint under the alternate
    "s4_jcqp_h20": (0, 0, (1, 0, 0, 0), [
        L("FILL_EVFLAGS"),
        L("SOLVE", cls=3, grid=1024, clear_counts=1, next="slot3", next_count=CNT_BIGLIST),
        L("BIG_PRODUCER", cls=5, grid=256, list="slot3", count=CNT_BIGLIST, qhead=grp(2, 0) + 2, sk=2, list_hi=1024),
        L("ADMM_BIG", cls=5, grid=1024, sk=2, list_hi=1024)]),
    #    the same handle in command mode solves exactly: class 3 split, then the large-problem stage with its engine
    #    (256 resident) and both hand-back launches
    "s4_jcqp_h20_commands": (1, 1, (2, 0, 0, 0), [
        L("SWEEP", cls=3, grid=1024, sk=1, list_hi=1024, clear_counts=1, next="slot3", next_count=CNT_BIGLIST),
        L("ENGINE", cls=3, grid=256, sk=1, list_hi=1024),
        L("FILL_EVFLAGS"),
        handback(1, 256),
        L("BIG_PRODUCER", cls=5, grid=256, list="slot3", count=CNT_BIGLIST, qhead=grp(2, 0) + 2, sk=2, list_hi=1024),
        L("ENGINE", cls=5, grid=256, sk=2, list_hi=1024),
        L("FILL_EVFLAGS"),
        handback(2, 256)]),
    #    h = 20 exact with max_stance = 64 (3 * 64 <= 192): no large-problem stage
    "s4_h20_exact_s64": (0, 1, (1, 0, 0, 0), [
        L("SWEEP", cls=3, grid=256, sk=1, list_hi=256, clear_counts=1),
        L("ENGINE", cls=3, grid=256, sk=1, list_hi=256),
        L("FILL_EVFLAGS"),
        handback(1, 256)]),
}

# settings block -> item pools the allocation must provide (sk 0: 128-row class, 1: 192-row class, 2: large problems)
POOLS = {
    "1024_h10_s20": set(), "16384_h10_s20": set(),     # the 64-row class alone
    "256_h14": {1},                                    # class 3 split from 128 robots on, class 2 only from 384
    "8192_h10": {0},                                   # 120 rows: the chain ends at class 2
    "512_h10_s40_chunks3": {0},
    "1024_h20_jcqp1": {1, 2},                          # the exact plan (command mode) and the alternate's, united
    "256_h20_s64": {1},
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    # host only, and the header alone: no HIP language, no device code, no runtime header
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "plan_dump.cpp"), "-o", exe],
                   check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def test_every_scenario_is_expected(plans):
    assert [p["name"] for p in plans] == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_plan(plans, name):
    got = next(p for p in plans if p["name"] == name)
    cset, leaves_hint, counters, launches = EXPECTED[name]
    assert got["set"] == cset
    assert got["leaves_hint"] == leaves_hint
    assert tuple(got["counters"]) == counters
    assert [g["kind"] for g in got["launches"]] == [e["kind"] for e in launches]
    for i, (g, e) in enumerate(zip(got["launches"], launches)):
        assert g == e, (i, {k: (g[k], e[k]) for k in e if g[k] != e[k]})


def test_pools_allocated_are_the_pools_reached(plans):
    """ONE rule: the pools the allocation derives from a settings block (plan_pools) are the pools the launches of the
    calls on that block go through -- no launch on a pool that was not allocated, no pool allocated for nothing."""
    assert {p["block"] for p in plans} == set(POOLS)
    for block, pools in POOLS.items():
        mine = [p for p in plans if p["block"] == block]
        for p in mine:
            assert {sk for sk in range(3) if p["pools"] >> sk & 1} == pools, (block, p["name"])
        reached = {l["sk"] for p in mine for l in p["launches"] if l["kind"] in ("SWEEP", "BIG_PRODUCER", "ENGINE", "ADMM_BIG")}
        assert reached == pools, (block, reached)


def test_plan_header_is_host_only():
    src = open(os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_plan.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    includes = [l.split()[1] for l in code.splitlines() if l.strip().startswith("#include")]
    assert all(i.startswith("<") or i == '"qmpc_device.h"' for i in includes), includes
    assert "hip" not in code.lower() and "qmpc_ctx" not in code and "*" not in code.replace(" * ", "")
