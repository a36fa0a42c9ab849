"""CPU suite: the compiled shape of the sweep loop (stage 3) in the 64-row classes' first-class kernel (tools/sweep_shape.py; no
GPU).  The loop over the four blocks of sixteen pivot columns is not unrolled, so the text between the two markers is ONE block:
eight pivot pairs, every wave's paths laid out together; the kernel holds one copy per instantiation of the solve in it.

                                                       class 1 (four per CU)     class 6 (five per CU)     the parent, both
  barriers per block of eight pairs                            4                         8                         8
  producer paths per block (one per step)                      4                         8                         8
  waits that name lgkmcnt in a producer path, from its
  first LDS load on (its loads are issued: what it stands for) 1                         1                         1
  LDS stores in a producer path (ds_write2: two vectors each)  4                         2                         2

Class 1 publishes two pivot pairs per barrier: a step is four columns, its producing wave loads the eight vectors of the step
behind one wait and stores the eight of the next.  Class 6 keeps one pair per barrier (Cfg::SWP_PAIRS: the second set of vectors
would make the sweep its largest LDS phase and cost the fifth workgroup of a CU).

The test holds the barriers and the producer's waits where the change left them.  It reads s_barrier, s_waitcnt and ds_
mnemonics and the markers, nothing else.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sweep_shape  # noqa: E402
from engine_iter_shape import assembly  # noqa: E402

PARENT_BARRIERS = 8
# class -> (barriers per block of eight pairs, producer paths per block, LDS store instructions per producer path)
HELD = {1: (4, 4, 4), 6: (8, 8, 2)}


@pytest.mark.parametrize("rb", [1, 6])
def test_sweep_shape(rb):
    got = sweep_shape.count(assembly(rb), rb)
    print(got)
    barriers, paths, stores = HELD[rb]
    assert got["loops"]                                               # (the loop is there, in every copy of the solve)
    for lp in got["loops"]:
        assert lp["instructions"] > 500
        assert lp["barriers"] == barriers
        assert len(lp["producer"]) == paths
        for p in lp["producer"]:
            assert p["load_waits"] == 1, p                            # one wait for LDS per step in the producing wave
            assert p["ds_stores"] == stores, p
    if rb == 1:                                                       # what the change is for
        assert all(lp["barriers"] * 2 == PARENT_BARRIERS for lp in got["loops"])
        assert all(p["ds_loads"] == 4 for lp in got["loops"] for p in lp["producer"])   # (the step's eight vectors, ds_read2)
