"""CPU suite: the compiled shape of one iteration of the event-form engine in the 64-row classes' first-class kernel, LDS-pool
instantiation (tools/engine_iter_shape.py; no GPU).  Classes 1 and 6 compile to the same iteration; per region of the device
assembly (the text between two markers, every path laid out there together):

                                            this tree      its parent (the same tool, the markers added to the parent's source)
  select  (loop top .. delta known)  waits that name lgkmcnt   4        6
                                     s_cbranch_*              13       16
                                     *_saveexec_*              2        8
                                     ds_ instructions         28       26
                                     instructions            329      310
  step    (delta known .. loop end)  waits that name lgkmcnt   6        4
                                     s_cbranch_*              27       23
                                     *_saveexec_*              6        7
                                     ds_ instructions         24       18
                                     instructions            363      346
  hcol    (the two columns of H^-1)  waits that name lgkmcnt   0        1
                                     s_cbranch_*               0        1
                                     *_saveexec_*              0        5
                                     instructions             19       33

What moved.  select: the x gather is no longer issued there (it is carried from the step that wrote x), its wait stands at the
loop top, and the column loads, the two diagonal entries and the first trip over the events wait together: a plain add step
passes TWO waits for LDS between the loop top and delta (the parent: five); the other two are the waits of the trips past the
first, add and drop events.  The first trip is unrolled in front of the loop (the ds_ and instruction counts).  hcol: two
compares, two selects, no exec region.  step: the text grew -- the gather's six ds_bpermute stand here now, and the ratio
test's reductions exist twice (lane 15 / lane 31) behind a scalar branch; a full step passes NO wait for LDS in this region
(the six are the drop event's: two accumulation loops, their entry and the column clears).

The test holds every count at or below where the change left it, so that a later edit cannot quietly bring the waits, the
exec regions or the branches back.  It reads wait, branch, exec and ds_ mnemonics and the markers, nothing else.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import engine_iter_shape  # noqa: E402

KEYS = ("lgkm_waits", "branches", "saveexec", "ds", "instructions")
HELD = {"select": (4, 13, 2, 28, 329), "step": (6, 27, 6, 24, 363), "hcol": (0, 0, 0, 2, 19)}
PARENT = {"select": (6, 16, 8, 26, 310), "step": (4, 23, 7, 18, 346), "hcol": (1, 1, 5, 2, 33)}


@pytest.mark.parametrize("rb", [1, 6])
def test_engine_iter_shape(rb):
    got = engine_iter_shape.count(engine_iter_shape.assembly(rb), rb)
    print(got)
    assert got["select"]["instructions"] > 100 and got["step"]["instructions"] > 100   # (the regions are there)
    assert got["hcol"]["ds"] == 2                                                      # (two column loads, one block of rows)
    for region, held in HELD.items():
        for key, bound in zip(KEYS, held):
            assert got[region][key] <= bound, (region, key, got[region][key], bound)
    # what the change is for: fewer waits for LDS in front of delta than the parent had, no exec region in the columns
    assert got["select"]["lgkm_waits"] < PARENT["select"][0]
    assert got["hcol"]["saveexec"] == 0 and got["hcol"]["branches"] == 0
