"""CPU suite: the compiled shape of stage 0's loads in the 64-row classes' first-class kernel (tools/stage0_waits.py; no GPU).

Between the kernel's entry and the issue of stage 0's last load -- the size-order builder cut out, the order-hint path
included -- the device assembly holds

                                   this tree      its parent (the same tool, the markers added to the parent's source)
  class 1 (four per CU)  kernarg waits  1             25
                         vmcnt waits    0             24
  class 6 (five per CU)  kernarg waits  1             17
                         vmcnt waits    0             14

A kernarg wait is an s_waitcnt lgkmcnt(0) behind a scalar load from the kernarg segment: a scalar round trip on a cold
scalar cache, in front of every load behind it.  A vmcnt wait in the region is a wave that waits for memory before its last
load of the stage is out: a second vector round trip.  The test holds the counts where the change left them, so that a later
edit cannot quietly bring the serialisation back.  It reads wait-count instructions, scalar loads' base registers and the
markers, nothing else.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stage0_waits  # noqa: E402

KERNARG_WAITS = {1: 1, 6: 1}


@pytest.mark.parametrize("rb", [1, 6])
def test_stage0_waits(rb):
    got = stage0_waits.count(stage0_waits.assembly(rb), rb)
    print(got)
    assert got["region_lines"] > 100            # (the region is there: entry, the batch, the stage's loads)
    assert got["vmcnt_waits"] == 0, got
    assert 1 <= got["kernarg_waits"] <= KERNARG_WAITS[rb], got
