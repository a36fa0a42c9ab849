"""CPU suite: the ratio test of the event-form engine's iteration as compiled (tools/engine_iter_shape.py; no GPU), in the
64-row classes' first-class kernel, LDS-pool instantiation.

The minimum ratio t1 is reduced over the wave only when some working-set slot blocks the full step (one compare of the
per-lane ratio against t2 and one ballot decide that), and then by ONE reduction over the first 32 lanes.  The parent held two
copies of the two-phase reduction (lane 15 / lane 31) behind a scalar branch and ran one of them on every iteration with a
non-empty working set.  In the "step" region (delta known .. loop end):

  v_min_u32_dpp   at most 10: one copy of the two-phase reduction (two phases of four row_shr steps and one row_bcast:15);
                  the parent had two copies;
  instructions    strictly below the parent's 363.

The test reads mnemonics and the existing markers, nothing else.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import engine_iter_shape as E  # noqa: E402

PARENT_STEP_INSTRUCTIONS = 363
ONE_COPY = 10


@pytest.mark.parametrize("rb", [1, 6])
def test_ratio_test_is_one_reduction(rb):
    step = E.between(E.kernel_text(E.assembly(rb), rb), E.DELTA, E.END)
    dpp = sum(1 for t in step if t.split()[:1] == ["v_min_u32_dpp"])
    n = E.tally(step)["instructions"]
    print("class", rb, "step region: v_min_u32_dpp", dpp, "instructions", n)
    assert 0 < dpp <= ONE_COPY, dpp          # (the reduction is there, once)
    assert n < PARENT_STEP_INSTRUCTIONS, n
