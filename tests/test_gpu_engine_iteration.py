"""GPU suite (-m gpu): the event-form engine's iteration (stage 5 of the solve kernels) at the smallest shapes at which it
changes path, in every instantiation that shares the iteration's lambda.  A rearrangement of the iteration -- when the x
gather is issued, which LDS loads wait together, how the wave reductions are sized -- changes no floating-point
expression, so every figure below stays where the parent commit's build left it, bit for bit.

Routes (solve_gpu.route; batches 1 and 65, except the helper-wave class: 8 robots).
  c1    the 64-row class four per CU (set_dense(0)): 28 events in LDS;
  c6    the same robots five per CU (set_dense(2)): 16 events in LDS, so a robot with 12 add events already moves to the
        overflow pool in global memory (status bit 128) -- the global-pool instantiation of the iteration;
  c4    the 96-row class (trot at h = 16, stance hint raised), helper waves present;
  c2    the 128-row class, one-kernel path (standing at h = 10, 8 robots): paired records, helper waves at work;
  warm  c1 with warm start on: the WARM instantiation, second solve of the same record.

Inputs (solve_gpu.family).  `still` (the trot cases): configs[1]'s robots, the first three replaced by robots that already
stand still on their reference (no constraint violated: 0 iterations).  `hard`: the same gait with f_max = 40 N and lateral
velocity commands of up to 2 m/s (tools/stress_parity.py's low-f_max family): long runs, force limits that bind.  `stairs`:
65 of 4096 robots of configs[4] (random contact tables, tilted bodies, feet at different heights) thinned to the 21 stance
foot-steps the 64-row class takes -- the 46 whose cold solve drops a constraint again (DROPS) and 19 ordinary ones.  The
recorded counts (tests/golden/engine_iteration/bits.npz, checked below) hold robots with 0 iterations, with 1-4 (one trip
over the events), with 5 or more (a second trip), with more iterations than constraints active at the solution (a drop
event: partial step), and robots that spill from either LDS pool.

Checks.
  (a) no error status (status & 47 == 0);
  (b) the solution against the reference's qpOASES on the GPU's own dumped QP (qmpc_set_debug), every robot: < 1e-8
      relative, the figure test_gpu_parity.py uses for these routes;
  (c) iters equal between c1 and c6 on the same robots;
  (d) grf bits, status and iters equal to the fixture, which was recorded with the parent commit's build (before the
      iteration was touched) by running record() below on it.
"""
import numpy as np
import pytest

import solve_gpu as S

pytestmark = pytest.mark.gpu
GOLD = S.bits_path("engine_iteration")
ONE = 40  # the robot solved alone (batch 1)

# case -> (family, route, batch of one?)
CASES = {
    "trot-c1": ("still", "c1", False), "trot-c6": ("still", "c6", False), "trot-c1-one": ("still", "c1", True),
    "trot-c6-one": ("still", "c6", True),
    "hard-c1": ("hard", "c1", False), "hard-c6": ("hard", "c6", False), "hard-c1-one": ("hard", "c1", True),
    "hard-c6-one": ("hard", "c6", True), "hard-warm": ("hard", "warm", False), "hard-warm-one": ("hard", "warm", True),
    "stairs-c1": ("stairs", "c1", False), "stairs-c6": ("stairs", "c6", False),
    "trot16-c4": ("trot16", "c4", False), "trot16-c4-one": ("trot16", "c4", True),
    "stand-c2": ("stand", "c2", False),
}


def solve_case(case, mpc_factory):
    """-> (inputs, result with the dumped QP) of one case on a fresh handle."""
    fam, route, one = CASES[case]
    b = S.family(fam)
    if one:
        b = S.take(b, [ONE])
    return b, S.solve_case(mpc_factory, b, route, S.B, warm=route == "warm")


def record(mpc_factory, path=GOLD):
    """Write the fixture (run once, on the parent commit's build)."""
    def run(case):
        b, res = solve_case(case, mpc_factory)
        err, nact = S.qpoases_error(b, res)
        return dict(S.bits_of(res), nact=nact), ("iters", np.sort(res["iters"]).tolist(), "status", np.unique(res["status"]).tolist(),
                                                 "qpOASES err", err.max(), "drops", int((res["iters"] > nact).sum()))
    S.record_bits(path, CASES, run)


gold = S.bits_fixture(GOLD)


def test_fixture_covers_the_paths(gold):
    it = np.concatenate([gold[f + "-c1/iters"] for f in ("trot", "hard", "stairs")])
    nact = np.concatenate([gold[f + "-c1/nact"] for f in ("trot", "hard", "stairs")])
    assert (it == 0).any() and ((it >= 1) & (it <= 4)).any() and (it >= 5).any()
    assert (it > nact).any()                                        # a constraint entered and left again: a drop event
    assert (it - nact >= 2).any()
    assert (gold["hard-c6/status"] & 128).any()                     # the LDS pool filled up: the iteration moved to global memory
    assert (gold["stairs-c1/status"] & 128).any()                   # ... the larger pool of the four-per-CU route too
    assert (gold["stand-c2/iters"] >= 12).all()                     # three trips and more: the helper waves take their share
    for case in CASES:
        assert ((gold[case + "/status"] & 47) == 0).all(), case


@pytest.mark.parametrize("case", list(CASES))
def test_engine_iteration(case, gold, mpc_factory):
    b, res = solve_case(case, mpc_factory)
    print(case, "iters", np.sort(res["iters"]).tolist(), "status", np.unique(res["status"]).tolist())
    assert ((res["status"] & 47) == 0).all(), np.unique(res["status"])
    err, nact = S.qpoases_error(b, res)
    print("   vs qpOASES on the dumped QP: worst", err.max())
    assert err.max() < 1e-8
    fam, route, one = CASES[case]
    if route == "c6":
        twin = case.replace("c6", "c1")
        assert np.array_equal(res["iters"], gold[twin + "/iters"]), "iters differ between the four- and five-per-CU routes"
    S.assert_same_bits(gold, case, S.bits_of(res))
