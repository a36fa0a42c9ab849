"""GPU suite (-m gpu): the ratio test's shortcut on the routes the engine-iteration fixture does not reach -- the handle's
default route on a handle large enough for the decoupled engine (sweep kernel -> qmpc_engine_kernel, csrc/qmpc_engine.hip), with
robots of the 64-row class in the same batch.  In the solve kernels' event-form iteration the minimum ratio t1 is reduced over
the wave only when some working-set slot blocks the full step (its ratio is below t2); on a full step no bit of t1 reaches a
result, so every figure below stays where the parent commit's build left it, bit for bit.  The decoupled engine keeps its own
ratio test (one 32-bit reduction on the ratios rounded to float): the same rule there was measured slower on standing robots
(profiles/ratio_shortcut_after.md) and is not in; its figures are pinned here all the same.  (test_gpu_engine_iteration.py pins
the event-form engine of the solve kernels -- c1, c6, c4, c2, warm -- the same way.)

Cases, each on a fresh handle at its default route and large enough for the decoupled path (solve_gpu.ROUTES "c3"; 384 robots
from which the 128-row class, 128 from which the 192-row class goes through work items), order hint off:
  stand, stand+vary      8 standing robots at h = 10 (128-row class), handle of max_batch = 384;
  stand14, stand14+vary  4 standing robots at h = 14 (192-row class), handle of max_batch = 128.
`+vary`: x_drag != 0, per-robot weights and alpha (solve_gpu.family).

On the parent's build none of the four families takes a partial step in the decoupled engine (every robot: iters <= nact), so
each case carries a few more robots behind its family, the same in the plain and the `+vary` case:
  h = 10   the first four robots of `stairs` (the default route sends them to the 64-row class: the event-form iteration of the
           solve kernels, a partial step each) and robot 7 of workloads.make_standing(32, 10), which drops two constraints in the
           decoupled engine;
  h = 14   robot 7 of workloads.make_standing(32, 14): two drops in the decoupled engine of the 192-row class.

Checks.
  (a) no error status (status & 47 == 0);
  (b) the solution against the reference's qpOASES on the GPU's own dumped QP (qmpc_set_debug), every robot: < 1e-8 relative;
  (c) grf bits, status and iters equal to the fixture (tests/golden/ratio_shortcut/bits.npz), which was recorded with the
      parent commit's build, before the kernels were touched, by running record() below on it;
  (d) coverage, on the fixture: in each case a robot with more iterations than constraints active at the solution (a partial
      step was taken: the reduction ran) and a robot with iters == nact >= 2 (only full steps on a non-empty working set: no
      slot ever blocked).
"""
import numpy as np
import pytest

import solve_gpu as S
from quadruped_ctrl_amd import workloads as W

pytestmark = pytest.mark.gpu
GOLD = S.bits_path("ratio_shortcut")

# case -> (family, max_batch of the handle)
CASES = {"stand": ("stand", 384), "stand14": ("stand14", 128), "stand+vary": ("stand+vary", 384),
         "stand14+vary": ("stand14+vary", 128)}


_INPUT = {}


def concat(a, b):
    """Batch a followed by batch b (same horizon and constants)."""
    out = {}
    for k, v in a.items():
        if isinstance(v, np.ndarray) and v.shape[:1] == (a["batch"],):
            out[k] = np.concatenate([v, b[k]])
        else:
            assert k == "batch" or v == b[k], k
            out[k] = v
    out["batch"] = a["batch"] + b["batch"]
    return out


def inputs(case):
    """The case's family and, behind it, the robots that take a partial step (built once, read-only)."""
    if case not in _INPUT:
        fam = CASES[case][0]
        h = S.family(fam)["horizon"]
        more = S.take(W.make_standing(32, h), [7])
        if h == 10:
            more = concat(S.take(S.family("stairs"), [0, 1, 2, 3]), more)
        _INPUT[case] = S.frozen(concat(S.family(fam), more))
    return _INPUT[case]


def solve_case(case, mpc_factory):
    """-> (inputs, result with the dumped QP) of one case on a fresh handle."""
    b = inputs(case)
    return b, S.solve_case(mpc_factory, b, "c3", CASES[case][1])


def record(mpc_factory, path=GOLD):
    """Write the fixture (run once, on the parent commit's build)."""
    def run(case):
        b, res = solve_case(case, mpc_factory)
        err, nact = S.qpoases_error(b, res)
        return dict(S.bits_of(res), nact=nact), ("iters", res["iters"].tolist(), "nact", nact.tolist(), "status",
                                                 np.unique(res["status"]).tolist(), "qpOASES err", err.max())
    S.record_bits(path, CASES, run)


gold = S.bits_fixture(GOLD)


@pytest.mark.parametrize("case", list(CASES))
def test_fixture_covers_both_paths(case, gold):
    it, nact = gold[case + "/iters"], gold[case + "/nact"]
    assert ((gold[case + "/status"] & 47) == 0).all()
    assert (it > nact).any()                     # a constraint entered and left again: a partial step, the reduction ran
    assert ((it == nact) & (nact >= 2)).any()    # full steps only, on a working set that is not empty: the shortcut ran


@pytest.mark.parametrize("case", list(CASES))
def test_ratio_shortcut(case, gold, mpc_factory):
    b, res = solve_case(case, mpc_factory)
    print(case, "iters", res["iters"].tolist(), "status", np.unique(res["status"]).tolist())
    assert ((res["status"] & 47) == 0).all(), np.unique(res["status"])
    err, nact = S.qpoases_error(b, res)
    print("   vs qpOASES on the dumped QP: worst", err.max())
    assert err.max() < 1e-8
    S.assert_same_bits(gold, case, S.bits_of(res))
