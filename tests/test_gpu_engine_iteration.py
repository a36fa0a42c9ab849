"""GPU suite (-m gpu): the event-form engine's iteration (stage 5 of the solve kernels) at the smallest shapes at which it
changes path, in every instantiation that shares the iteration's lambda.  A rearrangement of the iteration -- when the x
gather is issued, which LDS loads wait together, how the wave reductions are sized -- changes no floating-point
expression, so every figure below stays where the parent commit's build left it, bit for bit.

Routes (batches 1 and 65, except the helper-wave class: 8 robots).
  c1    the 64-row class four per CU (set_dense(0)): 28 events in LDS;
  c6    the same robots five per CU (set_dense(2)): 16 events in LDS, so a robot with 12 add events already moves to the
        overflow pool in global memory (status bit 128) -- the global-pool instantiation of the iteration;
  c4    the 96-row class (trot at h = 16, stance hint raised), helper waves present;
  c2    the 128-row class, one-kernel path (standing at h = 10, 8 robots): paired records, helper waves at work;
  warm  c1 with warm start on: the WARM instantiation, second solve of the same record.

Inputs.  `trot`: configs[1]'s robots, the first three replaced by robots that already stand still on their reference
(no constraint violated: 0 iterations).  `hard`: the same gait with f_max = 40 N and lateral velocity commands of up to
2 m/s (tools/stress_parity.py's low-f_max family): long runs, force limits that bind.  `stairs`: 65 of 4096 robots of
configs[4] (random contact tables, tilted bodies, feet at different heights) thinned to the 21 stance foot-steps the 64-row
class takes -- the 46 whose cold solve drops a constraint again (DROPS) and 19 ordinary ones.  The recorded counts
(tests/golden/engine_iteration/bits.npz, checked below) hold robots with 0 iterations, with 1-4 (one trip over the events),
with 5 or more (a second trip), with more iterations than constraints active at the solution (a drop event: partial step),
and robots that spill from either LDS pool.

Checks.
  (a) no error status (status & 47 == 0);
  (b) the solution against the reference's qpOASES on the GPU's own dumped QP (qmpc_set_debug), every robot: < 1e-8
      relative, the figure test_gpu_parity.py uses for these routes;
  (c) iters equal between c1 and c6 on the same robots;
  (d) grf bits, status and iters equal to the fixture, which was recorded with the parent commit's build (before the
      iteration was touched) by running record() below on it.
      (The fixture has a directory of its own: test_gpu_parity.py and test_oracle_cpu.py take every tests/golden/*.npz for a
      batch of solver inputs.)
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W
from test_gpu_parity import _take

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_iteration", "bits.npz")
B = 65
# robots of the thinned configs[4] pool whose cold solve takes more iterations than constraints end up active (measured once
# on the parent's build: 3 .. 50 iterations, 1 .. 38 active): at least one constraint entered and left again
DROPS = [66, 130, 155, 353, 398, 596, 668, 693, 732, 748, 771, 885, 901, 919, 1065, 1089, 1239, 1417, 1472, 1494, 1530, 1614,
         1730, 1789, 1822, 2153, 2193, 2367, 2451, 2537, 2585, 2712, 2740, 2861, 2926, 3187, 3219, 3303, 3366, 3431, 3482, 3527,
         3941, 3972, 3988, 4092]
ONE = 40  # the robot solved alone (batch 1)
_INPUT = {}


def family(name):
    if name in _INPUT:
        return _INPUT[name]
    if name in ("trot", "hard"):
        b = W.make_config(1, batch=B)
        if name == "trot":
            for i in range(3):  # standing still on the reference: nothing to correct
                b["p"][i] = (0.0, 0.0, 0.25)
                b["v"][i] = 0
                b["w"][i] = 0
                b["q"][i] = (1, 0, 0, 0)
                b["yaw"][i] = 0
                t = np.zeros((10, 12), np.float32)
                t[:, 5] = 0.25
                b["traj"][i] = t.reshape(-1)
        else:
            rng = np.random.default_rng(20260)
            b["f_max"] = 40.0
            b["traj"].reshape(B, 10, 12)[:, :, 10] = rng.uniform(-2, 2, (B, 1))
    elif name == "stairs":
        pool = W.make_config(4, batch=4096)
        rng = np.random.default_rng(20263)
        g = pool["gait"].copy()
        for i in range(4096):  # thinned to what the 64-row class takes, the first stance foot-step kept
            on = np.flatnonzero(g[i])
            if on.size > 21:
                g[i, rng.choice(on[1:], on.size - 21, replace=False)] = 0
        pool["gait"] = g
        b = _take(pool, np.array(DROPS + list(range(B - len(DROPS)))))
    elif name == "trot16":
        b = W.make_trot(B, 16)
    elif name == "stand":
        b = W.make_standing(8, 10)
    else:
        raise KeyError(name)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _INPUT[name] = b
    return b


# case -> (family, route, batch of one?)
CASES = {
    "trot-c1": ("trot", "c1", False), "trot-c6": ("trot", "c6", False), "trot-c1-one": ("trot", "c1", True),
    "trot-c6-one": ("trot", "c6", True),
    "hard-c1": ("hard", "c1", False), "hard-c6": ("hard", "c6", False), "hard-c1-one": ("hard", "c1", True),
    "hard-c6-one": ("hard", "c6", True), "hard-warm": ("hard", "warm", False), "hard-warm-one": ("hard", "warm", True),
    "stairs-c1": ("stairs", "c1", False), "stairs-c6": ("stairs", "c6", False),
    "trot16-c4": ("trot16", "c4", False), "trot16-c4-one": ("trot16", "c4", True),
    "stand-c2": ("stand", "c2", False),
}


def solve_case(case, mpc_factory):
    """-> (inputs, result with the dumped QP) of one case on a fresh handle."""
    fam, route, one = CASES[case]
    b = family(fam)
    if one:
        b = _take(b, [ONE])
    n = b["batch"]
    m = mpc_factory(b, max_batch=B)
    m.set_order_hint(0)
    if route in ("c1", "c6", "warm"):
        m.set_max_stance(21)
        m.set_dense(2 if route == "c6" else 0)
    elif route == "c4":
        m.set_min_stance(25)
    else:
        m.set_split(False)
    if route == "warm":
        m.warm_start(n, shift_steps=1)
        first = m.solve(b)
        assert ((first["status"] & 47) == 0).all()
    Hd, gd, ld = m.debug_dump(n)
    res = m.solve(b, full=True)
    m.debug_off()
    res["H"], res["g"] = Hd.cpu().numpy(), gd.cpu().numpy()
    return b, res


def qpoases_error(b, res):
    """Per robot: relative distance of the solution to qpOASES's on the dumped QP, and how many of the engine's constraints
    (four friction rows and the force limit per stance foot-step) are active at the GPU's solution."""
    err = np.zeros(b["batch"])
    h = b["horizon"]
    f = res["soln"].reshape(b["batch"], h, 4, 3)
    fx, fy, fz = f[..., 0] / b["mu"], f[..., 1] / b["mu"], f[..., 2]
    act = sum((np.abs(s) < 1e-6).astype(np.int64) for s in (fx + fz, fz - fx, fy + fz, fz - fy, b["f_max"] - fz))
    nact = (act * (b["gait"].reshape(b["batch"], h, 4) != 0)).sum((1, 2))
    for i in range(b["batch"]):
        H, g, A, lb, ub, x0 = O.assemble(b, i)
        ve, Hr, gr, Ar, lr, ur = O.reduce(H, g, A, lb, ub)
        n = gr.size
        if n == 0:
            continue
        xq, y, used, rc, irc = O.qpoases(res["H"][i][:n, :n], res["g"][i][:n], Ar, lr, ur, nwsr=20000)
        assert rc == 0 and irc == 0, (i, rc, irc)
        err[i] = np.abs(res["soln"][i][~ve] - xq).max() / max(np.abs(xq).max(), 1.0)
    return err, nact


def record(mpc_factory, path=GOLD):
    """Write the fixture (run once, on the parent commit's build)."""
    out = {}
    for case in CASES:
        b, res = solve_case(case, mpc_factory)
        err, nact = qpoases_error(b, res)
        print(case, "iters", np.sort(res["iters"]).tolist(), "status", np.unique(res["status"]).tolist(),
              "qpOASES err", err.max(), "drops", int((res["iters"] > nact).sum()))
        out[case + "/grf"] = res["grf"].view(np.uint32)
        out[case + "/status"] = res["status"]
        out[case + "/iters"] = res["iters"]
        out[case + "/nact"] = nact
    np.savez_compressed(path, **out)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


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
    err, nact = qpoases_error(b, res)
    print("   vs qpOASES on the dumped QP: worst", err.max())
    assert err.max() < 1e-8
    fam, route, one = CASES[case]
    if route == "c6":
        twin = case.replace("c6", "c1")
        assert np.array_equal(res["iters"], gold[twin + "/iters"]), "iters differ between the four- and five-per-CU routes"
    assert np.array_equal(res["grf"].view(np.uint32), gold[case + "/grf"])
    assert np.array_equal(res["status"], gold[case + "/status"])
    assert np.array_equal(res["iters"], gold[case + "/iters"])
