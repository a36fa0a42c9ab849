"""GPU suite (-m gpu): stages 1-2 of the solve kernels (E tables -> H_red in registers) on every path that reads the E tables,
at the smallest shapes at which their LDS layout (csrc/qmpc_etab.h) can go wrong.  The layout moves where an entry lies, not
what is computed from it: every figure below stays where the parent commit's build left it, bit for bit.

Fixture.  tests/golden/asm_lds_layout/bits.npz, recorded with the parent commit's build (two 12 x 12 tables of doubles) by
running record() below on it; per case and robot: sha256 of the dumped H_red and g_red (qmpc_set_debug), sha256 of the full
solution, the bits of grf, status and iters.

Cases (each with its whole batch and with one robot alone, ONE):
  trot-c1 / trot-c6       65 robots of configs[1] (trot, h = 10, 60 rows) on the four- and the five-per-CU route of the 64-row class
  stairs-c1 / stairs-c6   test_gpu_engine_iteration.py's `stairs` family: random contact tables thinned to at most 21 stance
                          foot-steps -- ragged stance lists, lane groups that do not hold all four feet, padding rows and columns
  few-c1 / few-c6         16 of those robots thinned further to 1 .. 16 stance foot-steps (robot k: k + 1): down to ONE foot-step
  trot16-c4               the 96-row class (trot at h = 16): a wave straddles two column groups
  stand-c2                the 128-row class, 8 robots standing at h = 10
  stand14-c3              the 192-row class, 4 robots standing at h = 14 (its own branch of `fill`)
  big-trot36              one robot of the large-problem path (trot at h = 36, 216 rows: H assembled element by element into
                          global memory; no dump there: the solution's hash stands for it)
Input variations: `vary` = x_drag != 0 with per-robot weights and alpha (trot-c1, trot-c6, trot16-c4, stand-c2, stand14-c3,
big-trot36); trot-c1-swing = robot 7 with an all-swing table; commands-c1 = qmpc_solve_commands on a trot batch (the COMMAND
instantiation of the same stages).
"""
import hashlib
import os

import numpy as np
import pytest

from quadruped_ctrl_amd import workloads as W
from test_gpu_engine_iteration import family as engine_family
from test_gpu_parity import _pack_setup, _take

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asm_lds_layout", "bits.npz")
B = 65
ONE = 40
_INPUT = {}


def _vary(b, seed):
    rng = np.random.default_rng(seed)
    n = b["batch"]
    b = dict(b)
    b["x_drag"] = rng.normal(0, 0.7, n).astype(np.float32)
    b["alpha"] = (4e-5 * rng.uniform(0.25, 2.0, n)).astype(np.float32)
    b["weights"] = (b["weights"] * rng.uniform(0.5, 2.0, (n, 12))).astype(np.float32)
    return b


def family(name):
    if name in _INPUT:
        return _INPUT[name]
    if name == "trot":
        b = W.make_config(1, batch=B)
    elif name == "stairs":
        b = engine_family("stairs")
    elif name == "few":
        s = engine_family("stairs")
        rng = np.random.default_rng(20311)
        g = s["gait"][:16].copy()
        for k in range(16):
            on = np.flatnonzero(g[k])
            assert on.size > k + 1
            g[k, rng.choice(on[1:], on.size - (k + 1), replace=False)] = 0
        b = _take(s, np.arange(16))
        b["gait"] = g
    elif name == "swing":
        b = dict(W.make_config(1, batch=B))
        g = b["gait"].copy()
        g[7] = 0
        b["gait"] = g
    elif name == "trot16":
        b = W.make_trot(B, 16)
    elif name == "stand":
        b = W.make_standing(8, 10)
    elif name == "stand14":
        b = W.make_standing(4, 14)
    elif name == "big":
        b = W.make_long_horizon(1, 36, "trot")
    elif name.endswith("+vary"):
        b = _vary(family(name[:-5]), 20312 + len(name))
    else:
        raise KeyError(name)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _INPUT[name] = b
    return b


# case -> (family, route, robot solved alone or None)
CASES = {}
for fam, routes in (("trot", ("c1", "c6")), ("stairs", ("c1", "c6")), ("few", ("c1", "c6")), ("trot+vary", ("c1", "c6")),
                    ("swing", ("c1",)), ("trot16", ("c4",)), ("trot16+vary", ("c4",)), ("stand", ("c2",)), ("stand+vary", ("c2",)),
                    ("stand14", ("c3",)), ("stand14+vary", ("c3",)), ("big", ("big",)), ("big+vary", ("big",))):
    for route in routes:
        CASES[f"{fam}-{route}"] = (fam, route, None)
for fam, route, one in (("trot", "c1", ONE), ("trot", "c6", ONE), ("stairs", "c1", ONE), ("stairs", "c6", ONE), ("few", "c1", 0),
                        ("few", "c6", 0), ("trot+vary", "c1", ONE), ("trot16", "c4", ONE), ("stand", "c2", 3), ("stand14", "c3", 2)):
    CASES[f"{fam}-{route}-one"] = (fam, route, one)
COMMANDS = "commands-c1"


def _sha(a):
    return np.stack([np.frombuffer(hashlib.sha256(np.ascontiguousarray(r).tobytes()).digest(), np.uint8) for r in a])


def _figures(res, H, g):
    return {"H": _sha(H), "g": _sha(g), "soln": _sha(res["soln"]), "grf": res["grf"].view(np.uint32).copy(),
            "status": res["status"].copy(), "iters": res["iters"].copy()}


def solve_case(case, mpc_factory):
    fam, route, one = CASES[case]
    b = family(fam)
    if one is not None:
        b = _take(b, [one])
    n = b["batch"]
    m = mpc_factory(b, max_batch=n if route == "big" else B)  # (a handle's pools grow with its horizon: no spare robots at h = 36)
    m.set_order_hint(0)
    if route in ("c1", "c6"):
        m.set_max_stance(21)
        m.set_dense(2 if route == "c6" else 0)
    elif route == "c4":
        m.set_min_stance(25)
    elif route == "c2":
        m.set_split(False)
    Hd, gd, ld = m.debug_dump(n)
    res = m.solve(b, full=True)
    m.debug_off()
    return _figures(res, Hd.cpu().numpy(), gd.cpu().numpy())


def solve_commands(mpc_factory):
    import torch
    cmd = W.make_commands(B, horizon=10, seed=20313, omni_mode=0, stand_fraction=0.0, calm=True)
    m = mpc_factory(_pack_setup(cmd), max_batch=B)
    m.set_order_hint(0)
    m.set_max_stance(21)
    m.set_dense(0)
    d = m.upload_command(cmd)
    rec = m.alloc_record(B)
    o = m.alloc_outputs(B, full=True)
    _, out = m.make_args(rec, o)
    f = torch.empty_like(o["grf"])
    Hd, gd, ld = m.debug_dump(B)
    m.solve_commands_async(B, m.make_command_args(d), out, f)
    torch.cuda.synchronize()
    m.debug_off()
    res = {k: o[k].cpu().numpy() for k in ("grf", "status", "iters", "soln")}
    fig = _figures(res, Hd.cpu().numpy(), gd.cpu().numpy())
    fig["f_ff"] = f.cpu().numpy().view(np.uint32).copy()
    return fig


def record(mpc_factory, path=GOLD):
    """Write the fixture (run once, on the parent commit's build)."""
    out = {}
    for case in list(CASES) + [COMMANDS]:
        fig = solve_commands(mpc_factory) if case == COMMANDS else solve_case(case, mpc_factory)
        print(case, "iters", np.sort(fig["iters"]).tolist(), "status", np.unique(fig["status"]).tolist())
        for k, v in fig.items():
            out[f"{case}/{k}"] = v
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_covers_the_shapes(gold):
    for case in list(CASES) + [COMMANDS]:
        assert ((gold[case + "/status"] & 47) == 0).all(), case
    few = family("few")
    assert ((few["gait"] != 0).sum(1) == np.arange(1, 17)).all()           # down to one stance foot-step
    assert (gold["swing-c1/grf"][7] == 0).all() and gold["swing-c1/iters"][7] == 0
    for case in ("trot-c1", "stairs-c6", "trot16-c4", "stand-c2", "stand14-c3", COMMANDS):  # (a dump was taken: no two alike)
        assert len({bytes(r) for r in gold[case + "/H"]}) == gold[case + "/H"].shape[0], case
    for fam in ("trot", "trot16", "stand", "stand14", "big"):                # x_drag, weights and alpha change the matrix
        route = [r for (f, r, o) in CASES.values() if f == fam][0]
        assert not np.array_equal(gold[f"{fam}-{route}/soln"], gold[f"{fam}+vary-{route}/soln"])
    for fam in ("trot", "stairs", "few"):                                    # the two routes assemble the same matrix
        assert np.array_equal(gold[f"{fam}-c1/H"], gold[f"{fam}-c6/H"]) and np.array_equal(gold[f"{fam}-c1/g"], gold[f"{fam}-c6/g"])


@pytest.mark.parametrize("case", list(CASES) + [COMMANDS])
def test_asm_lds_layout(case, gold, mpc_factory):
    fig = solve_commands(mpc_factory) if case == COMMANDS else solve_case(case, mpc_factory)
    print(case, "iters", np.sort(fig["iters"]).tolist(), "status", np.unique(fig["status"]).tolist())
    assert ((fig["status"] & 47) == 0).all()
    for k, v in fig.items():
        bad = np.flatnonzero((v != gold[f"{case}/{k}"]).reshape(v.shape[0], -1).any(1))
        assert bad.size == 0, f"{case}: {k} differs from the parent's build for robots {bad.tolist()}"
