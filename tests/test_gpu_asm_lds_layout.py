"""GPU suite (-m gpu): stages 1-2 of the solve kernels (E tables -> H_red in registers) on every path that reads the E tables,
at the smallest shapes at which their LDS layout (csrc/qmpc_etab.h) can go wrong.  The layout moves where an entry lies, not
what is computed from it: every figure below stays where the parent commit's build left it, bit for bit.

Fixture.  tests/golden/asm_lds_layout/bits.npz, recorded with the parent commit's build (two 12 x 12 tables of doubles) by
running record() below on it; per case and robot: sha256 of the dumped H_red and g_red (qmpc_set_debug), sha256 of the full
solution, the bits of grf, status and iters.

Cases (each with its whole batch and with one robot alone, ONE):
  trot-c1 / trot-c6       65 robots of configs[1] (trot, h = 10, 60 rows) on the four- and the five-per-CU route of the 64-row class
  stairs-c1 / stairs-c6   solve_gpu's `stairs` family: random contact tables thinned to at most 21 stance
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

import numpy as np
import pytest

import solve_gpu as S
from quadruped_ctrl_amd import workloads as W

pytestmark = pytest.mark.gpu
GOLD = S.bits_path("asm_lds_layout")
B = S.B
ONE = 40

# case -> (family of solve_gpu.family, route, robot solved alone or None)
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


def _figures(res):
    return {"H": _sha(res["H"]), "g": _sha(res["g"]), "soln": _sha(res["soln"]), **S.bits_of(res)}


def solve_case(case, mpc_factory):
    if case == COMMANDS:
        return solve_commands(mpc_factory)
    fam, route, one = CASES[case]
    b = S.family(fam)
    if one is not None:
        b = S.take(b, [one])
    # (a handle's pools grow with its horizon: no spare robots at h = 36)
    return _figures(S.solve_case(mpc_factory, b, route, b["batch"] if route == "big" else B))


def solve_commands(mpc_factory):
    import torch
    cmd = W.make_commands(B, horizon=10, seed=20313, omni_mode=0, stand_fraction=0.0, calm=True)
    m = mpc_factory(S.pack_setup(cmd), max_batch=B)
    m.set_order_hint(0)
    S.route(m, "c1")
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
    res["H"], res["g"] = Hd.cpu().numpy(), gd.cpu().numpy()
    fig = _figures(res)
    fig["f_ff"] = f.cpu().numpy().view(np.uint32).copy()
    return fig


def record(mpc_factory, path=GOLD):
    """Write the fixture (run once, on the parent commit's build)."""
    def run(case):
        fig = solve_case(case, mpc_factory)
        return fig, ("iters", np.sort(fig["iters"]).tolist(), "status", np.unique(fig["status"]).tolist())
    S.record_bits(path, list(CASES) + [COMMANDS], run)


gold = S.bits_fixture(GOLD)


def test_fixture_covers_the_shapes(gold):
    for case in list(CASES) + [COMMANDS]:
        assert ((gold[case + "/status"] & 47) == 0).all(), case
    few = S.family("few")
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
    fig = solve_case(case, mpc_factory)
    print(case, "iters", np.sort(fig["iters"]).tolist(), "status", np.unique(fig["status"]).tolist())
    assert ((fig["status"] & 47) == 0).all()
    S.assert_same_bits(gold, case, fig)
