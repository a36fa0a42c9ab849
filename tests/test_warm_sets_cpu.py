"""The warm-start buffer builders (tests/warm_sets.py) checked on the host, for every generator and family that
tests/test_gpu_warm_start.py uses: shapes, dtypes and id ranges; that H3 and H4 really contain dependent rows (rank of
the candidates' coefficient rows, fp64); that H1's candidates end with a negative multiplier on every non-empty robot
(dense fp64 equality-constrained solve; but for a robot whose active set is whole pyramid apexes, which the swap maps onto
itself) and that, in the fp64 model of the iteration (warm_sets.gi_iters), starting from
them takes MORE working-set changes than a cold start on at least half of those robots -- the fraction the GPU module
asserts; and that the reference's qpOASES (cap lifted) solves every robot the GPU module judges (rc == 0), so that it never
has to exclude one.  The QP is the fp64 Kronecker model's (oracle/kron_model.py), as in test_stress_large_problems."""
import functools

import numpy as np
import pytest

import warm_sets as WS
from oracle import kron_model as K
from oracle import oracle as O

CASES = WS.CASES


@functools.lru_cache(maxsize=None)
def problem(case):
    """The record, and per robot the reduced fp64 QP, qpOASES' minimiser as a full solution, and W*."""
    b = CASES[case][0]()
    B, h = b["batch"], b["horizon"]
    qps, soln = [], np.zeros((B, 12 * h))
    for i in range(B):
        H, g = K.assemble(b, i)
        Hf, gf, A, lb, ub, _ = O.assemble(b, i)
        ve, _, _, Ar, lr, ur = O.reduce(Hf, gf, A, lb, ub)
        vi = np.flatnonzero(~ve)
        assert np.array_equal(vi, (3 * WS.stance(b, i)[:, None] + np.arange(3)).reshape(-1))
        Hm, gm = H[np.ix_(vi, vi)], g[vi]
        xq, _, _, rc, irc = O.qpoases(Hm, gm, Ar, lr, ur, nwsr=100000)
        assert rc == 0 and irc == 0, (case, i)      # a robot the judge could not solve would have to be excluded: none is
        soln[i, vi] = xq
        qps.append((Hm, gm, Ar, lr))
    return b, qps, soln, WS.active_sets(b, soln)


def families(b, sets, seed=1):
    h = b["horizon"]
    n0 = WS.pack(sets)
    return {"N0": n0, "N1s1": WS.shifted(sets, 1, h), "N1s2": WS.shifted(sets, 2, h), "N2": WS.falls_off(b, 2),
            "H1": WS.opposite_faces(sets), "H2": WS.saturated(b), "H3": WS.whole_pyramids(b), "H4": WS.duplicates(sets),
            "H5": WS.another_robot(n0), "H6": WS.noise(b, seed)}


@pytest.mark.parametrize("case", list(CASES))
def test_buffers_shape_dtype_ranges(case):
    b, qps, soln, sets = problem(case)
    B, h = b["batch"], b["horizon"]
    st = [set(WS.stance(b, i).tolist()) for i in range(B)]
    assert any(sets), "no robot of the case has an active constraint"
    fam = families(b, sets)
    for name, buf in fam.items():
        assert buf.shape == (B, 64) and buf.dtype == np.int32, name
        for r in buf:     # entries first, -1 behind them
            n = int((r != -1).sum())
            assert (r[:n] != -1).all() and (r[n:] == -1).all(), name
    for i in range(B):
        own = lambda r: all(0 <= e < 20 * h and e // 5 in st[i] for e in r)  # noqa: E731
        rows = {k: WS.rows_of(v)[i] for k, v in fam.items()}
        assert rows["N0"] == sets[i][:64] and own(rows["N0"])
        for s in (1, 2):
            assert rows[f"N1s{s}"] == [e + 20 * s for e in sets[i] if e + 20 * s < 20 * h][:64]
        assert rows["N2"] and all(e // 20 < 2 for e in rows["N2"])
        assert len(rows["H1"]) == len(rows["N0"]) and own(rows["H1"])
        assert [e // 5 for e in rows["H1"]] == [e // 5 for e in rows["N0"]]
        assert all((a % 5, c % 5) in ((0, 1), (1, 0), (2, 3), (3, 2), (4, 4)) for a, c in zip(rows["N0"], rows["H1"]))
        nst = len(st[i])
        assert len(rows["H2"]) == min(64, nst) and own(rows["H2"]) and all(e % 5 == 4 for e in rows["H2"])
        assert len(set(rows["H2"])) == len(rows["H2"])
        assert len(rows["H3"]) == min(64, 5 * min(12, nst)) and own(rows["H3"])
        assert rows["H4"] == [e for e in sets[i] for _ in (0, 1)][:64]
        assert rows["H5"] == WS.rows_of(fam["N0"])[(i - 1) % B]
        r6 = rows["H6"]
        assert len(r6) == 64
        ok = [e for e in r6 if 0 <= e < 20 * h]
        junk = [e for e in r6 if not 0 <= e < 20 * h]
        assert len(junk) == 64 - 2 * (64 // 3) and set(junk) <= set(WS.junk_values(h))
        on_stance = sum(e // 5 in st[i] for e in ok)
        assert on_stance == (64 // 3 if nst < 4 * h else 2 * (64 // 3))
        # the decode keeps exactly the stance ids of the entries it reads, whatever else the row holds
        dec = WS.decode(b, fam["H6"], 0)[i]
        assert dec == [e for e in r6[:WS.lanes_read(b, i)] if 0 <= e < 20 * h and e // 5 in st[i]]
    # the shift: an id written s steps ago names the same foot-step s steps earlier in this cycle's table
    for s in (1, 2):
        dec = WS.decode(b, fam[f"N1s{s}"], s)
        for i in range(B):
            assert dec[i] == [e for e in sets[i] if e + 20 * s < 20 * h][:WS.lanes_read(b, i)]
    assert not any(WS.decode(b, fam["N2"], 2)) and not any(WS.decode(b, fam["N0"], h))


@pytest.mark.parametrize("case", list(CASES))
def test_h3_h4_contain_dependent_rows(case):
    b, qps, soln, sets = problem(case)
    fam = families(b, sets)
    n4 = 0
    for i in range(b["batch"]):
        ids = WS.decode(b, fam["H3"], 0)[i]
        Cm, _ = WS.coef_rows(b, i, ids)
        per = [sum(e // 5 == k for e in ids) for k in sorted(set(e // 5 for e in ids))]
        # (per foot-step the rows come in type order: the first three are independent, the fourth is their combination,
        #  and fz = f_max is a combination of the first two)
        assert max(per) == 5 and np.linalg.matrix_rank(Cm) == sum(min(c, 3) for c in per) < len(ids)
        assert len(WS.independent_prefix(b, i, ids)) == np.linalg.matrix_rank(Cm)
        ids = WS.decode(b, fam["H4"], 0)[i]
        if ids:
            Cm, _ = WS.coef_rows(b, i, ids)
            assert len(ids) == 1 or np.linalg.matrix_rank(Cm) <= (len(ids) + 1) // 2 < len(ids)
            n4 += len(ids) > 1
    assert n4 > 0


@pytest.mark.parametrize("case", list(CASES))
def test_h1_negative_multipliers_and_longer_path(case):
    b, qps, soln, sets = problem(case)
    cand = WS.decode(b, WS.opposite_faces(sets), 0)
    nonempty = longer = napex = 0
    for i in range(b["batch"]):
        if not cand[i]:
            continue
        nonempty += 1
        Hm, gm = qps[i][0], qps[i][1]
        keep = WS.independent_prefix(b, i, cand[i])
        Cm, d = WS.coef_rows(b, i, keep)
        _, lam = WS.eqp_multipliers(Hm, gm, Cm, d)
        if set(cand[i]) == set(sets[i]):
            # whole apexes only (fz = 0, all four friction rows active): the swap maps such a set onto itself, the
            # candidates ARE the optimal active set and no multiplier is negative -- the one exception to the rule
            assert all(sum(e // 5 == c // 5 and e % 5 < 4 for e in sets[i]) == 4 for c in cand[i]), (case, i)
            assert lam.min() > -1e-7 * max(1.0, np.abs(lam).max()), (case, i, lam.min())
            napex += 1
        else:
            assert lam.min() < 0, (case, i, lam.min())
        xc, Wc, itc = WS.gi_iters(b, i, Hm, gm)
        xw, Ww, itw = WS.gi_iters(b, i, Hm, gm, forced=cand[i])
        xq = soln[i][(3 * WS.stance(b, i)[:, None] + np.arange(3)).reshape(-1)]
        sc = max(np.abs(xq).max(), 1.0)
        assert np.abs(xc - xq).max() / sc < 1e-8 and np.abs(xw - xq).max() / sc < 1e-8, (case, i)
        longer += itw > itc
    print(f"{case}: H1 candidates on {nonempty} robots, model path longer than cold on {longer} "
          f"({napex} robots whose set is whole apexes: swapped onto itself)")
    assert nonempty > 0 and 2 * longer >= nonempty
