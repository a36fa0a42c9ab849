"""The judge of the capped solve (tests/cap_judge.py) and its inputs, pinned without a device.

For every record tests/test_gpu_iteration_cap.py uses, the dense fp64 model of the iteration (warm_sets.gi_iters) on the
fp64 Kronecker model's QP, stopped at every judged cap and at tol = 0.5 / 5.0, passes the properties the GPU module
asserts of the kernels (counts, minimiser of the active rows' QP, violated row, objective monotone); no judged iterate has
a row in the band the judge leaves out.  The judge is sharp: an iterate taken in the middle of an add and an optimum with
a negated multiplier are refused.  The inputs do what the GPU module needs of them: every cap flags somebody, the middle
cap of the mixed family leaves somebody alone, the many-active family overshoots a cap (a drop counts one, the cap is
looked at only when the next row is chosen) and tol = 5.0 stops a
quarter of the mixed family's robots early."""
import functools

import numpy as np
import pytest

import cap_judge as J
import warm_sets as WS

TOLS = (0.5, 5.0)


@functools.lru_cache(maxsize=None)
def uncapped(name):
    """The record, per robot the model QP, and the model's uncapped run: x [list], counts, never-dropped."""
    mk, xtol, extra = J.RECORDS[name]
    b = mk()
    B = int(b["batch"])
    qps = [J.model_qp(b, i) for i in range(B)]
    xs, c = [], np.zeros(B, int)
    for i in range(B):
        x, it, fl = J.model(b, i, *qps[i])
        assert not fl
        xs.append(x)
        c[i] = it
    soln = np.stack([J.full_solution(b, i, xs[i]) for i in range(B)])
    return b, qps, xs, c, J.never_dropped(b, soln, c), xtol, sorted(set(J.caps_of(c)) | set(extra))


@functools.lru_cache(maxsize=None)
def capped(name, k):
    b, qps, _, _, _, _, _ = uncapped(name)
    return [J.model(b, i, *qps[i], max_iter=k) for i in range(int(b["batch"]))]


@pytest.mark.parametrize("name", list(J.RECORDS))
def test_model_passes_the_judge_at_every_cap(name):
    b, qps, xs, c, nd, xtol, caps = uncapped(name)
    B = int(b["batch"])
    fopt = [J.objective(*qps[i], xs[i]) for i in range(B)]
    prev = [-np.inf] * B
    worst, over, nflag = 0.0, 0, []
    for k in caps:
        res = capped(name, k)
        fl = np.array([r[2] for r in res])
        it = np.array([r[1] for r in res])
        J.counts(k, fl, it, c, nd)
        nflag.append(int(fl.sum()))
        over = max(over, int((it - k)[fl].max()) if fl.any() else 0)
        for i in range(B):
            x = res[i][0]
            H, g = qps[i]
            if not fl[i]:                # not flagged: the uncapped run, to the bit
                assert it[i] == c[i] and np.array_equal(x, xs[i]), (name, k, i)
            else:
                assert J.violation(b, i, x) > 1e-9, (name, k, i)
            m = J.minimiser(b, i, H, g, x, xtol)
            assert m is not None, (name, k, i, "a row in the band")       # the model leaves out none
            assert m[0], (name, k, i, m[1])
            worst = max(worst, m[1][0])
            # every add and every drop counts one and changes the working set by one row: the GPU module tells a count
            # that restarted at 0 from one carried over from the fast engine (odd: module docstring there) by this parity
            rk = J.rank_active(b, i, x)
            assert it[i] >= rk and (it[i] - rk) % 2 == 0, (name, k, i, it[i], rk)
            f, sl = J.objective(H, g, x), J.objective_slack(H, g, x)
            assert f <= fopt[i] + sl and f >= prev[i] - sl, (name, k, i, f, fopt[i], prev[i])
            prev[i] = f
    print(f"{name}: model counts {c.min()}..{c.max()} median {int(np.median(c))} never dropped {int(nd.sum())}/{B} caps {caps} "
          f"flagged {nflag} worst x distance {worst:.1e} largest iters - cap {over}")
    # ---- the inputs are fit for purpose
    assert all(n > 0 for n in nflag), (caps, nflag)
    if name in J.MIXED:
        mid = caps[len(caps) // 2]
        assert not all(r[2] for r in capped(name, mid))
    if name == "many_active":
        assert over > 0                                  # a cap is overshot: drops of the last add


@pytest.mark.parametrize("name", ["mixed", "standing_h10", "many_active"])
def test_model_passes_the_judge_at_a_loose_tolerance(name):
    b, qps, xs, c, nd, xtol, _ = uncapped(name)
    B = int(b["batch"])
    early = {}
    for T in TOLS:
        n = 0
        for i in range(B):
            H, g = qps[i]
            x, it, fl = J.model(b, i, H, g, tol=T)
            assert not fl and it <= c[i], (name, T, i, it, c[i])
            assert J.violation(b, i, x) <= T, (name, T, i)
            m = J.minimiser(b, i, H, g, x, xtol)
            assert m is not None and m[0], (name, T, i, m)
            n += it < c[i]
        early[T] = n
    print(f"{name}: robots that stop early {early} of {B}")
    assert early[0.5] > 0 and 4 * early[5.0] >= B      # what the GPU module asks of the kernels


def _dropping_robot():
    """A robot of the many-active record whose cold run drops rows."""
    b, qps, xs, c, nd, xtol, _ = uncapped("many_active")
    i = int(np.flatnonzero(~nd)[0])
    return b, i, qps[i], xtol


def test_judge_refuses_an_iterate_taken_inside_an_add():
    b, i, (H, g), xtol = _dropping_robot()
    mids = J.mid_add_iterates(b, i, H, g)
    assert mids
    for x in mids:
        m = J.minimiser(b, i, H, g, x, xtol)
        assert m is not None and not m[0], m


def test_judge_refuses_a_negated_multiplier():
    for name in ("trot", "standing_h10"):
        b, qps, xs, c, nd, xtol, _ = uncapped(name)
        i = int(np.argmax(c))
        H, g = qps[i]
        ok = J.minimiser(b, i, H, g, xs[i], xtol)
        assert ok is not None and ok[0], ok
        g2, x = J.negated_multiplier(b, i, H, g)
        m = J.minimiser(b, i, H, g2, x, xtol)
        assert m is not None and not m[0], m


def test_counts_refuses_what_the_mutations_would_give():
    """`counts` (property 2) on hand-made cases: one iteration past the cap, a flag that is missing, a flag too many."""
    c, nd = np.array([5, 3, 9]), np.array([True, True, False])
    J.counts(4, np.array([True, False, True]), np.array([4, 3, 6]), c, nd)
    for fl, it in (([True, False, True], [5, 3, 6]),      # never dropped, iters == k + 1  (`>` in place of `>=`)
                   ([False, False, True], [5, 3, 6]),     # never dropped, c > k, not flagged
                   ([True, True, True], [4, 3, 6]),       # flagged with c <= k
                   ([True, False, True], [4, 3, 9])):     # flagged with iters == c
        with pytest.raises(AssertionError):
            J.counts(4, np.array(fl), np.array(it), c, nd)
