"""GPU suite (-m gpu): the warm start (qmpc_set_warm_start) on working sets the solver did NOT write itself.

The buffer is caller data.  Whatever it holds -- the exact previous set under another shift, the opposite faces of the
friction pyramids, whole pyramids, duplicates, another robot's set, values no cycle can write -- the warm handle must
return the cold minimiser.  The judge is test_gpu_stress's: a cold handle dumps its own reduced QP (fp64), the reference's
qpOASES (cap lifted) solves it (rc == 0 for EVERY robot), and the warm handle's full solution lies within 1e-8 relative of
that; the box and pyramid rows hold to 1e-7; no error bit ((status & 47) == 0; FALLBACK / SPILLED / COMPACTED are
informational).  The distance to the cold kernel is printed for every family and gated at 1e-9 for the natural ones.
Beyond 192 rows (trot, h = 36) nothing is dumped: the fp64 Kronecker model's QP stands in, with
test_stress_large_problems' bounds (x 1e-6, objective 1e-12, infeasibility 1e-9).

That the buffer is USED is pinned by the iteration count.  In the engine every forced add, every drop of the repair phase,
every full step and every partial step changes the working set by exactly one constraint and adds exactly one to `iters`;
a dependent forced candidate is skipped and counts nothing.  Hence, for a robot whose written-back row is complete (fewer
than 64 entries) and that was not re-run by the other engine,

    iters = adds + drops,   |row| = adds - drops          ->  iters - |row| is even, and
    iters >= |K| + |K \\ row| + |row \\ K|                    (K: the independent candidates the decode accepted),

and for the solver's OWN final working set handed back under the matching shift (N0, and N1 where no entry was lost)

    iters == |K|        on every robot whose working set the second solve confirms (the row comes back unchanged);
    iters == |K| + |row1 ^ row2|   otherwise (a multiplier that is zero to rounding: the degenerate case -- the row is
                                     dropped, or another one of the same apex takes its place, once each).

A decode that slid the ids the wrong way, divided by the wrong stride or looked the foot-step up in the wrong table
would turn these candidates into others or into none: the minimiser would not move, the count would.

Derived while reading `run` (quadruped_ctrl_amd/csrc/qmpc_kernels.hip): the `qslot < 0` exit cannot be taken while
candidates are being forced -- the decode reads min(KS, 64) entries, KS being the engine's slot count, and the forced phase
starts on an empty working set, so a free slot always exists; the exit is reachable only from the normal iteration.

Shapes are the smallest that reach each instantiation (tests/warm_sets.py: CASES)."""
import numpy as np
import pytest

import warm_sets as WS
from oracle import kron_model as K
from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W

pytestmark = pytest.mark.gpu

ERR_BITS = 47
ST_MAXITER, ST_FALLBACK = 1, 16   # include/qmpc.h
GUARD = 24                        # rows of the buffer behind the batch: no call may touch them
SENTINEL = -12345


def rel(x, ref):
    """[B] relative distance of full solutions."""
    return np.abs(x - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)


class Case:
    """One record: the cold handle's answer and dumped QP, the judge's answer, a warm handle."""

    def __init__(self, b, mpc_factory, dumped=True, sample=None):
        self.b, self.B, self.h = b, b["batch"], b["horizon"]
        B = self.B
        self.cold = mpc_factory(b)
        self.warm = mpc_factory(b, max_batch=B + GUARD)   # (the handle's size decides nothing below 128 robots)
        self.dumped = dumped
        self.sample = np.arange(B) if sample is None else np.asarray(sample)
        self.judge(b)

    def judge(self, b):
        """Cold solve of `b` (dumping) + qpOASES on the robots of the sample."""
        import torch  # noqa: F401
        B, h = self.B, self.h
        self.b = b
        if self.dumped:
            Hd, gd, _ = self.cold.debug_dump(B)
        self.rc = self.cold.solve(b, full=True)
        if self.dumped:
            self.cold.debug_off()
            Hd, gd = Hd.cpu().numpy(), gd.cpu().numpy()
        assert ((self.rc["status"] & ERR_BITS) == 0).all(), np.unique(self.rc["status"])
        self.xq = np.zeros((B, 12 * h))
        self.qp = {}
        for i in self.sample:
            Hf, gf, A, lb, ub, _ = O.assemble(b, i)
            ve, _, gr, Ar, lr, ur = O.reduce(Hf, gf, A, lb, ub)
            n = gr.size
            if self.dumped:
                assert 0 < n <= 192
                Hm, gm = Hd[i][:n, :n], gd[i][:n]
            else:
                Hk, gk = K.assemble(b, i)
                vi = np.flatnonzero(~ve)
                Hm, gm = Hk[np.ix_(vi, vi)], gk[vi]
            x, _, _, qrc, irc = O.qpoases(Hm, gm, Ar, lr, ur, nwsr=20000 if self.dumped else 100000)
            assert qrc == 0 and irc == 0, i       # (tests/test_warm_sets_cpu.py: holds for every robot; nobody is excluded)
            self.xq[i, ~ve] = x
            self.qp[i] = (Hm, gm, Ar, lr, ur, ~ve)
        self.sets = WS.active_sets(b, self.rc["soln"])    # W*, read off the cold solution
        self.check(self.rc, "cold")

    def set_buffer(self, buf, shift):
        """A fresh device buffer of B + GUARD rows on the warm handle: `buf` in the first B, a sentinel behind."""
        import torch
        ws = self.warm.warm_start(self.B + GUARD, shift_steps=shift)
        full = np.full((self.B + GUARD, 64), SENTINEL, np.int32)
        full[:self.B] = -1 if buf is None else buf
        ws.copy_(torch.from_numpy(full))
        return ws

    def reshift(self, ws, shift):
        """The same device buffer under another shift."""
        self.warm._check(self.warm.lib.qmpc_set_warm_start(self.warm.h, ws.data_ptr(), int(shift)), "qmpc_set_warm_start")

    def check(self, res, tag):
        """The judge's gates on one result; -> (worst distance to qpOASES, worst distance to cold)."""
        b, B, h, s = self.b, self.B, self.h, self.sample
        st = res["status"]
        assert ((st & ERR_BITS) == 0).all(), (tag, np.unique(st))
        f = res["soln"].reshape(B, 4 * h, 3)
        mi = WS.mu_inv(b)
        assert np.all(f[b["gait"] == 0] == 0), tag
        if self.dumped:
            assert (np.abs(f[..., 0]) <= f[..., 2] / mi + 1e-7).all() and (np.abs(f[..., 1]) <= f[..., 2] / mi + 1e-7).all(), tag
            assert (f[..., 2] >= -1e-7).all() and (f[..., 2] <= b["f_max"] + 1e-7).all(), tag
            dq = float(rel(res["soln"][s], self.xq[s]).max())
            assert dq < 1e-8, (tag, dq)
        else:   # the fp64 model's QP: test_stress_large_problems' bounds
            dq = wf = wi = 0.0
            for i in s:
                Hm, gm, Ar, lr, ur, keep = self.qp[i]
                xs, xq = res["soln"][i][keep], self.xq[i][keep]
                obj = lambda x: 0.5 * x @ Hm @ x + gm @ x  # noqa: E731
                ax = Ar @ xs
                wi = max(wi, np.maximum(lr - ax, 0).max(), np.maximum(ax - ur, 0).max())
                wf = max(wf, abs(obj(xs) - obj(xq)) / max(abs(obj(xq)), 1e-30))
                dq = max(dq, np.abs(xs - xq).max() / max(np.abs(xq).max(), 1.0))
            assert dq < 1e-6 and wf < 1e-12 and wi < 1e-9, (tag, dq, wf, wi)
        return dq, float(rel(res["soln"], self.rc["soln"]).max())

    def written(self, ws, res, tag, cand=None):
        """The write-back: ids in [0, 20 h) or -1, a subset of the active set of the robot's own solution, the guard rows
        untouched; and the count relations of the module's docstring.  -> the rows as lists."""
        b, B, h = self.b, self.B, self.h
        w = ws.cpu().numpy()
        assert (w[B:] == SENTINEL).all(), tag
        w = w[:B]
        assert (((w >= 0) & (w < 20 * h)) | (w == -1)).all(), tag
        rows = WS.rows_of(w)
        for i in range(B):
            assert len(set(rows[i])) == len(rows[i]), (tag, i)
            assert set(rows[i]) <= set(WS.active_set(b, res["soln"][i], i)), (tag, i)
            if len(rows[i]) >= 64 or res["status"][i] & ST_FALLBACK:
                continue
            it = int(res["iters"][i])
            assert it >= len(rows[i]) and (it - len(rows[i])) % 2 == 0, (tag, i, it, len(rows[i]))
            if cand is not None:
                k = set(WS.independent_prefix(b, i, cand[i]))
                assert it >= len(k) + len(k ^ set(rows[i])), (tag, i, it, len(k), len(rows[i]))
        return rows

    def family(self, name, buf, shift, natural=False, second=True):
        """One family: solve from `buf`, judge, check the write-back, solve again from the written row at shift 0.
        -> (report text, result, rows written, candidates)."""
        ws = self.set_buffer(buf, shift)
        cand = WS.decode(self.b, np.full((self.B, 64), -1, np.int32) if buf is None else buf, shift)
        res = self.warm.solve(self.b, full=True)
        dq, dc = self.check(res, name)
        rows = self.written(ws, res, name, cand)
        if natural:
            assert dc < 1e-9, (name, dc)
        if second:
            self.reshift(ws, 0)
            res2 = self.warm.solve(self.b, full=True)
            dq2, dc2 = self.check(res2, name + " second cycle")
            assert dc2 < 1e-9, (name, dc2)
            self.written(ws, res2, name + " second cycle", WS.decode(self.b, WS.pack(rows), 0))
        ic, iw = self.rc["iters"], res["iters"]
        nfb = int(((res["status"] & ST_FALLBACK) != 0).sum())
        txt = (f"{name}: qp {dq:.1e} cold {dc:.1e} iters warm {iw.mean():.1f}/{iw.max()} cold {ic.mean():.1f}/{ic.max()} "
               f"fallback {nfb}")
        return txt, res, rows, cand


def confirmed_counts(c, name, buf, shift, row1):
    """N0 / N1: the solver's own final working set `row1`, encoded in `buf` for `shift`.  The count relations for a set
    handed back exactly (module docstring)."""
    txt, res, rows, cand = c.family(name, buf, shift, natural=True)
    ic, nconf, nless, nwhole = c.rc["iters"], 0, 0, 0
    for i in range(c.B):
        if len(row1[i]) >= 64 or res["status"][i] & ST_FALLBACK:
            continue
        k = len(cand[i])
        whole = set(cand[i]) == set(row1[i])      # nothing fell off the end of the horizon under this shift
        if not whole:
            continue                              # (a subset of the final set: the general bounds of written() apply)
        nwhole += 1
        it = int(res["iters"][i])
        if set(rows[i]) == set(row1[i]):
            assert it == k, (name, i, it, k)
            nconf += k > 0
        else:
            assert it == k + len(set(rows[i]) ^ set(row1[i])), (name, i, it, k, rows[i], row1[i])
        assert k <= ic[i], (name, i, k, ic[i])
        nless += k < ic[i]
    if name == "N0":
        # the count must not exceed the cold count and is smaller on at least one robot -- unless the cold iteration never
        # dropped a row on ANY robot of the batch (cold count == |final set| throughout, which is the rule for the trot
        # records: DESIGN.md 3.3, "it almost never drops"); there the count of N0 cannot tell a buffer that was used from one
        # that was ignored, and the robots on which H1's count tells (test_warm_families: `pins`) stand in
        never_dropped = all(int(ic[i]) == len(row1[i]) for i in range(c.B))
        assert nconf > 0 and (nless > 0 or never_dropped), (name, nconf, nless)
    return txt + f" whole {nwhole} confirmed {nconf} below cold {nless}"


@pytest.mark.parametrize("case", list(WS.CASES))
def test_warm_families(case, mpc_factory):
    mk, full = WS.CASES[case]
    b = mk()
    B, h = b["batch"], b["horizon"]
    big = case == "trot_h36"
    c = Case(b, mpc_factory, dumped=not big)
    rc, sets = c.rc, c.sets
    out = []
    if big:
        # ---- robots beyond 192 rows: the warm instantiation of the 192-row class hands them to the large-problem path
        # without reading or writing their row (only an all-swing robot's row is filled with -1): the buffer comes back
        # as it went in, whatever it held, and the answer is the cold handle's, bit for bit
        assert (3 * (b["gait"] != 0).sum(1) > 192).all()
        for name, buf, s in (("H1", WS.opposite_faces(sets), 0), ("H3", WS.whole_pyramids(b), 0),
                             ("N1s1", WS.shifted(sets, 1, h), 1), ("N1s2", WS.shifted(sets, 2, h), 2)):
            ws = c.set_buffer(buf, s)
            res = c.warm.solve(b, full=True)
            dq, dc = c.check(res, name)
            w = ws.cpu().numpy()
            assert np.array_equal(w[:B], buf) and (w[B:] == SENTINEL).all(), name
            assert np.array_equal(res["soln"], rc["soln"]) and np.array_equal(res["iters"], rc["iters"]), name
            out.append(f"{name}: qp {dq:.1e} cold {dc:.1e} iters warm {res['iters'].mean():.1f}/{res['iters'].max()} cold "
                       f"{rc['iters'].mean():.1f}/{rc['iters'].max()} fallback {int(((res['status'] & ST_FALLBACK) != 0).sum())}")
        print(f"{case}: B={B} h={h} n_r=216 (rows left alone) | " + " | ".join(out))
        return
    try:
        _families(c, b, full, out)
    finally:
        print(f"{case}: B={B} h={h} | " + " | ".join(out))


def _families(c, b, full, out):
    B, h, rc, sets = c.B, c.h, c.rc, c.sets
    # ---- N0: a fresh buffer is the cold path inside the warm instantiation, bit for bit; its row, handed back at shift 0
    ws = c.set_buffer(None, 0)
    r0 = c.warm.solve(b, full=True)
    assert np.array_equal(r0["soln"], rc["soln"]) and np.array_equal(r0["iters"], rc["iters"])
    row1 = c.written(ws, r0, "N0 first", None)
    n0 = WS.pack(row1)
    out.append(confirmed_counts(c, "N0", n0, 0, row1))
    # ---- N1: the same set as the cycle s steps ago would have written it
    for s in (1, 2):
        out.append(confirmed_counts(c, f"N1s{s}", WS.shifted(row1, s, h), s, row1))
        # ... and W* as read off the solution (dependent rows of an apex included: skipped, not counted)
        out.append(c.family(f"N1s{s}*", WS.shifted(sets, s, h), s, natural=True)[0])
    if full:
        # ---- N2: everything falls off the front -> the cold bits
        for name, buf, s in (("N2h", WS.pack(sets), h), ("N2s", WS.falls_off(b, 2), 2)):
            txt, res, rows, cand = c.family(name, buf, s, natural=True)
            assert not any(cand)
            assert np.array_equal(res["soln"], rc["soln"]) and np.array_equal(res["iters"], rc["iters"]), name
            out.append(txt)
    # ---- the hostile families
    hostile = [("H1", WS.opposite_faces(sets)), ("H3", WS.whole_pyramids(b))]
    if full:
        hostile += [("H2", WS.saturated(b)), ("H4", WS.duplicates(sets)), ("H5", WS.another_robot(n0)),
                    ("H6", WS.noise(b, 20260928))]
    for name, buf in hostile:
        txt, res, rows, cand = c.family(name, buf, 0)
        if name == "H1":
            # the repair phase ran: more working-set changes than a cold start on at least half of the robots with candidates
            # (tests/test_warm_sets_cpu.py: the fp64 model of the iteration says all but the whole-apex robots)
            ne = np.array([len(x) > 0 for x in cand])
            longer = int((res["iters"][ne] > rc["iters"][ne]).sum())
            # ... and the robots on which the count PROVES the candidates were taken: |K| + |K ^ row| (which written()
            # asserted `iters` reaches) lies above the cold count, the count of a solve that ignored its buffer
            pins = sum(1 for i in range(B) if len(rows[i]) < 64 and not res["status"][i] & ST_FALLBACK and (
                lambda k: len(k) + len(k ^ set(rows[i])))(set(WS.independent_prefix(b, i, cand[i]))) > rc["iters"][i])
            txt += f" longer {longer}/{int(ne.sum())} pins {pins}"
            assert ne.any() and 2 * longer >= ne.sum() and pins > 0, (longer, int(ne.sum()), pins)
        out.append(txt)
    if full:
        # ---- H7: the repair runs into the iteration cap.  cap = the batch's largest cold count + 1: every robot's cold solve
        # fits under it.  After the forced adds `iters` = |K|, the saturated rows that are not active at the optimum (all
        # but n4 of them) must each be dropped, one count each, so a robot with  2 |K| - n4 > cap  meets `iters >= cap` with
        # a negative multiplier left and must start over cold with the other engine (FALLBACK), never stop half repaired
        cap = int(rc["iters"].max()) + 1
        buf = WS.saturated(b)
        cand = WS.decode(b, buf, 0)
        must = np.array([2 * len(cand[i]) - sum(e % 5 == 4 for e in sets[i]) > cap for i in range(B)])
        below = np.array([len(cand[i]) > cap for i in range(B)])
        c.warm.settings(max_iter=cap)
        try:
            txt, res, rows, _ = c.family("H7", buf, 0, second=False)
        finally:
            c.warm.settings()
        fb = (res["status"] & ST_FALLBACK) != 0
        out.append(txt + f" cap {cap} (below the candidate count on {int(below.sum())} robots) must fall back {int(must.sum())}")
        assert not (res["status"] & ST_MAXITER).any()
        assert must.any() and fb[must].all() and fb.any()
        assert (res["iters"] <= cap).all()


def test_gait_switch_between_cycles(mpc_factory):
    """Three warm cycles of a trot, then the contact tables become a bound's and three more cycles run warm with
    shift_steps = 1: the stale candidates land on swing foot-steps or on another support pattern.  Every cycle judged on
    every fourth robot (qpOASES on the cold handle's dumped QP), against the cold kernel on all."""
    B, h = 48, 10
    ro = W.Rollout(B, h, "trot", seed=11)
    bound = W.Rollout(B, h, "bound", seed=11)
    ro.demand(1.5)       # (a sustained acceleration: friction rows bind on every robot from the first cycle on)
    c = Case(ro.record(), mpc_factory, sample=np.arange(0, B, 4))
    ws = c.set_buffer(None, 1)
    out = []
    for cyc in range(6):
        if cyc == 3:
            ro.off, ro.dur = bound.off.copy(), bound.dur.copy()
        b = ro.record()
        if cyc:
            c.judge(b)
        prev = WS.rows_of(ws.cpu().numpy()[:B])
        cand = WS.decode(b, WS.pack(prev), 1)
        res = c.warm.solve(b, full=True)
        dq, dc = c.check(res, f"cycle {cyc}")
        c.written(ws, res, f"cycle {cyc}", cand)
        lost = sum(len(p) for p in prev) - sum(len(x) for x in cand)
        if cyc == 3:     # the switch: stale entries exist, and some of them land on swing foot-steps
            assert sum(len(x) for x in cand) > 0 and lost > sum(sum(e // 20 == 0 for e in p) for p in prev)
        out.append(f"cycle {cyc}{' (bound)' if cyc >= 3 else ''}: qp {dq:.1e} cold {dc:.1e} iters warm "
                   f"{res['iters'].mean():.1f}/{res['iters'].max()} cold {c.rc['iters'].mean():.1f}/{c.rc['iters'].max()} "
                   f"candidates {sum(len(x) for x in cand)} discarded {lost} fallback "
                   f"{int(((res['status'] & ST_FALLBACK) != 0).sum())}")
        ro.advance(c.rc["grf"])
    print("gait switch trot -> bound, h=10, B=48 | " + " | ".join(out))


def test_selective_warm_start_after_other_calls(mpc_factory):
    """Selective warm start (qmpc_set_warm_start_min_iters) selects by the handle's previous EAGER call of the same batch
    size and by nothing else.  (a) An eager call of the batch, one of a sub-batch, a captured call replayed once, then the
    batch again with the buffer holding family H1: the last call's predecessor of record had another size, nobody
    qualifies, and the result is the cold handle's bit for bit -- judged like everything else here.  (b) That call left
    counts of this batch size.  A replay of the graph -- captured over the SAME robots in reverse order, so whatever it
    left in the count array would belong to other robots -- then the batch again: exactly the robots whose own count of
    the last eager call reaches the threshold start warm from H1 (longer path, same minimiser); every other robot is the
    cold kernel's, bits and count.  A captured call or a replay that wrote the count array would move that selection."""
    import torch
    b = WS.CASES["trot_h10"][0]()
    B = b["batch"]
    c = Case(b, mpc_factory)
    m, cold = c.warm, c.rc
    rows = lambda f: {k: (f(v) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v)  # noqa: E731
                      for k, v in b.items()}
    sub, rev = rows(lambda v: v[:20]), rows(lambda v: np.ascontiguousarray(v[::-1]))
    sub["batch"] = 20
    h1 = WS.opposite_faces(c.sets)
    guard = np.full((GUARD, 64), SENTINEL, np.int32)
    ws = c.set_buffer(h1, 0)
    m.warm_start_min_iters(1)
    m.solve(b, full=True)
    rs = m.solve(sub, full=True)
    assert np.array_equal(rs["soln"], cold["soln"][:20])      # (no counts of this batch size: cold)
    d = m.upload(rev)
    o = m.alloc_outputs(B, full=True)
    inp, outp = m.make_args(d, o)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):           # (one stream, no parallel branches)
        m.solve_async(B, inp, outp, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(o["soln"].cpu().numpy(), cold["soln"][::-1])   # (a captured call: cold)
    ws.copy_(torch.from_numpy(np.concatenate([h1, guard])))
    res = m.solve(b, full=True)
    dq, dc = c.check(res, "after other calls")
    c.written(ws, res, "after other calls")
    assert np.array_equal(res["soln"], cold["soln"]) and np.array_equal(res["iters"], cold["iters"])
    # (b) the threshold: the median count of the robots that iterate at all (both sides of it are populated)
    thr = int(np.median(cold["iters"][cold["iters"] > 0]))
    m.warm_start_min_iters(thr)
    g.replay()
    torch.cuda.synchronize()
    ws.copy_(torch.from_numpy(np.concatenate([h1, guard])))
    res2 = m.solve(b, full=True)
    dq2, dc2 = c.check(res2, "selected")
    cand = WS.decode(b, h1, 0)
    took = np.array([len(cand[i]) > 0 and cold["iters"][i] >= thr for i in range(B)])
    stale = np.array([len(cand[i]) > 0 and cold["iters"][B - 1 - i] >= thr for i in range(B)])
    assert took.any() and (~took).any() and (took != stale).any()
    c.written(ws, res2, "selected", [cand[i] if took[i] else [] for i in range(B)])
    assert np.array_equal(res2["soln"][~took], cold["soln"][~took]) and np.array_equal(res2["iters"][~took], cold["iters"][~took])
    assert 2 * int((res2["iters"][took] > cold["iters"][took]).sum()) >= took.sum()
    print(f"selective warm start after a sub-batch call and a replayed graph: all cold, qp {dq:.1e} cold {dc:.1e}; then threshold "
          f"{thr}: {int(took.sum())} robots warm from H1 (stale counts would pick {int((took != stale).sum())} others): qp {dq2:.1e} "
          f"cold {dc2:.1e} iters {res2['iters'].mean():.1f}/{res2['iters'].max()} cold {cold['iters'].mean():.1f}/{cold['iters'].max()}")
