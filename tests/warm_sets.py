"""Working-set buffers for the warm-start tests (tests/test_gpu_warm_start.py, tests/test_warm_sets_cpu.py): pure numpy.

A buffer is what qmpc_set_warm_start reads: int32 [B, 64], row b = robot b, entries = global constraint ids
5 * (4 * step + foot) + type -- type 0..3 the friction rows  mi fx + fz, -mi fx + fz, mi fy + fz, -mi fy + fz  >= 0,
type 4 the row  f_max - fz >= 0 -- or -1 (empty).  The solver slides an id by `shift_steps` horizon steps
(id - 20 * shift), discards what falls off the front, what lies at or beyond 20 * h, what is negative and what lands on
a swing foot-step, and forces the rest into its working set in buffer order.

The families (N = natural, H = hostile) are built from the record and from W*, the active set of the cold solution
(rows with |row| < 1e-7).  `decode` restates the solver's decode on the host; `gi_iters` is a dense fp64 model of the
dual active-set iteration that counts working-set changes, cold or from a forced candidate set, so that statements
about iteration counts can be checked without a device.
"""
import numpy as np

WS = 64            # QMPC_WS_SLOTS


def _cases():
    from quadruped_ctrl_amd import workloads as W
    # case -> (record maker, dumped: the handle can dump its reduced QP (n_r <= 192) and the case carries every family)
    return {
        "trot_h10": (lambda: W.make_config(1, batch=48), True),                 # 64-row class, n_r = 60
        "mixed_h10": (lambda: W.make_config(2, batch=48), True),
        "standing_h10": (lambda: W.make_standing(32, 10), True),                # 128-row class
        "trot_h16": (lambda: W.make_trot(24, 16), True),                        # 96-row class
        "standing_h16": (lambda: W.make_standing(12, 16), True),                # 192-row class
        "trot_h24": (lambda: W.make_long_horizon(12, 24, "trot"), False),       # long horizon: the 4 h foot-step tables
        "trot_h36": (lambda: W.make_long_horizon(6, 36, "trot"), False),        # n_r = 216: leaves the warm kernel
    }


CASES = _cases()
SWAP = (1, 0, 3, 2, 4)
ACT_EPS = 1e-7


def mu_inv(b):
    """1 / mu as the solver forms it (float arithmetic, SolverMPC.cpp:366)."""
    return float(np.float32(1) / np.float32(b["mu"]))


def stance(b, i):
    """Foot-step indices k = 4 * step + foot of robot i's stance foot-steps, ascending."""
    return np.flatnonzero(np.asarray(b["gait"][i]) != 0)


def row_values(b, soln_i):
    """[4h, 5] values of the five inequality rows (each >= 0 when feasible) for one robot's full solution [12h]."""
    f = np.asarray(soln_i, np.float64).reshape(-1, 3)
    mi = mu_inv(b)
    return np.stack([mi * f[:, 0] + f[:, 2], -mi * f[:, 0] + f[:, 2], mi * f[:, 1] + f[:, 2], -mi * f[:, 1] + f[:, 2],
                     float(b["f_max"]) - f[:, 2]], 1)


def active_set(b, soln_i, i, eps=ACT_EPS):
    """W*: ids of the rows that are active (|row| < eps) on robot i's stance foot-steps, ascending."""
    r = row_values(b, soln_i)
    return [5 * int(k) + t for k in stance(b, i) for t in range(5) if abs(r[k, t]) < eps]


def active_sets(b, soln):
    return [active_set(b, soln[i], i) for i in range(int(b["batch"]))]


def pack(sets):
    """Lists of ids -> int32 [B, 64], truncated to 64, padded with -1."""
    out = np.full((len(sets), WS), -1, np.int32)
    for i, s in enumerate(sets):
        s = list(s)[:WS]
        out[i, :len(s)] = s
    return out


def rows_of(buf):
    """int32 [B, 64] -> list of lists of the non-empty entries (buffer order)."""
    return [[int(x) for x in r if x != -1] for r in np.asarray(buf)]


# ---- natural families
def shifted(sets, s, h):
    """N1: W* as the PREVIOUS cycle would have numbered it were the table `s` steps younger: every id + 20 s; ids that
    reach 20 h cannot be written by any cycle and are dropped."""
    return pack([[e + 20 * s for e in w if e + 20 * s < 20 * h] for w in sets])


def falls_off(b, s):
    """N2: per robot up to 64 ids, every one on a step < s (any foot, any type): all of them fall off the front."""
    B = int(b["batch"])
    ids = np.arange(20 * s)[:WS]
    return pack([ids.tolist()] * B)


# ---- hostile families
def opposite_faces(sets):
    """H1: W* with the friction types 0 <-> 1 and 2 <-> 3 swapped (the opposite face of the pyramid), type 4 kept."""
    return pack([[5 * (e // 5) + SWAP[e % 5] for e in w] for w in sets])


def saturated(b):
    """H2: fz = f_max (type 4) on the first min(64, n_stance) stance foot-steps."""
    return pack([[5 * int(k) + 4 for k in stance(b, i)[:WS]] for i in range(int(b["batch"]))])


def whole_pyramids(b, nfoot=12):
    """H3: all five rows on the first 12 stance foot-steps (three independent, one dependent, f_max against the apex)."""
    return pack([[5 * int(k) + t for k in stance(b, i)[:nfoot] for t in range(5)] for i in range(int(b["batch"]))])


def duplicates(sets):
    """H4: every entry of W* twice, truncated to 64."""
    return pack([[e for e in w for _ in (0, 1)] for w in sets])


def another_robot(buf):
    """H5: the rows of a buffer rolled by one robot."""
    return np.roll(np.asarray(buf), 1, axis=0).copy()


def junk_values(h):
    return [20 * h, 20 * h + 3, 5 * 4 * 36 + 4, 2 ** 30, -2, -7]


def noise(b, seed):
    """H6: 64 seeded draws per robot -- a third ids of stance foot-steps, a third ids of swing foot-steps (stance ids
    again for a robot without swing foot-steps: there are none to draw), the rest values no cycle can write."""
    rng = np.random.default_rng(seed)
    B, h = int(b["batch"]), int(b["horizon"])
    junk = junk_values(h)
    out = []
    for i in range(B):
        st = stance(b, i)
        sw = np.flatnonzero(np.asarray(b["gait"][i]) == 0)
        n1, n2 = WS // 3, WS // 3
        a = 5 * rng.choice(st, n1) + rng.integers(0, 5, n1)
        c = 5 * rng.choice(sw if sw.size else st, n2) + rng.integers(0, 5, n2)
        d = rng.choice(junk, WS - n1 - n2)
        out.append(rng.permutation(np.concatenate([a, c, d])).tolist())
    return pack(out)


# ---- the solver's decode, restated
def lanes_read(b, i):
    """Entries of row i the solver looks at: the 64-row class's engine holds 32 working-set slots and reads the first 32
    entries; every other class reads all 64.  (Horizons beyond 16 are solved by the 192-row class alone.)"""
    return 32 if (int(b["horizon"]) <= 16 and 3 * stance(b, i).size <= 64) else WS


def decode(b, buf, s):
    """Per robot the candidates the solver accepts from `buf` at shift_steps = s, as THIS cycle's ids, in buffer order
    (duplicates kept: the solver skips them as dependent, it does not filter them)."""
    h = int(b["horizon"])
    out = []
    for i, r in enumerate(np.asarray(buf)):
        g = np.asarray(b["gait"][i])
        c = []
        for e in r[:lanes_read(b, i)]:
            e = int(e)
            if e < 0:
                continue
            k = e // 5 - 4 * s
            if 0 <= k < 4 * h and g[k]:
                c.append(5 * k + e % 5)
        out.append(c)
    return out


# ---- fp64 algebra on a robot's reduced QP (variables: the stance foot-steps ascending, fx fy fz each)
def coef_rows(b, i, ids):
    """(C [len(ids), n_r], d): rows C x >= d of the ids in robot i's reduced variables."""
    st = stance(b, i)
    pos = {int(k): j for j, k in enumerate(st)}
    mi = mu_inv(b)
    Cm = np.zeros((len(ids), 3 * st.size))
    d = np.zeros(len(ids))
    for r, e in enumerate(ids):
        j, t = pos[int(e) // 5], int(e) % 5
        if t < 4:
            Cm[r, 3 * j + t // 2] = mi if t % 2 == 0 else -mi
            Cm[r, 3 * j + 2] = 1.0
        else:
            Cm[r, 3 * j + 2] = -1.0
            d[r] = -float(b["f_max"])
    return Cm, d


def independent_prefix(b, i, ids):
    """The ids the forced phase keeps: in order, each one that is linearly independent of those kept before."""
    Cm, _ = coef_rows(b, i, ids)
    keep, rk = [], 0
    for r in range(len(ids)):
        if np.linalg.matrix_rank(Cm[keep + [r]]) > rk:
            keep.append(r)
            rk += 1
    return [ids[r] for r in keep]


def eqp_multipliers(H, g, Cm, d):
    """Minimiser of 1/2 x'Hx + g'x subject to C x = d (rows independent) and its multipliers (H x + g = C' lam)."""
    n, m = g.size, d.size
    K = np.block([[H, -Cm.T], [Cm, np.zeros((m, m))]])
    sol = np.linalg.solve(K, np.concatenate([-g, d]))
    return sol[:n], sol[n:]


def gi_iters(b, i, H, g, forced=(), tol=1e-9, max_iter=1000):
    """Dense fp64 model of the solver's iteration (Goldfarb-Idnani, the most violated normalised row next; with `forced`:
    those candidates added first whatever the sign of the step, the dependent ones skipped, negative multipliers dropped
    one by one, then the normal iteration).  Returns (x, working set, iters); iters counts one per add and one per drop,
    as the kernel's `iters` does."""
    st = stance(b, i)
    allid = [5 * int(k) + t for k in st for t in range(5)]
    Ca, da = coef_rows(b, i, allid)
    mi = mu_inv(b)
    nrm = np.array([1.0 if e % 5 == 4 else 1.0 / np.sqrt(mi * mi + 1.0) for e in allid])
    Hi = np.linalg.inv(H)
    x = -Hi @ g
    W, lam, iters = [], np.zeros(0), 0

    def operators():
        if not W:
            return Hi, np.zeros((0, g.size))
        N = Ca[W].T
        S = np.linalg.inv(N.T @ Hi @ N)
        Ns = S @ N.T @ Hi
        return Hi - Hi @ N @ Ns, Ns

    for p in [allid.index(e) for e in forced]:
        if p in W:
            continue
        P, Ns = operators()
        c = Ca[p]
        z, r = P @ c, Ns @ c
        delta = c @ z
        if not delta > 1e-11 * (c @ Hi @ c):
            continue
        t = -(c @ x - da[p]) / delta
        x = x + t * z
        lam = np.append(lam - t * r, t)
        W.append(p)
        iters += 1
    while W and (lam < 0).any():
        l = int(np.flatnonzero(lam < 0)[0])
        W.pop(l)
        x, lam = eqp_multipliers(H, g, Ca[W], da[W]) if W else (-Hi @ g, np.zeros(0))
        iters += 1
    while iters < max_iter:
        viol = (Ca @ x - da) * nrm
        viol[W] = 0.0
        p = int(np.argmin(viol))
        if not viol[p] < -tol:
            break
        lp = 0.0
        while True:
            P, Ns = operators()
            c = Ca[p]
            z, r = P @ c, Ns @ c
            delta = c @ z
            dep = not delta > 1e-11 * (c @ Hi @ c)
            t2 = np.inf if dep else -(c @ x - da[p]) / delta
            ratio = np.where(r > 0, np.maximum(lam, 0.0) / np.where(r > 0, r, 1.0), np.inf) if W else np.zeros(0)
            t1 = ratio.min() if W else np.inf
            t = min(t1, t2)
            assert np.isfinite(t), "infeasible"
            if not dep:
                x = x + t * z
            lam = lam - t * r
            lp += t
            iters += 1
            if t2 <= t1:
                W.append(p)
                lam = np.append(lam, lp)
                break
            l = int(np.argmin(ratio))
            W.pop(l)
            lam = np.delete(lam, l)
    return x, sorted(allid[p] for p in W), iters
