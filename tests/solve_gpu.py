"""What the solve's GPU tests share (no tests here): the end-to-end bound and its report, batch helpers, the routes through the
size classes, the input families of the stage tests, the solve with the QP dump on and its comparisons (fp64 model, the
reference's qpOASES on the dumped QP), and the bit-fixture harness of the tests that pin one stage of the solve kernels
against a fixture recorded on the parent commit.  The tolerances are stated in test_gpu_parity.py's docstring, with the tests
that use them."""
import json
import os

import numpy as np
import pytest

from oracle import kron_model as K
from oracle import noise_floor as NF
from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------- the end-to-end bound
def rel_f0(f, ref):
    ref12 = ref[:, :12]
    return np.abs(f.astype(np.float64) - ref12).max(1) / np.maximum(np.abs(ref12).max(1), 1.0)


def load_gold(path):
    z = np.load(path)
    b = {k: z[k] for k in z.files}
    for k in ("batch", "horizon"):
        b[k] = int(b[k])
    for k in ("dt", "mu", "f_max"):
        b[k] = float(b[k])
    return b


NOISE = json.load(open(os.path.join(GOLDEN, "noise_floor.json")))["families"]


def bound_for(b, idx=None, family=None, full=False, err=None):
    """Per-robot end-to-end bound max(1e-4, 1.5 spread_i) at every horizon, with spread_i = the
    pairwise spread of the reference's six float evaluation orders on that robot
    (oracle/noise_floor.py: spread12 / spread_full -- reference pipeline only, no fp64 term, so the
    bound does not know what the GPU computes).  family = golden file name -> committed per-robot
    spreads; otherwise computed live with the oracle.  err (the measured errors of the same robots):
    the spread is then evaluated only for the robots over the flat 1e-4 -- a robot at or under it
    passes whatever its spread is, so the others keep the bound 1e-4."""
    idx = list(range(b["batch"])) if idx is None else list(idx)
    if family is not None:
        fl = np.array(NOISE[family]["per_robot_spread_full" if full else "per_robot_spread_first_step"])[idx]
    else:
        key = "spread_full" if full else "spread12"
        need = np.ones(len(idx), bool) if err is None else ~(np.asarray(err) < 1e-4)
        if err is None and b["horizon"] <= 10:
            need[:] = False     # (callers that give no errors assert against the flat 1e-4 at h <= 10, as before)
        fl = np.zeros(len(idx))
        for k in np.flatnonzero(need):
            fl[k] = NF.robot_floor(b, idx[k])[key]
    # six evaluation orders are six SAMPLES of the reference's rounding noise; the exactly-assembled answer the GPU
    # reproduces need not lie inside their hull (measured: up to 1.6x the pairwise spread on the committed
    # families below 1e-4, 1.25x on a robot of configs[3] over it), hence the factor -- still a function of the
    # reference alone
    return np.maximum(1e-4, SPREAD_FACTOR * fl)


SPREAD_FACTOR = 1.5


def report(name, err, bound):
    over = err > 1e-4
    print(f"{name}: rel err median {np.median(err):.2e} p99 {np.percentile(err, 99):.2e} max {err.max():.2e}; "
          f"bound (reference float-order spread) min {bound.min():.2e} max {bound.max():.2e}; "
          f"robots over 1e-4: {over.sum()}/{err.size} = {over.mean():.4f}")
    # robots outside the reference's own pairwise spread (1.0 x), whether or not they pass the 1.5 x bound, are named
    raw = np.where(bound > 1e-4, bound / SPREAD_FACTOR, bound)
    for i in np.nonzero(~(err < raw))[0][:20]:
        print(f"   robot {i}: err {err[i]:.3e} vs float-order spread {raw[i]:.3e} (bound {bound[i]:.3e})"
              + ("  FAIL" if not err[i] < bound[i] else ""))


# ---------------------------------------------------------------- batches
def take(b, idx):
    out = {k: (v[idx] if isinstance(v, np.ndarray) and v.shape[:1] == (b["batch"],) else v) for k, v in b.items()}
    out["batch"] = len(idx)
    return out


def frozen(b):
    """b with every array read-only: a cached batch that several tests share."""
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def thin_to(g, i, nst, rng):
    """Robot i's contact table g[i] (more than nst stance foot-steps) thinned to nst, the first stance foot-step kept."""
    on = np.flatnonzero(g[i])
    g[i, rng.choice(on[1:], on.size - nst, replace=False)] = 0


# ---------------------------------------------------------------- caller side on the GPU
REC_KEYS = ("p", "v", "q", "w", "r", "yaw", "traj", "gait", "weights", "alpha", "x_drag")


def gpu_pack(m, cmd):
    import torch
    dcmd = m.upload_command(cmd)
    rec = m.alloc_record(cmd["batch"])
    m.pack_async(dcmd, rec)
    torch.cuda.synchronize()
    got = {k: rec[k].cpu().numpy() for k in REC_KEYS}
    return got, dcmd["world_position_desired"].cpu().numpy(), dcmd["x_comp_integral"].cpu().numpy(), rec


def pack_setup(cmd, dt=0.026):
    return {"batch": cmd["batch"], "horizon": cmd["horizon"], "dt": dt, "mu": 0.4, "f_max": 120.0}


# ---------------------------------------------------------------- routes through the size classes
# name -> (max_stance, min_stance, dense, split): every knob of qmpc_ctx (csrc/qmpc_host.h) that chooses the kernels, the
# ones a route does not need at the handle's defaults (0, 0, 1, 1), so that a route can follow another on one handle
ROUTES = {
    "c1": (21, 0, 0, 1),    # the 64-row class four per CU
    "c6": (21, 0, 2, 1),    # ... five per CU
    "c4": (0, 25, 1, 1),    # the 96-row class first (no robot below 25 stance foot-steps: the 64-row class is skipped)
    "c2": (0, 0, 1, 0),     # the 128-row class, one-kernel path
    "c3": (0, 0, 1, 1),     # the handle as it comes: the 192-row class, the large-problem path
}
ROUTES["warm"] = ROUTES["c1"]
ROUTES["big"] = ROUTES["c3"]


def route(m, name):
    """Send handle m's solves through the route `name`.  The order hint and warm start are the caller's."""
    max_stance, min_stance, dense, split = ROUTES[name]
    m.set_max_stance(max_stance)
    m.set_min_stance(min_stance)
    m.set_dense(dense)
    m.set_split(split)


# ---------------------------------------------------------------- input families of the stage tests
B = 65
# robots of the thinned configs[4] pool whose cold solve takes more iterations than constraints end up active (measured once
# on the parent's build: 3 .. 50 iterations, 1 .. 38 active): at least one constraint entered and left again
DROPS = [66, 130, 155, 353, 398, 596, 668, 693, 732, 748, 771, 885, 901, 919, 1065, 1089, 1239, 1417, 1472, 1494, 1530, 1614,
         1730, 1789, 1822, 2153, 2193, 2367, 2451, 2537, 2585, 2712, 2740, 2861, 2926, 3187, 3219, 3303, 3366, 3431, 3482, 3527,
         3941, 3972, 3988, 4092]
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
    """A named batch of solver inputs, built once and read-only.  `trot`: configs[1]; `still`: the same with the first
    three robots standing still on their reference; `hard`: f_max = 40 N and lateral velocity commands of up to 2 m/s;
    `stairs`: 65 robots of configs[4] thinned to 21 stance foot-steps, DROPS first; `few`: 16 of those thinned to 1 .. 16;
    `swing`: configs[1], robot 7 all swing; `trot16`, `stand`, `stand14`, `big`: one robot shape per larger class;
    `<family>+vary`: x_drag != 0, per-robot weights and alpha."""
    if name in _INPUT:
        return _INPUT[name]
    if name == "trot":
        b = W.make_config(1, batch=B)
    elif name in ("still", "hard"):
        b = W.make_config(1, batch=B)
        if name == "still":
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
        count = (g != 0).sum(1)
        for i in range(4096):  # thinned to what the 64-row class takes
            if count[i] > 21:
                thin_to(g, i, 21, rng)
        pool["gait"] = g
        b = take(pool, np.array(DROPS + list(range(B - len(DROPS)))))
    elif name == "few":
        s = family("stairs")
        rng = np.random.default_rng(20311)
        g = s["gait"][:16].copy()
        for k in range(16):
            assert (g[k] != 0).sum() > k + 1
            thin_to(g, k, k + 1, rng)
        b = take(s, np.arange(16))
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
    _INPUT[name] = frozen(b)
    return b


# ---------------------------------------------------------------- the solve with the QP dump on
def solve_with_dump(m, b):
    """m.solve(b, full=True) with the dumped QP (qmpc_set_debug) attached as res["H"], res["g"]."""
    Hd, gd, ld = m.debug_dump(b["batch"])
    res = m.solve(b, full=True)
    m.debug_off()
    res["H"], res["g"] = Hd.cpu().numpy(), gd.cpu().numpy()
    return res


def solve_case(mpc_factory, b, route_name, max_batch, warm=False):
    """One case of a stage test on a fresh handle: order hint off, the route, with warm a first solve that leaves its
    working sets behind, then the solve with the QP dump on."""
    m = mpc_factory(b, max_batch=max_batch)
    m.set_order_hint(0)
    route(m, route_name)
    if warm:
        m.warm_start(b["batch"], shift_steps=1)
        first = m.solve(b)
        assert ((first["status"] & 47) == 0).all()
    return solve_with_dump(m, b)


def dump_model_compare(m, b, idx):
    """GPU H_red, g_red (fp64) of robots idx vs the fp64 model fed the kernel's own float
    transcendentals -> worst relative differences (H, g)."""
    B = b["batch"]
    Hd, gd, ld = m.debug_dump(B)
    aux = m.debug_aux(B)
    res = m.solve(b, full=True)
    m.debug_off()
    assert ((res["status"] & 47) == 0).all()
    sel = np.asarray(list(idx))
    import torch
    ti = torch.as_tensor(sel, device=Hd.device)
    Hc, gc, ac = Hd[ti].cpu().numpy(), gd[ti].cpu().numpy(), aux[ti].cpu().numpy()
    worst_h = worst_g = 0.0
    for k, i in enumerate(sel):
        a = ac[k]
        # the transcendentals themselves: float evaluations of the same angles (<= 2 ulp of float)
        assert abs(a[0] - np.cos(np.float64(b["yaw"][i]))) < 3e-7 and abs(a[1] - np.sin(np.float64(b["yaw"][i]))) < 3e-7
        r64 = K.quat_to_rpy(b["q"][i])
        assert np.abs(a[2:5] - np.array(r64)).max() < 1e-6
        H, g = K.assemble(b, i, trig=(a[0], a[1]), rpy=(a[2], a[3], a[4]))
        st = np.flatnonzero(b["gait"][i])
        vi = (3 * st[:, None] + np.arange(3)[None]).reshape(-1)
        n = vi.size
        Hr, gr = H[np.ix_(vi, vi)], g[vi]
        worst_h = max(worst_h, np.abs(Hc[k][:n, :n] - Hr).max() / np.abs(Hr).max())
        worst_g = max(worst_g, np.abs(gc[k][:n] - gr).max() / np.abs(gr).max())
    return worst_h, worst_g


def qpoases_on_own_qp(b, res, idx, nwsr=20000, skip_empty=False):
    """The reference's qpOASES (iteration cap lifted) on the GPU's own dumped QP, robot by robot of idx
    -> (i, relative distance of the GPU's solution to qpOASES's, qpOASES's solution, its rows Ar, lr, ur)."""
    for i in idx:
        H, g, A, lb, ub, x0 = O.assemble(b, i)
        ve, Hr, gr, Ar, lr, ur = O.reduce(H, g, A, lb, ub)
        n = gr.size
        if skip_empty and n == 0:
            continue
        xq, y, used, rc, irc = O.qpoases(res["H"][i][:n, :n], res["g"][i][:n], Ar, lr, ur, nwsr=nwsr)
        assert rc == 0 and irc == 0, (i, rc, irc)
        yield i, np.abs(res["soln"][i][~ve] - xq).max() / max(np.abs(xq).max(), 1.0), xq, Ar, lr, ur


def solver_parity_on_own_qp(m, b, pick, tol=1e-8, nwsr=20000):
    """Solve b with the QP dump on and compare the robots `pick(res)` selects with the reference's qpOASES
    (iteration cap lifted) on the GPU's own assembled QP."""
    res = solve_with_dump(m, b)
    assert ((res["status"] & 47) == 0).all()
    idx = pick(res)
    worst, nact = 0.0, []
    for i, err, xq, Ar, lr, ur in qpoases_on_own_qp(b, res, idx, nwsr=nwsr):
        worst = max(worst, err)
        ax = Ar @ xq
        nact.append(int(((ax - lr < 1e-7) | (ur - ax < 1e-7)).sum()))   # rows at a bound at the solution
    assert worst < tol, worst
    return res, idx, worst, nact


def qpoases_error(b, res):
    """Per robot: relative distance of the solution to qpOASES's on the dumped QP, and how many of the engine's constraints
    (four friction rows and the force limit per stance foot-step) are active at the GPU's solution."""
    err = np.zeros(b["batch"])
    h = b["horizon"]
    f = res["soln"].reshape(b["batch"], h, 4, 3)
    fx, fy, fz = f[..., 0] / b["mu"], f[..., 1] / b["mu"], f[..., 2]
    act = sum((np.abs(s) < 1e-6).astype(np.int64) for s in (fx + fz, fz - fx, fy + fz, fz - fy, b["f_max"] - fz))
    nact = (act * (b["gait"].reshape(b["batch"], h, 4) != 0)).sum((1, 2))
    for i, e, *_ in qpoases_on_own_qp(b, res, range(b["batch"]), skip_empty=True):
        err[i] = e
    return err, nact


# ---------------------------------------------------------------- bit fixtures: "<case>/<figure>" arrays in one npz
def bits_path(name):
    """tests/golden/<name>/bits.npz (a directory of its own: test_gpu_parity.py and test_oracle_cpu.py take every
    tests/golden/*.npz for a batch of solver inputs)."""
    return os.path.join(GOLDEN, name, "bits.npz")


def bits_fixture(path):
    """The module-scoped pytest fixture that loads the bit fixture at path."""
    return pytest.fixture(scope="module")(lambda: np.load(path))


def bits_of(res):
    """The figures every bit test compares: the bits of grf, status and iters."""
    return {"grf": res["grf"].view(np.uint32).copy(), "status": res["status"].copy(), "iters": res["iters"].copy()}


def record_bits(path, cases, run):
    """Write a bit fixture.  run(case) -> (the case's figures {name: array}, what to print behind the case's name)."""
    out = {}
    for case in cases:
        fig, line = run(case)
        print(case, *line)
        for k, v in fig.items():
            out[f"{case}/{k}"] = v
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)


def assert_same_bits(gold, case, fig):
    """Every figure of the case equals the fixture's exactly; names the figure and the robots that differ."""
    for k, v in fig.items():
        want = gold[f"{case}/{k}"]
        assert v.shape == want.shape, f"{case}: {k} has shape {v.shape}, the fixture {want.shape}"
        bad = np.flatnonzero((v != want).reshape(v.shape[0], -1).any(1))
        assert bad.size == 0, f"{case}: {k} differs from the parent's build for robots {bad.tolist()}"
