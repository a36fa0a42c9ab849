"""The inputs of the error-exit suite (tests/test_gpu_error_exits.py, pinned on the host by tests/test_error_cases_cpu.py):
the poison kinds, where they are placed, and the family table.  Plain numpy, no device.

A `kind` writes ONE field of ONE robot's row of a record (workloads layout) or of a fused command (make_commands layout):

  non-finite            NaN in p, q (one component), w, yaw, weights (one entry), alpha, x_drag, traj (an entry of the last
                        horizon step); +Inf in v; -Inf in r.  Fused call: NaN in position, p_foot, rpy, r_body, vel_des,
                        x_comp_integral, world_position_desired.
  finite, not positive  (a) "zero_hessian": that robot's weights all zero and alpha zero, so H = 0;
  definite              (b) "negative_alpha": alpha = NEG_ALPHA (below).
  infeasible            not a kind of a row: qmpc_setup with F_MAX_INFEASIBLE = -5 makes 0 <= fz <= f_max empty for every
                        stance foot-step of every robot of the handle.  One robot of that call gets an all-swing table
                        (`all_swing`: nothing to solve) and one a table of a few foot-steps (`small_table`: the first
                        engine can tell by itself; every other robot of these records needs more slots than it has).

NEG_ALPHA.  The reduced Hessian is H = 2 (S + alpha I) with S = sum_pq kron(C_pq, B_p' W B_q) positive semi-definite, so its
first pivot is negative exactly when alpha < -S_00.  S does not depend on alpha: test_error_cases_cpu.py evaluates the fp64
model (oracle/kron_model) at alpha = 0 on every robot of every record below and finds the largest first pivot
S_00 = H_00 / 2: 2e-3 .. 4e-3 at horizons 10 and 14, 9e-3 at horizon 20, 5.3e-2 at horizon 36 (it grows with the horizon:
every later step adds its square).  The test asserts S_00 < 0.1 everywhere; NEG_ALPHA = -1 is ten times that bound, is exact
in float, and the test proves a negative first pivot and a negative eigenvalue with it for every robot.  (The first pivot is what the register sweep looks at first; the sparse model's Hessian has the same
form with another S, checked with oracle/sparse_model in the same test.)"""
import numpy as np

NEG_ALPHA = -1.0
F_MAX_INFEASIBLE = -5.0
# include/qmpc.h on QMPC_ST_INFEASIBLE: the dual method can tell only once its working set has about n_r rows
# (gi_until_infeasible below, pinned in test_error_cases_cpu.py), so n_r <= 96 -- the Schur-form engine's slots -- reports
# QMPC_ST_INFEASIBLE and a larger robot QMPC_ST_WS_FULL
INFEASIBLE_ROWS = 96

# QMPC_ST_* (include/qmpc.h)
ST_MAXITER, ST_NOT_PD, ST_INFEASIBLE, ST_WS_FULL, ST_FALLBACK, ST_NONFINITE = 1, 2, 4, 8, 16, 32
ST_ERROR_MASK = 15 | 32

NAN, INF = float("nan"), float("inf")


def _set(field, index, value):
    def poison(b, i):
        row = b[field][i:i + 1].reshape(-1)      # a view of robot i's row (1-d fields: its one entry)
        row[index(b) if callable(index) else index] = value
    return (field,), poison


def _zero_hessian(b, i):
    b["weights"][i, :] = 0.0
    b["alpha"][i] = 0.0


def _negative_alpha(b, i):
    b["alpha"][i] = NEG_ALPHA


# kind -> (the fields it writes, poison(b, i)); the traj entry: x position of the last horizon step (weight 50 / 10)
NONFINITE_KINDS = {
    "nan_p": _set("p", 0, NAN), "nan_q": _set("q", 2, NAN), "nan_w": _set("w", 1, NAN), "nan_yaw": _set("yaw", 0, NAN),
    "nan_weights": _set("weights", 5, NAN), "nan_alpha": _set("alpha", 0, NAN), "nan_x_drag": _set("x_drag", 0, NAN),
    "nan_traj_last": _set("traj", lambda b: 12 * (int(b["horizon"]) - 1) + 3, NAN),
    "inf_v": _set("v", 1, INF), "ninf_r": _set("r", 3, -INF),
}
NOT_PD_KINDS = {"zero_hessian": (("weights", "alpha"), _zero_hessian), "negative_alpha": (("alpha",), _negative_alpha)}
RECORD_KINDS = {**NONFINITE_KINDS, **NOT_PD_KINDS}
COMMAND_KINDS = {
    "nan_position": _set("position", 1, NAN), "nan_p_foot": _set("p_foot", 4, NAN), "nan_rpy": _set("rpy", 2, NAN),
    "nan_r_body": _set("r_body", 0, NAN), "nan_vel_des": _set("vel_des", 0, NAN),
    "nan_x_comp_integral": _set("x_comp_integral", 0, NAN),
    "nan_world_position_desired": _set("world_position_desired", 1, NAN),
}
FINITE_KINDS = tuple(NOT_PD_KINDS)


def copy(b):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def poisoned(b, plan, kinds):
    """A copy of record / command `b` with plan = {robot: kind} written in."""
    out = copy(b)
    for i, kind in plan.items():
        kinds[kind][1](out, i)
    return out


def plans(B, kinds, allowed=None):
    """The calls of a family: a list of {robot: kind}.  Even calls poison robots 0, 2, 4, ..., odd calls B-1, B-3, ... --
    B // 2 robots each, at most half of the batch -- and the kinds go round over them, as many calls as it takes for every
    kind to be used, two at the least: robot 0 and robot B-1 are poisoned, and with B even every robot is, once.
    allowed = {kind: [B] bool}: the robots whose solve reads that kind's field; a robot takes the next kind it may."""
    queue = list(kinds)
    half = B // 2
    assert half >= 1 and queue
    out, used = [], set()
    while len(used) < len(queue) or len(out) < 2:
        assert len(out) < 16, "a kind fits no robot"
        robots = [2 * j for j in range(half)] if len(out) % 2 == 0 else [B - 1 - 2 * j for j in range(half)]
        plan = {}
        for i in robots:
            fits = [k for k in queue if allowed is None or k not in allowed or allowed[k][i]]
            plan[i] = fits[0]
            queue.append(queue.pop(queue.index(fits[0])))      # ... which goes to the back of the queue
            used.add(fits[0])
        out.append(plan)
    return out


# The standing branch of the packer (gait_type == 4, ConvexMPCLocomotion.cpp:514-531) builds the trajectory from stand_traj
# and does not touch the desired position: vel_des, r_body (which only rotates vel_des) and world_position_desired are
# read for a robot that walks and for no other.  Those kinds go to walking robots.
WALKING_ONLY = ("nan_vel_des", "nan_r_body", "nan_world_position_desired")


def command_allowed(cmd):
    walks = np.asarray(cmd["gait_type"]) != 4
    return {k: walks for k in WALKING_ONLY}


def all_swing(b, i, command=False):
    """Robot i never touches the ground in the horizon: an empty QP."""
    if command:
        b["gait_durations"][i, :] = 0         # (Gait.cpp:142-166: a foot is down while its progress < duration)
        b["gait_type"][i] = 0
    else:
        b["gait"][i, :] = 0


SMALL_ROWS = 32     # a reduced size below the smallest working-set capacity of any engine (the 64-row class's 32 slots)


def small_table(b, i, command=False):
    """Robot i with a few stance foot-steps only: n_r = 18 (a record: feet 0 and 3 down for the first three steps) or 12
    (a command: every foot down for one segment).  A working set holds independent rows, at most n_r < SMALL_ROWS of them:
    whichever engine takes this robot can decide by itself that the rows are inconsistent, without running out of slots."""
    if command:
        b["gait_durations"][i, :] = 1
        b["gait_type"][i] = 0
    else:
        g = np.zeros((int(b["horizon"]), 4), np.uint8)
        g[:3, 0] = g[:3, 3] = 1
        b["gait"][i, :] = g.reshape(-1)


def gi_until_infeasible(b, i, H, g, tol=1e-9, max_iter=5000):
    """warm_sets.gi_iters' cold loop on a QP whose rows are inconsistent, run until the method can tell (no step length is
    finite) -> (iters, the largest working set on the way, the working set when it told); None if it never did."""
    import warm_sets as WS
    st = WS.stance(b, i)
    allid = [5 * int(k) + t for k in st for t in range(5)]
    Ca, da = WS.coef_rows(b, i, allid)
    mi = WS.mu_inv(b)
    nrm = np.array([1.0 if e % 5 == 4 else 1.0 / np.sqrt(mi * mi + 1.0) for e in allid])
    Hi = np.linalg.inv(H)
    x = -Hi @ g
    Wk, lam, iters, most = [], np.zeros(0), 0, 0
    while iters < max_iter:
        viol = (Ca @ x - da) * nrm
        viol[Wk] = 0.0
        p = int(np.argmin(viol))
        if not viol[p] < -tol:
            return None
        lp = 0.0
        while True:
            if Wk:
                N = Ca[Wk].T
                Ns = np.linalg.solve(N.T @ Hi @ N, N.T @ Hi)
                P = Hi - Hi @ N @ Ns
            else:
                P, Ns = Hi, np.zeros((0, g.size))
            c = Ca[p]
            z, r = P @ c, Ns @ c
            delta = c @ z
            dep = not delta > 1e-11 * (c @ Hi @ c)
            t2 = np.inf if dep else -(c @ x - da[p]) / delta
            ratio = np.where(r > 0, np.maximum(lam, 0.0) / np.where(r > 0, r, 1.0), np.inf) if Wk else np.zeros(0)
            t1 = ratio.min() if Wk else np.inf
            t = min(t1, t2)
            if not np.isfinite(t):
                return iters, most, len(Wk)
            if not dep:
                x = x + t * z
            lam = lam - t * r
            lp += t
            iters += 1
            if t2 <= t1:
                Wk.append(p)
                lam = np.append(lam, lp)
                most = max(most, len(Wk))
                break
            l = int(np.argmin(ratio))
            Wk.pop(l)
            lam = np.delete(lam, l)
    return None


# ---- the families
# The nine engine families are cap_judge.FAMILIES as they are; ENGINE_FAMILIES names them so that a new one
# added there cannot be forgotten here (test_error_cases_cpu.py compares the two).  Which exit a family's method has:
EXACT, ADMM = "exact", "admm"
ENGINE_FAMILIES = ("trot", "mixed", "standing_h10_one_kernel", "standing_h10_decoupled", "decoupled_handed_back",
                   "standing_h14_one_kernel", "standing_h14_decoupled", "many_active", "beyond_192_rows")
# further record families: name -> (record maker key, what is switched on); makers in `record_of`
MORE_FAMILIES = {
    "jcqp1_trot": ("trot", ("jcqp", 1)),
    "jcqp2_trot": ("trot", ("jcqp", 2)),
    "jcqp1_stand_h20": ("stand_h20", ("jcqp", 1)),           # the big ADMM kernel
    "sparse_mixed": ("mixed_sparse", ("sparse",)),
    "warm_trot": ("trot", ("warm",)),
    "warm_standing_h10": ("standing_h10", ("warm",)),
}
FUSED_FAMILIES = {"fused_h10": 10, "fused_h14": 14}         # qmpc_solve_commands on make_commands(33, horizon, stand_fraction 0.3)
FUSED_BATCH, FUSED_STAND = 33, 0.3
JCQP_MAX_ITER = 10000                                        # the binding's default, the reference caller's setting


def record_of(key):
    """The record of a family (cap_judge.RECORDS for the engine families' keys)."""
    import cap_judge as J
    from quadruped_ctrl_amd import workloads as W
    if key in J.RECORDS:
        return J.RECORDS[key][0]()
    if key == "stand_h20":
        return W.make_long_horizon(4, 20, "stand")
    if key == "mixed_sparse":                                # SparseCMPC's parameters, as in test_sparse_formulation_model
        from oracle import sparse_model as SM
        b = J.RECORDS["mixed"][0]()
        b["mu"] = SM.SPARSE_MU
        b["weights"] = np.tile(SM.SPARSE_WEIGHTS.astype(np.float32), (int(b["batch"]), 1))
        return b
    raise KeyError(key)


def commands_of(name):
    from quadruped_ctrl_amd import workloads as W
    return W.make_commands(FUSED_BATCH, horizon=FUSED_FAMILIES[name], stand_fraction=FUSED_STAND)


def record_kinds(name):
    """The kinds a record family takes: every one whose field the family reads (the sparse model ignores x_drag)."""
    return [k for k in RECORD_KINDS if not (name == "sparse_mixed" and k == "nan_x_drag")]


def method(name):
    return ADMM if name.startswith("jcqp") else EXACT


def iters_bound(name, h, max_iter=1000):
    """qmpc.h: the exact solve's count may pass the cap by the drops of the last add, and no more rows exist than 20 h;
    the ADMM looks at its residual every tenth iteration and stops there at the latest at max_iter rounded up."""
    return -(-JCQP_MAX_ITER // 10) * 10 if method(name) == ADMM else max_iter + 20 * h
