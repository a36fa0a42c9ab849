"""GPU suite (-m gpu): the error exits of the solve on every engine -- flagged, zeroed, contained.

include/qmpc.h promises QMPC_ST_NOT_PD, QMPC_ST_INFEASIBLE, QMPC_ST_WS_FULL and QMPC_ST_NONFINITE for records that cannot
be solved, zero forces for a robot the method abandoned, and nothing for anybody else.  The families are the nine engine
paths of tests/test_gpu_iteration_cap.py (imported), the JCQP alternate (both modes, and the big ADMM kernel), the sparse
model, the warm start and the fused command call; the kinds and their placement are tests/error_cases.py (pinned on the
host by tests/test_error_cases_cpu.py).  The judges are the clean call of the same handle, qmpc.h, and nothing else:

  1. flagged     every poisoned robot has a bit of QMPC_ST_ERROR_MASK; the two finite kinds QMPC_ST_NOT_PD itself; for EVERY
                 robot of every call a non-finite value in grf or soln implies QMPC_ST_NONFINITE;
  2. bounded     the call returns; 0 <= iters <= max_iter + 20 h (exact solve), <= the ADMM's max_iter rounded up to 10;
  3. contained   every robot that is not poisoned has grf, soln, status, iters (fused call: f_ff and the in/out controller
     in space    state as well) bit-identical to the clean call;
  4. zeroed      a robot with QMPC_ST_INFEASIBLE or QMPC_ST_WS_FULL reads exactly zero in grf and soln (every call's output
                 arrays are filled with 7 before it: a row that is not written shows); swing rows of soln are exactly zero
                 for every robot of every call (JCQP mode 1 solves the full problem: no eliminated rows);
  5. infeasible  qmpc_setup with f_max = -5: every robot with a stance foot-step carries QMPC_ST_INFEASIBLE or
                 QMPC_ST_WS_FULL (the trot family: QMPC_ST_INFEASIBLE itself) -- qmpc.h says which: the method can tell only
                 once its working set has about n_r rows (test_error_cases_cpu.py), so QMPC_ST_INFEASIBLE up to the last
                 engine's 96 slots and QMPC_ST_WS_FULL beyond; a robot with a few foot-steps (n_r < 32, the smallest slot
                 count of any engine) is decided by its first engine, without QMPC_ST_FALLBACK; a robot with an all-swing
                 table reads status 0, zeros, iters 0;
  6. contained   after the poisoned calls, and after the infeasible call and qmpc_setup with the record's own f_max, the
     in time     clean record gives the clean bits again (order hint and size order at their defaults).  Warm start: every
                 call of 3 starts from a cleared buffer (so that the clean bits are the judge); the clean call that
                 DIRECTLY follows a poisoned call starts from what that call stored, has no error bit and lies within
                 cap_judge.X_TOL = 1e-8 relative of the cold clean solution -- the figure of test_gpu_warm_start.Case.check
                 (`assert dq < 1e-8`, no constant there).  Fused: a clean call on a fresh handle gives the same bits.

Which exit reaches which "abandoned iterate" output block (the block is written three times): f_max = -5 ends in the
Schur-form engine's (csrc/qmpc_kernels.hip) for every robot but the one with a few foot-steps, which ends in the event-form
engine's; alpha = -1 makes the step length unbounded (QMPC_ST_NOT_PD | QMPC_ST_INFEASIBLE) in whichever engine has the
robot, the decoupled engine's (csrc/qmpc_engine.hip) in the decoupled families.

One line is printed per family: B, h, calls, robots poisoned, the statuses seen per kind, the largest iters."""
import numpy as np
import pytest

import cap_judge as J
import error_cases as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 7.0                        # what every output array holds before a call
KEYS = ("grf", "soln", "status", "iters")
STATE = ("world_position_desired", "x_comp_integral")
DEAD = E.ST_INFEASIBLE | E.ST_WS_FULL


def _bits(a, b, sel=None):
    a, b = (a, b) if sel is None else (a[sel], b[sel])
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same(r, clean, sel=None, keys=KEYS):
    """The keys on which r differs from clean (over the robots `sel`), bit for bit: NaN equals the same NaN only."""
    return [k for k in keys if not _bits(np.ascontiguousarray(r[k]), np.ascontiguousarray(clean[k]), sel)]


class Family:
    """One handle, its clean call, and the checks every later call on it has to pass."""

    def __init__(self, name, mpc_factory):
        self.name, self.fused = name, name in E.FUSED_FAMILIES
        self.split = self.events = None
        opts = ()
        if self.fused:
            self.b = b = E.commands_of(name)
            self.kinds = E.COMMAND_KINDS
            self.kind_names = list(E.COMMAND_KINDS)
            self.setup_of = {"batch": E.FUSED_BATCH, "horizon": E.FUSED_FAMILIES[name], "dt": 0.026, "mu": 0.4, "f_max": 120.0}
        else:
            if name in J.FAMILIES:
                rec, self.split, self.events, _ = J.FAMILIES[name]
            else:
                rec, opts = E.MORE_FAMILIES[name]
            self.b = b = E.record_of(rec)
            self.kinds = E.RECORD_KINDS
            self.kind_names = E.record_kinds(name)
            self.setup_of = b
        self.B, self.h = int(b["batch"]), int(b["horizon"])
        self.mode1 = opts[:2] == ("jcqp", 1)
        self.opts, self.factory = opts, mpc_factory
        self.m = self.handle()
        self.ws = self.m.warm_start(self.B) if opts == ("warm",) else None
        self.bound = E.iters_bound(name, self.h)
        self.seen, self.poisoned, self.calls, self.most = {}, 0, 0, 0
        self.line = f"{name}: (stopped before the report)"
        self.clean = self.call(self.b)
        assert ((self.clean["status"] & E.ST_ERROR_MASK) == 0).all(), (name, np.unique(self.clean["status"]))
        self.checks(self.clean, self.b, {}, "clean")

    def handle(self):
        m = self.factory(self.setup_of)
        if self.split is not None:
            m.set_split(self.split)
        if self.events:
            m.set_debug_engine_events(self.events)
        if self.opts[:1] == ("jcqp",):
            m.settings_jcqp(self.opts[1], max_iter=E.JCQP_MAX_ITER)
        if self.opts == ("sparse",):
            m.set_robot(9.0, (0.07, 0.26, 0.242), -9.81)
            m.set_model(1)
        return m

    def set_f_max(self, f_max):
        s = self.setup_of
        self.m.setup(s["dt"], s["horizon"], s["mu"], f_max)

    def gait(self, b):
        """[B, 4 h] contact table of record / command b."""
        if not self.fused:
            return np.asarray(b["gait"]).reshape(self.B, -1)
        finite = E.copy(b)      # the table is integer data; the packer's float fields are not looked at here
        for k, v in finite.items():
            if isinstance(v, np.ndarray) and v.dtype.kind == "f":
                finite[k] = np.nan_to_num(v)
        return np.asarray(O.pack_commands(finite, self.setup_of["dt"])[0]["gait"]).reshape(self.B, -1)

    def call(self, b, m=None, cold=True):
        """One call on output arrays that hold FILL (status, iters: -1).  Warm start: from a cleared buffer unless cold=False."""
        import torch
        m = self.m if m is None else m
        if self.ws is not None and cold:
            self.ws.fill_(-1)
        B = self.B
        o = m.alloc_outputs(B, full=True)
        o["grf"].fill_(FILL), o["soln"].fill_(FILL), o["status"].fill_(-1), o["iters"].fill_(-1)
        if self.fused:
            d = m.upload_command(b)
            rec = m.alloc_record(B)
            _, out = m.make_args(rec, o)
            f = torch.full_like(o["grf"], FILL)
            m.solve_commands_async(B, m.make_command_args(d), out, f)
        else:
            d = m.upload(b)
            inp, out = m.make_args(d, o)
            m.solve_async(B, inp, out)
        torch.cuda.synchronize()
        r = {k: o[k].cpu().numpy() for k in KEYS}
        if self.fused:
            r["f_ff"] = f.cpu().numpy()
            for k in STATE:
                r[k] = d[k].cpu().numpy()
        return r

    def checks(self, r, b, plan, tag):
        """1 (the implication), 2 and 4 on every robot of a call; 1 (flagged) on the robots of `plan`."""
        name, B, h = self.name, self.B, self.h
        st, it = r["status"], r["iters"]
        assert st.dtype == np.int32 and it.dtype == np.int32
        assert (it >= 0).all() and (it <= self.bound).all(), (name, tag, "iters out of range", it.min(), it.max(), self.bound)
        assert (st >= 0).all() and (st < 256).all(), (name, tag, np.unique(st))
        nonfin = ~np.isfinite(r["grf"]).all(1) | ~np.isfinite(r["soln"]).all(1)
        assert ((st[nonfin] & E.ST_NONFINITE) != 0).all(), (name, tag, "non-finite result without QMPC_ST_NONFINITE",
                                                            np.flatnonzero(nonfin & ((st & E.ST_NONFINITE) == 0)), st[nonfin])
        dead = (st & DEAD) != 0
        assert not r["grf"][dead].any() and not r["soln"][dead].any(), (
            name, tag, "an abandoned robot does not read zero", np.flatnonzero(dead), st[dead])
        if not self.mode1:
            f = r["soln"].reshape(B, 4 * h, 3)
            sw = self.gait(b) == 0
            assert np.all(f[sw] == 0), (name, tag, "swing rows of soln", np.flatnonzero((f[sw] != 0).any(-1))[:8])
            assert np.all(r["grf"].reshape(B, 4, 3)[sw[:, :4]] == 0), (name, tag, "swing feet of grf")
        for i, kind in plan.items():
            s = int(st[i])
            self.seen.setdefault(kind, set()).add(s)
            assert s & E.ST_ERROR_MASK, (name, tag, i, kind, "poisoned and not flagged", s)
            if kind in E.FINITE_KINDS:
                assert s & E.ST_NOT_PD, (name, tag, i, kind, "no QMPC_ST_NOT_PD", s)
        self.most = max(self.most, int(it.max()))

    def contained(self, r, plan, tag, clean=None):
        others = np.ones(self.B, bool)
        others[list(plan)] = False
        diff = same(r, self.clean if clean is None else clean, others, KEYS + (("f_ff",) + STATE if self.fused else ()))
        assert not diff, (self.name, tag, "a robot that is not poisoned differs from the clean call in", diff)

    def follows(self, tag):
        """Warm start: the clean call directly behind a poisoned one, started from what that call stored."""
        r = self.call(self.b, cold=False)
        self.checks(r, self.b, {}, tag + ", the clean call behind it")
        st = r["status"]
        assert ((st & E.ST_ERROR_MASK) == 0).all(), (self.name, tag, "error bit in the clean call that follows", np.unique(st))
        ref = self.clean["soln"]
        d = float((np.abs(r["soln"] - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())
        self.warm_worst = max(getattr(self, "warm_worst", 0.0), d)
        assert d < J.X_TOL, (self.name, tag, "warm clean call too far from the cold clean solution", d)

    def poisoned_calls(self):
        allowed = E.command_allowed(self.b) if self.fused else None     # (a standing robot's solve does not read every field)
        for c, plan in enumerate(E.plans(self.B, self.kind_names, allowed)):
            tag = f"call {c}"
            assert len(plan) <= self.B // 2
            bad = E.poisoned(self.b, plan, self.kinds)
            r = self.call(bad)
            self.calls += 1
            self.poisoned += len(plan)
            self.checks(r, bad, plan, tag)
            self.contained(r, plan, tag)
            if self.ws is not None:
                self.follows(tag)
        self.back_to_clean("after the poisoned calls")

    def back_to_clean(self, tag):
        diff = same(self.call(self.b), self.clean, None, KEYS + (("f_ff",) + STATE if self.fused else ()))
        assert not diff, (self.name, tag, "the clean record no longer gives the clean bits in", diff)

    def infeasible(self):
        """5, and 6 behind it: f_max = -5 for the whole handle, one robot with an all-swing table."""
        name, B = self.name, self.B
        free, small = B // 2, B // 2 - 1
        b = E.copy(self.b)
        E.all_swing(b, free, command=self.fused)
        E.small_table(b, small, command=self.fused)
        try:
            self.set_f_max(E.F_MAX_INFEASIBLE)
            r = self.call(b)
            self.calls += 1
        finally:
            self.set_f_max(self.setup_of["f_max"])
        if self.ws is not None:
            self.follows("f_max = -5")
        st = r["status"]
        rest = (np.arange(B) != free) & (np.arange(B) != small)
        self.seen["f_max=-5"] = set(st[rest].tolist())
        self.seen["f_max=-5, few foot-steps"] = {int(st[small])}
        self.checks(r, b, {}, "f_max = -5")
        gait = self.gait(b)
        stance = (gait != 0).any(1)
        assert not stance[free] and stance.sum() == B - 1
        assert ((st[stance] & DEAD) != 0).all(), (name, "f_max = -5: a robot is neither INFEASIBLE nor WS_FULL", st[stance])
        if name == "trot":
            assert ((st[stance] & E.ST_INFEASIBLE) != 0).all(), (name, "QMPC_ST_INFEASIBLE itself", st[stance])
        # which of the two: qmpc.h -- the method can tell once its working set has about n_r rows, the last engine has 96 slots
        rows = 3 * (gait != 0).sum(1)
        fits = stance & (rows <= E.INFEASIBLE_ROWS)
        assert ((st[fits] & E.ST_INFEASIBLE) != 0).all(), (name, "n_r <= 96 and not QMPC_ST_INFEASIBLE", rows[fits], st[fits])
        assert ((st[stance & ~fits] & E.ST_WS_FULL) != 0).all(), (name, "n_r > 96 and not QMPC_ST_WS_FULL", st[stance & ~fits])
        # a robot of a few foot-steps: its first engine has the slots to decide by itself, nobody solves it a second time
        assert rows[small] < E.SMALL_ROWS and (st[small] & E.ST_INFEASIBLE) and not (st[small] & E.ST_FALLBACK), (
            name, "the robot with a few foot-steps", int(rows[small]), int(st[small]))
        assert st[free] == 0 and r["iters"][free] == 0 and not r["grf"][free].any() and not r["soln"][free].any(), (
            name, "the all-swing robot", int(st[free]), int(r["iters"][free]))
        if self.fused:      # qmpc.h: a robot that is not solved has its controller state advanced like everybody else's
            assert not same(r, self.clean, rest, STATE), (name, "controller state of the abandoned robots")
            assert not r["f_ff"][stance].any(), (name, "f_ff of the abandoned robots")
        self.back_to_clean("after f_max = -5 and qmpc_setup with the record's f_max")

    def report(self):
        seen = "; ".join(f"{k} {sorted(v)}" for k, v in self.seen.items())
        warm = f" warm clean call within {self.warm_worst:.1e}" if hasattr(self, "warm_worst") else ""
        self.line = (f"{self.name}: B={self.B} h={self.h} calls {self.calls} robots poisoned {self.poisoned} largest iters "
                     f"{self.most} (bound {self.bound}){warm} statuses: {seen}")


ALL = list(E.ENGINE_FAMILIES) + list(E.MORE_FAMILIES) + list(E.FUSED_FAMILIES)


@pytest.mark.parametrize("name", ALL)
def test_error_exits(name, mpc_factory):
    fam = None
    try:
        fam = Family(name, mpc_factory)
        fam.poisoned_calls()
        if E.method(name) == E.EXACT:
            fam.infeasible()
        if fam.fused:       # 6: a fresh handle's clean call gives the bits this handle gives after all of the above
            fresh = fam.call(fam.b, m=fam.handle())
            assert not same(fresh, fam.clean, None, KEYS + ("f_ff",) + STATE), (name, "fresh handle")
            assert not same(fam.call(fam.b), fresh, None, KEYS + ("f_ff",) + STATE), (name, "used handle against a fresh one")
    finally:
        if fam is not None:
            fam.report()
            print(fam.line)
        else:
            print(f"{name}: (stopped before the report)")
