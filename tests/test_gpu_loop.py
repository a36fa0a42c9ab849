"""GPU suite (-m gpu) for the loop run (include/qmpc_loop.h; rollout_loop, BatchedController.loop_info).

Every test feeds two handles identically, advances `a` by the per-tick sequence the header states -- rollout() /
rollout_episodes() with the actuators: qmpc_ctrl_tick_state -> the actuator call -> qmpc_plant_step, and on a check tick
qmpc_episode_step -> the actuator reset -- and `b` through qmpc_loop_run, and compares RAW BITS: effort, state, motor,
every controller array qmpc_debug_ctrl_read knows, every array of the plant's view and its statistics, the actuators'
ring, head, age and seven accumulators, the manager's view, the bound vel / gait arrays, T and the counters.  Two things
are compared as sets: the due list (per robot, its order is undefined on both paths) and the result log (keyed by robot
and episode: a wave of the loop kernel holds 16 robots, one of the decision kernel 64).

Fleet sizes of the actuator tests: 1, 17 and 150 robots, as tests/test_gpu_fleet_run.py; the episode tests run
tests/episode_gpu.py's fleet of 96 with its pushes from the first tick on.
"""
import ctypes as C

import numpy as np
import pytest

import episode_gpu as EG
import episode_model as EM
import fleet_gpu as G
import plant_loop as L

pytestmark = pytest.mark.gpu

SIZES = (1, 17, 150)
CTRL = EG.CTRL
ACT_KEYS = ("ring", "head", "age", "n", "n_vsat", "n_tsat", "tau_peak", "e_heat", "e_mech", "e_pos")
EP_KEYS = ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "mask", "xyyaw", "log_count",
           "log_dropped")
LOG_ROWS = 4000
_np, _dev = EG.to_np, G.dev


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b, what):
    G.equal(raw(a), raw(b), what)


def commands(B, mode):
    """The plant source's commands (tools/ctrl_bench.py --source plant), as tests/test_gpu_fleet_run.py."""
    k = np.arange(B)
    gait = np.array([0, 4, 5, 10], np.int32)[k % 4] if mode == 0 else np.full(B, 9, np.int32)
    vel = np.zeros((B, 3))
    vel[:, 0] = 0.5 * ((k * 7) % 16) / 15.0
    vel[:, 2] = 0.1 * ((k % 3) - 1)
    if mode == 0:
        vel[gait == 4] = 0.0
    xyyaw = np.stack([0.5 * (k % 16), 0.5 * (k // 16), 0.05 * ((k % 5) - 2)], 1).astype(np.float64)
    return gait, vel, xyyaw


def actuators(c, p, B):
    """max_delay 3 and per-robot delay b % 4, so the ring is read 0 .. 3 rows back and the age matters; every third robot
    on a weak battery, every fourth with a low torque cap, every fifth at 70 % strength: both saturation counters move."""
    from quadruped_ctrl_amd.binding import BatchedActuators
    k = np.arange(B)
    a = BatchedActuators(p)
    a.init(max_delay=3)
    a.set_params(delay=_dev(c, (k % 4).astype(np.int32)), battery_v=_dev(c, np.where(k % 3 == 0, 3.0, 24.0)),
                 tau_max=_dev(c, np.where(k % 4 == 1, 0.4, 3.0)), strength=_dev(c, np.where(k % 5 == 2, 0.7, 1.0)))
    return a


def compare_ctrl(ca, cb, what, ticks_too=True, mask=None):
    """mask: the robots the manager reset behind the last tick (the same on both handles), or None.  The controller's
    reset of robot b writes 0 into due_list[b] and due_count[b] -- rows of the fleet's list, on both paths: behind such a
    reset the list of the last tick (which its solve has consumed by then) has holes at the places b < count of the reset
    robots, and WHICH robot's entry a hole took depends on the list's order, which neither path defines.  Then the list
    is held to what is defined: a zero at every such place, and elsewhere distinct robots that were due or are reset."""
    ra, rb = ({n: c.read(n) for n in CTRL} for c in (ca, cb))
    for n in CTRL:
        if n == "due_list":                                    # the order is undefined on both paths: per robot
            na, nb = int(ra["due_count"][0, 0]), int(rb["due_count"][0, 0])
            holes = mask[:na] if mask is not None else np.zeros(na, bool)
            if na != nb or not holes.any():
                G.equal(np.sort(ra[n][:na, 0]), np.sort(rb[n][:nb, 0]), f"{what}: the due robots of the last tick")
                continue
            may = set(np.flatnonzero((ra["due"][:, 0] != 0) | mask).tolist())
            for r, path in ((ra, "per tick"), (rb, "fused")):
                lst = r[n][:na, 0]
                assert (lst[holes] == 0).all(), f"{what}: {path}: the due list's places of the reset robots are not zero"
                rest = lst[~holes].tolist()
                assert len(set(rest)) == len(rest) and set(rest) <= may, f"{what}: {path}: the due list holds {rest}"
        else:
            same_bits(ra[n], rb[n], f"{what}: controller array {n}")
    va, vb = ca.view(), cb.view()
    if ticks_too:
        assert va["ticks"] == vb["ticks"], f"{what}: T is {va['ticks']} by the per-tick path and {vb['ticks']} fused"
    G.equal(_np(va["counter"]), _np(vb["counter"]), f"{what}: the counters")


def compare_plant(pa, pb, what):
    for k in ("effort", "state", "motor"):
        same_bits(_np(getattr(pa, k)), _np(getattr(pb, k)), f"{what}: {k}")
    sa, sb = G.snap(pa), G.snap(pb)
    for k in G.PLANT_KEYS:
        same_bits(sa[k], sb[k], f"{what}: plant view {k}")


def compare_act(aa, ab, what):
    va, vb = aa.view(), ab.view()
    for k in ACT_KEYS:
        same_bits(_np(va[k]), _np(vb[k]), f"{what}: actuator {k}")
    return {k: _np(vb[k]) for k in ACT_KEYS}


def fused_only(info, ticks, what):
    assert info["reason"] == 0 and info["fused_ticks"] == info["ticks"] == ticks and info["fallback_ticks"] == 0, (what, info)
    assert 0 < info["fused_launches"], (what, info)


class Twin:
    """Two plain pairs with actuators, fed identically: `a` walks by the per-tick path, `b` by the loop run."""

    def __init__(self, B, schedule="lockstep", mode=None, act=True):
        self.B = B
        self.gait, self.vel, self.xyyaw = commands(B, mode or 0)
        self.h = []
        for _ in range(2):
            c, p = G.pair(B, schedule, mode, xyyaw=self.xyyaw)
            keep = [_dev(c, self.gait), _dev(c, self.vel)]
            c.set_gait(keep[0])
            c.set_vel(keep[1])
            self.h.append((c, p, keep, actuators(c, p, B) if act else None))
        (self.ca, self.pa, _, self.aa), (self.cb, self.pb, _, self.ab) = self.h

    def both(self, f):
        for c, p, keep, a in self.h:
            f(c, p, keep, a)

    def compare(self, what, ticks_too=True):
        import torch
        torch.cuda.synchronize()
        compare_plant(self.pa, self.pb, what)
        compare_ctrl(self.ca, self.cb, what, ticks_too)
        return compare_act(self.aa, self.ab, what) if self.aa is not None else None

    def close(self):
        self.both(lambda c, p, keep, a: c.close())


# ---- 1. actuators only -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", SIZES)
def test_actuators_mode0_lockstep_across_three_solves(B):
    """Five per-tick ticks on both handles (with the actuators, so the ring and the age are mid-way), then 40 ticks, which
    cross the solves of ticks 13, 26 and 39: four launches of the loop kernel."""
    from quadruped_ctrl_amd.binding import rollout, rollout_loop
    t = Twin(B)
    t.both(lambda c, p, keep, a: rollout(c, p, 5, actuators=a))
    t.compare(f"B = {B}, the common prefix")
    rollout(t.ca, t.pa, 40, actuators=t.aa)
    rollout_loop(t.cb, t.pb, 40, actuators=t.ab)
    v = t.compare(f"B = {B}, 40 ticks from T = 5")
    assert t.cb.view()["ticks"] == 45
    info = t.cb.loop_info()
    fused_only(info, 40, B)
    assert info["fused_launches"] == 4, info
    assert t.ca.loop_info() == dict(ticks=0, fused_ticks=0, fused_launches=0, fallback_ticks=0, reason=0)
    assert t.cb.fleet_info()["ticks"] == 0                      # (the fleet run's counts are its own)
    # the stage did something: every period counted, the ring full, the rows of all four delays in use, both counters moved
    assert (v["n"] == 45).all() and (v["age"] == 3).all() and (v["head"] == 45 % 4).all(), (v["n"], v["age"], v["head"])
    assert np.abs(v["ring"]).max() > 1.0 and (v["e_heat"] > 0).all() and (v["tau_peak"] > 0).all()
    if B >= 17:
        assert v["n_vsat"].sum() > 0 and v["n_tsat"].sum() > 0, (v["n_vsat"].sum(), v["n_tsat"].sum())
    t.close()


@pytest.mark.parametrize("B", SIZES)
def test_actuators_mode1_per_robot_schedule(B):
    """Robot mode 1 with the per-robot schedule, group b % 13 reset before tick g so that a thirteenth of the fleet is due
    on every tick (as tests/test_gpu_fleet_run.py); then 30 ticks: 31 launches and 30 solves over the due list."""
    from quadruped_ctrl_amd.binding import rollout, rollout_loop
    t = Twin(B, "per_robot", 1)
    group = np.arange(B) % 13

    def stagger(c, p, keep, a):
        for g in range(13):
            c.reset(_dev(c, group == g))
            c.set_gait(keep[0])                                # (a reset zeroes the robot's commands)
            c.set_vel(keep[1])
            rollout(c, p, 1, actuators=a)
    t.both(stagger)
    t.compare(f"B = {B}, the staggered prefix")
    rollout(t.ca, t.pa, 30, actuators=t.aa)
    rollout_loop(t.cb, t.pb, 30, actuators=t.ab)
    v = t.compare(f"B = {B}, 30 ticks")
    same_bits(t.ca.read("status"), t.cb.read("status"), f"B = {B}: status")
    info = t.cb.loop_info()
    fused_only(info, 30, B)
    assert info["fused_launches"] == 31, info
    assert (v["n"] == 43).all()
    t.close()


# ---- 2. episodes, with and without actuators -------------------------------------------------------------------------------

class Fleets:
    """Two episode_gpu.Fleet (96 robots on flat ground, per-robot payloads, statistics on) with the pushes on from the first
    tick, RULE_ALL and a log with room; optionally actuators whose accumulators a reset clears."""

    def __init__(self, schedule, act, rule=EG.RULE_ALL, ground=None):
        self.f, self.e, self.a = [], [], []
        for _ in range(2):
            f = EG.Fleet(schedule, "flat")
            if ground is not None:
                ground(f)
            f.push()
            self.f.append(f)
            self.e.append(EG.episodes(f, rule, LOG_ROWS))
            self.a.append(actuators(f.c, f.p, EG.B) if act else None)
        self.torch = self.f[0].torch

    def run(self, ticks, every, calls=None, graph=False):
        """`ticks` on a by rollout_episodes; on b through qmpc_loop_run, in one call or in `calls` -> b's graph."""
        from quadruped_ctrl_amd.binding import rollout_episodes, rollout_loop
        (fa, fb), (ea, eb), (aa, ab) = self.f, self.e, self.a
        rollout_episodes(fa.c, fa.p, ea, ticks, every=every, actuators=aa, actuator_stats=True)
        g = None
        for n in calls or (ticks,):
            g = rollout_loop(fb.c, fb.p, n, graph=graph, actuators=ab, episodes=eb, every=every, actuator_stats=True)["graph"]
        return g

    def compare(self, what, ticks_too=True):
        (fa, fb), (ea, eb), (aa, ab) = self.f, self.e, self.a
        EG.same(fa, fb, what)                                  # plant view, controller view, effort, statistics, ...
        compare_plant(fa.p, fb.p, what)
        va, vb = ea.view(), eb.view()
        for k in EP_KEYS:
            same_bits(_np(va[k]), _np(vb[k]), f"{what}: manager {k}")
        compare_ctrl(fa.c, fb.c, what, ticks_too, _np(va["mask"]) != 0)
        same_bits(_np(fa.vel), _np(fb.vel), f"{what}: the bound velocities")
        same_bits(_np(fa.gait), _np(fb.gait), f"{what}: the bound gaits")
        la, lb = ea.log(), eb.log()                             # sorted by (robot, episode): the log as a set
        assert la["dropped"] == lb["dropped"] == 0, (what, la["dropped"], lb["dropped"])
        assert len({(r[0], r[1]) for r in lb["rows"]}) == len(lb["rows"]), f"{what}: a (robot, episode) key twice in the fused log"
        assert EG.rows_equal(la["rows"], lb["rows"]), f"{what}: the logs differ as sets ({len(la['rows'])} and {len(lb['rows'])} rows)"
        if aa is not None:
            compare_act(aa, ab, what)
        return la["rows"]

    def not_vacuous(self, rows, lockstep):
        """On the per-tick handle: every robot finished an episode, each of the six causes is in the log, and a robot was
        reset on a tick that is no multiple of 13 (a robot's first episode starts at T = 0, so it ends at T = its age)."""
        ep = _np(self.e[0].view()["episode"])
        assert (ep >= 1).all(), f"robots that finished no episode: {np.flatnonzero(ep < 1)[:8]}"
        cause = rows[:, 2].astype(np.int64)
        for k, name in enumerate(EM.NAMES):
            assert (cause >> k & 1).any(), f"no episode ended by {name}"
        first = rows[rows[:, 1] == 0]
        assert len(first) == EG.B and (first[:, 3] % 13 != 0).any(), "every first episode ended on a multiple of 13"
        assert not lockstep or (_np(self.f[0].c.view()["counter"]) % 13 == self.f[0].c.view()["ticks"] % 13).all()

    def close(self):
        for f in self.f:
            f.close()


@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("act", [False, True], ids=["episodes", "episodes+actuators"])
@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_episodes_90_ticks(schedule, act, every):
    """90 ticks with a check on every tick, and on every fifth: robots tilt, sink, run away, latch, go NaN and time out, and
    every reset -- controller (T mod 13 in lockstep), commands, plant, statistics, actuators -- lands inside the launch."""
    fl = Fleets(schedule, act)
    fl.compare("start")
    fl.run(90, every)
    rows = fl.compare(f"{schedule}, every {every}, 90 ticks")
    fl.not_vacuous(rows, schedule == "lockstep")
    info = fl.f[1].c.loop_info()
    fused_only(info, 90, schedule)
    # the plan is the span's: in lockstep 6 solves in 90 ticks, 7 launches; per robot a launch per tick and the last C, P
    assert info["fused_launches"] == (7 if schedule == "lockstep" else 91), info
    if act:
        age = _np(fl.a[1].view()["age"])
        assert (age < 3).any() and (age == 3).any(), "no robot's ring was refilling at the end"
    fl.close()


def test_call_splitting():
    """1 + 12 + 13 + 14 ticks in four calls equal 40 per-tick ticks, with a check on every tick and the actuators in: a
    call ends on a whole tick wherever it ends, and the check ticks are the call's own."""
    fl = Fleets("lockstep", True)
    fl.run(40, 1, calls=(1, 12, 13, 14))
    fl.compare("four calls")
    info = fl.f[1].c.loop_info()
    fused_only(info, 40, "four calls")
    # T = 0: 1 -> one launch; 12 -> E..L of tick 13 | C..P (2); 13 -> up to tick 26 | rest (2); 14 -> up to 39 | rest (2)
    assert info["fused_launches"] == 7, info
    fl.close()


# ---- 3. graphs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_graph_of_26_ticks_replayed(schedule):
    """A captured block of 26 ticks, replayed twice in all, equals 52 eager per-tick ticks; the command table and the
    actuators' torque caps are rewritten in place between the two replays, and both show."""
    fl = Fleets(schedule, True)
    new = EG.COMMANDS.copy()
    new[:, 0] = [0.11, 0.12, 0.13, 0.14, 0.15]
    new[:, 3] = 0
    from quadruped_ctrl_amd.binding import rollout_episodes, rollout_loop
    (fa, fb), (ea, eb), (aa, ab) = fl.f, fl.e, fl.a
    rollout_episodes(fa.c, fa.p, ea, 26, actuators=aa, actuator_stats=True)
    g = rollout_loop(fb.c, fb.p, 26, graph=True, actuators=ab, episodes=eb, actuator_stats=True)["graph"]
    fl.compare(f"{schedule}: 26 captured ticks against 26 eager")
    before = _np(eb.view()["episode"])
    for f, a in zip(fl.f, fl.a):
        f.cmd.copy_(_dev(f.c, new))
        a._params["tau_max"].mul_(0.5)
    rollout_episodes(fa.c, fa.p, ea, 26, actuators=aa, actuator_stats=True)
    g.replay()
    rows = fl.compare(f"{schedule}: 2 x 26 captured ticks against 52 eager", ticks_too=False)
    assert fb.c.view()["ticks"] == 26                           # (a replay does not advance the host's count)
    fl.not_vacuous(rows, False)
    after = _np(eb.view()["episode"])
    again = np.flatnonzero(after > before)
    assert len(again) > EG.B // 2
    _, cr = EM.draw(EG.SEED, again, after[again], 7, len(new))
    assert np.array_equal(_np(fb.vel)[again], new[cr, :3]) and (_np(fb.gait)[again] == 0).all()
    info = fb.c.loop_info()
    fused_only(info, 26, schedule)
    assert info["fused_launches"] == (3 if schedule == "lockstep" else 27), info
    fl.close()


def test_graph_of_20_ticks_is_refused_in_lockstep():
    from quadruped_ctrl_amd.binding import QmpcError, rollout_loop
    t = Twin(17)
    with pytest.raises(QmpcError, match="multiple of 13"):
        rollout_loop(t.cb, t.pb, 20, graph=True, actuators=t.ab)
    assert t.cb.view()["ticks"] == 0 and t.cb.loop_info()["ticks"] == 0
    t.close()


# ---- 4. fallback, equivalence, errors --------------------------------------------------------------------------------------

def test_fallback_on_ground_decided_contact():
    """Contact decided by the ground: the call enqueues the per-tick sequence itself -- the contact kernels, the decision
    kernel with the ground rows, the actuators' two launches -- and says why."""
    from quadruped_ctrl_amd.binding import LOOP_REASONS
    fl = Fleets("lockstep", True, ground=lambda f: f.p.set_contact(**G.ON))
    fl.run(15, 5)
    fl.compare("contact decided by the ground, 15 ticks")
    info = fl.f[1].c.loop_info()
    assert info == dict(ticks=15, fused_ticks=0, fused_launches=0, fallback_ticks=15, reason=LOOP_REASONS["contact"]), info
    ca, cb = (f.p.contact() for f in fl.f)
    for k in G.CONTACT_KEYS:
        same_bits(_np(ca[k]), _np(cb[k]), f"contact {k}")
    fl.close()


@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_no_option_is_the_fleet_run(schedule):
    """All three options 0: the call is qmpc_fleet_run -- the same bits, the same launches."""
    from quadruped_ctrl_amd.binding import rollout, rollout_loop
    t = Twin(150, schedule, act=False)
    t.both(lambda c, p, keep, a: rollout(c, p, 5))
    rollout(t.ca, t.pa, 30, fused=True)
    rollout_loop(t.cb, t.pb, 30)
    t.compare(f"{schedule}: 30 ticks, no option")
    fi, li = t.ca.fleet_info(), t.cb.loop_info()
    assert fi == li and li["fused_ticks"] == 30, (fi, li)
    t.close()


def test_errors_enqueue_nothing():
    """Every refusal of include/qmpc_loop.h: the code, and state, T and the counts as they were."""
    import torch
    from quadruped_ctrl_amd.binding import BatchedActuators, BatchedController, BatchedEpisodes, BatchedPlant, LoopOpts, QmpcError, rollout_loop
    fl = Fleets("lockstep", True)
    fl.run(3, 1)
    f, e, a = fl.f[1], fl.e[1], fl.a[1]
    c, p, B = f.c, f.p, EG.B
    torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        s = f.snapshot()
        s.update({f"read.{n}": c.read(n) for n in CTRL})
        s.update({f"act.{k}": _np(v) for k, v in a.view().items() if k in ACT_KEYS})
        s.update({f"ep.{k}": _np(v) for k, v in e.view().items() if k in EP_KEYS})
        return s, c.view()["ticks"], c.loop_info()

    before = state()
    eff, st, mo, h, lib = p.effort.data_ptr(), p.state.data_ptr(), p.motor.data_ptr(), c.mpc.h, c.lib
    run = lambda batch, ticks, o, *ptrs: lib.qmpc_loop_run(h, batch, ticks, None if o is None else C.byref(o), *ptrs, None)
    full, none = LoopOpts(1, 1, 1), LoopOpts(0, 0, 0)
    assert run(B, 13, None, eff, st, mo) == 1                                          # null opts
    for ptrs in ((None, st, mo), (eff, None, mo), (eff, st, None)):
        assert run(B, 13, full, *ptrs) == 1 and run(B, 13, none, *ptrs) == 1           # null pointers
    assert run(B + 1, 13, full, eff, st, mo) == 1                                      # wrong batch
    assert run(B, 0, full, eff, st, mo) == 1 and run(B, -3, none, eff, st, mo) == 1    # ticks < 1
    assert run(B, 13, LoopOpts(0, -1, 0), eff, st, mo) == 1                            # negative episodes_every
    assert run(B, 13, LoopOpts(1, 5, 0), eff, st, mo) == 1                             # ticks % episodes_every != 0
    other = torch.zeros((B, 24), dtype=torch.float64, device=c.device)
    assert run(B, 13, LoopOpts(0, 1, 0), eff, other.data_ptr(), mo) == 1               # episodes: not the plant's own rows
    assert run(B, 13, LoopOpts(0, 1, 0), eff, st, other.data_ptr()) == 1
    assert run(B, 13, LoopOpts(1, 0, 0), mo, st, mo) == 1                              # effort over the plant's motor rows
    assert run(B, 13, LoopOpts(1, 0, 0), mo + 8 * (24 * B - 1), st, mo) == 1           # ... its last element
    assert lib.qmpc_loop_run_info(h, None) == 1
    with pytest.raises(QmpcError):
        rollout_loop(c, p, 7, episodes=e, every=2)
    with pytest.raises(QmpcError):
        rollout_loop(c, p, 0, actuators=a)
    after = state()
    assert set(before[0]) == set(after[0])
    for k in before[0]:
        same_bits(before[0][k], after[0][k], f"refused calls: {k}")
    assert before[1] == after[1] == 3 and before[2] == after[2], (before[1:], after[1:])
    # QMPC_ERR_STATE: before the controller's, the plant's, the actuators' and the manager's init, and before its set
    c2 = BatchedController(0, max_batch=8)
    buf = torch.zeros((8, 24), dtype=torch.float64, device=c2.device)
    run2 = lambda o, s=None, m=None: c2.lib.qmpc_loop_run(c2.mpc.h, 8, 13, C.byref(o), buf.data_ptr(), s or buf.data_ptr(),
                                                         m or buf.data_ptr(), None)
    assert run2(none) == 3
    c2.init(8, L.FREQ, L.PID)
    assert run2(none) == 3
    with pytest.raises(QmpcError, match="before init"):
        rollout_loop(c2, BatchedPlant(c2), 13)
    p2 = BatchedPlant(c2)
    p2.init(0.4, 1)
    s2, m2 = p2.state.data_ptr(), p2.motor.data_ptr()
    assert run2(LoopOpts(1, 0, 0), s2, m2) == 3                                         # actuators before their init
    assert run2(LoopOpts(0, 1, 0), s2, m2) == 3                                         # episodes before their init
    e2 = BatchedEpisodes(p2)
    e2.init(1)
    assert run2(LoopOpts(0, 1, 0), s2, m2) == 3                                         # ... and before qmpc_episode_set
    a2 = BatchedActuators(p2)
    a2.init()
    assert run2(LoopOpts(1, 1, 0), s2, m2) == 3
    assert c2.loop_info()["ticks"] == 0 and c2.view()["ticks"] == 0
    c2.close()
    fl.close()
