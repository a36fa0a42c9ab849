"""GPU suite (-m gpu) for episodes on the sensor path (include/qmpc_episode_sense.h; SensedEpisodes,
rollout_sensed_episodes).

Everything but the last test compares two runs of the library BIT FOR BIT (np.array_equal / bytes): a robot the manager
holds against a robot that is settled by the calls that existed before (sensors.sense -> ctrl.prework on a fresh
controller), a fleet the device manages against a fleet the host drives with tests/episode_sense_model.py deciding, a
captured block against eager ticks.  There is no tolerance.  The last test is the envelope test of
tests/test_gpu_sense.py for the SECOND episode of a fleet that the manager has reset and warmed up; it keeps its own
run() phases and takes the statistics and the envelope assertion from tests/fleet_gpu.py.  The managed fleet (Managed) and
the manager's checks are tests/episode_gpu.py's.

B = 96: one full wave and one half wave, so held, newly held and walking robots meet in one wave and the log's append
crosses waves.

The loop senses AFTER the manager's step, so a robot reset at step t reads n = 0 there, is held at steps t+1 .. t+W -- its
ticks t+1 .. t+W count as pre_work on readings 0 .. W-1 -- and walks from tick t+W+1 on reading W.  The host-driven
counterpart is therefore  W x (sense -> prework), sense, ticks.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import episode_gpu as EG
import episode_model as EM
import episode_sense_model as ESM
import fleet_gpu as G
import plant_loop as L
import sense_loop as SL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SEED_E, SEED_N, CTRL = EG.B, EG.SEED, EG.SEED_N, EG.CTRL     # (the draws' seed, the noise's, the controller's arrays)
_dev, _all, _np, _bits, _snap, _stats = G.dev, G.all_robots, EG.to_np, EG.bits, G.snap, G.plant_stats
KEPT = ("q", "qd", "leg_J", "leg_p", "leg_v", "kf_p", "kf_v", "orientation", "rpy", "r_body", "omega_body", "omega_world",
        "a_world", "ori_ini_inv", "xhat", "P", "position", "v_world", "v_body", "first_visit")
SCRATCH = ("due_list", "due_count")   # a tick's dense list of due robots and its length: not a robot's own state
LIST = ("due_list",)                  # ... and the list's order across waves is the atomics': two runs may differ in it
assert set(KEPT) < set(CTRL) and set(SCRATCH) < set(CTRL)


class _Fleet:
    """Controller + plant + sensors on plant_loop's commands over n robots, the commands as device tensors to bind."""

    def __init__(self, schedule, mode=0, noisy=True, n=B, seed=SEED_N, noise=None):
        import torch
        self.torch, self.n = torch, n
        self.c, self.p, self.s, (gait, vel, xyyaw) = G.trio(n, schedule, 1 if mode == 1 else None, seed=seed)
        self.gait_np, self.vel_np, self.xyyaw = gait, vel, xyyaw
        self.gait, self.vel = _dev(self.c, gait), _dev(self.c, vel)
        self.keep = G.sense_bind(self.c, self.s, G.sense_values(n, 11) if noise is None else noise) if noisy else None
        self.e = self.se = None

    def manage(self, W, spawn=None, commands=None, log_rows=0, **rule):
        from quadruped_ctrl_amd.binding import BatchedEpisodes, SensedEpisodes
        self.e = BatchedEpisodes(self.p)
        self.e.init(SEED_E)
        self.spawn_np = self.xyyaw[:, None, :].copy() if spawn is None else spawn
        self.spawn_t = _dev(self.c, self.spawn_np)
        self.cmd_t = None if commands is None else _dev(self.c, commands)
        self.e.set(self.vel, self.gait, self.spawn_t, self.cmd_t, log_rows=log_rows, **rule)
        self.se = SensedEpisodes(self.e, self.s)
        self.se.init(W)
        return self.se

    def tick(self, effort=True):
        """One period of rollout_sensed_episodes up to, not including, the reading."""
        self.c.tick(self.s.imu, self.s.motor, self.p.effort)
        self.p.step(self.p.effort)
        if self.se is not None:
            self.se.step(self.p.effort if effort else None)

    def host_reset(self, mask, rows, W=None):
        """What the manager does for a robot that finished, by the calls that existed before, and the hold."""
        mt = _dev(self.c, mask)
        self.c.reset(mt)
        self.c.set_gait(self.gait)
        self.c.set_vel(self.vel)
        self.p.reset(mt, _dev(self.c, rows))
        self.s.reset(mt)
        if W is not None:
            self.se.hold(mt, W)

    def snapshot(self):
        self.torch.cuda.synchronize()
        d = {f"ctrl.{k}": self.c.read(k) for k in CTRL}
        d.update({f"plant.{k}": v for k, v in _snap(self.p).items()})
        d.update(effort=_np(self.p.effort), imu=_np(self.s.imu), motor=_np(self.s.motor))
        v = self.s.view()
        d["sense.n"], d["sense.epoch"] = _np(v["n"]), _np(v["epoch"])
        return d

    def close(self):
        self.c.close()


def _same_rows(sa, sb, rows, what, skip=SCRATCH):
    assert set(sa) == set(sb) and len(sa) > 60
    for k in sa:
        if k.split(".")[-1] in skip:
            continue
        a, b = sa[k][rows], sb[k][rows]
        assert _bits(a, b), (what, k, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:8])


def _same(fa, fb, what, skip=LIST):
    sa, sb = fa.snapshot(), fb.snapshot()
    _same_rows(sa, sb, slice(None), what, skip)
    return sa


# ---- 1. the partial re-initialisation -------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["per_robot", "lockstep"])
def test_partial_init_keeps_the_prework_set_and_nothing_else(schedule):
    """30 closed-loop ticks, hold(all), one step: every array outside the kept set is what qmpc_ctrl_reset leaves on a twin
    that walked the same 30 ticks (with the per-robot schedule that is a freshly initialised controller's, which is also
    compared) with the commands handed over again, every kept array is what it was, effort is zero."""
    from quadruped_ctrl_amd.binding import rollout_sensed
    fa, fb = _Fleet(schedule), _Fleet(schedule)
    for f in (fa, fb):
        f.s.settle(5)
        rollout_sensed(f.c, f.p, f.s, 30)
    se = fa.manage(3, causes=0)
    before = fa.snapshot()
    assert np.abs(before["effort"]).max() > 1.0 and (before["ctrl.first_run"] == 0).all() and np.abs(before["ctrl.f_ff"]).max() > 1.0
    se.hold()
    se.step(fa.p.effort)
    after = fa.snapshot()
    fb.c.reset(_all(fb.c, B))
    fb.c.set_gait(fb.gait)
    fb.c.set_vel(fb.vel)
    twin = fb.snapshot()
    fresh = _Fleet(schedule)
    new = fresh.snapshot()
    for k in CTRL:
        if k in KEPT:
            assert _bits(after[f"ctrl.{k}"], before[f"ctrl.{k}"]), k
        else:
            assert _bits(after[f"ctrl.{k}"], twin[f"ctrl.{k}"]), k
            if schedule == "per_robot":
                assert _bits(after[f"ctrl.{k}"], new[f"ctrl.{k}"]), k
    assert (after["ctrl.counter"] == (0 if schedule == "per_robot" else 30 % 13)).all()
    assert not _bits(before["ctrl.P"], new["ctrl.P"]) and (after["ctrl.contact_phase"] == 0.5).all()
    assert (after["effort"] == 0).all() and (after["ctrl.safe"] == 1).all() and (after["ctrl.first_visit"] == 0).all()
    v = se.view()
    assert (_np(v["hold"]) == 1).all() and (_np(v["warm"]) == 2).all() and v["warm_ticks"] == 3 and v["batch"] == B
    assert not _np(fa.e.view()["mask"]).any() and (_np(fa.e.view()["age"]) == 0).all()
    # the plant stands where it walked to, upright: x, y kept, the reset's height, at rest
    assert _bits(after["plant.p"][:, :2], before["plant.p"][:, :2]) and (after["plant.p"][:, 2] == 0.29).all()
    assert (after["plant.v"] == 0).all() and (after["plant.q"][:, 1:3] == 0).all()
    for f in (fa, fb, fresh):
        f.close()


# ---- 2. a held robot is a settled robot -----------------------------------------------------------------------------------

@pytest.mark.parametrize("noisy", [True, False], ids=["noisy", "ideal"])
@pytest.mark.parametrize("schedule,mode,W", [("per_robot", 0, 1), ("per_robot", 0, 5), ("per_robot", 1, 1), ("per_robot", 1, 5),
                                             ("lockstep", 0, 5)])
def test_a_held_robot_is_a_settled_robot(schedule, mode, W, noisy):
    """On ideal sensors (nothing bound: the readings do not depend on n or the epoch) and with all six noise arrays bound.
    Fleet A walks with the manager off (causes == 0: only holds are processed).  After the step of tick 40 the host
    resets the robots X -- ctrl.reset, plant.reset at new rows with yaws that are not zero, sensors.reset -- and holds them
    W periods; after the step of tick 42 the same for Y.  For each event a fleet C of the same size and seeds is reset
    whole at the same rows, its sensors reset for those rows, and settled by W x (sense -> prework), sense; then it walks.
    Rows X (Y) of A at tick 40 (42) + W + k and of C after k ticks agree in every controller array, the plant, effort and
    the readings, k = 0, 1, 13, 14, 40.  The rows nobody touched equal a fleet U that has no manager.
    After step 42 and its event the view shows the mix: with W = 5 X is held (3 periods to go), Y newly held, the rest
    walks -- X and Y have members in both waves; with W = 1 X walks again already.
    Lockstep: a reset robot's counter restarts at T mod 13, so C first burns (T + W) mod 13 ticks -- T + W is the tick
    after which A's last hold wrote the counter."""
    idx = np.arange(B)
    X, Y = idx % 7 == 2, idx % 7 == 5
    assert X[:64].any() and X[64:].any() and Y[:64].any() and Y[64:].any()
    fa, fu = _Fleet(schedule, mode, noisy), _Fleet(schedule, mode, noisy)
    se = fa.manage(W, causes=0)
    rows = {40: fa.xyyaw + np.array([0.25, -0.15, 0.3]), 42: fa.xyyaw + np.array([-0.1, 0.2, -0.4])}
    who = {40: X, 42: Y}
    for f in (fa, fu):
        f.s.settle(13)
    cs = {}                                                      # event tick -> (fleet C, its ticks so far)
    checks = (0, 1, 13, 14, 40)
    done_checks = 0
    for t in range(1, 42 + W + 40 + 1):
        fa.tick()
        fu.tick()
        if t in who:
            fa.host_reset(who[t], rows[t], W)
            fa.torch.cuda.synchronize()                          # the hold wrote the robots' pose and start
            held_at = _np(fa.e.view()["xyyaw"])[who[t]]
            assert _bits(held_at[:, :2], rows[t][who[t], :2]) and np.abs(held_at[:, 2] - rows[t][who[t], 2]).max() < 1e-15
            assert _bits(_np(fa.e.view()["start"])[who[t]], rows[t][who[t], :2])
            fc = _Fleet(schedule, mode, noisy)
            if schedule == "lockstep":
                fc.s.sense()
                for _ in range((t + W) % 13):
                    fc.tick()
                    fc.s.sense()
                fc.c.reset(_all(fc.c, B))
                fc.c.set_gait(fc.gait)
                fc.c.set_vel(fc.vel)
            fc.p.reset(_all(fc.c, B), _dev(fc.c, rows[t]))
            fc.s.reset(_dev(fc.c, who[t]))
            fc.p.effort.zero_()                                  # (the burnt ticks' output: pre_work writes no effort)
            cs[t] = [fc, -W]
        if t == 42:
            fa.torch.cuda.synchronize()
            v = se.view()
            hold, warm = _np(v["hold"]), _np(v["warm"])
            assert (warm[Y] == W).all() and not hold[Y].any() and not hold[~X].any() and not warm[~(X | Y)].any()
            assert (hold[X] == (1 if W >= 2 else 0)).all() and (warm[X] == max(W - 2, 0)).all()
        for f in (fa, fu):
            f.s.sense()
        for t0, st in cs.items():
            fc = st[0]
            if t == t0:                                          # (A's reading above is C's first, in the next period)
                continue
            if st[1] < 0:                                        # the warm-up by the calls that existed before
                fc.s.sense()
                fc.c.prework(fc.s.imu, fc.s.motor)
                st[1] += 1
                if st[1] == 0:
                    fc.s.sense()
            else:
                fc.tick()
                fc.s.sense()
                st[1] += 1
            if st[1] in checks and t - t0 - W == st[1]:
                sa, sc = fa.snapshot(), fc.snapshot()
                _same_rows(sa, sc, who[t0], f"event {t0}, {st[1]} ticks after the hold")
                if st[1] == 0:
                    assert (sa["effort"][who[t0]] == 0).all() and (sa["sense.n"][who[t0]] == W + 1).all()
                    assert (sa["sense.epoch"][who[t0]] == 1).all()
                if st[1] == 40:
                    assert np.abs(sa["effort"][who[t0]]).max() > 1.0 and (sa["ctrl.safe"][who[t0]] == 1).all()
                done_checks += 1
    assert done_checks == 2 * len(checks)
    _same_rows(fa.snapshot(), fu.snapshot(), ~(X | Y), "the rows nobody touched")
    assert not _np(se.view()["warm"]).any() and (_np(fa.e.view()["age"]) == 0).all()
    for f in [fa, fu] + [st[0] for st in cs.values()]:
        f.close()


def test_hold_keeps_a_placed_robot_on_its_pose_over_the_whole_circle_of_yaw():
    """4096 robots placed by plant.reset at yaws over [-pi, pi] (the ends, zero, both signs of tiny angles, a fine sweep
    and random ones), on flat ground and on the height field: hold(all) and one step, whose plant reset runs on the yaw the
    hold kernel recovered from the quaternion -- p, q, the feet and the read-out are the bits the caller's reset left,
    for every robot.  This pins the hold kernel to the expression the plant's reset kernels build q with."""
    import plant_loop_field as LF
    n = 4096
    rng = np.random.default_rng(7)
    yaw = np.concatenate([[-np.pi, np.pi, 0.0, -0.0, 1e-300, -1e-300, 1e-17, -1e-9, np.pi / 2, -np.pi / 2, 3.0, -3.141592],
                          np.linspace(-np.pi, np.pi, 2042), rng.uniform(-np.pi, np.pi, 2042)])
    assert len(yaw) == n
    for ground in ("flat", "field"):
        f = _Fleet("per_robot", n=n, noisy=False)
        rows = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), yaw], 1)
        if ground == "field":
            z, place, cell = LF.field_for(n, LF.RUNGS["contact"])
            keep = [_dev(f.c, z), _dev(f.c, place)]
            f.p.set_field(keep[0], keep[1], cell, clamp_swing=True)
        f.p.reset(_all(f.c, n), _dev(f.c, rows))
        before = _snap(f.p)
        se = f.manage(2, causes=0)
        f.s.sense()
        se.hold()
        f.tick()
        after = _snap(f.p)
        got = _np(f.e.view()["xyyaw"])
        assert _bits(got[:, :2], rows[:, :2]) and np.abs(got[:, 2] - yaw).max() < 1e-15
        assert (_np(se.view()["hold"]) == 1).all()
        for k in ("p", "q", "v", "omega", "foot", "state", "motor"):
            assert _bits(after[k], before[k]), (ground, k, np.flatnonzero((after[k] != before[k]).reshape(n, -1).any(1))[:8])
        f.close()


# ---- 3. the device manager equals host-driven resets and holds ----------------------------------------------------------

RULE_ALL, COMMANDS, W3, _Managed = EG.RULE_ALL, EG.SENSE_COMMANDS, EG.W3, EG.Managed


@pytest.mark.parametrize("ground", ["flat", "field"])
def test_device_manager_equals_host_driven_resets_and_holds(ground):
    """Fleet A: rollout_sensed_episodes.  Fleet B, one tick at a time: its own manager is off (causes == 0: its step only
    processes holds), tests/episode_sense_model.py decides, and the host calls ctrl.reset, the commands, plant.reset,
    reset_stats, sensors.reset and hold(mask) -- and zeroes the reset robots' effort rows, as the step does.  Both fleets
    start with hold(all).  The commands table has four speeds, and from tick 10 on the plant is pushed per robot class as
    in tests/test_gpu_episode.py (a fleet that merely walks does not leave a range of centimetres within 130 ticks), so
    that robots finish on different steps and for different causes; 130 ticks, compared every tenth:
    controller, plant, contact, ground, statistics, effort, readings, counters, warm and hold in every bit; A's manager
    state and log (as sets) and both fleets' warm against the model."""
    from quadruped_ctrl_amd.binding import rollout_sensed_episodes
    a = _Managed("per_robot", ground, W3, RULE_ALL, 4000)
    b = _Managed("per_robot", ground, W3, dict(causes=0), 0)
    b.torch.cuda.synchronize()
    m = ESM.EpisodeSenseModel(B, SEED_E, _np(b.p.view()["p"]), W3)
    m.set(_np(b.f.vel), _np(b.f.gait), b.f.spawn(), COMMANDS, log_rows=4000, **RULE_ALL)
    for x in (a, b):                                             # the initial settle, through the same mechanism
        x.s.sense()
        x.se.hold()
    a.torch.cuda.synchronize()
    held_at = _np(a.e.view()["xyyaw"])                           # the pose the kernel recovered from the plant
    assert _bits(held_at[:, :2], a.f.xyyaw0[:, :2]) and np.abs(held_at[:, 2] - a.f.xyyaw0[:, 2]).max() < 1e-15
    assert _bits(held_at, _np(b.e.view()["xyyaw"])) and _bits(_np(a.e.view()["start"]), held_at[:, :2])
    m.hold_robots(xyyaw=held_at)
    masks, holds = [], []
    for chunk in range(13):
        if chunk == 1:
            a.f.push()
            b.f.push()
        rollout_sensed_episodes(a.c, a.p, a.s, a.se, 10)
        for _ in range(10):
            b.c.tick(b.s.imu, b.s.motor, b.p.effort)
            b.p.step(b.p.effort)
            b.se.step(b.p.effort)
            b.torch.cuda.synchronize()
            v = b.p.view()
            mask, hold, xyyaw = m.step(_np(v["p"]), _np(v["q"]), _np(b.c.view()["safe"])[:, 0], b.f.ground_rows())
            assert np.array_equal(_np(b.se.view()["hold"]) != 0, hold)
            if mask.any():
                mt = _dev(b.c, mask)
                b.f.gait.copy_(_dev(b.c, m.gait))
                b.f.vel.copy_(_dev(b.c, m.vel))
                b.c.reset(mt)
                b.c.set_gait(b.f.gait)
                b.c.set_vel(b.f.vel)
                b.p.reset(mt, _dev(b.c, xyyaw))
                b.p.reset_stats(mt)
                b.s.reset(mt)
                b.se.hold(mt, W3)
                b.p.effort[mt] = 0.0
            b.s.sense()
            masks.append(mask.copy())
            holds.append(hold.copy())
        what = f"tick {10 * (chunk + 1)}"
        sa, sb = a.snapshot(), b.snapshot()
        assert set(sa) == set(sb)
        for k in sa:
            if k.split(".")[-1] not in LIST:
                assert _bits(sa[k], sb[k]), (what, k, np.flatnonzero((sa[k] != sb[k]).reshape(B, -1).any(1))[:8])
        assert _bits(_np(a.f.vel), m.vel) and _bits(_np(a.f.gait), m.gait), what
        assert np.array_equal(sa["warm"], m.warm) and np.array_equal(sa["hold"] != 0, m.hold), what
        EG.check_manager(a.e, m, what)
    masks, holds = np.array(masks), np.array(holds)
    walking = ~masks & ~holds
    print("resets per tick", masks.sum(1).tolist(), "held per tick", holds.sum(1).tolist(), "per cause",
          dict(zip(EM.NAMES, m.count.sum(0))))
    # held and walking robots together in one wave, in both waves; robots finished on many different steps
    assert (holds[:, :64].any(1) & walking[:, :64].any(1) & holds[:, 64:].any(1) & walking[:, 64:].any(1)).any()
    assert (masks.any(1)).sum() >= 6 and (m.count.sum(0) > 0).sum() >= 4 and (m.episode > 1).any()
    # a finished robot is held exactly W3 steps and not judged meanwhile
    for b_ in np.flatnonzero(masks.any(0))[:8]:
        t0 = int(np.flatnonzero(masks[:, b_])[0])
        if t0 + W3 + 1 < len(masks):
            assert holds[t0 + 1:t0 + 1 + W3, b_].all() and not holds[t0 + 1 + W3, b_] and not masks[t0 + 1:t0 + 1 + W3, b_].any()
    a.c.close()
    b.c.close()


# ---- 4. W = 0 is the plain manager followed by the sensors' reset --------------------------------------------------------

def test_w0_is_the_plain_manager_and_the_sensors_reset():
    """65 ticks with warm_ticks = 0 (effort not given: the plain manager leaves it alone) equal, in every bit, a twin
    fleet on which episodes.step() is followed by sensors.reset(the manager's mask)."""
    rule = dict(causes=EM.ALL, max_ticks=25, cos_tilt_min=0.8, z_min=0.2, range=0.05)
    fa, fb = _Fleet("per_robot"), _Fleet("per_robot")
    spawn = fa.xyyaw[:, None, :] + np.array([[0.0, 0.0, 0.0], [0.2, 0.1, 0.3]])[None]
    se = fa.manage(0, spawn, COMMANDS, 1000, **rule)
    fb.manage(0, spawn, COMMANDS, 1000, **rule)
    for f in (fa, fb):
        f.s.settle(13)
    for t in range(65):
        fa.tick(effort=False)
        fa.s.sense()
        fb.c.tick(fb.s.imu, fb.s.motor, fb.p.effort)
        fb.p.step(fb.p.effort)
        fb.e.step()
        fb.s.reset(fb.e.view()["mask"])
        fb.s.sense()
        if t % 16 == 15 or t == 64:
            _same(fa, fb, f"tick {t + 1}")
    va, vb = fa.e.view(), fb.e.view()
    for k in ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "mask", "xyyaw", "log_count"):
        assert _bits(_np(va[k]), _np(vb[k])), k
    assert EG.rows_equal(fa.e.log()["rows"], fb.e.log()["rows"]) and len(fa.e.log()["rows"]) > B
    assert not _np(se.view()["warm"]).any() and not _np(se.view()["hold"]).any()
    assert (_np(fa.s.view()["epoch"]) == _np(va["episode"])).all() and _np(va["episode"]).max() > 1
    fa.close()
    fb.close()


# ---- 5. off changes no bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_off_changes_no_bit(schedule):
    """causes == 0 and nobody held: 39 ticks of rollout_sensed_episodes against rollout_sensed -- controller, plant,
    effort and sensors in every bit; the manager's state does not move."""
    from quadruped_ctrl_amd.binding import rollout_sensed, rollout_sensed_episodes
    fa, fb = _Fleet(schedule), _Fleet(schedule)
    se = fa.manage(7, causes=0)
    for f in (fa, fb):
        f.s.settle(13)
    for n in (13, 26):
        rollout_sensed_episodes(fa.c, fa.p, fa.s, se, n)
        rollout_sensed(fb.c, fb.p, fb.s, n)
        s = _same(fa, fb, f"{n} ticks")
    assert np.abs(s["effort"]).max() > 1.0 and (s["sense.n"] == 13 + 39).all()
    v = fa.e.view()
    assert not _np(v["mask"]).any() and not _np(v["episode"]).any() and not _np(v["age"]).any()
    assert not _np(se.view()["warm"]).any() and not _np(se.view()["hold"]).any()
    fa.close()
    fb.close()


# ---- 6. graph ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["per_robot", "lockstep"])
def test_graph_replays_equal_eager_ticks(schedule):
    """A 26-tick block captured and replayed five times equals 130 eager ticks in every bit -- warm and hold are device
    state and go on across replays --, the logs are equal as sets, and a commands table rewritten between the second and
    the third replay shows in the vel of every robot reset after it."""
    from quadruped_ctrl_amd.binding import rollout_sensed_episodes
    rule = dict(causes=EM.ALL, max_ticks=30, cos_tilt_min=0.8, z_min=0.2, range=0.05)
    fa, fb = _Fleet(schedule), _Fleet(schedule)
    spawn = fa.xyyaw[:, None, :] + np.array([[0.0, 0.0, 0.0], [0.2, 0.1, 0.3], [-0.1, 0.2, -0.2]])[None]
    for f in (fa, fb):
        f.manage(4, spawn, COMMANDS, 4000, **rule)
        f.s.sense()
        f.se.hold()
    new = COMMANDS.copy()
    new[:, 0] = [0.11, 0.12, 0.13, 0.14]
    new[:, 3] = 0
    g = rollout_sensed_episodes(fa.c, fa.p, fa.s, fa.se, 26, graph=True)["graph"]
    g.replay()
    rollout_sensed_episodes(fb.c, fb.p, fb.s, fb.se, 52)
    _same(fa, fb, "52 ticks")
    for f in (fa, fb):
        f.cmd_t.copy_(_dev(f.c, new))
    fa.torch.cuda.synchronize()
    before = _np(fa.e.view()["episode"])
    for _ in range(3):
        g.replay()
    rollout_sensed_episodes(fb.c, fb.p, fb.s, fb.se, 78)
    _same(fa, fb, "130 ticks")
    assert _bits(_np(fa.vel), _np(fb.vel)) and _bits(_np(fa.gait), _np(fb.gait))
    la, lb = fa.e.log(), fb.e.log()
    assert la["dropped"] == lb["dropped"] == 0 and len(la["rows"]) > B and EG.rows_equal(la["rows"], lb["rows"])
    va, vb = fa.e.view(), fb.e.view()
    for k in ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "mask", "xyyaw", "log_count"):
        assert _bits(_np(va[k]), _np(vb[k])), k
    for k in ("warm", "hold"):
        assert _bits(_np(fa.se.view()[k]), _np(fb.se.view()[k])), k
    after = _np(va["episode"])
    again = np.flatnonzero(after > before)
    assert len(again) > B // 2
    _, cr = EM.draw(SEED_E, again, after[again], 3, len(new))
    assert np.array_equal(_np(fa.vel)[again], new[cr, :3]) and (_np(fa.gait)[again] == 0).all()
    if schedule == "lockstep":
        with pytest.raises(Exception, match="multiple of 13"):
            rollout_sensed_episodes(fa.c, fa.p, fa.s, fa.se, 12, graph=True)
    fa.close()
    fb.close()


# ---- 7. errors and state -------------------------------------------------------------------------------------------------

def test_errors_and_state():
    from quadruped_ctrl_amd import binding as Bd
    import torch
    c = Bd.BatchedController(0, max_batch=B)
    lib, h = c.lib, c.mpc.h
    OK, ARG, STATE = 0, 1, 3
    view = Bd.EpisodeSenseView()

    def calls(n=16):
        return (lib.qmpc_episode_sense_hold(h, n, None, 3, None), lib.qmpc_episode_sense_step(h, n, None, None))

    assert lib.qmpc_episode_sense_init(h, 16, 5, None) == STATE                    # before qmpc_ctrl_init
    c.init(16, L.FREQ, L.PID)
    c.set_schedule("per_robot")
    assert lib.qmpc_episode_sense_init(h, 16, 5, None) == STATE                    # ... qmpc_plant_init
    p = Bd.BatchedPlant(c)
    p.init()
    assert lib.qmpc_episode_sense_init(h, 16, 5, None) == STATE                    # ... qmpc_episode_init
    e = Bd.BatchedEpisodes(p)
    e.init(3)
    assert lib.qmpc_episode_sense_init(h, 16, 5, None) == STATE                    # ... qmpc_sense_init
    s = Bd.BatchedSensors(p)
    s.init(4)
    assert calls() == (STATE, STATE) and lib.qmpc_episode_sense_view_get(h, C.byref(view)) == STATE
    se = Bd.SensedEpisodes(e, s)
    with pytest.raises(Bd.QmpcError):
        se.step()
    with pytest.raises(Bd.QmpcError):
        se.hold()
    assert lib.qmpc_episode_sense_init(h, 8, 5, None) == ARG and lib.qmpc_episode_sense_init(h, 16, -1, None) == ARG
    assert lib.qmpc_episode_sense_init(h, 16, 0, None) == OK
    se.init(5)
    assert lib.qmpc_episode_sense_step(h, 16, None, None) == STATE                 # before qmpc_episode_set
    assert lib.qmpc_episode_sense_hold(h, 16, None, 2, None) == OK                 # (the hold needs no rule)
    vel = torch.zeros((16, 3), dtype=torch.float64, device=c.device)
    gait = torch.zeros(16, dtype=torch.int32, device=c.device)
    spawn = torch.zeros((1, 3), dtype=torch.float64, device=c.device)
    e.set(vel, gait, spawn, causes=EM.TIMEOUT, max_ticks=3)
    assert lib.qmpc_episode_sense_step(h, 8, None, None) == ARG and lib.qmpc_episode_sense_hold(h, 8, None, 2, None) == ARG
    assert lib.qmpc_episode_sense_hold(h, 16, None, -1, None) == ARG and lib.qmpc_episode_sense_view_get(h, None) == ARG
    assert lib.qmpc_episode_sense_view_get(h, C.byref(view)) == OK and (view.batch, view.warm_ticks) == (16, 5)
    v1, v2 = se.view(), se.view()
    for k in ("warm", "hold"):
        assert v1[k].data_ptr() == v2[k].data_ptr() == getattr(view, k), k
    torch.cuda.synchronize()
    assert (v1["warm"] == 2).all() and v1["warm"].dtype == torch.int32 and v1["hold"].dtype == torch.uint8
    # two held steps, three judged ones: everybody times out at age 3 and gets warm_ticks
    ages = []
    for _ in range(5):
        assert lib.qmpc_episode_sense_step(h, 16, None, None) == OK
        torch.cuda.synchronize()
        ages.append((int(e.view()["age"][0]), int(v1["warm"][0]), int(v1["hold"][0]), int(e.view()["mask"][0])))
    assert ages == [(0, 1, 1, 0), (0, 0, 1, 0), (1, 0, 0, 0), (2, 0, 0, 0), (0, 5, 0, 1)]
    assert (e.view()["episode"] == 1).all() and (s.view()["epoch"] == 1).all()
    # a mask holds its robots only; the effort rows of held robots are zeroed, the others' are not
    mask = torch.arange(16, device=c.device) % 4 == 1
    se.init(5)
    se.hold(mask, 1)
    eff = torch.ones((16, 12), dtype=torch.float64, device=c.device)
    se.step(eff)
    torch.cuda.synchronize()
    assert (se.view()["hold"].bool() == mask).all() and (eff[mask] == 0).all() and (eff[~mask] == 1).all()
    with pytest.raises(Bd.QmpcError):
        se.step(torch.ones((16, 11), dtype=torch.float64, device=c.device))
    # qmpc_episode_init again forgets the rule: STATE until the next set
    e.init(3)
    assert lib.qmpc_episode_sense_step(h, 16, None, None) == STATE
    # another batch needs every init again
    c.init(8, L.FREQ, L.PID)
    p.init()
    assert calls(8) == (ARG, ARG) and calls(16) == (ARG, ARG)
    c.close()


# ---- 8. the fleet gets up and walks on noisy sensors -------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_the_fleet_gets_up_and_walks_on_noisy_sensors(mode):
    """The CPU yardstick's commands, four robots per command, per-robot schedule, sense_loop.noise(), warm_ticks = the
    recorded run's settle; every robot's spawn table holds its own start, commands unbound.  hold(all) is the initial
    settle, the fleet walks 100 ticks, TIMEOUT at 100 resets everybody (a new noise epoch), the manager warms everybody up
    again and resets the statistics, and the SECOND episode walks 650 ticks.  No robot is latched, no judged robot's
    solve reports an error bit, and the second episode's five statistics lie inside plant_loop.envelope() of
    tests/golden/sense_closed_loop_cpu.json.
    That file records noise epoch 0; the second episode draws epoch 1.  The reference loop alone
    (sense_loop.cpu_loop_sensed with the sensor model's epoch set to 1, same seed and settle:
    episode_sense_model.reference_loop_on_epoch, whose docstring holds the command) stays inside the envelope:
    the largest distance from the recorded run is 0.069 of the allowed one in mode 0 (z_min) and 0.039 in mode 1, every
    robot safe, every solve's return code 0 -- so the recorded envelope is the yardstick here too, unchanged."""
    from quadruped_ctrl_amd.binding import rollout_sensed_episodes
    reps = 4
    n = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "sense_closed_loop_cpu.json")))
    rec, W = gold[f"mode{mode}"]["noisy"], gold["settle"]
    nz = SL.noise(n)
    for k, v in nz.items():
        assert np.array_equal(np.asarray(gold["noise"][k]), v[:L.N_CMD]), k
    f = _Fleet("per_robot", mode, n=n, seed=gold["seed"], noise=nz)
    assert np.array_equal(gold[f"mode{mode}"]["vel"], f.vel_np[:L.N_CMD]) and np.array_equal(gold[f"mode{mode}"]["gait"], f.gait_np[:L.N_CMD])
    f.p.enable_stats()
    start = _np(f.p.state)
    se = f.manage(W, log_rows=2 * n, causes=EM.TIMEOUT | EM.UNSAFE, max_ticks=100)
    f.s.sense()
    se.hold()

    def run(ticks, judged=True):
        for _ in range(ticks):
            rollout_sensed_episodes(f.c, f.p, f.s, se, 1)
            if judged:
                assert (f.c.read("status")[:, 0] & 47 == 0).all()

    run(W, judged=False)
    f.torch.cuda.synchronize()
    assert not _np(se.view()["warm"]).any() and (_np(f.e.view()["age"]) == 0).all() and (_np(f.s.view()["n"]) == W + 1).all()
    run(99)
    assert (f.c.read("safe") == 1).all() and (_np(f.e.view()["age"]) == 99).all() and (_stats(f.p)["n"] == 99).all()
    run(1, judged=False)                                         # tick 100: everybody times out
    ev = f.e.view()
    f.torch.cuda.synchronize()
    assert (_np(ev["episode"]) == 1).all() and (_np(ev["last_cause"]) == EM.TIMEOUT).all() and (_np(se.view()["warm"]) == W).all()
    assert (_np(f.s.view()["epoch"]) == 1).all() and (_stats(f.p)["n"] == 0).all()
    f.e.set(f.vel, f.gait, f.spawn_t, None, log_rows=2 * n, causes=EM.UNSAFE)     # the second episode has no time limit
    run(W, judged=False)
    assert (_stats(f.p)["n"] == 0).all() and _bits(_np(f.p.state), start)
    run(L.TICKS - int(L.FREQ))
    at150 = _stats(f.p)
    run(int(L.FREQ))
    end = _stats(f.p)
    assert (f.c.read("safe") == 1).all() and (_np(ev["episode"]) == 1).all() and len(f.e.log()["rows"]) == n
    assert (at150["n"] == 150).all() and (end["n"] == L.TICKS).all() and (_np(f.s.view()["n"]) == W + 1 + L.TICKS).all()
    G.assert_inside_envelope(G.stats_from_accumulators(start, at150, end), rec, reps, f"mode {mode}")
    f.close()
