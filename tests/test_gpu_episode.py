"""GPU suite (-m gpu) for the episode manager (include/qmpc_episode.h; BatchedEpisodes, rollout_episodes).

Everything here compares two runs of the library BIT FOR BIT -- a fleet whose episodes the device manages against a
fleet the host drives through the calls that existed before (ctrl.reset, set_gait, set_vel, plant.reset, reset_stats)
with tests/episode_model.py deciding and drawing -- and the manager's own state and log against that model.  There is
no tolerance: the decision is comparisons and single fp64 operations, the draw is integer arithmetic.

B = 96: one full wave and one half wave, so the log's append crosses waves and meets a partial one.

The fleets, the manager's model and the host-driven counterpart are tests/episode_gpu.py's (tests/test_gpu_episode_sense.py
and tests/test_gpu_act.py run them too).

The workload (one definition, episode_gpu.Fleet.push): after a quiet first episode that every robot ends by timing out on the same
tick, the plant -- not the controller -- is pushed per robot class k = b mod 16 mod 4:
  0  a roll torque of 0.15 Ixx / dt^2: the roll passes 0.45, 0.9 rad on consecutive ticks, TILT (cos 0.8) fires first
  1  1500 N downwards: the body sinks below z_min = 0.2 m in about twenty ticks (HEIGHT)
  2  400 N forwards: 0.06 m from the start in about thirty ticks (RANGE)
  3  nothing: TIMEOUT at 40 ticks
robots with b mod 32 == 16 instead get a roll torque of 0.006 Ixx / dt^2 (about 100 N m), slow enough that the
controller's own check (|roll| >= 0.5 rad) latches before the tilt criterion at 0.64 rad: UNSAFE; and robot 5's mass
is NaN: NONFINITE on every tick.  The assertions on the host-driven fleet say that this is what happened.
"""
import ctypes as C

import numpy as np
import pytest

import episode_gpu as EG
import episode_model as EM
import fleet_gpu as G
import plant_loop as L

pytestmark = pytest.mark.gpu

B, SEED, DT, RULE_ALL, COMMANDS = EG.B, EG.SEED, EG.DT, EG.RULE_ALL, EG.COMMANDS
RULE_LATCH = dict(causes=EM.UNSAFE | EM.TIMEOUT, max_ticks=40, cos_tilt_min=0.8, z_min=0.2, range=0.06)
_dev, _all, _np, _bits, _rows_equal = G.dev, G.all_robots, EG.to_np, EG.bits, EG.rows_equal
_Fleet, _same, _episodes, _model, _host_check, _check_manager = (EG.Fleet, EG.same, EG.episodes, EG.model, EG.host_check,
                                                                 EG.check_manager)


# ---- 1. the device manager equals host-driven resets ---------------------------------------------------------------------

@pytest.mark.parametrize("rule", ["all", "latch"])
@pytest.mark.parametrize("ground", ["flat", "field"])
@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_device_manager_equals_host_driven_resets(schedule, ground, rule):
    """Fleet A: rollout_episodes, eager.  Fleet B: rollout one tick at a time, then _host_check.  130 ticks, compared
    every tenth: plant view, controller view, effort, commands, contact counters, ground, statistics -- every bit; A's
    manager state and log against the model.  The log holds 200 rows and overflows."""
    from quadruped_ctrl_amd.binding import rollout, rollout_episodes
    rl = RULE_ALL if rule == "all" else RULE_LATCH
    fa, fb = _Fleet(schedule, ground), _Fleet(schedule, ground)
    ea = _episodes(fa, rl, 200)
    m = _model(fb, rl, 200)
    _same(fa, fb, "start")
    masks = []
    for chunk in range(13):
        if chunk == 4:                                   # after the common time-out at tick 40
            fa.push()
            fb.push()
        rollout_episodes(fa.c, fa.p, ea, 10)
        for _ in range(10):
            rollout(fb.c, fb.p, 1)
            masks.append(_host_check(fb, m))
        s = _same(fa, fb, f"tick {10 * (chunk + 1)}", m.vel, m.gait)
        _check_manager(ea, m, f"tick {10 * (chunk + 1)}")
    # the reference side saw what the test is about
    masks = np.array(masks)
    per_cause = m.count.sum(0)
    print("episodes per cause", dict(zip(EM.NAMES, per_cause)), "total", m.total, "dropped", m.dropped,
          "resets per tick", masks.sum(1).tolist())
    for k, name in enumerate(EM.NAMES):
        if rl["causes"] >> k & 1:
            assert per_cause[k] > 0, name
        else:
            assert per_cause[k] == 0, name
    assert (masks[:, :64].any(1) & masks[:, 64:].any(1) & ~masks.all(1)).any()
    assert masks.all(1).any() and (~masks.any(1)).any() and m.dropped > 0
    assert masks[39].all() and not masks[:39].any()      # the quiet first episode
    assert np.isnan(s["plant.p"]).any() or rule == "all"   # (the NaN robot is reset every tick under the full rule)
    assert len(np.unique(m.gait)) > 2 and (m.episode > 1).sum() > B // 2
    fa.close()
    fb.close()


# ---- 2. graph --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["per_robot", "lockstep"])
def test_graph_replays_equal_eager_ticks(schedule):
    """A 26-tick block captured and replayed five times equals 130 eager ticks in every bit, the logs are equal as sets
    (4000 rows: no overflow), and a commands table rewritten between the second and the third replay shows in the vel
    of every robot reset after it."""
    from quadruped_ctrl_amd.binding import rollout_episodes
    fa, fb = _Fleet(schedule, "flat"), _Fleet(schedule, "flat")
    ea, eb = _episodes(fa, RULE_ALL, 4000), _episodes(fb, RULE_ALL, 4000)
    for f in (fa, fb):
        f.push()
    new = COMMANDS.copy()
    new[:, 0] = [0.11, 0.12, 0.13, 0.14, 0.15]
    new[:, 3] = 0
    g = rollout_episodes(fa.c, fa.p, ea, 26, graph=True)["graph"]
    g.replay()
    rollout_episodes(fb.c, fb.p, eb, 52)
    _same(fa, fb, "52 ticks")
    for f in (fa, fb):
        f.cmd.copy_(_dev(f.c, new))
    fa.torch.cuda.synchronize()
    before = _np(ea.view()["episode"])
    for _ in range(3):
        g.replay()
    rollout_episodes(fb.c, fb.p, eb, 78)
    _same(fa, fb, "130 ticks")
    assert _bits(_np(fa.vel), _np(fb.vel)) and _bits(_np(fa.gait), _np(fb.gait))
    la, lb = ea.log(), eb.log()
    assert la["dropped"] == lb["dropped"] == 0 and len(la["rows"]) > 200 and _rows_equal(la["rows"], lb["rows"])
    va, vb = ea.view(), eb.view()
    for k in ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "mask", "xyyaw", "log_count"):
        assert _bits(_np(va[k]), _np(vb[k])), k
    # the rewritten table: a robot reset after the rewrite is commanded from it
    after = _np(va["episode"])
    again = np.flatnonzero(after > before)
    assert len(again) > B // 2
    _, cr = EM.draw(SEED, again, after[again], 7, len(new))
    assert np.array_equal(_np(fa.vel)[again], new[cr, :3]) and (_np(fa.gait)[again] == 0).all()
    fa.close()
    fb.close()


# ---- 3. off changes no bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", ["causes 0", "cannot fire"])
@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_off_changes_no_bit(schedule, rule):
    """39 ticks of rollout_episodes with causes == 0, and with a rule whose criteria cannot fire (no threshold finite,
    max_ticks at the end of int; UNSAFE and NONFINITE left out), against rollout: no bit differs, no log row, mask zero."""
    from quadruped_ctrl_amd.binding import rollout, rollout_episodes
    rl = dict(causes=0) if rule == "causes 0" else dict(causes=EM.TILT | EM.HEIGHT | EM.RANGE | EM.TIMEOUT,
                                                         max_ticks=2 ** 31 - 1, cos_tilt_min=float("inf"),
                                                         z_min=float("inf"), range=float("-inf"))
    fa, fb = _Fleet(schedule, "flat"), _Fleet(schedule, "flat")
    ea = _episodes(fa, rl, 50)
    for n in (13, 26):
        rollout_episodes(fa.c, fa.p, ea, n)
        rollout(fb.c, fb.p, n)
        s = _same(fa, fb, f"{n} ticks")
    assert np.abs(s["effort"]).max() > 1.0
    lg, v = ea.log(), ea.view()
    assert len(lg["rows"]) == 0 and lg["dropped"] == 0 and not _np(v["mask"]).any() and not _np(v["episode"]).any()
    assert (_np(v["age"]) == (0 if rule == "causes 0" else 39)).all()
    fa.close()
    fb.close()


# ---- 4. every = 13 -----------------------------------------------------------------------------------------------------

def test_every_13():
    """The manager checks every 13th tick: ages advance by 13, a robot that latches between two checks is reset at the
    next one, and the run equals the host-driven loop that checks on the same ticks."""
    from quadruped_ctrl_amd.binding import rollout, rollout_episodes
    rl = dict(RULE_LATCH, max_ticks=52)
    fa, fb = _Fleet("per_robot", "flat"), _Fleet("per_robot", "flat")
    ea = _episodes(fa, rl, 2000)
    m = _model(fb, rl, 2000)
    for f in (fa, fb):
        f.push()
    reset_at_check = np.zeros(B, bool)
    for block in range(10):
        latched_between = np.zeros(B, bool)
        rollout_episodes(fa.c, fa.p, ea, 13, every=13)
        for t in range(13):
            rollout(fb.c, fb.p, 1)
            if t < 12:
                fb.torch.cuda.synchronize()
                latched_between |= _np(fb.c.view()["safe"])[:, 0] == 0
        mask = _host_check(fb, m, 13)
        reset_at_check |= mask & latched_between & ((m.last_cause & EM.UNSAFE) != 0)
        _same(fa, fb, f"tick {13 * (block + 1)}", m.vel, m.gait)
        _check_manager(ea, m, f"tick {13 * (block + 1)}")
        age = _np(ea.view()["age"])
        assert (age % 13 == 0).all() and (block > 0 or (age[~mask] == 13).all())
    assert reset_at_check.any() and m.count[:, 0].sum() > 0 and m.count[:, 5].sum() > 0
    assert (m.last_ticks[m.last_cause != 0] % 13 == 0).all()
    fa.close()
    fb.close()


# ---- 5. errors and state -----------------------------------------------------------------------------------------------

def test_errors_and_state():
    from quadruped_ctrl_amd import binding as Bd
    import torch
    c = Bd.BatchedController(0, max_batch=B)
    lib, h = c.lib, c.mpc.h
    view = Bd.EpisodeView()
    OK, ARG, STATE = 0, 1, 3
    # before qmpc_ctrl_init / qmpc_plant_init / qmpc_episode_init
    assert lib.qmpc_episode_init(h, 16, 1, None) == STATE
    c.init(16, L.FREQ, L.PID)
    assert lib.qmpc_episode_init(h, 16, 1, None) == STATE
    p = Bd.BatchedPlant(c)
    p.init()
    rule, bind = Bd.EpisodeRule(Bd.EP_TIMEOUT, 5, 0.0, 0.0, 0.0), Bd.EpisodeBind()
    assert lib.qmpc_episode_step(h, 16, 1, None) == STATE and lib.qmpc_episode_set(h, 16, C.byref(rule), C.byref(bind)) == STATE
    assert lib.qmpc_episode_log_clear(h, None) == STATE and lib.qmpc_episode_view_get(h, C.byref(view)) == STATE
    assert lib.qmpc_episode_init(h, 8, 1, None) == ARG
    e = Bd.BatchedEpisodes(p)
    with pytest.raises(Bd.QmpcError):
        e.step()
    e.init(3)
    assert lib.qmpc_episode_step(h, 16, 1, None) == STATE         # no rule yet
    vel = torch.zeros((16, 3), dtype=torch.float64, device=c.device)
    gait = torch.zeros(16, dtype=torch.int32, device=c.device)
    spawn = torch.zeros((2, 3), dtype=torch.float64, device=c.device)
    cmds = torch.zeros((3, 4), dtype=torch.float64, device=c.device)
    log = torch.zeros((4, 8), dtype=torch.float64, device=c.device)

    def binding(**kw):
        b = Bd.EpisodeBind(vel.data_ptr(), gait.data_ptr(), spawn.data_ptr(), cmds.data_ptr(), log.data_ptr(), 2, 3, 4, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def set_rc(rule, b, batch=16):
        return lib.qmpc_episode_set(h, batch, C.byref(rule) if rule else None, C.byref(b) if b else None)

    assert set_rc(rule, binding()) == OK
    assert set_rc(rule, binding(), batch=8) == ARG and set_rc(None, binding()) == ARG and set_rc(rule, None) == ARG
    assert set_rc(Bd.EpisodeRule(64, 5, 0.0, 0.0, 0.0), binding()) == ARG and set_rc(Bd.EpisodeRule(-1, 5, 0.0, 0.0, 0.0), binding()) == ARG
    assert set_rc(rule, binding(flags=2)) == ARG
    for k in ("vel", "gait", "spawn"):
        assert set_rc(rule, binding(**{k: None})) == ARG, k
    assert set_rc(rule, binding(n_spawn=0)) == ARG and set_rc(rule, binding(n_commands=0)) == ARG
    assert set_rc(rule, binding(log_rows=-1)) == ARG
    assert set_rc(rule, binding(commands=None, n_commands=0)) == OK and set_rc(rule, binding(log=None, log_rows=0)) == OK
    nan = float("nan")
    assert set_rc(Bd.EpisodeRule(63, 5, nan, float("inf"), -float("inf")), binding()) == OK     # allowed: they never fire
    assert set_rc(rule, binding()) == OK
    assert lib.qmpc_episode_step(h, 16, 0, None) == ARG and lib.qmpc_episode_step(h, 16, -3, None) == ARG
    assert lib.qmpc_episode_step(h, 8, 1, None) == ARG and lib.qmpc_episode_view_get(h, None) == ARG
    assert lib.qmpc_episode_step(h, 16, 3, None) == OK
    # view() aliases and does not copy
    v1, v2 = e.view(), e.view()
    assert lib.qmpc_episode_view_get(h, C.byref(view)) == OK and view.batch == 16 and view.seed == 3
    for k in Bd.EPISODE_VIEW_FIELDS:
        assert v1[k].data_ptr() == v2[k].data_ptr() == getattr(view, k), k
    assert v1["log_count"].data_ptr() == view.log_count and v1["log_dropped"].data_ptr() == view.log_dropped
    torch.cuda.synchronize()
    assert (v1["age"] == 3).all() and v1["count"].shape == (16, 6) and v1["ticks_sum"].dtype == torch.int64
    assert lib.qmpc_episode_step(h, 16, 2, None) == OK           # age 5: everybody times out
    torch.cuda.synchronize()
    assert (v1["age"] == 0).all() and (v1["episode"] == 1).all() and (v1["mask"] == 1).all()     # the same tensors
    assert int(v1["log_count"][0]) == 4 and int(v1["log_dropped"][0]) == 12
    assert _np(log)[:, 0].tolist() == [0, 1, 2, 3] and (_np(log)[:, 2] == Bd.EP_TIMEOUT).all() and (_np(log)[:, 3] == 5).all()
    e.clear_log()
    torch.cuda.synchronize()
    assert int(v1["log_count"][0]) == 0 and int(v1["log_dropped"][0]) == 0
    # qmpc_plant_init with the same batch keeps the episodes
    p.init()
    assert lib.qmpc_episode_step(h, 16, 1, None) == OK
    torch.cuda.synchronize()
    assert (e.view()["episode"] == 1).all() and (e.view()["age"] == 1).all()
    # ... another batch needs qmpc_episode_init again
    c.init(8, L.FREQ, L.PID)
    p.init()
    assert lib.qmpc_episode_step(h, 8, 1, None) == ARG and lib.qmpc_episode_step(h, 16, 1, None) == ARG
    e.init(4)
    assert lib.qmpc_episode_step(h, 8, 1, None) == STATE          # init forgets the rule
    assert (e.view()["age"] == 0).all() and e.view()["age"].shape == (8,)
    c.close()


# ---- 6. a handle of one robot, and a hostile gait column ---------------------------------------------------------------

def test_one_robot_handle_and_hostile_gait_column():
    """max_batch = 1 (the smallest legal handle: the init kernel has no lane 1 below max_batch): both log words are 0
    after init(), also after an init() that follows an overflow; a one-row log holds the first episode and drops the
    second.  The commands table's gait column holds NaN, 1e300 and -7: the robot's gait number is the clamped one, the
    model's, on every reset."""
    from quadruped_ctrl_amd import binding as Bd
    import torch
    c = Bd.BatchedController(0, max_batch=1)
    c.init(1, L.FREQ, L.PID)
    p = Bd.BatchedPlant(c)
    p.init()
    e = Bd.BatchedEpisodes(p)
    table = np.array([[0.1, 0.0, 0.0, np.nan], [0.2, 0.0, 0.0, 1e300], [0.3, 0.0, 0.0, -7.0], [0.4, 0.0, 0.0, 10.9]])
    for seed in (11, 12):
        e.init(seed)
        torch.cuda.synchronize()
        v = e.view()
        assert int(v["log_count"][0]) == 0 and int(v["log_dropped"][0]) == 0, seed
        lg = e.log()
        assert len(lg["rows"]) == 0 and lg["dropped"] == 0
        vel = torch.zeros((1, 3), dtype=torch.float64, device=c.device)
        gait = torch.full((1,), 5, dtype=torch.int32, device=c.device)
        e.set(vel, gait, _dev(c, np.array([[0.5, -0.5, 0.1]])), _dev(c, table), log_rows=1, causes=EM.TIMEOUT, max_ticks=1)
        seen = set()
        for k in range(1, 13):
            e.step()
            torch.cuda.synchronize()
            _, cr = EM.draw(seed, np.array([0]), np.array([k]), 1, len(table))
            assert int(gait[0]) == int(EM.gait_of(table[cr, 3])[0]) and 0 <= int(gait[0]) <= 31, (k, cr)
            assert _bits(_np(vel)[0], table[cr[0], :3])
            seen.add(int(cr[0]))
            assert int(v["log_count"][0]) == 1 and int(v["log_dropped"][0]) == k - 1, k
        assert seen == {0, 1, 2, 3}
        lg = e.log()
        assert lg["dropped"] == 11 and lg["rows"][:, :4].tolist() == [[0.0, 0.0, float(EM.TIMEOUT), 1.0]]
        assert _np(c.view()["safe"]).tolist() == [[1]] and np.array_equal(_np(p.view()["p"])[0, :2], [0.5, -0.5])
    c.close()
