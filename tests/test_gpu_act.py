"""GPU suite (-m gpu) for the actuator stage (include/qmpc_act.h; BatchedActuators, the rollouts' `actuators`).

The kernel is compared with tests/act_model.py BIT FOR BIT: the path holds one fp64 operation at a time -- no
transcendental function, no contraction -- and the accumulators' sums run in the order the header fixes.  (A NaN is
compared as a NaN: the device and numpy may sign a fresh one differently.)  The closed-loop fleets are held to the CPU
loop's recorded walking rungs (tests/golden/act_closed_loop_cpu.json) by plant_loop.envelope(); everything else compares
two runs of the library bit for bit.  The shared helpers and the walk are tests/fleet_gpu.py's, the episode fleets
tests/episode_gpu.py's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import act_cases as AC
import act_loop as AL
import act_model as AM
import episode_gpu as EG
import fleet_gpu as G
import plant_loop as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "act_closed_loop_cpu.json")))
DT = 1.0 / L.FREQ
_pair, _dev, _snap = G.pair, G.dev, G.snap
STATE_KEYS = ("ring", "head", "age") + AM.ACCUMULATORS


def _fleet(B, schedule="lockstep", mode=None, max_batch=None):
    """Controller + plant + actuators (not initialised) on plant_loop's commands, repeated over B robots."""
    from quadruped_ctrl_amd.binding import BatchedActuators
    gait, vel, xyyaw = L.commands(mode or 0)
    k = np.arange(B) % L.N_CMD
    c, plant = _pair(B, schedule, mode, xyyaw=xyyaw[k], max_batch=max_batch)
    c.set_gait(_dev(c, gait[k]))
    c.set_vel(_dev(c, vel[k]))
    return c, plant, BatchedActuators(plant)


def _state(a):
    """The actuators' whole device state as numpy copies (synchronises)."""
    import torch
    torch.cuda.synchronize()
    v = a.view()
    return {k: v[k].cpu().numpy().copy() for k in STATE_KEYS}


def _same(got, want):
    """Equal bits; a NaN equals a NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind != "f":
        return got.shape == want.shape and np.array_equal(got, want)
    g, w = got.astype(np.float64), np.asarray(want, np.float64)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64))


def _check_state(a, m, what):
    s = _state(a)
    want = dict(ring=m.ring, head=m.head, age=m.age, **m.acc)
    for k in STATE_KEYS:
        assert s[k].dtype == want[k].dtype and _same(s[k], want[k]), (what, k)
    return s


def _bind(c, a, m, prm, names):
    """Bind the arrays named (and the model's) -> the device tensors, for the caller to keep."""
    t = {k: _dev(c, prm[k]) for k in names}
    a.set_params(**t)
    m.set_params(**{k: prm[k] for k in names})
    return t


def _run_table(B, D, in_place, hostile=True, calls=70, friction=1, check=True):
    """70 consecutive periods of the case table on a handle of B robots with a ring of D + 1 rows: the binding changes
    every 8 periods through act_cases.BINDINGS (nothing, each array alone, all), a masked reset without and one with
    the accumulators, the rates written into the plant's motor rows.  Every period's output and state against the
    model.  -> (outputs [calls, B, 12], the final state)."""
    import torch
    c, plant, a = _fleet(B)
    a.init(max_delay=D, friction=friction)
    m = AM.ActModel(B, DT, dict(max_delay=D, friction=friction))
    assert a.view()["dt"] == DT and a.config["max_delay"] == D
    prm = AC.params(B)
    motor = plant.view()["motor"]
    eff_t = torch.zeros((B, 12), dtype=torch.float64, device=c.device)
    out_t = eff_t if in_place else torch.full((B, 12), 7.0, dtype=torch.float64, device=c.device)
    keep, outs = None, []
    for call in range(calls):
        if call % 8 == 0:
            keep = _bind(c, a, m, prm, AC.BINDINGS[min(call // 8, len(AC.BINDINGS) - 1)])
        if call in (30, 50):
            ma, mb = np.arange(B) % 3 == 0, np.arange(B) % 5 == 1
            a.reset(_dev(c, ma), _dev(c, mb) if call == 50 else None, stats=call == 50)
            m.reset(ma, mb if call == 50 else None, stats=call == 50)
        eff, qd = AC.period(call, B, hostile=hostile)
        motor[:, 12:].copy_(_dev(c, qd))
        eff_t.copy_(_dev(c, eff))
        res = a.apply(eff_t, None if in_place else out_t)
        assert res is out_t
        want = m.apply(eff, qd)
        if check:
            got = out_t.cpu().numpy()
            assert _same(got, want), (call, np.flatnonzero(~(np.isnan(want) | (got == want)).all(1)))
            if not in_place:
                assert _same(eff_t.cpu().numpy(), eff), call              # the input is left alone
            _check_state(a, m, call)
        outs.append(out_t.cpu().numpy().copy())
    final = _check_state(a, m, "end") if check else _state(a)
    del keep
    c.close()
    return np.stack(outs), final, m


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("D", [0, 5, 64])
def test_kernel_is_the_model_bit_for_bit(D, in_place):
    """37 robots (a partial last wave, a robot group that ends mid-wave), max_delay 0, 5 and 64, in place and out of
    place: torques, ring, head, age and every accumulator after every one of 70 periods."""
    outs, final, m = _run_table(AC.B, D, in_place)
    good = np.arange(AC.B) != AC.NAN_ROBOT
    assert (final["n"] == np.where((np.arange(AC.B) % 3 == 0) | (np.arange(AC.B) % 5 == 1), 20, 70)).all()
    # (rows 9.. hold random commands and rates; rows 7 and 8 command nothing)
    assert (final["n_vsat"][9:] > 0).all() and (final["n_tsat"][9:] > 0).all() and (final["e_heat"][9:] > 0).all()
    assert (final["n_tsat"][7:9] == 0).all() and (final["e_heat"][7:9] == 0).all()
    assert np.isfinite(outs[:, good]).all() and np.isnan(outs[:, AC.NAN_ROBOT]).any()
    assert (final["age"] == min(D, 20)).any() and (final["age"] == D).any() and (final["head"] == 70 % (D + 1)).all()
    if D:
        # the latency is felt: with every array bound (periods 56..) robots with a delay receive an older command
        assert (m.last_row != (m.head - 1) % (D + 1)).any()


def test_a_nan_robot_changes_no_bit_of_its_neighbours():
    """The table with NaN and inf in robot 5's commands and rates against the table with finite values there (ring of 6
    rows, friction off as well as on): every other robot's outputs, ring rows and accumulators are the same bits."""
    good = np.arange(AC.B) != AC.NAN_ROBOT
    for friction in (1, 0):
        a_out, a_fin, _ = _run_table(AC.B, 5, True, hostile=True, calls=24, friction=friction, check=False)
        b_out, b_fin, _ = _run_table(AC.B, 5, True, hostile=False, calls=24, friction=friction, check=False)
        assert np.array_equal(a_out[:, good].view(np.uint64), b_out[:, good].view(np.uint64))
        for k in STATE_KEYS:
            x, y = (a_fin[k][:, good], b_fin[k][:, good]) if k == "ring" else (a_fin[k][good], b_fin[k][good])
            assert x.tobytes() == y.tobytes(), k
        assert np.isnan(a_out[:, AC.NAN_ROBOT]).any() and np.isfinite(b_out).all()


def test_one_robot_handle():
    outs, final, m = _run_table(1, 5, True, calls=20)
    assert final["n"].tolist() == [20] and final["ring"].shape == (6, 1, 12) and np.isfinite(outs).all()


def test_identity_motor_and_rollout_without_actuators():
    """friction 0, V and tau_max huge, delay 0: the output is the model's value -- the command through the divide and
    multiply chain, close to it and not equal --, nothing saturates.  And rollout(actuators=None) enqueues what the loop
    tick_state -> step enqueues: the same bits."""
    import torch
    from quadruped_ctrl_amd.binding import rollout
    B = 37
    c, plant, a = _fleet(B)
    a.init(friction=0, battery_v=1e300, tau_max=1e300)
    m = AM.ActModel(B, DT, dict(friction=0, battery_v=1e300, tau_max=1e300))
    rng = np.random.default_rng(2)
    eff, qd = rng.uniform(-30, 30, (B, 12)), rng.uniform(-30, 30, (B, 12))
    plant.view()["motor"][:, 12:].copy_(_dev(c, qd))
    out = a.apply(_dev(c, eff), torch.zeros((B, 12), dtype=torch.float64, device=c.device)).cpu().numpy()
    want = m.apply(eff, qd)
    assert _same(out, want) and not np.array_equal(out, eff)
    g = np.tile(np.asarray(m.cfg["gear"]), 4)[None, :]
    scale = np.maximum(np.abs(eff), np.abs(qd * g * 0.05 * 2.0) * (0.05 * 1.5) / 0.173 * g)
    assert (np.abs(out - eff) <= 16 * np.spacing(scale)).all()
    s = _check_state(a, m, "identity")
    assert (s["n_vsat"] == 0).all() and (s["n_tsat"] == 0).all() and (s["n"] == 1).all()
    c.close()
    runs = []
    for by_hand in (False, True):
        c, plant, a = _fleet(B)
        if by_hand:
            for _ in range(27):
                c.tick_state(plant.state, plant.motor, plant.effort)
                plant.step(plant.effort)
        else:
            rollout(c, plant, 27, actuators=None)
        snap = _snap(plant)
        snap["effort"] = plant.effort.cpu().numpy().copy()
        runs.append(snap)
        c.close()
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert np.abs(runs[0]["effort"]).max() > 1.0


def test_reset_under_either_mask_touches_only_its_robots():
    """After 9 periods on a ring of 6 rows: mask_a alone, mask_b alone, both, and both NULL; stats = 0 keeps the
    accumulators, stats = 1 zeroes them; a robot outside the masks keeps every bit."""
    B, D = 37, 5
    ma, mb = np.arange(B) % 4 == 1, np.arange(B) % 6 == 2
    for pa, pb, stats in ((ma, None, 0), (None, mb, 1), (ma, mb, 1), (ma, mb, 0), (None, None, 0), (None, None, 1)):
        c, plant, a = _fleet(B)
        a.init(max_delay=D)
        m = AM.ActModel(B, DT, dict(max_delay=D))
        prm = AC.params(B)
        keep = _bind(c, a, m, prm, AM.PARAMS)
        for call in range(9):
            eff, qd = AC.period(call, B, hostile=False)
            plant.view()["motor"][:, 12:].copy_(_dev(c, qd))
            a.apply(_dev(c, eff))
            m.apply(eff, qd)
        before = _check_state(a, m, "before")
        a.reset(None if pa is None else _dev(c, pa), None if pb is None else _dev(c, pb), stats=bool(stats))
        m.reset(pa, pb, stats=bool(stats))
        after = _check_state(a, m, "after")
        hit = np.ones(B, bool) if pa is None and pb is None else (np.zeros(B, bool) if pa is None else pa) | (np.zeros(B, bool) if pb is None else pb)
        assert (after["age"][hit] == 0).all() and (before["age"][hit] == D).all()
        for k in STATE_KEYS:
            keepers = ~hit if k in ("age",) + (AM.ACCUMULATORS if stats else ()) else np.ones(B, bool)
            x, y = (before[k][:, keepers], after[k][:, keepers]) if k == "ring" else (before[k][keepers], after[k][keepers])
            assert x.tobytes() == y.tobytes(), (k, stats)
        if stats:
            assert all((after[k][hit] == 0).all() for k in AM.ACCUMULATORS) and (before["e_heat"][9:][hit[9:]] > 0).all()
        # the robot reset receives its newest command at once, its neighbour the delayed one
        eff, qd = AC.period(9, B, hostile=False)
        plant.view()["motor"][:, 12:].copy_(_dev(c, qd))
        a.apply(_dev(c, eff))
        m.apply(eff, qd)
        _check_state(a, m, "next")
        assert (m.last_row[hit] == (m.head[hit] - 1) % (D + 1)).all() and (m.last_row[~hit] != (m.head[~hit] - 1) % (D + 1)).any() == (~hit).any()
        del keep
        c.close()


def test_graph_replays_continue_the_ring():
    """Lockstep, 64 robots, a ring of 9 rows with per-robot latencies, 13 eager ticks, then a captured block of 13 ticks
    of rollout(actuators=...) replayed 5 times against 65 eager ticks: plant, effort, ring, counters and accumulators,
    bit for bit.  The latencies are rewritten in place after the second replay (after 26 of the 65 eager ticks): the
    next replay reads them, and a run without the rewrite ends elsewhere."""
    import torch
    from quadruped_ctrl_amd.binding import rollout
    B, D = 64, 8
    d0, d1 = (np.arange(B) % 7).astype(np.int32), ((np.arange(B) * 3 + 1) % 9).astype(np.int32)
    out = {}
    for how in ("eager", "graph", "no_rewrite"):
        c, plant, a = _fleet(B)
        a.init(max_delay=D)
        delay = _dev(c, d0)
        a.set_params(delay=delay)
        rollout(c, plant, 13, actuators=a)
        if how == "graph":
            res = rollout(c, plant, 13, graph=True, actuators=a)
            res["graph"].replay()
            delay.copy_(_dev(c, d1))
            for _ in range(3):
                res["graph"].replay()
        else:
            rollout(c, plant, 26, actuators=a)
            if how == "eager":
                delay.copy_(_dev(c, d1))
            rollout(c, plant, 39, actuators=a)
        snap = _snap(plant)
        snap["effort"] = plant.effort.cpu().numpy().copy()
        snap.update(_state(a))
        out[how] = snap
        c.close()
    for k in out["eager"]:
        assert out["eager"][k].tobytes() == out["graph"][k].tobytes(), k
    assert (out["graph"]["n"] == 78).all() and (out["graph"]["head"] == 78 % (D + 1)).all() and (out["graph"]["age"] == D).all()
    assert np.abs(out["graph"]["effort"]).max() > 1.0 and (out["graph"]["e_heat"] > 0).all()
    assert not np.array_equal(out["graph"]["state"], out["no_rewrite"]["state"])


# ---- the fleet on the recorded walking rungs ------------------------------------------------------------------------------

def _walking():
    cases = []
    for mode in (0, 1):
        for name, rungs in AL.LADDERS.items():
            for rname, actuator in rungs:
                if GOLD[f"mode{mode}"]["ladders"][name][rname]["walks"]:
                    cases.append(pytest.param(mode, name, rname, False, id=f"mode{mode}-{rname}"))
    cases.append(pytest.param(0, "delay", "delay_8", True, id="mode0-delay_8-sensed"))
    return cases


@pytest.mark.parametrize("mode,ladder,rung,sensed", _walking())
def test_the_fleet_walks_on_the_recorded_rung(mode, ladder, rung, sensed):
    """The CPU yardstick's commands, six robots per command (96), the rung's actuator -- its torque cap or battery
    voltage bound as a per-robot array, its latency as per-robot delays on a ring of exactly that length --, 650 ticks of
    tick_state -> apply -> step (sensed: settle(50), then tick -> apply -> step -> sense).  No robot is latched, no solve
    reports an error bit, and the five statistics -- from the plant's device accumulators at tick 150 and at the end --
    lie inside plant_loop.envelope() of the rung's recorded row.  The accumulators counted every period."""
    from quadruped_ctrl_amd.binding import BatchedSensors, rollout, rollout_sensed
    reps = 6
    B = L.N_CMD * reps
    rec = GOLD[f"mode{mode}"]["ladders"][ladder][rung]
    actuator = dict(dict(AL.LADDERS[ladder])[rung])
    assert rec["walks"] and rec["actuator"] == actuator
    c, plant, a = _fleet(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None)
    delay = int(actuator.pop("delay", 0))
    a.init(max_delay=delay)
    keep = {k: _dev(c, np.full(B, float(v))) for k, v in actuator.items()}
    if delay:
        keep["delay"] = _dev(c, np.full(B, delay, np.int32))
    a.set_params(**keep)
    plant.enable_stats()

    def sensors():
        nonlocal s
        s = BatchedSensors(plant)
        s.init(1)
        s.settle(50)

    s = None
    tick = (lambda t: rollout_sensed(c, plant, s, 1, actuators=a)) if sensed else (lambda t: rollout(c, plant, 1, actuators=a))
    start, at150, end = G.walk(c, plant, tick, L.TICKS, lambda t: (t + 1) % 13 == 0, settle=sensors if sensed else None)
    G.assert_inside_envelope(G.stats_from_accumulators(start, at150, end), rec, reps, f"mode {mode} {rung}")
    st = _state(a)
    print(f"mode {mode} {rung}: n_vsat {int(st['n_vsat'].sum()) // reps} (CPU {sum(rec['counters']['n_vsat'])}), "
          f"n_tsat {int(st['n_tsat'].sum()) // reps} (CPU {sum(rec['counters']['n_tsat'])}), "
          f"e_heat {st['e_heat'].mean():.3f} J (CPU {np.mean(rec['counters']['e_heat']):.3f})")
    assert (st["n"] == L.TICKS).all() and (st["e_heat"] > 0).all() and (st["e_pos"] >= st["e_mech"]).all()
    del keep
    c.close()


# ---- episodes -------------------------------------------------------------------------------------------------------------

def test_managed_fleet_with_actuators_equals_host_driven_resets():
    """tests/test_gpu_episode.py's fleets (96 robots, per-robot schedule, flat ground, the full rule, the pushes after the
    common time-out) with the actuators in the loop, per-robot latencies on a ring of 7 rows.  Fleet A:
    rollout_episodes(actuators=..., actuator_stats=True).  Fleet B: rollout(actuators=...) one tick at a time, the host
    decides with the episode model and resets through the same calls with its own mask.  90 ticks, compared every tenth:
    plant, controller, effort, statistics, and the actuators' ring, counters and accumulators -- every bit."""
    from quadruped_ctrl_amd.binding import BatchedActuators, rollout, rollout_episodes
    B, D = EG.B, 6
    fa, fb = EG.Fleet("per_robot", "flat"), EG.Fleet("per_robot", "flat")
    acts = []
    for f in (fa, fb):
        a = BatchedActuators(f.p)
        a.init(max_delay=D)
        f.delay = _dev(f.c, (np.arange(B) % (D + 2)).astype(np.int32))
        a.set_params(delay=f.delay)
        acts.append(a)
    aa, ab = acts
    ea = EG.episodes(fa, EG.RULE_ALL, 200)
    m = EG.model(fb, EG.RULE_ALL, 200)
    masks = []
    for chunk in range(9):
        if chunk == 4:
            fa.push()
            fb.push()
        rollout_episodes(fa.c, fa.p, ea, 10, actuators=aa, actuator_stats=True)
        for _ in range(10):
            rollout(fb.c, fb.p, 1, actuators=ab)
            mask = EG.host_check(fb, m)
            ab.reset(_dev(fb.c, mask), stats=True)
            masks.append(mask)
        EG.same(fa, fb, f"tick {10 * (chunk + 1)}", m.vel, m.gait)
        sa, sb = _state(aa), _state(ab)
        for k in STATE_KEYS:
            assert sa[k].tobytes() == sb[k].tobytes(), (chunk, k)
    masks = np.array(masks)
    # robots finished, at different times, and a robot that finished started with an empty ring and fresh accumulators
    assert masks[39].all() and not masks[:39].any() and (masks[40:].any(1) & ~masks[40:].all(1)).any()
    last = np.array([np.flatnonzero(masks[:, b])[-1] for b in range(B)])
    since = len(masks) - 1 - last
    assert np.array_equal(sa["age"], np.minimum(since, D)) and np.array_equal(sa["n"], since)
    assert len(np.unique(since)) > 3
    fa.close()
    fb.close()


def test_sensor_path_episodes_reset_the_ring_under_mask_and_hold():
    """tests/test_gpu_episode_sense.py's managed fleet (96 robots, sensors, warm-up of 5 periods, the pushes from tick 10)
    with the actuators in rollout_sensed_episodes, one tick at a time: after every tick the stage's age and call count are
    what the manager's mask and hold flags of that tick say -- a robot reset or held has age 0 and n 0, every other robot
    one more, saturated at the ring's length -- so a robot leaves its warm-up with an empty ring."""
    from quadruped_ctrl_amd.binding import BatchedActuators, rollout_sensed_episodes
    B, D = EG.B, 6
    f = EG.Managed("per_robot", "flat", EG.W3, EG.RULE_ALL, 4000)
    a = BatchedActuators(f.p)
    a.init(max_delay=D)
    delay = _dev(f.c, (np.arange(B) % (D + 2)).astype(np.int32))
    a.set_params(delay=delay)
    f.s.sense()
    f.se.hold()
    age, n = np.zeros(B, np.int32), np.zeros(B, np.int32)
    cleared, left = [], 0
    prev = np.zeros(B, bool)
    for t in range(70):
        if t == 10:
            f.f.push()
        rollout_sensed_episodes(f.c, f.p, f.s, f.se, 1, actuators=a, actuator_stats=True)
        f.torch.cuda.synchronize()
        m = (f.e.view()["mask"].cpu().numpy() != 0) | (f.se.view()["hold"].cpu().numpy() != 0)
        age, n = np.minimum(age + 1, D), n + 1
        age[m], n[m] = 0, 0
        st = _state(a)
        assert np.array_equal(st["age"], age) and np.array_equal(st["n"], n), t
        assert (st["e_heat"][m] == 0).all() and (st["tau_peak"][m] == 0).all(), t
        left += int((prev & ~m).sum())
        prev = m
        cleared.append(int(m.sum()))
    print("robots reset or held per tick", cleared, "robots that left a warm-up", left)
    assert cleared[0] == B and 0 in cleared and any(0 < x < B for x in cleared) and left > B
    assert (age == D).any() and (age < D).any()
    f.c.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import ActConfig, ActParams, ActView, BatchedController, PlantView
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    eff = torch.ones((B, 12), dtype=torch.float64, device=c.device)
    out = torch.zeros((B, 12), dtype=torch.float64, device=c.device)
    tm = torch.full((B,), 1.0, dtype=torch.float64, device=c.device)
    prm, v, cfg = ActParams(tau_max=tm.data_ptr()), ActView(), ActConfig()
    assert lib.qmpc_act_config_default(None) == ARG and lib.qmpc_act_config_default(C.byref(cfg)) == OK
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_act_init(h, B, None, None) == STATE                         # before qmpc_plant_init
    assert lib.qmpc_act(h, B, eff.data_ptr(), out.data_ptr(), None) == STATE
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_act(h, B, eff.data_ptr(), out.data_ptr(), None) == STATE     # before qmpc_act_init
    assert lib.qmpc_act_set_params(h, B, C.byref(prm)) == STATE
    assert lib.qmpc_act_reset(h, B, None, None, 0, None) == STATE
    assert lib.qmpc_act_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_act_init(None, B, None, None) == ARG
    assert lib.qmpc_act_init(h, B + 1, None, None) == ARG                       # a batch other than the plant's

    def bad(**kw):
        k = ActConfig()
        lib.qmpc_act_config_default(C.byref(k))
        for name, val in kw.items():
            if name.startswith("gear"):
                k.gear[int(name[4])] = val
            else:
                setattr(k, name, val)
        return lib.qmpc_act_init(h, B, C.byref(k), None)

    assert bad(max_delay=-1) == ARG and bad(max_delay=65) == ARG
    assert bad(kt=0.0) == ARG and bad(kt=-0.05) == ARG and bad(kt=float("nan")) == ARG
    assert bad(R=0.0) == ARG and bad(R=-1.0) == ARG
    assert bad(gear0=0.0) == ARG and bad(gear1=-6.0) == ARG and bad(gear2=float("nan")) == ARG
    assert lib.qmpc_act_view_get(h, C.byref(v)) == STATE                         # a refused init initialises nothing
    assert bad(max_delay=64) == OK and bad(max_delay=0) == OK
    assert lib.qmpc_act_init(h, B, None, None) == OK                             # NULL: the default
    assert lib.qmpc_act_view_get(h, None) == ARG and lib.qmpc_act_view_get(None, C.byref(v)) == ARG
    assert lib.qmpc_act_view_get(h, C.byref(v)) == OK
    assert (v.batch, v.dt, v.config.max_delay, v.config.tau_max, tuple(v.config.gear)) == (B, 1.0 / 500.0, 0, 3.0, (6.0, 6.0, 9.33))
    assert lib.qmpc_act_set_params(h, B - 1, C.byref(prm)) == ARG
    assert lib.qmpc_act_set_params(h, B, C.byref(prm)) == OK
    assert lib.qmpc_act_set_params(h, B, None) == OK                              # unbinds
    assert lib.qmpc_act_reset(h, B + 1, None, None, 0, None) == ARG
    assert lib.qmpc_act_reset(h, B, None, None, 1, None) == OK
    assert lib.qmpc_act(h, B + 1, eff.data_ptr(), out.data_ptr(), None) == ARG
    assert lib.qmpc_act(h, B, None, out.data_ptr(), None) == ARG
    assert lib.qmpc_act(h, B, eff.data_ptr(), None, None) == ARG
    pv = PlantView()
    assert lib.qmpc_plant_view_get(h, C.byref(pv)) == OK
    assert lib.qmpc_act(h, B, eff.data_ptr(), pv.motor, None) == ARG              # the plant's motor rows as the output
    assert lib.qmpc_act(h, B, eff.data_ptr(), pv.motor + 8 * 13, None) == ARG     # ... or a part of them
    assert lib.qmpc_act(h, B, pv.motor, out.data_ptr(), None) == OK               # as the input they are only read
    assert lib.qmpc_act(h, B, eff.data_ptr(), out.data_ptr(), None) == OK
    assert lib.qmpc_act(h, B, eff.data_ptr(), eff.data_ptr(), None) == OK         # in place
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, eff) and float(out.abs().max()) > 0.5
    # a later qmpc_plant_init with the same batch keeps the actuators; another batch wants a new qmpc_act_init
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == OK
    assert lib.qmpc_act(h, B, eff.data_ptr(), out.data_ptr(), None) == OK
    c.init(B - 2, 500.0, L.PID)
    assert lib.qmpc_plant_init(h, B - 2, 0.4, 1, None, None) == OK
    assert lib.qmpc_act(h, B - 2, eff.data_ptr(), out.data_ptr(), None) == ARG
    assert lib.qmpc_act_init(h, B - 2, None, None) == OK
    assert lib.qmpc_act(h, B - 2, eff.data_ptr(), out.data_ptr(), None) == OK
    torch.cuda.synchronize()
    c.close()
