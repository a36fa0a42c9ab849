"""Robot-ticks/s of the batched locomotion controller (include/qmpc_ctrl.h) on one GPU.

For each batch size: mixed reference gaits (every gait number 0 .. 11 and its omni variant), the calm synthetic
stream of workloads.make_tick_stream, warm-up ticks, then HIP-event timing of every tick (one tick per event pair):
the median and the MAXIMUM over the timed window, the window's robot-ticks/s, and -- in lockstep, where the ticks of the
whole batch are of two kinds -- the medians of the non-MPC and of the MPC ticks separately.  Prints one JSON line per
batch size and, with --out, writes them as a JSON list.  The kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/ctrl_bench.py --batches 4096 --cycles 4`.

--schedule per_robot selects the per-robot MPC schedule (qmpc_ctrl_set_schedule); without --stagger every robot is in
phase (all solve on the same ticks, as in lockstep).  --stagger resets group b % 13 before tick b % 13 of thirteen
untimed ticks in front of the warm-up, so that one thirteenth of the fleet solves on every tick.

--robot-mode 1 selects the speed-adaptive `aio` gait (qmpc_ctrl_set_robot_mode; implies --schedule per_robot): per-robot
x velocity commands spread evenly over [0, 2] m/s, so that standing, walking, walk-to-trot, trot and the fast trot all
occur; the robots' counters restart on their own there, which spreads the solves over the ticks without --stagger.  The
warm-up should then cover the settling of the velocity filter (--warmup 600).  Reports the histogram of the robots'
segment counts at the end.

--source state drives the ticks with simulator ground truth (qmpc_ctrl_tick_state on workloads.make_state_stream: the
cheater estimators, no Kalman filter) instead of the sensor path (--source imu, the default); nothing else changes.

--source plant closes the loop on the device: qmpc_ctrl_tick_state on the read-out of the reduced-order plant
(include/qmpc_plant.h), qmpc_plant_step on the tick's efforts -- states a walking robot visits.  Gaits from {0, 4, 5, 10},
x commands over [0, 0.5] m/s and small yaw rates (the family tests/plant_loop.py walks on); the warm-up should cover the
first steps (--warmup 260).  The tick and the plant step are timed separately (us_per_plant_step_median).  --vary binds
the per-robot body, floor and push of include/qmpc_plant_vary.h (the set the closed-loop tests walk on: payloads, floors, and a
30 N lateral push during ticks 300 .. 349 of the run, written into the bound array between two ticks) and turns the plant's statistics on: the step then runs its <VARY, STATS> instantiation.
--terrain binds the per-robot ground of include/qmpc_terrain.h (the set the closed-loop tests walk on, by robot index mod 4:
four treads of 0.1 m x 0.04 m up, a cross slope of 0.15, the same treads down, 0.15 uphill; flights start 0.10 m ahead of
each robot along its start yaw), with swing feet clamped to the surface and, for --source plant, the state row's height
re-based on the stance feet; the robots are reset onto their ground first.  The step then runs the terrain kernels of
csrc/qmpc_terrain.hip (with --vary: their <VARY, STATS> instantiation).
--contact lets the ground decide contact (include/qmpc_contact.h: early and late touch-down and slip, the binding's default
parameters), on flat ground or with --terrain on its ground: the step then runs the kernels of csrc/qmpc_contact.hip; the
counters are reported.
--field binds height-field terrain from memory (include/qmpc_field.h): one 256 x 256 map of workloads.random_blocks on
0.05 m cells at amplitude 0.02 m (the reference simulation's `random1` recipe; the amplitude both closed-loop ladders walk),
shared by the fleet, the robots' start positions spread over 13 x 13 patches of it; swing feet clamped to the surface and,
for --source plant, the height re-based, as with --terrain.  It combines with --terrain (the field lies on the slopes and
stairs), --contact and --vary: the step then runs the kernels of csrc/qmpc_field.hip.
--episodes (with --source plant) puts the episode manager of include/qmpc_episode.h behind the plant step: all six causes
(time-out after 300 ticks, tilt cosine below 0.8, height below 0.15 m, 2 m from the start), the fleet's start poses as the
shared spawn table, a table of eight commands of the same family, a log of 4096 rows; --every k checks on every k-th tick
only (qmpc_episode_step(elapsed = k)).  The step is timed separately on the ticks it runs on (us_per_episode_step_median);
the episodes finished per cause and the log's words are reported.

--source sensor closes the same loop through the SENSOR path: qmpc_ctrl_tick -- the VectorNav orientation estimator and
the Kalman filter -- on the readings of the sensor model (include/qmpc_sense.h), qmpc_plant_step on the tick's efforts,
qmpc_sense on the plant's read-out; 50 untimed qmpc_sense -> qmpc_ctrl_prework calls on the standing plant come first
(without them the filter, which starts at height 0, makes most of the fleet fall).  The same commands as --source plant.
The tick, the plant step and the sensor launch are timed separately (us_per_sense_median).  --noise binds per-robot
accelerometer and gyro biases (within +-0.2 m/s^2, +-0.02 rad/s) and white noise (sigma 0.3 m/s^2, 0.02 rad/s, encoders
0.002 rad and 0.05 rad/s: the levels the closed-loop tests walk on); without it the sensors are ideal.
us_per_period_median is the whole period, tick to reading.
--episodes with --source sensor puts the manager of include/qmpc_episode_sense.h between the plant step and the reading
(qmpc_episode_sense_step on every tick; --every stays 1): a robot that finishes is reset and warmed up for --warm W periods
(50) while the others walk.  The timed window runs twice: as it comes (robots_held_per_step says how quiet it was), and again
after qmpc_episode_sense_hold has put every 100th robot into a warm-up longer than the run, so that 1 % of the fleet is
held on every step (the held_* fields).  launches_per_episode_step counts what one step enqueues in this configuration.

--actuators puts the actuator stage of include/qmpc_act.h (the Mini Cheetah's motor, friction on) between the tick and the
plant step of every --source -- with --source imu / state, which have no plant in the loop, a plant standing beside the
stream supplies the joint rates the launch reads --; --delay D gives the ring D + 1 rows and robot b a latency of b mod
(D + 1) ticks.  The timed window then runs 2 x --repeats times in ONE session, alternating without and with the launch
(off, on, off, on, ...): us_per_period_without_act / _with_act are the medians over the windows' median periods (tick to the
period's last launch), us_added_per_period their difference, us_per_act_median the event pair around the launch itself.
Without --actuators the stage is never initialised and the loop enqueues what it enqueued before.

--fused (with --source plant) runs the loop through qmpc_fleet_run (include/qmpc_fleet.h: everything between two MPC
solves in one launch); --graph adds a captured 13-tick block, replayed.  Either one switches to timing in blocks of ticks
(run_blocks: the per-tick windows cut at the same places; --warmup a multiple of 13), so `--source plant --graph` is the
per-tick path's figure to hold `--source plant --fused --graph` against.
With --actuators [--delay D] and / or --episodes [--every K], --fused routes the loop through qmpc_loop_run
(include/qmpc_loop.h: the actuator stage and the episode step inside the same launch) and --graph alone through
rollout_episodes() / rollout() with the actuators, in the same block windows; with --every K > 1 only the whole 13-tick
blocks are timed (K must divide 13: a block ends on a check tick).
--ground-run (with --fused, and --terrain and / or --field) turns the handle's switch of include/qmpc_ground_run.h on: both
run calls then serve the bound ground through the fused launch instead of falling back to the per-tick launches.  The
result carries the info struct's counts (fleet_info / loop_info: fused_ticks, fallback_ticks, reason) and the flags, so a
fallback cannot pass for a fused run: without the switch `--fused --terrain` times the fallback.

    python tools/ctrl_bench.py [--batches 1024,4096,16384] [--cycles 8] [--warmup 26] [--schedule lockstep|per_robot]
                               [--stagger] [--robot-mode 0|1] [--source imu|state|plant|sensor] [--vary] [--terrain] [--contact] [--field]
                               [--noise] [--episodes] [--every K] [--warm W] [--actuators] [--delay D] [--repeats R]
                               [--fused] [--ground-run] [--graph] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_blocks(ctrl, plant, B, cycles, warmup, schedule, stagger, robot_mode, fused, graph, acts=None, manager=None, every=1,
               tags=None):
    """--source plant with --fused and / or --graph: the closed loop timed in BLOCKS of ticks (HIP events around rollout()
    calls), because a fused span has no event between its ticks.  The windows are the per-tick report's, cut at the same
    places: in lockstep, per 13-tick period, the twelve ticks without a solve in one block (us_per_nonmpc_period: block /
    12, tick + step) and the MPC tick in another (us_per_mpc_period: tick + step; the per-tick report's us_per_mpc_tick
    plus its plant step); then whole 13-tick periods in one block each (us_per_13_tick_cycle, robot_ticks_per_s); with
    --graph the same 13-tick block captured once and replayed (us_per_13_tick_cycle_graph, robot_ticks_per_s_graph).
    With the per-robot schedule every tick solves and only the whole blocks are reported.
    acts / manager (--actuators / --episodes): the longer loop -- fused through rollout_loop() (qmpc_loop_run), else
    through rollout_episodes() / rollout(actuators=...), the per-tick launches; the blocks are cut at the same places."""
    import torch
    from quadruped_ctrl_amd.binding import rollout, rollout_episodes, rollout_loop
    if warmup % 13:
        raise SystemExit("--fused / --graph: --warmup must be a multiple of 13 (the blocks are cut at the MPC ticks)")
    longer = acts is not None or manager is not None
    if not longer:
        go = lambda n, g=False: rollout(ctrl, plant, n, graph=g, fused=fused)
    elif fused:
        go = lambda n, g=False: rollout_loop(ctrl, plant, n, graph=g, actuators=acts, episodes=manager, every=every)
    elif manager is not None:
        go = lambda n, g=False: rollout_episodes(ctrl, plant, manager, n, graph=g, every=every, actuators=acts)
    else:
        go = lambda n, g=False: rollout(ctrl, plant, n, graph=g, actuators=acts)
    pair = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    med = lambda evs: float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs]))
    go(warmup)
    lockstep = schedule == "lockstep" and not stagger and robot_mode == 0
    res = {"batch": B, "source": "plant", "schedule": schedule, "stagger": bool(stagger), "robot_mode": robot_mode,
           "fused": bool(fused), "cycles_timed": cycles}
    res.update(tags or {})   # (what is bound under the plant and the ground-run switch, as the caller set them)
    if longer:
        res.update({"actuators": acts is not None, "episodes": manager is not None, "every": every})
    if lockstep and every == 1:
        non, mpc = [], []
        for _ in range(cycles):
            a, b = pair()
            a.record(); go(12); b.record()
            non.append((a, b))
            a, b = pair()
            a.record(); go(1); b.record()
            mpc.append((a, b))
        torch.cuda.synchronize()
        res.update({"us_per_nonmpc_period": round(med(non) / 12, 2), "us_per_mpc_period": round(med(mpc), 2)})
    whole = []
    for _ in range(cycles):
        a, b = pair()
        a.record(); go(13); b.record()
        whole.append((a, b))
    torch.cuda.synchronize()
    us13 = med(whole)
    res.update({"us_per_13_tick_cycle": round(us13, 1), "robot_ticks_per_s": float(f"{13 * B / (us13 * 1e-6):.4g}")})
    if graph:
        g = go(13, True)["graph"]
        torch.cuda.synchronize()
        reps = []
        for _ in range(cycles):
            a, b = pair()
            a.record(); g.replay(); b.record()
            reps.append((a, b))
        torch.cuda.synchronize()
        us13g = med(reps)
        res.update({"us_per_13_tick_cycle_graph": round(us13g, 1),
                    "robot_ticks_per_s_graph": float(f"{13 * B / (us13g * 1e-6):.4g}")})
    info, v = (ctrl.loop_info() if longer else ctrl.fleet_info()), ctrl.view()
    pz = plant.view()["p"][:, 2]
    if manager is not None:
        ev_ = manager.view()
        res.update({"episodes_finished": int(ev_["episode"].sum().item()),
                    "episodes_per_cause": [int(x) for x in ev_["count"].sum(0).tolist()]})
    if acts is not None:
        res["act_calls"] = int(acts.stats()["n"].min().item())
    res.update({"loop_info" if longer else "fleet_info": info, "body_height_min": round(float(pz.min().item()), 4),
                "body_height_max": round(float(pz.max().item()), 4),
                "status_error_robots": int((torch.from_numpy(ctrl.read("status")[:, 0]) & 47 != 0).sum()),
                "all_finite": bool(torch.isfinite(plant.effort).all().item()), "latched": int((v["safe"] == 0).sum())})
    ctrl.close()
    return res


def run(B, cycles, warmup, schedule="lockstep", stagger=False, robot_mode=0, source="imu", vary=False, noise=False, terrain=False,
        contact=False, field=False, episodes=False, every=1, warm=50, actuators=False, delay=0, repeats=3, fused=False,
        graph=False, ground_run=False):
    import torch
    from quadruped_ctrl_amd import workloads as W
    from quadruped_ctrl_amd.binding import BatchedController
    ctrl = BatchedController(0, max_batch=B)
    # (the plant takes the reference's simulation gains: a joint spring towards q = 0 pushes a real leg off its stance)
    closed = source in ("plant", "sensor")
    ctrl.init(B, freq=500.0, pid=(100.0, 1.0, 0.0, 0.05) if closed else (0.0, 0.0, 3.0, 0.3))
    if schedule != "lockstep":
        ctrl.set_schedule(schedule)
    if robot_mode:
        ctrl.set_robot_mode(robot_mode)
    g = (np.arange(B) % 12).astype(np.int32)
    g = np.where(np.arange(B) % 24 >= 12, g + 20, g).astype(np.int32)
    g = torch.from_numpy(g).cuda()
    ctrl.set_gait(g)
    rng = np.random.default_rng(B)
    vel = np.stack([rng.uniform(-0.5, 1.2, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-0.5, 0.5, B)], 1)
    if robot_mode == 1:
        vel[:, 0] = np.linspace(0.0, 2.0, B)[rng.permutation(B)]
        vel[::16, 1:] = 0.0      # (x command 0 with no yaw command: the standing case for robot 0's neighbours)
    if closed:
        g = torch.from_numpy(np.array([0, 4, 5, 10], np.int32)[np.arange(B) % 4]).cuda()
        ctrl.set_gait(g)
        vel = np.stack([rng.uniform(0.0, 0.5, B), np.zeros(B), rng.uniform(-0.1, 0.1, B)], 1)
        if robot_mode == 0:
            vel[np.arange(B) % 4 == 1] = 0.0     # (gait 4 stands)
    vel = torch.from_numpy(vel).cuda()
    ctrl.set_vel(vel)
    n = warmup + 13 * cycles
    plant = sensors = manager = sensed = None
    if closed:
        from quadruped_ctrl_amd.binding import BatchedPlant
        plant = BatchedPlant(ctrl)
        xyyaw = np.stack([np.arange(B) % 128 * 1.0, np.arange(B) // 128 * 1.0, rng.uniform(-0.1, 0.1, B)], 1)
        plant.init(0.4, 1, torch.from_numpy(xyyaw).cuda())
        if vary:   # tests/plant_loop_varied.py: variation(), restated (the tools do not import the test tree)
            k = np.arange(B) % 16
            scale = np.array([0.8, 1.0, 1.2, 1.4])[(k // 4) % 4]
            push = np.zeros((B, 3))
            push[:, 1] = np.where(k % 2 == 1, 30.0, -30.0)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
            push, force = dev(push), dev(np.zeros((B, 3)))
            plant.set_params(mass=dev(9.0 * scale), ibody=dev(np.array([0.07, 0.26, 0.242])[None, :] * scale[:, None]),
                             mu=dev(np.array([0.3, 0.4, 0.6, 0.8])[k % 4]), force=force, torque=dev(np.zeros((B, 3))))
            plant.enable_stats()
        if terrain:   # tests/plant_loop_terrain.py: terrain(), restated (the tools do not import the test tree)
            kind, psi = np.arange(B) % 4, xyyaw[:, 2]
            rows = np.zeros((B, 8))
            stairs = (kind == 0) | (kind == 2)
            rows[stairs, 3] = np.where(kind == 0, 0.04, -0.04)[stairs]
            rows[stairs, 4], rows[stairs, 5] = 0.1, 4.0
            rows[stairs, 6] = ((xyyaw[:, 0] * np.cos(psi) + xyyaw[:, 1] * np.sin(psi)) + 0.10)[stairs]
            rows[stairs, 7] = psi[stairs]
            rows[kind == 1, 2], rows[kind == 3, 1] = 0.15, 0.15
            rows = torch.from_numpy(rows).cuda()
            plant.set_terrain(rows, clamp_swing=True, rebase_z=source == "plant")
        if field:
            k = np.arange(B)
            place = np.stack([np.zeros(B), xyyaw[:, 0] - (1.5 + 0.75 * (k % 13)), xyyaw[:, 1] - (1.5 + 0.75 * (k // 13 % 13)),
                              np.ones(B)], 1)
            zmap, place = torch.from_numpy(W.random_blocks(B, amp=0.02)[None]).cuda(), torch.from_numpy(place).cuda()
            plant.set_field(zmap, place, 0.05, clamp_swing=True, rebase_z=source == "plant")
        if terrain or field:
            plant.reset(torch.ones(B, dtype=torch.bool, device="cuda"), torch.from_numpy(xyyaw).cuda())
        if contact:
            plant.set_contact(early=True, late=True, slip=True)
        if episodes:
            from quadruped_ctrl_amd.binding import BatchedEpisodes
            manager = BatchedEpisodes(plant)
            manager.init(seed=B)
            table = np.array([[0.0, 0, 0, 4], [0.1, 0, 0.05, 0], [0.2, 0, -0.05, 5], [0.3, 0, 0, 10], [0.4, 0, 0.1, 0],
                              [0.5, 0, 0, 5], [0.25, 0, -0.1, 10], [0.0, 0, 0, 4]])
            ep_vel, ep_gait = vel.clone(), g.clone()      # (the fleet's commands: the manager rewrites a reset robot's rows)
            manager.set(ep_vel, ep_gait, torch.from_numpy(xyyaw).cuda(), torch.from_numpy(table).cuda(), log_rows=4096,
                        causes=63, max_ticks=300, cos_tilt_min=0.8, z_min=0.15, range=2.0)
        imu, motor = plant.state.expand(26, B, 16), plant.motor.expand(26, B, 24)    # (every "slot" is the plant's read-out)
        tick = ctrl.tick_state
        if source == "sensor":
            from quadruped_ctrl_amd.binding import BatchedSensors
            sensors = BatchedSensors(plant)
            sensors.init(seed=B)
            if noise:   # tests/sense_loop.py: noise(), restated (the tools do not import the test tree)
                dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
                full = lambda x: dev(np.full(B, x))
                sensors.set_params(acc_bias=dev(rng.uniform(-0.2, 0.2, (B, 3))), gyro_bias=dev(rng.uniform(-0.02, 0.02, (B, 3))),
                                   acc_sigma=full(0.3), gyro_sigma=full(0.02), q_sigma=full(0.002), qd_sigma=full(0.05))
            sensors.settle(50)
            if manager is not None:
                from quadruped_ctrl_amd.binding import SensedEpisodes
                sensed = SensedEpisodes(manager, sensors)
                sensed.init(warm)
            imu, motor = sensors.imu.expand(26, B, 10), sensors.motor.expand(26, B, 24)
            tick = ctrl.tick
    elif source == "state":
        imu, motor = W.make_state_stream(B, 26, seed=B)      # (`imu` below: the tick's first input, whichever it is)
        tick = ctrl.tick_state
    else:
        imu, motor = W.make_tick_stream(B, 26, seed=B)
        tick = ctrl.tick
    if plant is None:
        imu, motor = torch.from_numpy(imu).cuda(), torch.from_numpy(motor).cuda()
    eff = torch.empty((B, 12), dtype=torch.float64, device="cuda")
    acts = None
    if actuators:
        from quadruped_ctrl_amd.binding import BatchedActuators, BatchedPlant
        rates = plant
        if rates is None:        # (no plant in the loop: one standing beside the stream, for the rates the launch reads)
            rates = BatchedPlant(ctrl)
            rates.init()
        acts = BatchedActuators(rates)
        acts.init(max_delay=delay)
        if delay:
            act_delay = (torch.arange(B, device="cuda") % (delay + 1)).to(torch.int32)
            acts.set_params(delay=act_delay)
        ep_mask = manager.view()["mask"] if manager is not None else None
    if stagger:
        group = torch.arange(B, device="cuda") % 13
        for t in range(13):
            ctrl.reset(group == t)
            ctrl.set_gait(g)     # (a reset zeroes the robot's gait and velocity command)
            ctrl.set_vel(vel)
            tick(imu[t], motor[t], eff)
            if plant is not None:
                plant.step(eff)
            if sensors is not None:
                sensors.sense()
    if ground_run:
        ctrl.set_ground_run()
    if fused or graph:
        tags = {"vary": bool(vary), "terrain": bool(terrain), "contact": bool(contact), "field": bool(field),
                "ground_run": ctrl.ground_run}
        return run_blocks(ctrl, plant, B, cycles, warmup, schedule, stagger, robot_mode, fused, graph, acts, manager, every, tags)
    held_seen = []

    hold_flags = sensed.view()["hold"] if sensed is not None else None

    def window(act_on=actuators):
        ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(6 if actuators else 5 if manager is not None else 4))
              for _ in range(n)]
        for t in range(n):
            if vary and t in (300, 350):     # (outside the timed pairs: the push starts and ends)
                force.copy_(push) if t == 300 else force.zero_()
            ev[t][0].record()
            tick(imu[t % 26], motor[t % 26], eff)
            ev[t][1].record()
            if acts is not None:         # (the pair 1 -> 5 is recorded either way; it brackets the launch when it is on)
                if act_on:
                    acts.apply(eff)
                ev[t][5].record()
            if plant is not None:
                plant.step(eff)
                ev[t][2].record()
            if sensed is not None:       # the sensor path's manager sits between the plant step and the reading
                sensed.step(eff)
                if acts is not None and act_on:
                    acts.reset(ep_mask, hold_flags)
                ev[t][4].record()
            if sensors is not None:
                sensors.sense()
                ev[t][3].record()
            if sensed is not None:       # (behind the period's last event; a device scalar: no synchronisation)
                held_seen.append(hold_flags.sum(dtype=torch.int32))
            if manager is not None and sensed is None and (t + 1) % every == 0:
                manager.step(every)
                if acts is not None and act_on:
                    acts.reset(ep_mask)
                ev[t][4].record()
        torch.cuda.synchronize()
        return ev

    act_res = None
    if acts is None:
        ev = window()
    else:
        # the period's last event: the reading, else the plant step, else the (possibly empty) actuator pair
        last = 3 if sensors is not None else 2 if plant is not None else 5
        kept = np.arange(n) >= warmup
        med = {False: [], True: []}
        act_us = []
        for _ in range(repeats):
            for on in (False, True):
                ev = window(on)
                med[on].append(float(np.median(np.array([e[0].elapsed_time(e[last]) * 1e3 for e in ev])[kept])))
                if on:
                    act_us.append(float(np.median(np.array([e[1].elapsed_time(e[5]) * 1e3 for e in ev])[kept])))
        st = acts.stats()
        off_, on_ = float(np.median(med[False])), float(np.median(med[True]))
        act_res = {"actuators": True, "delay": delay, "repeats": repeats,
                   "us_per_period_without_act": round(off_, 2), "us_per_period_with_act": round(on_, 2),
                   "us_added_per_period": round(on_ - off_, 2), "us_per_act_median": round(float(np.median(act_us)), 2),
                   "us_per_period_without_act_windows": [round(x, 2) for x in med[False]],
                   "us_per_period_with_act_windows": [round(x, 2) for x in med[True]],
                   "act_calls": int(st["n"].min().item()), "n_vsat": int(st["n_vsat"].sum().item()),
                   "n_tsat": int(st["n_tsat"].sum().item()), "e_heat_mean_J": round(float(st["e_heat"].mean().item()), 3),
                   "tau_peak_max": round(float(st["tau_peak"].max().item()), 3)}
    us = np.array([e[0].elapsed_time(e[1]) * 1e3 for e in ev])
    mpc = (np.arange(n) + 1) % 13 == 0
    keep = np.arange(n) >= warmup
    t_non, t_mpc = float(np.median(us[keep & ~mpc])), float(np.median(us[keep & mpc]))
    per_cycle = 12 * t_non + t_mpc
    v = ctrl.view()
    res = {"batch": B, "source": source, "schedule": schedule, "stagger": bool(stagger), "robot_mode": robot_mode, "ticks_timed": int(keep.sum()),
           "us_per_tick_median": round(float(np.median(us[keep])), 2), "us_per_tick_max": round(float(us[keep].max()), 2),
           "robot_ticks_per_s_window": float(f"{B * int(keep.sum()) / (float(us[keep].sum()) * 1e-6):.4g}")}
    if sensors is not None:
        us_s = np.array([e[4 if sensed is not None else 2].elapsed_time(e[3]) * 1e3 for e in ev])[keep]
        us_all = np.array([e[0].elapsed_time(e[3]) * 1e3 for e in ev])[keep]
        res.update({"us_per_period_median": round(float(np.median(us_all)), 2), "us_per_period_max": round(float(us_all.max()), 2)})
        res.update({"noise": bool(noise), "us_per_sense_median": round(float(np.median(us_s)), 2),
                    "us_per_sense_max": round(float(us_s.max()), 2), "sense_calls": int(sensors.view()["n"].min().item())})
    if vary:
        res["vary"] = True
        res["stats_steps"] = int(plant.stats()["n"].min().item())
    if terrain:
        t_ = plant.terrain()
        res.update({"terrain": True, "support_min": round(float(t_["support"].min().item()), 4),
                    "support_max": round(float(t_["support"].max().item()), 4)})
    if field:
        f_ = plant.field()
        res.update({"field": True, "field_samples": [f_["count"], f_["ny"], f_["nx"]], "ground_min": round(float(plant.terrain()["ground"].min().item()), 4),
                    "ground_max": round(float(plant.terrain()["ground"].max().item()), 4)})
    if contact:
        c_ = plant.contact()
        res.update({"contact": True, "early_foot_ticks": int(c_["early"].sum().item()), "late_foot_ticks": int(c_["late"].sum().item()),
                    "slip_m": round(float(c_["slip"].sum().item()), 4)})
    if stagger or robot_mode == 1:
        res["robot_ticks_per_s"] = res["robot_ticks_per_s_window"]
        if robot_mode == 1:
            n_, k_ = np.unique(ctrl.read("nseg"), return_counts=True)
            res["nseg_histogram"] = {str(int(a)): int(b) for a, b in zip(n_, k_)}
            res["due_last_tick"] = int(ctrl.read("due").sum())
    else:   # every robot solves on the same ticks: the two kinds of tick separately
        res.update({"us_per_nonmpc_tick": round(t_non, 2), "us_per_mpc_tick": round(t_mpc, 2),
                    "us_per_13_tick_cycle": round(per_cycle, 1),
                    "robot_ticks_per_s": float(f"{13 * B / (per_cycle * 1e-6):.4g}")})
    if act_res is not None:
        res.update(act_res)
    if plant is not None:
        us_p = np.array([e[5 if acts is not None else 1].elapsed_time(e[2]) * 1e3 for e in ev])[keep]
        pz = plant.view()["p"][:, 2]
        res.update({"us_per_plant_step_median": round(float(np.median(us_p)), 2), "us_per_plant_step_max": round(float(us_p.max()), 2),
                    "body_height_min": round(float(pz.min().item()), 4), "body_height_max": round(float(pz.max().item()), 4),
                    "status_error_robots": int((torch.from_numpy(ctrl.read("status")[:, 0]) & 47 != 0).sum())})
    if manager is not None:
        ran = keep & ((np.arange(n) + 1) % every == 0)
        us_e = np.array([ev[t][2].elapsed_time(ev[t][4]) * 1e3 for t in np.flatnonzero(ran)])
        ev_, lg = manager.view(), manager.log()
        res.update({"episodes": True, "every": every, "episode_steps_timed": int(ran.sum()),
                    "us_per_episode_step_median": round(float(np.median(us_e)), 2), "us_per_episode_step_max": round(float(us_e.max()), 2),
                    "episodes_finished": int(ev_["episode"].sum().item()),
                    "episodes_per_cause": [int(x) for x in ev_["count"].sum(0).tolist()],
                    "log_rows_written": int(len(lg["rows"])), "log_dropped": int(lg["dropped"])})
    if sensed is not None:
        # what one qmpc_episode_sense_step enqueues here, by include/qmpc_episode_sense.h's list (a count from the
        # configuration, not a trace: it follows qmpc_capi_stages.cpp's entry point by hand): decision, re-initialisation,
        # commands, plant reset (+ the contact counters'), statistics' reset (while on), sensors' reset
        held = np.array([int(x) for x in torch.stack(held_seen).cpu()])[keep]
        res.update({"warm": warm, "launches_per_episode_step": 5 + int(bool(contact)) + int(bool(vary)),
                    "robots_held_per_step_mean": round(float(held.mean()), 2), "robots_held_per_step_max": int(held.max())})
        # ... and the window again with every 100th robot in a warm-up longer than the run: 1 % of the fleet held on every step
        del held_seen[:]
        sensed.hold(torch.arange(B, device="cuda") % 100 == 99, 10 * n)
        ev2 = window()
        us2 = np.array([e[0].elapsed_time(e[3]) * 1e3 for e in ev2])[keep]
        us_e2 = np.array([e[2].elapsed_time(e[4]) * 1e3 for e in ev2])[keep]
        held = np.array([int(x) for x in torch.stack(held_seen).cpu()])[keep]
        res.update({"held_us_per_period_median": round(float(np.median(us2)), 2), "held_us_per_period_max": round(float(us2.max()), 2),
                    "held_us_per_episode_step_median": round(float(np.median(us_e2)), 2),
                    "held_robots_per_step_mean": round(float(held.mean()), 2),
                    "episodes_finished_end": int(manager.view()["episode"].sum().item())})
        v = ctrl.view()
    res.update({"all_finite": bool(torch.isfinite(eff).all().item()), "latched": int((v["safe"] == 0).sum())})
    ctrl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,4096,16384")
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=26)
    ap.add_argument("--schedule", choices=("lockstep", "per_robot"), default="lockstep")
    ap.add_argument("--stagger", action="store_true")
    ap.add_argument("--robot-mode", type=int, choices=(0, 1), default=0)
    ap.add_argument("--source", choices=("imu", "state", "plant", "sensor"), default="imu")
    ap.add_argument("--vary", action="store_true")
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--contact", action="store_true")
    ap.add_argument("--field", action="store_true")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--episodes", action="store_true")
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--actuators", action="store_true")
    ap.add_argument("--delay", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--ground-run", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if (a.fused or a.graph) and a.source != "plant":
        ap.error("--fused and --graph go with --source plant")
    if a.ground_run and not (a.fused and (a.terrain or a.field)):
        ap.error("--ground-run goes with --fused and --terrain and / or --field")
    if (a.fused or a.graph) and a.episodes and 13 % a.every:
        ap.error("--fused / --graph with --episodes: --every K must divide 13 (the blocks are 13 ticks)")
    if a.vary and a.source not in ("plant", "sensor"):
        ap.error("--vary needs --source plant or sensor")
    if a.terrain and a.source not in ("plant", "sensor"):
        ap.error("--terrain needs --source plant or sensor")
    if a.contact and a.source not in ("plant", "sensor"):
        ap.error("--contact needs --source plant or sensor")
    if a.field and a.source not in ("plant", "sensor"):
        ap.error("--field needs --source plant or sensor")
    if a.episodes and a.source not in ("plant", "sensor"):
        ap.error("--episodes needs --source plant or sensor")
    if a.episodes and a.source == "sensor" and a.every != 1:
        ap.error("--every K > 1 is out of scope on the sensor path (qmpc_episode_sense_step runs on every tick)")
    if a.warm < 0 or (a.warm != 50 and not (a.episodes and a.source == "sensor")):
        ap.error("--warm W >= 0 goes with --source sensor --episodes")
    if a.every < 1 or (a.every != 1 and not a.episodes):
        ap.error("--every K >= 1 goes with --episodes")
    if not 0 <= a.delay <= 64 or a.repeats < 1 or ((a.delay or a.repeats != 3) and not a.actuators):
        ap.error("--delay D (0 .. 64) and --repeats R >= 1 go with --actuators")
    if a.noise and a.source != "sensor":
        ap.error("--noise needs --source sensor")
    if a.robot_mode == 1:
        a.schedule = "per_robot"
    if a.stagger and a.schedule != "per_robot":
        ap.error("--stagger needs --schedule per_robot (a lockstep reset keeps the robot on the batch's MPC ticks)")
    out = []
    for B in [int(x) for x in a.batches.split(",")]:
        r = run(B, a.cycles, a.warmup, a.schedule, a.stagger, a.robot_mode, a.source, a.vary, a.noise, a.terrain, a.contact, a.field,
                a.episodes, a.every, a.warm, a.actuators, a.delay, a.repeats, a.fused, a.graph, a.ground_run)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
