"""What the GPU suites of the fleet share (-m gpu: tests/test_gpu_plant*.py, test_gpu_sense.py, test_gpu_terrain.py,
test_gpu_contact.py, test_gpu_field.py, test_gpu_act.py, test_gpu_episode*.py) -- TEST SIDE ONLY, no test in here.

Three parts:

  1. the set-up and read-back helpers every one of those files needs: pair(), dev(), snap*(), close() / compare*() at
     TOL, walk_pair(), stand_on(), trio(), plant_stats(), and the bodies that more than one file runs
     (single_step, teacher_forced_closed_loop, masked_reset_is_the_models);
  2. THE device walk, once: walk() runs a caller's single-tick callable, checks the status word on the ticks the caller
     names and reads the device accumulators a second before the end and at the end; stats_from_accumulators() rebuilds
     the five plant_loop.STATS from them (tests/test_plant_varied_cpu.py pins that formula to plant_loop.Recorder on the
     CPU); assert_inside_envelope() holds them to plant_loop.envelope() of the recorded CPU run;
  3. nothing else: the episode fleets are in tests/episode_gpu.py.

This module is not rewritten by pytest's assertion rewriting, so every assert in here carries its own message: which
quantity, which robots, by how much.  torch and the binding are imported inside the functions: importing the module needs
no GPU.
"""
import numpy as np

import plant_loop as L
import plant_model as PM
import plant_model_varied as PV
import sense_loop as SL
from plant_cases import DEFAULTS, parity_case

TOL = 1e-10                       # relative to max(1, |x|): see tests/test_gpu_plant.py
PLANT_KEYS = ("p", "v", "q", "omega", "foot", "grf", "stance", "state", "motor")
CONTACT_KEYS = ("early", "late", "slip", "drop")
ON = dict(early=True, late=True, slip=True)
assert DEFAULTS["freq"] == L.FREQ


def _where(bad):
    """The first robots (rows) of a boolean array that are set, for a message."""
    bad = np.asarray(bad)
    return np.flatnonzero(bad.reshape(len(bad), -1).any(1))[:8].tolist()


def equal(a, b, what):
    """np.array_equal, with a message that says where."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} and {b.shape}"
    assert np.array_equal(a, b), f"{what}: differs in rows {_where(a != b)}"


# ---- set-up --------------------------------------------------------------------------------------------------------------

def pair(B, schedule="lockstep", mode=None, substeps=1, xyyaw=None, max_batch=None, consts=None):
    """consts: a dict like DEFAULTS; its body goes to qmpc_set_robot (gravity -9.81, which the plant does not read) and
    its geometry to qmpc_set_leg_geometry, None leaves the handle as created."""
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant
    k = consts or DEFAULTS
    c = BatchedController(0, max_batch=max_batch or B)
    c.init(B, k["freq"], L.PID)
    if consts is not None:
        c.mpc.set_robot(float(k["mass"]), [float(x) for x in k["ibody"]], -9.81)
        c.mpc.set_leg_geometry(*[float(x) for x in k["geom"]])
    if schedule != "lockstep":
        c.set_schedule(schedule)
    if mode is not None:
        c.set_robot_mode(mode)
    p = BatchedPlant(c)
    p.init(k["mu"], substeps, None if xyyaw is None else torch.from_numpy(np.ascontiguousarray(xyyaw, np.float64)).to(c.device))
    return c, p


def dev(c, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(c.device)


def all_robots(c, B):
    import torch
    return torch.ones(B, dtype=torch.bool, device=c.device)


def walk_setup(mode, reps):
    gait, vel, xyyaw = L.commands(mode)
    return np.tile(gait, reps), np.tile(vel, (reps, 1)), np.tile(xyyaw, (reps, 1))


def walk_pair(B, schedule="lockstep", mode=None):
    """pair() on plant_loop's commands tiled over B robots, the commands set -> (c, plant, (gait, vel, xyyaw))."""
    gait, vel, xyyaw = walk_setup(mode or 0, B // L.N_CMD)
    c, plant = pair(B, schedule, mode, xyyaw=xyyaw)
    c.set_gait(dev(c, gait))
    c.set_vel(dev(c, vel))
    return c, plant, (gait, vel, xyyaw)


def trio(B, schedule="lockstep", mode=None, seed=SL.SEED):
    """Controller + plant + sensors on plant_loop's commands, repeated over B robots (B need not be a multiple of 16)."""
    from quadruped_ctrl_amd.binding import BatchedSensors
    gait, vel, xyyaw = L.commands(mode or 0)
    k = np.arange(B) % L.N_CMD
    gait, vel, xyyaw = gait[k], vel[k], xyyaw[k]
    c, plant = pair(B, schedule, mode, xyyaw=xyyaw)
    c.set_gait(dev(c, gait))
    c.set_vel(dev(c, vel))
    s = BatchedSensors(plant)
    s.init(seed)
    return c, plant, s, (gait, vel, xyyaw)


def sense_values(B, seed):
    """All six arrays of qmpc_sense_params, every robot its own values."""
    rng = np.random.default_rng(seed)
    return dict(acc_bias=rng.uniform(-0.5, 0.5, (B, 3)), gyro_bias=rng.uniform(-0.05, 0.05, (B, 3)),
                acc_sigma=rng.uniform(0.05, 0.5, B), gyro_sigma=rng.uniform(0.005, 0.05, B),
                q_sigma=rng.uniform(0.0005, 0.005, B), qd_sigma=rng.uniform(0.01, 0.1, B))


def sense_bind(c, s, vals):
    t = {k: dev(c, v) for k, v in vals.items()}
    s.set_params(**t)
    return t


def noisy_sensors(c, plant, seed, settle):
    """Sensors on `plant` with sense_loop.noise() bound, after settle(`settle`) -> (the sensors, the bound tensors: keep
    them referenced)."""
    from quadruped_ctrl_amd.binding import BatchedSensors
    s = BatchedSensors(plant)
    s.init(seed)
    keep = sense_bind(c, s, SL.noise(plant.batch))
    s.settle(settle)
    return s, keep


def stand_on(c, plant, rows, xyyaw, **flags):
    """init -> set_terrain -> reset(all): -> the device rows (bound: keep them referenced)."""
    d = dev(c, rows)
    plant.set_terrain(d, **flags)
    plant.reset(all_robots(c, plant.batch), None if xyyaw is None else dev(c, xyyaw))
    return d


def start(c, plant, m, cs, pd, vd):
    """The model's state and the controller outputs the plant reads, put on the device: the views alias the state."""
    B = m.B
    pv, cv = plant.view(), c.view()
    for key, val in (("p", m.p), ("v", m.v), ("q", m.q), ("omega", m.w), ("foot", m.foot.reshape(B, 12))):
        pv[key].copy_(dev(c, val))
    pv["stance"].copy_(dev(c, m.stance.astype(np.int32)))
    cv["contact_state"].copy_(dev(c, cs))
    cv["p_des"].copy_(dev(c, pd.reshape(B, 12)))
    cv["v_des"].copy_(dev(c, vd.reshape(B, 12)))


def start_contact(c, plant, m0, cs, pd, vd, rows, tflags, flags, params):
    """The model's state on the device, the terrain and the contact as the model has them -> what must stay referenced."""
    start(c, plant, m0, cs, pd, vd)
    d = None
    if rows is not None:
        d = dev(c, rows)
        plant.set_terrain(d, clamp_swing=tflags[0], rebase_z=tflags[1])
    plant.terrain()["support"].copy_(dev(c, m0.support))
    plant.set_contact(*flags, **params)
    v = plant.contact()
    for k in CONTACT_KEYS:
        v[k].copy_(dev(c, getattr(m0, k)))
    return d


# ---- read-back -----------------------------------------------------------------------------------------------------------

def snap(plant):
    import torch
    torch.cuda.synchronize()
    v = plant.view()
    return {k: v[k].cpu().numpy().copy() for k in PLANT_KEYS}


def snap_legs(plant, B):
    """snap() with foot and grf as [B, 4, 3]."""
    s = snap(plant)
    s["foot"], s["grf"] = s["foot"].reshape(B, 4, 3), s["grf"].reshape(B, 4, 3)
    return s


def snap3(plant, B):
    """The plant's views and the terrain's, as numpy copies (synchronises)."""
    s = snap_legs(plant, B)
    t = plant.terrain()
    s["ground"], s["support"] = t["ground"].cpu().numpy().copy(), t["support"].cpu().numpy().copy()
    return s


def snap4(plant, B):
    """The plant's views, the terrain's and the contact's, as numpy copies (synchronises)."""
    s = snap3(plant, B)
    v = plant.contact()
    s.update({k: v[k].cpu().numpy().copy() for k in CONTACT_KEYS})
    return s


def plant_stats(plant):
    """The plant's device accumulators (plant_model_varied.STAT_KEYS) as numpy copies (synchronises)."""
    import torch
    torch.cuda.synchronize()
    s = plant.stats()
    return {k: s[k].cpu().numpy().copy() for k in PV.STAT_KEYS}


# ---- comparisons ---------------------------------------------------------------------------------------------------------

def close(got, want, what):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: worst error relative to max(1, |x|) {err.max():.3e}")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def compare(s, model, what):
    for k, mk in (("state", "state"), ("motor", "motor"), ("p", "p"), ("v", "v"), ("q", "q"), ("omega", "w"),
                  ("foot", "foot"), ("grf", "grf")):
        close(s[k], getattr(model, mk), f"{what} {k}")
    equal(s["stance"] != 0, model.stance, f"{what} stance")


def compare_terrain(s, m, what):
    compare(s, m, what)
    close(s["ground"], m.ground, f"{what} ground")
    close(s["support"], m.support, f"{what} support")


def compare_contact(s, m, what):
    compare_terrain(s, m, what)                           # every view array, state, motor, ground, support; stance exactly
    close(s["drop"], m.drop, f"{what} drop")
    close(s["slip"], m.slip, f"{what} slip")
    equal(s["early"], m.early, f"{what} early")
    equal(s["late"], m.late, f"{what} late")


def same(a, b, what):
    """Two plants: every view array and the effort, bit for bit."""
    sa, sb = snap(a), snap(b)
    for k in PLANT_KEYS:
        equal(sa[k], sb[k], f"{what} {k}")
    equal(a.effort.cpu().numpy(), b.effort.cpu().numpy(), f"{what} effort")


# ---- bodies that more than one file runs ---------------------------------------------------------------------------------

def single_step(substeps, consts=None):
    """The body of test_gpu_plant.test_single_step_parity; consts: see pair()."""
    B, m, old, new, tau, cs, pd, vd = parity_case(substeps, consts or DEFAULTS)
    c, plant = pair(B, substeps=substeps, consts=consts)
    start(c, plant, m, cs, pd, vd)
    state, motor = plant.step(dev(c, tau.reshape(B, 12)))
    m.step(tau.reshape(B, 12), cs, pd, vd)
    s = snap_legs(plant, B)
    compare(s, m, f"substeps {substeps}")
    equal(state.cpu().numpy(), s["state"], "the state step() returned against the view's")
    equal(motor.cpu().numpy(), s["motor"], "the motor rows step() returned against the view's")
    # the cases are there: both edges, zero and saturated forces, the clamp
    assert (new & ~old).any() and (old & ~new).any() and (~new).all(1).any() and new.all(1).any(), \
        "the case lost a stance pattern: touch-down, lift-off, all-swing or all-stance"
    g = m.grf
    on_cone = np.abs(np.hypot(g[..., 0], g[..., 1]) - m.mu * g[..., 2]) < 1e-12
    n_cone = int((on_cone & (g[..., 2] > 1)).sum())
    assert n_cone > 20 and (g[0][new[0]] == 0).all(), f"{n_cone} saturated feet (want > 20), robot 0's forces {g[0]}"
    # (with substeps the body has dropped off the singularity by the second)
    assert substeps > 1 or (g[256] == 0).all(), f"robot 256's forces at the singular leg: {g[256]}"
    assert abs(m.motor[5, 2] - PM.KNEE_MIN) < 1e-9 or new[5, 0], f"robot 5's knee {m.motor[5, 2]} is not at KNEE_MIN"
    c.close()


def teacher_forced_closed_loop(B, ticks, consts=None):
    """The body of test_gpu_plant.test_teacher_forced_closed_loop; consts: see pair()."""
    k = consts or DEFAULTS
    gait, vel, xyyaw = walk_setup(0, B // L.N_CMD)
    c, plant = pair(B, xyyaw=xyyaw, consts=consts)
    c.set_gait(dev(c, gait))
    c.set_vel(dev(c, vel))
    m = PM.PlantModel(B, k["freq"], k["mu"], 1, xyyaw, mass=k["mass"], ibody=k["ibody"], geom=k["geom"])
    s = snap_legs(plant, B)
    compare(s, m, "init")
    moved = 0.0
    for t in range(ticks):
        m.load(s)
        eff = c.tick_state(plant.state, plant.motor, plant.effort).cpu().numpy()
        v = c.view()
        cs, pd, vd = (v[k].cpu().numpy() for k in ("contact_state", "p_des", "v_des"))
        plant.step(plant.effort)
        m.step(eff, cs, pd, vd)
        s = snap_legs(plant, B)
        compare(s, m, f"tick {t}")
        moved = max(moved, float(np.abs(eff).max()))
    safe = c.read("safe")
    assert moved > 1.0, f"the largest effort of the run is {moved}: the fleet did not move"
    assert (safe == 1).all(), f"robots latched unsafe: {_where(safe != 1)}"
    assert c.view()["ticks"] == ticks, f"the controller counted {c.view()['ticks']} ticks, not {ticks}"
    c.close()


def masked_reset_is_the_models(ground):
    """Contact on, on `ground` = "flat", "terrain" or "field": five robots (20 lanes, a third of one wave: every lane past
    n is a padding lane) walk 13 closed-loop ticks, every counter, drop, support and ground is then made non-zero, and
    reset(robots 1 and 3) leaves what tests/plant_model_field.py's reset leaves from the same state: the two robots
    standing on their ground with their counters and drop at zero (without rows, support and ground too), at the parity's
    tolerance and the integers exactly; the other three bit for bit as they were."""
    from quadruped_ctrl_amd.binding import rollout
    import plant_loop_field as LF
    import plant_loop_terrain as LT
    import plant_model_field as PF
    B = 5
    gait, vel, xyyaw = (a[:B] for a in L.commands(0))
    c, plant = pair(B, xyyaw=xyyaw)
    c.set_gait(dev(c, gait))
    c.set_vel(dev(c, vel))
    m = PF.FieldPlantModel(B, DEFAULTS["freq"], DEFAULTS["mu"], 1, xyyaw)
    keep = []
    if ground == "terrain":
        rows = LT.terrain(B)
        keep.append(dev(c, rows))
        plant.set_terrain(keep[-1], clamp_swing=True, rebase_z=True)
        m.set_terrain(rows, clamp_swing=True, rebase_z=True)
    if ground == "field":
        z, place, cell = LF.field_for(B, 0.06)
        keep += [dev(c, z), dev(c, place)]
        plant.set_field(keep[-2], keep[-1], cell, clamp_swing=True, rebase_z=True)
        m.set_field(z, place, cell, clamp_swing=True, rebase_z=True)
    plant.set_contact(**ON)
    m.set_contact(**ON)
    plant.reset(all_robots(c, B), dev(c, xyyaw))
    rollout(c, plant, 13)
    v, t = plant.contact(), plant.terrain()
    print(ground, "after 13 ticks:", {k: float(np.abs(a).max()) for k, a in snap4(plant, B).items() if k in CONTACT_KEYS + ("support", "ground")})
    for k in CONTACT_KEYS:
        v[k].add_(1)
    for k in ("support", "ground"):
        t[k].add_(0.125)
    before = snap4(plant, B)
    for k in CONTACT_KEYS + ("support", "ground"):
        assert before[k].all(), f"{ground}: {k} has zeros before the reset: {before[k]}"
    m.load(before)
    for k in ("grf", "state", "motor", "ground", "support") + CONTACT_KEYS:
        setattr(m, k, before[k].copy())
    mask = np.zeros(B, bool)
    mask[[1, 3]] = True
    plant.reset(dev(c, mask), dev(c, xyyaw))
    m.reset(mask, xyyaw)
    after = snap4(plant, B)
    compare_contact(after, m, f"masked reset on {ground}")
    for k in CONTACT_KEYS + (("support", "ground") if ground == "flat" else ()):
        assert not after[k][mask].any(), f"{ground}: {k} of the reset robots is not zero: {after[k][mask]}"
    if ground != "flat":
        equal(after["p"][mask][:, 2], 0.29 + after["ground"][mask], f"{ground}: the reset robots' height above their ground")
    for k in before:
        equal(after[k][~mask], before[k][~mask], f"{ground}: {k} of the robots outside the mask")
    assert (after["stance"][mask] == 1).all(), f"{ground}: the reset robots' stance {after['stance'][mask]}"
    assert plant.contact()["flags"] == 7, f"{ground}: the reset changed the contact flags to {plant.contact()['flags']}"
    del keep
    c.close()


# ---- the device walk -----------------------------------------------------------------------------------------------------

def walk(c, plant, tick, ticks, check, settle=None):
    """The walk of the closed-loop tests: `ticks` times tick(t) -- the caller's single period (a rollout of one tick, after
    whatever it rewrites on the stream before it) -- with a host read after every one.

    check(t) names the ticks after which no robot's solve status may hold an error bit (status & 47); settle(), if given,
    runs after the start state is read and before the first tick (the sensor path's set-up).  The plant's device
    accumulators are read a second before the end (after tick `ticks - int(FREQ)`) and at the end; both must have
    counted every tick, and no robot may be latched unsafe at the end.
    -> (start state [B, 16], mid, end): what stats_from_accumulators takes."""
    start_state = plant.state.cpu().numpy().copy()
    if settle is not None:
        settle()
    n_mid = ticks - int(L.FREQ)
    for t in range(ticks):
        tick(t)
        if check(t):
            bits = c.read("status")[:, 0] & 47
            assert (bits == 0).all(), f"tick {t}: solve status error bits {bits[bits != 0][:8]} on robots {_where(bits != 0)}"
        if t + 1 == n_mid:
            mid = plant_stats(plant)
    end = plant_stats(plant)
    safe = c.read("safe")
    assert (safe == 1).all(), f"robots latched unsafe after {ticks} ticks: {_where(safe != 1)}"
    assert (mid["n"] == n_mid).all(), f"the accumulators counted {np.unique(mid['n'])} periods by tick {n_mid}"
    assert (end["n"] == ticks).all(), f"the accumulators counted {np.unique(end['n'])} periods by tick {ticks}"
    return start_state, mid, end


def ground_walk(c, plant, path, mode, ticks, seed, settle):
    """walk() as the terrain, contact and field tests run it: rollout() one tick at a time (path "state"), or noisy_sensors()
    and rollout_sensed() (path "sensed"); the status word is checked after every tick in robot mode 1 and after every
    13th -- the solves' -- in mode 0."""
    from quadruped_ctrl_amd.binding import rollout, rollout_sensed
    sensors = []                                         # [the sensors, their bound tensors] once walk() has set them up
    if path == "sensed":
        tick = lambda t: rollout_sensed(c, plant, sensors[0], 1)
    else:
        tick = lambda t: rollout(c, plant, 1)
    return walk(c, plant, tick, ticks, lambda t: mode == 1 or (t + 1) % 13 == 0,
                settle=(lambda: sensors.extend(noisy_sensors(c, plant, seed, settle))) if path == "sensed" else None)


def stats_from_accumulators(start_state, mid, end):
    """plant_loop.STATS per robot from the start state [B, 16] and the plant's accumulators (device or model) read a
    second before the end and at the end: the accumulators' extremes do not hold the start, plant_loop.Recorder's do; the
    mean forward speed is over the periods between the two reads."""
    rpy0 = L.rpy_of(start_state[:, 0:4])
    return dict(z_min=np.minimum(end["z_min"], start_state[:, 6]), z_max=np.maximum(end["z_max"], start_state[:, 6]),
                roll_max=np.maximum(end["roll_max"], np.abs(rpy0[:, 0])),
                pitch_max=np.maximum(end["pitch_max"], np.abs(rpy0[:, 1])),
                vx_mean=(end["vx_sum"] - mid["vx_sum"]) / (end["n"] - mid["n"]))


def assert_inside_envelope(stats, rec, reps, label):
    """Every robot's five statistics inside plant_loop.envelope() of the recorded CPU run `rec` (16 commands), tiled over
    `reps` robots per command."""
    env = L.envelope(rec)
    for k in L.STATS:
        lo, hi = np.tile(env[k][0], reps), np.tile(env[k][1], reps)
        want = np.tile(np.asarray(rec[k]), reps)
        print(f"{label} {k}: largest distance from the CPU run {np.abs(stats[k] - want).max():.3e}, "
              f"allowed {float((hi - want).max()):.3e}")
        assert (stats[k] >= lo).all() and (stats[k] <= hi).all(), (label, k, stats[k], lo, hi)
