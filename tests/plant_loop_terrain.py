"""The closed loops of tests/plant_loop.py and tests/sense_loop.py on per-robot slopes and stairs -- TEST SIDE ONLY.

terrain(B) is the single definition of the ground the closed-loop tests walk on (include/qmpc_terrain.h): robot b's row
depends on k = b % 16 through plant_loop.commands() -- its start position and yaw -- and on its kind k % 4:

    0  stairs up        2  stairs down
    1  cross slope gy   3  uphill gx        (the robots of kind 1 stand in robot mode 0)

Flights start START m ahead of the robot's start position along its start yaw (psi = start yaw) and have TREADS treads.
The amplitudes RUNGS are MEASURED: for each kind the largest rung of its ladder at which the reference pipeline (the
controller's restatements with the reference's qpOASES for every solve) keeps every robot safe in both robot modes on both
paths, with every qpOASES return code 0 and nWSR < 100; tests/golden/make_plant_terrain_closed_loop.py climbs the ladders
and records what it found, tests/test_terrain_cpu.py holds RUNGS and TICKS to the record.  The controller and the oracle
are not told about the ground.

cpu_loop_terrain(mode, path) is plant_loop.cpu_loop (path "state", with rebase_z) or sense_loop.cpu_loop_sensed with
sense_loop.noise() (path "sensed"), on TerrainPlantModel with clamp_swing.
"""
import numpy as np

from oracle import oracle as O

import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_loop as L
import plant_model_terrain as PT
import sense_loop as SL
import sense_model as SM
from ctrl_model_state import estimate_state

f32 = np.float32
KINDS = ("stairs_up", "cross_slope", "stairs_down", "uphill")          # by k % 4
START, TREADS = 0.10, 4
# the ladders: (run, |rise|) from the reference's own boxes (scripts/walking_simulation.py: depth 0.2, heights 0.01 .. 0.04),
# then the same rises on a sharper flight that a walk of 1300 ticks can cross; slopes
STAIRS_LADDER = ((0.2, 0.01), (0.2, 0.02), (0.2, 0.03), (0.2, 0.04), (0.1, 0.01), (0.1, 0.02), (0.1, 0.03), (0.1, 0.04))
SLOPE_LADDER = (0.02, 0.05, 0.10, 0.15)
LADDERS = dict(stairs_up=STAIRS_LADDER, cross_slope=SLOPE_LADDER, stairs_down=STAIRS_LADDER, uphill=SLOPE_LADDER)
PATHS = ("state", "sensed")
# the measured choice (None: no safe rung above flat, that kind's robots get flat rows) and the tick count
RUNGS = dict(stairs_up=(0.1, 0.04), cross_slope=0.15, stairs_down=(0.1, 0.04), uphill=0.15)   # every rung was walked
TICKS = 1300


def terrain(B, rungs=None):
    """-> rows [B, 8] (z0, gx, gy, rise, run, count, s0, psi) for B robots; rungs: a dict like RUNGS (default: RUNGS)."""
    rungs = RUNGS if rungs is None else rungs
    _, _, xyyaw = L.commands(0)                      # (the start poses are the same in both robot modes)
    k = np.arange(B) % L.N_CMD
    x0, y0, psi = xyyaw[k, 0], xyyaw[k, 1], xyyaw[k, 2]
    rows = np.zeros((B, 8))
    for kind, name in enumerate(KINDS):
        sel = k % 4 == kind
        r = rungs[name]
        if r is None:
            continue
        if name in ("stairs_up", "stairs_down"):
            run, rise = r
            rows[sel, 3] = rise if name == "stairs_up" else -rise
            rows[sel, 4], rows[sel, 5] = run, TREADS
            rows[sel, 6] = ((x0 * np.cos(psi) + y0 * np.sin(psi)) + START)[sel]
            rows[sel, 7] = psi[sel]
        else:
            rows[sel, 2 if name == "cross_slope" else 1] = r
    return rows


def cpu_loop_terrain(mode, path, rungs=None, ticks=None, settle=SL.SETTLE, seed=SL.SEED, substeps=1, mu=0.4):
    """-> (stats, info): plant_loop.cpu_loop's fields; info's safe, nwsr_max and rc_bad are PER ROBOT here ([16] each),
    plus travel [16]: the body's final abscissa along its flight's heading from its start, and rows."""
    assert path in PATHS
    ticks = TICKS if ticks is None else ticks
    gait, vel, xyyaw = L.commands(mode)
    B = L.N_CMD
    rows = terrain(B, rungs)
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(B, L.FREQ, L.PID)
    m.set_gait(gait)
    m.set_vel(vel)
    plant = PT.TerrainPlantModel(B, L.FREQ, mu, substeps, xyyaw)                    # init -> set_terrain -> reset(all)
    plant.set_terrain(rows, clamp_swing=True, rebase_z=path == "state")
    plant.reset(np.ones(B, bool), xyyaw)
    rec = L.Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    if path == "sensed":
        sens = SM.SenseModel(B, seed)
        sens.set_params(**SL.noise(B))
        for _ in range(settle):                       # BatchedSensors.settle: sense -> pre_work on the standing plant
            imu, motor = sens.sense(plant.state, plant.motor)
            m.estimate(imu, motor)
    nwsr_max, rc_bad, n_solves = np.zeros(B, int), np.zeros(B, int), 0
    for t in range(ticks):
        e = estimate_state(m, plant.state, plant.motor) if path == "state" else m.estimate(imu, motor)
        m.loco(e)
        if mode == 0:
            due = np.arange(B) if (t + 1) % 13 == 0 else np.zeros(0, int)
        else:
            due = np.flatnonzero(m.due)
        if len(due):
            if mode == 0:
                r, wpd, xci = O.pack_commands(m.command(e), float(m.dt_mpc))
            else:
                cmd, tables = m.command_mode1(e, due)
                r, wpd, xci = O.pack_commands(cmd, float(m.dt_mpc))
                r["gait"] = tables
            m.wpd[due], m.xci[due] = wpd, xci
            r.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)        # the MPC's model: flat ground
            soln, nwsr, rc = O.solve_batch(r)
            rc_bad[due] += (rc != 0)
            nwsr_max[due] = np.maximum(nwsr_max[due], nwsr)
            n_solves += len(due)
            m.f_ff[due] = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(f32))
        eff = m.legcmd(e, m.f_ff)
        plant.step(eff, m.contact_state, m.p_des, m.v_des)
        rec.add(plant.state)
        if path == "sensed":
            imu, motor = sens.sense(plant.state, plant.motor)
    stats = rec.stats()
    # the model's own accumulators are the Recorder's extremes without the initial state
    s = plant.stats
    assert (s["n"] == ticks).all()
    psi = xyyaw[:, 2]
    d = plant.p[:, :2] - xyyaw[:, :2]
    travel = d[:, 0] * np.cos(psi) + d[:, 1] * np.sin(psi)
    return stats, dict(safe=m.safe.copy(), nwsr_max=nwsr_max, n_solves=n_solves, rc_bad=rc_bad, travel=travel, rows=rows,
                       support=plant.support.copy(), ground=plant.ground.copy())
