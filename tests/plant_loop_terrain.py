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

cpu_loop_terrain(mode, path) is plant_loop.closed_loop (the only copy of the tick) on TerrainPlantModel with clamp_swing:
through the cheater estimators with rebase_z (path "state"), or through sense_loop.noise() and the filter (path "sensed").
walk() is the part the loops on contact and on the field share with it.
"""
import numpy as np

import plant_loop as L
import plant_model_terrain as PT
import sense_loop as SL

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


def travel(plant, xyyaw):
    """The bodies' final abscissa along their start headings from their starts [B]."""
    psi = xyyaw[:, 2]
    d = plant.p[:, :2] - xyyaw[:, :2]
    return d[:, 0] * np.cos(psi) + d[:, 1] * np.sin(psi)


def walk(m, plant, xyyaw, path, ticks, settle, seed):
    """plant_loop.closed_loop on a plant that stands on its ground, through the cheater estimators (path "state") or
    through sense_loop.noise() and the filter (path "sensed") -> (stats, info): safe, nwsr_max and rc_bad PER ROBOT, n_solves
    and travel [16].  The loops on terrain, contact and the field are this plus their plant's own arrays."""
    assert path in PATHS
    sens = SL.sensors_for(plant.B, seed) if path == "sensed" else None
    stats, info = L.closed_loop(m, plant, ticks, sensors=sens, settle=settle)
    assert (plant.stats["n"] == ticks).all()          # (the model's own accumulators counted every step)
    return stats, dict(safe=info["safe"], nwsr_max=info["nwsr_max"], n_solves=info["n_solves"], rc_bad=info["rc_bad"],
                       travel=travel(plant, xyyaw))


def cpu_loop_terrain(mode, path, rungs=None, ticks=None, settle=SL.SETTLE, seed=SL.SEED, substeps=1, mu=0.4):
    """-> (stats, info): plant_loop.cpu_loop's fields; info's safe, nwsr_max and rc_bad are PER ROBOT here ([16] each),
    plus travel [16]: the body's final abscissa along its flight's heading from its start, and rows."""
    m, xyyaw = L.controller_for(mode)
    rows = terrain(L.N_CMD, rungs)
    plant = PT.TerrainPlantModel(L.N_CMD, L.FREQ, mu, substeps, xyyaw)              # init -> set_terrain -> reset(all)
    plant.set_terrain(rows, clamp_swing=True, rebase_z=path == "state")
    plant.reset(np.ones(L.N_CMD, bool), xyyaw)
    stats, info = walk(m, plant, xyyaw, path, TICKS if ticks is None else ticks, settle, seed)
    return stats, dict(info, rows=rows, support=plant.support.copy(), ground=plant.ground.copy())


