"""The closed loops of tests/plant_loop_terrain.py with contact decided by the ground -- TEST SIDE ONLY.

cpu_loop_contact(mode, path, ...) is plant_loop_terrain.cpu_loop_terrain on tests/plant_model_contact.py's
ContactPlantModel (include/qmpc_contact.h): the reference pipeline -- the controller's restatements with the reference's
qpOASES for every solve -- on a plant whose feet land when they meet the ground, stub on treads and slide.  The
controller and the MPC are not told: the MPC keeps planning on mu = 0.4 and flat ground.

The ladders (tests/golden/make_plant_contact_closed_loop.py climbs them; each stops at its first fallen rung; a rung
counts when every robot is safe in both robot modes on both paths with every qpOASES return code 0 and nWSR < 100):

    flat      flat ground, EARLY | LATE
    stairs    robots k % 4 == 0 climb and k % 4 == 2 descend four treads of run 0.1 m (the others walk on flat rows),
              EARLY | LATE, rises STAIRS_LADDER
    friction  flat ground, EARLY | LATE | SLIP, the plant's mu from FRICTION_LADDER

RUNGS is the MEASURED record: the top walked rung of the stairs' and the friction's ladder (None: even the first fell),
and `flat`.  The walk the fixture records and the GPU suite repeats is walk_config(): the top stairs rung under
EARLY | LATE | SLIP on the top friction rung's floor.
"""
import numpy as np

from oracle import oracle as O

import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_loop as L
import plant_loop_terrain as LT
import plant_model_contact as PCM
import sense_loop as SL
import sense_model as SM
from ctrl_model_state import estimate_state

f32 = np.float32
PATHS = LT.PATHS
RUN = 0.1
STAIRS_LADDER = (0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.10)
FRICTION_LADDER = (0.4, 0.3, 0.2, 0.15, 0.1, 0.05)
TICKS = 1300
# the measured record (tests/golden/plant_contact_closed_loop_cpu.json; tests/test_contact_cpu.py holds it to the file)
RUNGS = dict(flat=True, stairs=0.02, friction=0.15)     # the stairs fell at 0.03 m, the floor at mu = 0.1


def rows_for(B, rise):
    """LT.terrain with stairs of RUN x rise up (k % 4 == 0) and down (k % 4 == 2), flat rows for the others."""
    r = None if rise is None else (RUN, rise)
    return LT.terrain(B, dict(stairs_up=r, cross_slope=None, stairs_down=r, uphill=None))


def ladder_config(ladder, rung):
    """-> dict(rise, mu, flags) of a rung of a ladder."""
    if ladder == "flat":
        return dict(rise=None, mu=0.4, flags=PCM.EARLY | PCM.LATE)
    if ladder == "stairs":
        return dict(rise=rung, mu=0.4, flags=PCM.EARLY | PCM.LATE)
    assert ladder == "friction"
    return dict(rise=None, mu=rung, flags=PCM.EARLY | PCM.LATE | PCM.SLIP)


def walk_config(rungs=None):
    rungs = RUNGS if rungs is None else rungs
    return dict(rise=rungs["stairs"], mu=0.4 if rungs["friction"] is None else rungs["friction"],
                flags=PCM.EARLY | PCM.LATE | PCM.SLIP)


def cpu_loop_contact(mode, path, config=None, ticks=None, settle=SL.SETTLE, seed=SL.SEED, substeps=1):
    """-> (stats, info): plant_loop_terrain.cpu_loop_terrain's fields (per robot), plus early, late [16] (foot-ticks) and
    slip [16] (metres); config: walk_config() / ladder_config()."""
    assert path in PATHS
    cfg = walk_config() if config is None else config
    ticks = TICKS if ticks is None else ticks
    gait, vel, xyyaw = L.commands(mode)
    B = L.N_CMD
    rows = rows_for(B, cfg["rise"])
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(B, L.FREQ, L.PID)
    m.set_gait(gait)
    m.set_vel(vel)
    plant = PCM.ContactPlantModel(B, L.FREQ, cfg["mu"], substeps, xyyaw)     # init -> set_terrain -> set_contact -> reset
    plant.set_terrain(rows, clamp_swing=True, rebase_z=path == "state")
    fl = cfg["flags"]
    plant.set_contact(early=bool(fl & PCM.EARLY), late=bool(fl & PCM.LATE), slip=bool(fl & PCM.SLIP))
    plant.reset(np.ones(B, bool), xyyaw)
    rec = L.Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    if path == "sensed":
        sens = SM.SenseModel(B, seed)
        sens.set_params(**SL.noise(B))
        for _ in range(settle):
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
            r.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)        # the MPC's model: flat ground, mu 0.4
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
    assert (plant.stats["n"] == ticks).all()
    psi = xyyaw[:, 2]
    d = plant.p[:, :2] - xyyaw[:, :2]
    travel = d[:, 0] * np.cos(psi) + d[:, 1] * np.sin(psi)
    return stats, dict(safe=m.safe.copy(), nwsr_max=nwsr_max, n_solves=n_solves, rc_bad=rc_bad, travel=travel, rows=rows,
                       support=plant.support.copy(), early=plant.early.copy(), late=plant.late.copy(),
                       slip=plant.slip.copy())
