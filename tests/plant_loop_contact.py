"""The closed loops of tests/plant_loop_terrain.py with contact decided by the ground -- TEST SIDE ONLY.

cpu_loop_contact(mode, path, ...) is plant_loop_terrain.walk -- plant_loop.closed_loop, the only copy of the tick -- on
tests/plant_model_contact.py's ContactPlantModel (include/qmpc_contact.h): the reference pipeline -- the controller's
restatements with the reference's
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

import plant_loop as L
import plant_loop_terrain as LT
import plant_model_contact as PCM
import sense_loop as SL

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


def set_contact(plant, flags):
    plant.set_contact(early=bool(flags & PCM.EARLY), late=bool(flags & PCM.LATE), slip=bool(flags & PCM.SLIP))


def cpu_loop_contact(mode, path, config=None, ticks=None, settle=SL.SETTLE, seed=SL.SEED, substeps=1):
    """-> (stats, info): plant_loop_terrain.cpu_loop_terrain's fields (per robot), plus early, late [16] (foot-ticks) and
    slip [16] (metres); config: walk_config() / ladder_config()."""
    cfg = walk_config() if config is None else config
    m, xyyaw = L.controller_for(mode)
    rows = rows_for(L.N_CMD, cfg["rise"])
    plant = PCM.ContactPlantModel(L.N_CMD, L.FREQ, cfg["mu"], substeps, xyyaw)   # init -> set_terrain -> set_contact -> reset
    plant.set_terrain(rows, clamp_swing=True, rebase_z=path == "state")
    set_contact(plant, cfg["flags"])
    plant.reset(np.ones(L.N_CMD, bool), xyyaw)
    stats, info = LT.walk(m, plant, xyyaw, path, TICKS if ticks is None else ticks, settle, seed)
    return stats, dict(info, rows=rows, support=plant.support.copy(), early=plant.early.copy(), late=plant.late.copy(),
                       slip=plant.slip.copy())


