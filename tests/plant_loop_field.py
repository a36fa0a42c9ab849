"""The closed loops of tests/plant_loop_terrain.py and tests/plant_loop_contact.py on height-field terrain from memory --
TEST SIDE ONLY.

field_for(B, amp) is the single definition of the rough ground the closed-loop tests walk on (include/qmpc_field.h): one
map of quadruped_ctrl_amd.workloads.random_blocks -- the recipe of the reference simulation's `random1`: 256 x 256 samples
on 0.05 m cells, every 2 x 2 block one height from uniform(0, amp) -- shared by the fleet, robot b placed on it through
k = b % 16: its start position (plant_loop.commands()) lies at map point (2 + 2.9 (k % 4), 2 + 2.9 (k // 4)) m, so the 16
robots walk 16 different patches.  No terrain rows are bound; the field binding carries clamp_swing (and rebase_z on the
state path).  The controller and the MPC are not told.

The ladder (tests/golden/make_plant_field_closed_loop.py climbs it) starts at the reference's own amplitudes 0.02, 0.04,
0.06 m and goes on to 0.10 and 0.15.  It is climbed twice: with scheduled contact, and with contact decided by the ground
(EARLY | LATE | SLIP).  A rung counts when every robot is safe in both robot modes on both paths with every qpOASES return
code 0 and nWSR < 100; each climb stops at its first fallen rung.  RUNGS is the MEASURED record: the top walked rung of each
climb, None when even the first fell -- that combination's walk then runs at amplitude 0 (an all-zero map).  Nothing about
the plant is tuned to move a rung.

cpu_loop_field() is plant_loop_terrain.walk -- plant_loop.closed_loop, the only copy of the tick -- on FieldPlantModel.
"""
import numpy as np

from quadruped_ctrl_amd import workloads as W

import plant_loop as L
import plant_loop_contact as LC
import plant_loop_terrain as LT
import plant_model_contact as PCM
import plant_model_field as PF
import sense_loop as SL

PATHS = LT.PATHS
KINDS = ("scheduled", "contact")
LADDER = (0.02, 0.04, 0.06, 0.10, 0.15)
N_MAP, BLOCK, CELL, MAP_SEED = 256, 2, 0.05, 20260
TICKS = 1300
# the measured record (tests/golden/plant_field_closed_loop_cpu.json; tests/test_field_cpu.py holds it to the file)
RUNGS = dict(scheduled=0.02, contact=0.04)      # scheduled contact fell at 0.04 m, contact on at 0.06 m


def field_for(B, amp):
    """-> (z [1, 256, 256] float32, place [B, 4] float64, cell); amp None or 0: the all-zero map."""
    z = W.random_blocks(MAP_SEED, N_MAP, BLOCK, amp or 0.0)[None]
    _, _, xyyaw = L.commands(0)                      # (the start poses are the same in both robot modes)
    k = np.arange(B) % L.N_CMD
    place = np.zeros((B, 4))
    place[:, 1] = xyyaw[k, 0] - (2.0 + 2.9 * (k % 4))
    place[:, 2] = xyyaw[k, 1] - (2.0 + 2.9 * (k // 4))
    place[:, 3] = 1.0
    return np.ascontiguousarray(z), place, CELL


def contact_flags(kind):
    return PCM.EARLY | PCM.LATE | PCM.SLIP if kind == "contact" else 0


def cpu_loop_field(mode, path, kind, amp="rung", ticks=None, settle=SL.SETTLE, seed=SL.SEED, substeps=1, mu=0.4,
                   plant=None):
    """-> (stats, info): plant_loop_contact.cpu_loop_contact's fields on FieldPlantModel; amp "rung": RUNGS[kind].
    plant: walk THIS plant model (bound, set and reset by the caller) instead; info["plant"] is the plant walked."""
    assert kind in KINDS
    amp = RUNGS[kind] if isinstance(amp, str) else amp
    m, xyyaw = L.controller_for(mode)
    if plant is None:
        z, place, cell = field_for(L.N_CMD, amp)
        plant = PF.FieldPlantModel(L.N_CMD, L.FREQ, mu, substeps, xyyaw)       # init -> set_field -> set_contact -> reset
        plant.set_field(z, place, cell, clamp_swing=True, rebase_z=path == "state")
        LC.set_contact(plant, contact_flags(kind))
        plant.reset(np.ones(L.N_CMD, bool), xyyaw)
    stats, info = LT.walk(m, plant, xyyaw, path, TICKS if ticks is None else ticks, settle, seed)
    return stats, dict(info, support=plant.support.copy(), ground=plant.ground.copy(), early=plant.early.copy(),
                       late=plant.late.copy(), slip=plant.slip.copy(), plant=plant)


