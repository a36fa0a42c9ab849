"""The closed loop of tests/plant_loop.py on a plant the controller was not told about -- TEST SIDE ONLY.

variation(B) is the single definition of the walk's disturbance (include/qmpc_plant_vary.h): per robot a payload
(mass and inertia scaled together), another floor, and a 30 N shove in the side for a tenth of a second.  The controller
and the oracle keep the MPC's model: 9 kg, mu 0.4.  cpu_loop_varied() is plant_loop.closed_loop (the only copy of the
tick) on that plant, the push set before every step; tests/golden/make_plant_varied_closed_loop.py records its
statistics, tests/test_gpu_plant_varied.py holds the GPU loop to them by plant_loop.envelope().
"""
import numpy as np

import plant_loop as L
import plant_model_varied as PV

SCALES = (0.8, 1.0, 1.2, 1.4)
MUS = (0.3, 0.4, 0.6, 0.8)
PUSH_N = 30.0
PUSH_TICKS = (300, 350)          # ticks 300 .. 349


def variation(B, push_ticks=PUSH_TICKS):
    """-> dict(mass [B], ibody [B,3], mu [B], torque [B,3], push [B,3], push_ticks, force(t) -> [B,3]): the force is
    `push` while push_ticks[0] <= t < push_ticks[1] (t: the index of the tick whose step feels it) and zero otherwise."""
    k = np.arange(B) % 16
    scale = np.array(SCALES)[(k // 4) % 4]
    push = np.zeros((B, 3))
    push[:, 1] = np.where(k % 2 == 1, PUSH_N, -PUSH_N)
    zero = np.zeros((B, 3))
    return dict(mass=9.0 * scale, ibody=np.array([0.07, 0.26, 0.242])[None, :] * scale[:, None], mu=np.array(MUS)[k % 4],
                torque=np.zeros((B, 3)), push=push, push_ticks=tuple(push_ticks), scale=scale,
                force=lambda t: push if push_ticks[0] <= t < push_ticks[1] else zero)


def cpu_loop_varied(mode, ticks=L.TICKS, substeps=1, mu=0.4, each_tick=None):
    """plant_loop.cpu_loop on the varied plant -> (stats, info): the same fields.  each_tick(t, plant): called before the
    step of tick t, after the tick's push is in place."""
    var = variation(L.N_CMD)
    m, xyyaw = L.controller_for(mode)
    plant = PV.VariedPlantModel(L.N_CMD, L.FREQ, mu, substeps, xyyaw, mass_b=var["mass"], ibody_b=var["ibody"],
                                mu_b=var["mu"], force=var["force"](0), torque=var["torque"])

    def push(t, plant):
        plant.force = var["force"](t)
        if each_tick is not None:
            each_tick(t, plant)

    stats, info = L.closed_loop(m, plant, ticks, each_tick=push)
    # the model's own accumulators are the Recorder's extremes without the initial state
    s = plant.stats
    assert (s["n"] == ticks).all() and np.array_equal(np.minimum(s["z_min"], L.PM.HEIGHT), stats["z_min"])
    return stats, L.scalars(info)


