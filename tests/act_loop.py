"""plant_loop.cpu_loop with the actuator stage of include/qmpc_act.h between the controller and the plant -- TEST SIDE
ONLY: plant_loop.closed_loop (the only copy of the tick) with `actuators`.  tests/golden/make_act_closed_loop.py records
its ladders; tests/test_act_cpu.py reads them and re-runs a prefix, tests/test_gpu_act.py holds the GPU fleet to the
walking rungs by plant_loop.envelope().
"""
import numpy as np

import act_model as AM
import plant_loop as L
import plant_model as PM

COUNTERS = AM.ACCUMULATORS
# the rungs of the recorded ladders: (name, actuator arguments); `delay` is every robot's latency in ticks
LADDERS = {
    "default": [("default", {})],
    "tau_max": [(f"tau_max_{v}", dict(tau_max=v)) for v in (1.5, 1.25, 1.0, 0.75)],
    "delay": [(f"delay_{d}", dict(delay=d)) for d in (8, 12, 16)],
    "battery_v": [(f"battery_v_{v}", dict(battery_v=v)) for v in (4.0, 2.0, 1.0)],
}


def model_for(B, actuator):
    """The ActModel of a rung: `delay` is bound for every robot (max_delay = the delay), the rest goes into the config."""
    actuator = dict(actuator)
    delay = int(actuator.pop("delay", 0))
    m = AM.ActModel(B, 1.0 / L.FREQ, dict(actuator, max_delay=delay))
    if delay:
        m.set_params(delay=np.full(B, delay, np.int32))
    return m


def cpu_loop_act(mode, ticks=L.TICKS, trace=False, **actuator):
    """plant_loop.cpu_loop(mode) with the motor, the latency and the accumulators in the loop
    -> (stats, info): info holds safe [B], the counters and, with trace, the state after every tick."""
    m, xyyaw = L.controller_for(mode)
    plant = PM.PlantModel(L.N_CMD, L.FREQ, 0.4, 1, xyyaw)
    states = []

    def record(t, plant):                              # (called before the step: the state after tick t - 1)
        if t:
            states.append(np.asarray(plant.state, np.float64).copy())

    stats, info = L.closed_loop(m, plant, ticks, actuators=model_for(L.N_CMD, actuator), each_tick=record if trace else None)
    out = dict(L.scalars(info), counters={k: info["actuators"].acc[k].copy() for k in COUNTERS})
    if trace:
        out["states"] = np.stack(states + [np.asarray(plant.state, np.float64).copy()])
    return stats, out


