"""plant_loop.cpu_loop with the actuator stage of include/qmpc_act.h between the controller and the plant -- TEST SIDE
ONLY.  tests/golden/make_act_closed_loop.py records its ladders; tests/test_act_cpu.py reads them and re-runs a prefix,
tests/test_gpu_act.py holds the GPU fleet to the walking rungs by plant_loop.envelope().
"""
import numpy as np

from oracle import oracle as O

import act_model as AM
import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_loop as L
import plant_model as PM
from ctrl_model_state import estimate_state

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
    gait, vel, xyyaw = L.commands(mode)
    B = L.N_CMD
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(B, L.FREQ, L.PID)
    m.set_gait(gait)
    m.set_vel(vel)
    plant = PM.PlantModel(B, L.FREQ, 0.4, 1, xyyaw)
    act = model_for(B, actuator)
    rec = L.Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    nwsr_max, n_solves, rc_bad, states = 0, 0, 0, []
    for t in range(ticks):
        state, motor = plant.state, plant.motor
        e = estimate_state(m, state, motor)
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
            r.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)
            soln, nwsr, rc = O.solve_batch(r)
            rc_bad += int((rc != 0).sum())
            nwsr_max = max(nwsr_max, int(nwsr.max()))
            n_solves += len(due)
            m.f_ff[due] = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(np.float32))
        eff = m.legcmd(e, m.f_ff)
        eff = act.apply(eff, np.asarray(motor, np.float64)[:, 12:24])
        plant.step(eff, m.contact_state, m.p_des, m.v_des)
        rec.add(plant.state)
        if trace:
            states.append(np.asarray(plant.state, np.float64).copy())
    info = dict(safe=m.safe.copy(), nwsr_max=nwsr_max, n_solves=n_solves, rc_bad=rc_bad,
                counters={k: act.acc[k].copy() for k in COUNTERS})
    if trace:
        info["states"] = np.stack(states)
    return rec.stats(), info
