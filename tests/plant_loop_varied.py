"""The closed loop of tests/plant_loop.py on a plant the controller was not told about -- TEST SIDE ONLY.

variation(B) is the single definition of the walk's disturbance (include/qmpc_plant_vary.h): per robot a payload
(mass and inertia scaled together), another floor, and a 30 N shove in the side for a tenth of a second.  The controller
and the oracle keep the MPC's model: 9 kg, mu 0.4.  cpu_loop_varied() is plant_loop.cpu_loop with that plant;
tests/golden/make_plant_varied_closed_loop.py records its statistics, tests/test_gpu_plant_varied.py holds the GPU loop
to them by plant_loop.envelope().
"""
import numpy as np

from oracle import oracle as O

import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_loop as L
import plant_model_varied as PV
from ctrl_model_state import estimate_state

f32 = np.float32
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


def cpu_loop_varied(mode, ticks=L.TICKS, substeps=1, mu=0.4):
    """plant_loop.cpu_loop on the varied plant -> (stats, info): the same fields."""
    gait, vel, xyyaw = L.commands(mode)
    B = L.N_CMD
    var = variation(B)
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(B, L.FREQ, L.PID)
    m.set_gait(gait)
    m.set_vel(vel)
    plant = PV.VariedPlantModel(B, L.FREQ, mu, substeps, xyyaw, mass_b=var["mass"], ibody_b=var["ibody"], mu_b=var["mu"],
                                force=var["force"](0), torque=var["torque"])
    rec = L.Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    nwsr_max, n_solves, rc_bad = 0, 0, 0
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
            r.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)        # the MPC's model: not the plant's floor
            soln, nwsr, rc = O.solve_batch(r)
            rc_bad += int((rc != 0).sum())
            nwsr_max = max(nwsr_max, int(nwsr.max()))
            n_solves += len(due)
            m.f_ff[due] = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(f32))
        eff = m.legcmd(e, m.f_ff)
        plant.force = var["force"](t)
        plant.step(eff, m.contact_state, m.p_des, m.v_des)
        rec.add(plant.state)
    stats = rec.stats()
    # the model's own accumulators are the Recorder's extremes without the initial state
    s = plant.stats
    assert (s["n"] == ticks).all() and np.array_equal(np.minimum(s["z_min"], L.PM.HEIGHT), stats["z_min"])
    return stats, dict(safe=m.safe.copy(), nwsr_max=nwsr_max, n_solves=n_solves, rc_bad=rc_bad)
