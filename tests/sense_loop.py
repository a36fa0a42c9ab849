"""The closed loop controller <-> plant THROUGH THE SENSOR PATH on the CPU -- TEST SIDE ONLY.

cpu_loop_sensed() is plant_loop.cpu_loop with the sensor model (tests/sense_model.py) between the plant and the
controller and CtrlModel.estimate -- the VectorNav orientation estimator and the Kalman filter -- in place of the cheater
estimators: sense -> estimate -> control -> plant step, in the order of binding.rollout_sensed.  The filter starts at
xhat = 0, P = 100 I while the body stands at 0.29 m, so the loop is preceded by SETTLE pre_work calls on the standing
plant (the reference's own protocol: init_controller, pre_work ..., then torques); without them most of the fleet falls.
noise(B) is the single definition of the imperfect sensors the closed-loop tests walk on.
tests/golden/make_sense_closed_loop.py records the statistics; tests/test_gpu_sense.py holds the GPU loop (library
controller + device plant + device sensors) to them by plant_loop.envelope().
"""
import numpy as np

from oracle import oracle as O

import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_loop as L
import plant_model as PM
import sense_model as SM

f32 = np.float32
SETTLE = 50
SEED = 0                     # the noise stream's seed (qmpc_sense_init)
BIAS_SEED = 20240           # numpy seed of the per-robot biases, drawn once
ACC_BIAS, ACC_SIGMA = 0.2, 0.3        # m/s^2: bias uniform in +-0.2, white noise sigma 0.3
GYRO_BIAS, GYRO_SIGMA = 0.02, 0.02    # rad/s
Q_SIGMA, QD_SIGMA = 0.002, 0.05       # rad, rad/s


def noise(B):
    """-> qmpc_sense_params' six arrays for B robots (robot b's values depend on b % 16 only)."""
    rng = np.random.default_rng(BIAS_SEED)
    k = np.arange(B) % L.N_CMD
    ab, gb = rng.uniform(-ACC_BIAS, ACC_BIAS, (L.N_CMD, 3)), rng.uniform(-GYRO_BIAS, GYRO_BIAS, (L.N_CMD, 3))
    return dict(acc_bias=ab[k], gyro_bias=gb[k], acc_sigma=np.full(B, ACC_SIGMA), gyro_sigma=np.full(B, GYRO_SIGMA),
                q_sigma=np.full(B, Q_SIGMA), qd_sigma=np.full(B, QD_SIGMA))


def cpu_loop_sensed(mode, noisy, ticks=L.TICKS, settle=SETTLE, seed=SEED, substeps=1, mu=0.4):
    """-> (stats, info): plant_loop.cpu_loop's fields, plus the filter's final height error in info."""
    gait, vel, xyyaw = L.commands(mode)
    B = L.N_CMD
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(B, L.FREQ, L.PID)
    m.set_gait(gait)
    m.set_vel(vel)
    plant = PM.PlantModel(B, L.FREQ, mu, substeps, xyyaw)
    sens = SM.SenseModel(B, seed)
    if noisy:
        sens.set_params(**noise(B))
    rec = L.Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    for _ in range(max(settle, 1)):                   # BatchedSensors.settle: sense -> pre_work on the standing plant
        imu, motor = sens.sense(plant.state, plant.motor)
        if settle:
            m.estimate(imu, motor)
    nwsr_max, n_solves, rc_bad = 0, 0, 0
    for t in range(ticks):
        e = m.estimate(imu, motor)
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
            m.f_ff[due] = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(f32))
        eff = m.legcmd(e, m.f_ff)
        z_seen = plant.p[:, 2].copy()                 # the height the estimate of this tick was about
        plant.step(eff, m.contact_state, m.p_des, m.v_des)
        rec.add(plant.state)
        imu, motor = sens.sense(plant.state, plant.motor)
    z_err = float(np.abs(e["position"][:, 2].astype(np.float64) - z_seen).max())
    return rec.stats(), dict(safe=m.safe.copy(), nwsr_max=nwsr_max, n_solves=n_solves, rc_bad=rc_bad, z_err=z_err,
                             sense_n=sens.n.copy())

