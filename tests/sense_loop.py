"""The closed loop controller <-> plant THROUGH THE SENSOR PATH on the CPU -- TEST SIDE ONLY.

cpu_loop_sensed() is plant_loop.closed_loop (the only copy of the tick) with the sensor model (tests/sense_model.py)
between the plant and the controller and CtrlModel.estimate -- the VectorNav orientation estimator and the Kalman filter
-- in place of the cheater estimators: sense -> estimate -> control -> plant step, in the order of
binding.rollout_sensed.  The filter starts at
xhat = 0, P = 100 I while the body stands at 0.29 m, so the loop is preceded by SETTLE pre_work calls on the standing
plant (the reference's own protocol: init_controller, pre_work ..., then torques); without them most of the fleet falls.
noise(B) is the single definition of the imperfect sensors the closed-loop tests walk on.
tests/golden/make_sense_closed_loop.py records the statistics; tests/test_gpu_sense.py holds the GPU loop (library
controller + device plant + device sensors) to them by plant_loop.envelope().
"""
import numpy as np

import plant_loop as L
import plant_model as PM
import sense_model as SM

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


def sensors_for(B, seed, noisy=True):
    """The sensor model of the closed-loop walks: seed `seed`, noise(B) bound unless noisy is False."""
    sens = SM.SenseModel(B, seed)
    if noisy:
        sens.set_params(**noise(B))
    return sens


def cpu_loop_sensed(mode, noisy, ticks=L.TICKS, settle=SETTLE, seed=SEED, substeps=1, mu=0.4):
    """-> (stats, info): plant_loop.cpu_loop's fields, plus the filter's final height error in info."""
    m, xyyaw = L.controller_for(mode)
    seen = {}

    def height(t, plant):
        seen["z"] = plant.p[:, 2].copy()              # the height the estimate of this tick was about

    stats, info = L.closed_loop(m, PM.PlantModel(L.N_CMD, L.FREQ, mu, substeps, xyyaw), ticks,
                                sensors=sensors_for(L.N_CMD, seed, noisy), settle=settle, each_tick=height)
    z_err = float(np.abs(info["estimate"]["position"][:, 2].astype(np.float64) - seen["z"]).max())
    return stats, dict(L.scalars(info), z_err=z_err, sense_n=info["sensors"].n.copy())


