"""Records the CPU closed loop's statistics through the sensor path (tests/golden/sense_closed_loop_cpu.json):

    python tests/golden/make_sense_closed_loop.py

tests/sense_loop.py: cpu_loop_sensed() is plant_loop.cpu_loop() -- the controller's numpy restatements and the
reference's own qpOASES for every solve, 16 robots, 650 ticks, robot modes 0 and 1, the commands of plant_loop.commands()
-- with the sensor model of tests/sense_model.py between the plant and CtrlModel.estimate (VectorNav orientation
estimator + Kalman filter), after sense_loop.SETTLE pre_work calls on the standing plant.  Both sensors are recorded:
"ideal" (nothing bound) and "noisy" (sense_loop.noise(): per-robot accelerometer and gyro bias, white noise on the
accelerometer, the gyro and the encoders).  Recorded only if the reference pipeline keeps every robot safe (safe == 1,
every solve below the reference's nWSR cap of 100, qpOASES return code 0): the rule of make_plant_closed_loop.py.  The
same fields as that fixture, plus the noise.  The GPU loop of tests/test_gpu_sense.py is held to the noisy numbers by
plant_loop.envelope().
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plant_loop as L  # noqa: E402
import sense_loop as SL  # noqa: E402


def main():
    out = {"ticks": L.TICKS, "freq": L.FREQ, "pid": list(L.PID), "settle": SL.SETTLE, "seed": SL.SEED,
           "noise": {k: v.tolist() for k, v in SL.noise(L.N_CMD).items()}}
    for mode in (0, 1):
        gait, vel, xyyaw = L.commands(mode)
        rec = dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist())
        for name, noisy in (("ideal", False), ("noisy", True)):
            stats, info = SL.cpu_loop_sensed(mode, noisy)
            assert (info["safe"] == 1).all() and info["nwsr_max"] < 100 and info["rc_bad"] == 0, (mode, name, info)
            rec[name] = dict(n_solves=info["n_solves"], nwsr_max=info["nwsr_max"], z_err=info["z_err"],
                             **{k: [float(x) for x in stats[k]] for k in L.STATS})
        out[f"mode{mode}"] = rec
    with open(os.path.join(ROOT, "tests", "golden", "sense_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
