"""Records the CPU closed loop's statistics on the varied plant (tests/golden/plant_varied_closed_loop_cpu.json):

    python tests/golden/make_plant_varied_closed_loop.py

tests/plant_loop_varied.py: cpu_loop_varied() is plant_loop.cpu_loop() -- the controller's numpy restatements and the
reference's own qpOASES for every solve, 16 robots, 650 ticks, robot modes 0 and 1, the commands of plant_loop.commands()
-- on the plant of tests/plant_model_varied.py with the disturbance of plant_loop_varied.variation(): per-robot payload,
floor friction and a lateral push the controller is not told about.  Recorded only if the reference pipeline keeps every
robot safe (safe == 1, every solve below the reference's nWSR cap of 100, qpOASES return code 0): the rule of
make_plant_closed_loop.py.  The same fields as that fixture, plus the variation.  The GPU loop of
tests/test_gpu_plant_varied.py is held to these numbers by plant_loop.envelope().
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plant_loop as L  # noqa: E402
import plant_loop_varied as LV  # noqa: E402


def main():
    var = LV.variation(L.N_CMD)
    out = {"ticks": L.TICKS, "freq": L.FREQ, "pid": list(L.PID),
           "variation": dict(mass=var["mass"].tolist(), ibody=var["ibody"].tolist(), mu=var["mu"].tolist(),
                             push=var["push"].tolist(), push_ticks=list(var["push_ticks"]), torque=var["torque"].tolist())}
    for mode in (0, 1):
        stats, info = LV.cpu_loop_varied(mode)
        assert (info["safe"] == 1).all() and info["nwsr_max"] < 100 and info["rc_bad"] == 0, (mode, info)
        gait, vel, xyyaw = L.commands(mode)
        out[f"mode{mode}"] = dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist(), n_solves=info["n_solves"],
                                  nwsr_max=info["nwsr_max"], **{k: [float(x) for x in stats[k]] for k in L.STATS})
    with open(os.path.join(ROOT, "tests", "golden", "plant_varied_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
