"""Records the CPU closed loop's statistics as a fixture (tests/golden/plant_closed_loop_cpu.json):

    python tests/golden/make_plant_closed_loop.py

tests/plant_loop.py: cpu_loop() runs the numpy plant (tests/plant_model.py) against the reference pipeline -- the
controller's numpy restatements and the reference's own qpOASES for every solve -- 16 robots, 650 ticks, robot modes 0
and 1, on the command set of plant_loop.commands().  A command set is only recorded if the reference pipeline keeps
every robot safe on it (safe == 1, every solve below the reference's nWSR cap of 100, qpOASES return code 0).  Per robot:
minimum / maximum body height, maximum |roll| and |pitch|, mean forward speed over the last second.  The GPU loop of
tests/test_gpu_plant.py is held to these numbers by plant_loop.envelope().
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plant_loop as L  # noqa: E402


def main():
    out = {"ticks": L.TICKS, "freq": L.FREQ, "pid": list(L.PID)}
    for mode in (0, 1):
        stats, info = L.cpu_loop(mode)
        assert (info["safe"] == 1).all() and info["nwsr_max"] < 100 and info["rc_bad"] == 0, (mode, info)
        gait, vel, xyyaw = L.commands(mode)
        out[f"mode{mode}"] = dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist(), n_solves=info["n_solves"],
                                  nwsr_max=info["nwsr_max"], **{k: [float(x) for x in stats[k]] for k in L.STATS})
    with open(os.path.join(ROOT, "tests", "golden", "plant_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
