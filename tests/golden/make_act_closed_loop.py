"""Records the CPU closed loop with the actuator stage as a fixture (tests/golden/act_closed_loop_cpu.json):

    python tests/golden/make_act_closed_loop.py

tests/act_loop.py: cpu_loop_act() is plant_loop.cpu_loop() -- the numpy plant against the controller's numpy
restatements and the reference's own qpOASES, 16 robots, 650 ticks, robot modes 0 and 1 -- with tests/act_model.py (the
reference's ActuatorModel::getTorque, a command latency, the accumulators of include/qmpc_act.h) between the
controller's effort and the plant.  Recorded per mode: the Mini Cheetah's motor, and three ladders that each run from a
rung on which all 16 robots stay safe to one on which the reference pipeline loses robots -- the motor-side torque cap,
the latency in ticks, the battery voltage.  A rung holds plant_loop.STATS per robot, the safe flags and their count, the
accumulators, and `walks` (16 of 16 safe).  `prefix` is one rung cut at 130 ticks, state and accumulators, which
tests/test_act_cpu.py runs again.  The GPU fleet of tests/test_gpu_act.py is held to the walking rungs by
plant_loop.envelope(); the falling rungs are asserted on the CPU only.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import act_loop as AL  # noqa: E402
import act_model as AM  # noqa: E402
import plant_loop as L  # noqa: E402

PREFIX_RUNG, PREFIX_TICKS = ("delay", "delay_8"), 130


def rung(mode, actuator, ticks=L.TICKS, trace=False):
    stats, info = AL.cpu_loop_act(mode, ticks=ticks, trace=trace, **actuator)
    row = dict(actuator=actuator, safe=[int(x) for x in info["safe"]], safe_count=int((info["safe"] == 1).sum()),
               nwsr_max=info["nwsr_max"], rc_bad=info["rc_bad"], n_solves=info["n_solves"],
               counters={k: [float(x) if v.dtype.kind == "f" else int(x) for x in v] for k, v in info["counters"].items()},
               **{k: [float(x) for x in stats[k]] for k in L.STATS})
    row["walks"] = row["safe_count"] == L.N_CMD
    return row, info


def main():
    out = {"ticks": L.TICKS, "freq": L.FREQ, "pid": list(L.PID), "config": AM.config(),
           "prefix_rung": list(PREFIX_RUNG), "prefix_ticks": PREFIX_TICKS}
    for mode in (0, 1):
        gait, vel, xyyaw = L.commands(mode)
        rec = dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist(), ladders={})
        for name, rungs in AL.LADDERS.items():
            rec["ladders"][name] = {}
            for rname, actuator in rungs:
                row, info = rung(mode, actuator, trace=(name, rname) == PREFIX_RUNG)
                rec["ladders"][name][rname] = row
                print(mode, rname, "safe", row["safe_count"], "z_min %.3f roll %.3f pitch %.3f" % (
                    np.nanmin(row["z_min"]), np.nanmax(row["roll_max"]), np.nanmax(row["pitch_max"])),
                    "n_vsat", sum(row["counters"]["n_vsat"]), "n_tsat", sum(row["counters"]["n_tsat"]), flush=True)
                if (name, rname) == PREFIX_RUNG:
                    short, sinfo = rung(mode, actuator, ticks=PREFIX_TICKS, trace=True)
                    # the short run IS the long run's prefix
                    assert np.array_equal(sinfo["states"][-1], info["states"][PREFIX_TICKS - 1], equal_nan=True)
                    rec["prefix"] = dict(state=sinfo["states"][-1].tolist(), counters=short["counters"], safe=short["safe"])
        out[f"mode{mode}"] = rec
    with open(os.path.join(ROOT, "tests", "golden", "act_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
