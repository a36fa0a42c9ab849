"""Climbs the height-field ladder with the CPU closed loop and records what it found
(tests/golden/plant_field_closed_loop_cpu.json):

    python tests/golden/make_plant_field_closed_loop.py [--jobs N]

tests/plant_loop_field.py: cpu_loop_field(mode, path, kind, amp) is the reference pipeline on the plant of
tests/plant_model_field.py (include/qmpc_field.h), 16 robots spread over one random_blocks map.  The amplitude ladder is
climbed twice -- with scheduled contact and with contact decided by the ground (EARLY | LATE | SLIP) -- and judged rung by
rung by the terrain rule: all 16 robots safe in both robot modes on both paths, every qpOASES return code 0 and nWSR < 100.
A climb ends at its first fallen rung: the rungs above it are run (all runs are independent and go to one pool) and
recorded under `beyond`, but they do not count.  Nothing about the model is tuned to move a rung; what the ladder shows is
the result.

The walk that is recorded per robot (and that tests/test_gpu_field.py repeats on the device) is the top walked rung of each
climb -- amplitude 0 where none was walked.  It has to pass the same rule, or nothing is written.
plant_loop_field.RUNGS must then be set to what the file says; tests/test_field_cpu.py holds the two together.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plant_loop as L  # noqa: E402
import plant_loop_field as LF  # noqa: E402

RUNS = [(mode, path) for mode in (0, 1) for path in LF.PATHS]


def ok_per_robot(info):
    return (info["safe"].reshape(-1) == 1) & (info["rc_bad"] == 0) & (info["nwsr_max"] < 100)


def per_robot(stats, info):
    return dict(ok=ok_per_robot(info).tolist(), n_solves=int(info["n_solves"]), nwsr_max=int(info["nwsr_max"].max()),
                travel=[float(x) for x in info["travel"]], early=[int(x) for x in info["early"]],
                late=[int(x) for x in info["late"]], slip=[float(x) for x in info["slip"]],
                support=[float(x) for x in info["support"]],
                **{k: [float(x) for x in stats[k]] for k in L.STATS})


def run(task):
    kind, amp, mode, path = task
    stats, info = LF.cpu_loop_field(mode, path, kind, amp)
    return kind, amp, mode, path, per_robot(stats, info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    tasks = [(kind, amp, mode, path) for kind in LF.KINDS for amp in LF.LADDER for mode, path in RUNS]
    with mp.Pool(args.jobs) as pool:
        res = pool.map(run, tasks, chunksize=1)
        by = {}
        for kind, amp, mode, path, rec in res:
            by.setdefault((kind, amp), {})[f"mode{mode}_{path}"] = rec
        ladders, rungs = {}, {}
        for kind in LF.KINDS:
            walked, fell, beyond, top = [], None, [], None
            for amp in LF.LADDER:
                runs = by[(kind, amp)]
                good = all(all(r["ok"]) for r in runs.values())
                summary = dict(rung=amp, walked=good, runs={
                    k: dict(fallen=[b for b, o in enumerate(r["ok"]) if not o], nwsr_max=r["nwsr_max"],
                            z_min=float(np.min(r["z_min"])), roll_max=float(np.max(r["roll_max"])),
                            pitch_max=float(np.max(r["pitch_max"])), early=int(np.sum(r["early"])),
                            late=int(np.sum(r["late"])), slip=float(np.sum(r["slip"])))
                    for k, r in runs.items()})
                if fell is not None:
                    beyond.append(summary)
                elif good:
                    walked.append(summary)
                    top = amp
                else:
                    fell = summary
            ladders[kind] = dict(rungs=list(LF.LADDER), walked=walked, fell=fell, beyond=beyond)
            rungs[kind] = top
            print(kind, "walked:", [w["rung"] for w in walked], "fell at:", None if fell is None else fell["rung"],
                  "beyond:", [(w["rung"], w["walked"]) for w in beyond])
        out = {"ticks": LF.TICKS, "freq": L.FREQ, "pid": list(L.PID), "settle": LF.SL.SETTLE, "seed": LF.SL.SEED,
               "map": dict(n=LF.N_MAP, block=LF.BLOCK, cell=LF.CELL, seed=LF.MAP_SEED), "ladders": ladders, "rungs": rungs,
               "place": LF.field_for(L.N_CMD, 0.0)[1].tolist(), "walk": {}}
        fin = pool.map(run, [(kind, rungs[kind] or 0.0, mode, path) for kind in LF.KINDS for mode, path in RUNS],
                       chunksize=1)
        for kind, amp, mode, path, rec in fin:
            assert all(rec["ok"]), ("the walk falls", kind, mode, path, rec)
            gait, vel, xyyaw = L.commands(mode)
            out["walk"].setdefault(kind, dict(amp=amp)).setdefault(
                f"mode{mode}", dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist()))[path] = rec
    with open(os.path.join(ROOT, "tests", "golden", "plant_field_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("rungs:", rungs, "" if rungs == LF.RUNGS else "-- set plant_loop_field.RUNGS to this")


if __name__ == "__main__":
    main()
