"""Climbs the contact ladders with the CPU closed loop and records what it found
(tests/golden/plant_contact_closed_loop_cpu.json):

    python tests/golden/make_plant_contact_closed_loop.py [--jobs N]

tests/plant_loop_contact.py: cpu_loop_contact(mode, path, config) is the reference pipeline on the plant of
tests/plant_model_contact.py (include/qmpc_contact.h).  Three ladders -- flat ground, stairs up and down of run 0.1 m,
floor friction -- each judged rung by rung by the terrain rule: all 16 robots safe in both robot modes on both paths,
every qpOASES return code 0 and nWSR < 100.  A ladder ends at its first fallen rung: the rungs above it are run (all runs
are independent and go to one pool) and recorded under `beyond`, but they do not count.  Nothing about the model is tuned
to move a rung; what the ladders show is the result.

The walk that is recorded per robot (and that tests/test_gpu_contact.py repeats on the device) is
plant_loop_contact.walk_config() of the rungs found: the top walked stairs under EARLY | LATE | SLIP on the top walked
floor.  It has to pass the same rule, or nothing is written.  plant_loop_contact.RUNGS must then be set to what the file
says; tests/test_contact_cpu.py holds the two together.
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
import plant_loop_contact as LC  # noqa: E402

RUNS = [(mode, path) for mode in (0, 1) for path in LC.PATHS]
LADDERS = dict(flat=(True,), stairs=LC.STAIRS_LADDER, friction=LC.FRICTION_LADDER)


def ok_per_robot(info):
    return (info["safe"].reshape(-1) == 1) & (info["rc_bad"] == 0) & (info["nwsr_max"] < 100)


def per_robot(stats, info):
    return dict(ok=ok_per_robot(info).tolist(), n_solves=int(info["n_solves"]), nwsr_max=int(info["nwsr_max"].max()),
                travel=[float(x) for x in info["travel"]], early=[int(x) for x in info["early"]],
                late=[int(x) for x in info["late"]], slip=[float(x) for x in info["slip"]],
                **{k: [float(x) for x in stats[k]] for k in L.STATS})


def run(task):
    ladder, rung, mode, path, cfg = task
    stats, info = LC.cpu_loop_contact(mode, path, cfg)
    return ladder, rung, mode, path, per_robot(stats, info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    tasks = [(name, rung, mode, path, LC.ladder_config(name, rung)) for name, lad in LADDERS.items() for rung in lad
             for mode, path in RUNS]
    with mp.Pool(args.jobs) as pool:
        res = pool.map(run, tasks, chunksize=1)
        by = {}
        for ladder, rung, mode, path, rec in res:
            by.setdefault((ladder, rung), {})[f"mode{mode}_{path}"] = rec
        ladders, rungs = {}, {}
        for name, lad in LADDERS.items():
            walked, fell, beyond, top = [], None, [], None
            for rung in lad:
                runs = by[(name, rung)]
                good = all(all(r["ok"]) for r in runs.values())
                summary = dict(rung=rung, walked=good, runs={
                    k: dict(fallen=[b for b, o in enumerate(r["ok"]) if not o], nwsr_max=r["nwsr_max"],
                            early=int(np.sum(r["early"])), late=int(np.sum(r["late"])), slip=float(np.sum(r["slip"])))
                    for k, r in runs.items()})
                if fell is not None:
                    beyond.append(summary)
                elif good:
                    walked.append(summary)
                    top = rung
                else:
                    fell = summary
            ladders[name] = dict(rungs=list(lad), walked=walked, fell=fell, beyond=beyond)
            rungs[name] = top
            print(name, "walked:", [w["rung"] for w in walked], "fell at:", None if fell is None else fell["rung"],
                  "beyond:", [(w["rung"], w["walked"]) for w in beyond])
        out = {"ticks": LC.TICKS, "freq": L.FREQ, "pid": list(L.PID), "settle": LC.SL.SETTLE, "seed": LC.SL.SEED,
               "run": LC.RUN, "ladders": ladders, "rungs": rungs,
               "top": {name: (None if rungs[name] is None else by[(name, rungs[name])]) for name in LADDERS}}
        if rungs["flat"]:
            cfg = LC.walk_config(rungs)
            fin = pool.map(run, [("walk", None, mode, path, cfg) for mode, path in RUNS], chunksize=1)
            out["walk"] = dict(config=cfg, rows=LC.rows_for(L.N_CMD, cfg["rise"]).tolist())
            for _, _, mode, path, rec in fin:
                assert all(rec["ok"]), ("the walk falls", mode, path, rec)
                gait, vel, xyyaw = L.commands(mode)
                out.setdefault(f"mode{mode}", dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist()))[path] = rec
    with open(os.path.join(ROOT, "tests", "golden", "plant_contact_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("rungs:", rungs, "" if rungs == LC.RUNGS else "-- set plant_loop_contact.RUNGS to this")


if __name__ == "__main__":
    main()
