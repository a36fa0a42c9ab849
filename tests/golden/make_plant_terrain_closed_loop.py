"""Climbs the terrain ladders with the CPU closed loop and records what it found
(tests/golden/plant_terrain_closed_loop_cpu.json):

    python tests/golden/make_plant_terrain_closed_loop.py [--jobs N]

tests/plant_loop_terrain.py: cpu_loop_terrain(mode, path) is the reference pipeline -- the controller's numpy restatements
and the reference's own qpOASES for every solve, 16 robots, the commands of plant_loop.commands() -- on the plant of
tests/plant_model_terrain.py, through the cheater estimators with the re-based height (path "state") and through the
sensor model with sense_loop.noise() and the Kalman filter (path "sensed"), swing feet clamped to the surface on both.

Nobody had run this controller on this plant on a slope, so the amplitudes are measured here.  Level j of the climb gives
every kind rung j of its own ladder (plant_loop_terrain.LADDERS; the slopes' ladder is shorter and is not climbed past its
end).  The 16 robots of the CPU loop are independent of one another -- one numpy row and one qpOASES problem each -- so a
kind's rung is judged by that kind's four robots: safe in both robot modes on both paths, every qpOASES return code 0 and
nWSR < 100.  The choice is the largest safe rung of each kind (None when even the first falls: that kind's robots then
walk on flat rows, and the finding is recorded).  The reference's own 0.01 m stairs must be among the walked rungs, or
nothing is written.  The chosen combination is then run once more as a whole and recorded only if all 16 robots pass the
same rule; plant_loop_terrain.RUNGS must be what was found (the generator says so and refuses to write otherwise).

The tick count is plant_loop_terrain.TICKS = 1300 for every run, the cap, fixed before the climb so that every rung is
judged on the same walk: the fastest third of the robots that move on stairs (0.4 and 0.47 m/s, two of seven) has to
leave its flight, which ends 0.9 m ahead of the start when the run is 0.2 m -- about 1100 ticks for the slower of the two.
`left_flight` records who did on the chosen rungs, and the fastest third must be among them or nothing is written.
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
import plant_loop_terrain as LT  # noqa: E402

RUNS = [(mode, path) for mode in (0, 1) for path in LT.PATHS]


def level_rungs(j):
    return {k: (lad[j] if j < len(lad) else None) for k, lad in LT.LADDERS.items()}


def ok_per_robot(info):
    return (info["safe"].reshape(-1) == 1) & (info["rc_bad"] == 0) & (info["nwsr_max"] < 100)


def climb(task):
    j, mode, path = task
    _, info = LT.cpu_loop_terrain(mode, path, rungs=level_rungs(j))
    return j, mode, path, ok_per_robot(info).tolist()


def final(task):
    mode, path, rungs = task
    stats, info = LT.cpu_loop_terrain(mode, path, rungs=rungs)
    return mode, path, {k: [float(x) for x in stats[k]] for k in L.STATS}, dict(
        ok=ok_per_robot(info).tolist(), n_solves=int(info["n_solves"]), nwsr_max=int(info["nwsr_max"].max()),
        travel=[float(x) for x in info["travel"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    levels = max(len(lad) for lad in LT.LADDERS.values())
    with mp.Pool(args.jobs) as pool:
        res = pool.map(climb, [(j, mode, path) for j in range(levels) for mode, path in RUNS], chunksize=1)
        kind_of = np.arange(L.N_CMD) % 4
        safe = {k: [True] * len(lad) for k, lad in LT.LADDERS.items()}
        detail = {}
        for j, mode, path, ok in res:
            for kind, name in enumerate(LT.KINDS):
                if j < len(LT.LADDERS[name]):
                    good = bool(np.asarray(ok)[kind_of == kind].all())
                    safe[name][j] = safe[name][j] and good
                    detail.setdefault(name, {}).setdefault(str(j), {})[f"mode{mode}_{path}"] = good
        chosen, fell = {}, {}
        for name, lad in LT.LADDERS.items():
            walked = [j for j in range(len(lad)) if safe[name][j]]
            chosen[name] = lad[walked[-1]] if walked else None
            fell[name] = [lad[j] for j in range(len(lad)) if not safe[name][j]]
            print(name, "safe:", [lad[j] for j in walked], "fell:", fell[name], "->", chosen[name])
        for name in ("stairs_up", "stairs_down"):
            assert safe[name][0], f"{name}: the reference's own 0.01 m stairs fall on the CPU -- nothing recorded"
        mine = {k: (None if v is None else (tuple(v) if isinstance(v, (tuple, list)) else v)) for k, v in LT.RUNGS.items()}
        assert mine == chosen, f"plant_loop_terrain.RUNGS is {mine}, the climb found {chosen}: set it and run again"
        fin = pool.map(final, [(mode, path, chosen) for mode, path in RUNS], chunksize=1)
    rows = LT.terrain(L.N_CMD, chosen)
    out = {"ticks": LT.TICKS, "freq": L.FREQ, "pid": list(L.PID), "settle": LT.SL.SETTLE, "seed": LT.SL.SEED,
           "kinds": list(LT.KINDS), "start": LT.START, "treads": LT.TREADS,
           "ladders": {k: [list(r) if isinstance(r, tuple) else r for r in lad] for k, lad in LT.LADDERS.items()},
           "rungs": {k: (list(v) if isinstance(v, tuple) else v) for k, v in chosen.items()},
           "walked": {k: [list(lad[j]) if isinstance(lad[j], tuple) else lad[j] for j in range(len(lad)) if safe[k][j]]
                      for k, lad in LT.LADDERS.items()},
           "fell": {k: [list(r) if isinstance(r, tuple) else r for r in v] for k, v in fell.items()},
           "climb": detail, "rows": rows.tolist()}
    end = np.where(rows[:, 5] > 0, LT.START + rows[:, 5] * rows[:, 4], np.inf)
    for mode, path, stats, info in fin:
        assert all(info["ok"]), (mode, path, info)
        gait, vel, xyyaw = L.commands(mode)
        left = (np.asarray(info["travel"]) > end).tolist()
        moving = np.flatnonzero((rows[:, 5] > 0) & (np.abs(vel[:, 0]) > 0))
        fastest = moving[np.argsort(-vel[moving, 0])][:len(moving) // 3]
        assert all(left[b] for b in fastest), (mode, path, fastest, info["travel"])
        out.setdefault(f"mode{mode}", dict(gait=gait.tolist(), vel=vel.tolist(), xyyaw=xyyaw.tolist()))[path] = dict(
            n_solves=info["n_solves"], nwsr_max=info["nwsr_max"], travel=info["travel"], left_flight=left, **stats)
    with open(os.path.join(ROOT, "tests", "golden", "plant_terrain_closed_loop_cpu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
