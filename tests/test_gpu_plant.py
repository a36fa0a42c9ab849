"""GPU suite (-m gpu) for the reduced-order plant (include/qmpc_plant.h; BatchedPlant, rollout).

The kernel is compared with tests/plant_model.py (numpy float64, the same expressions in the same order) at 1e-10
relative to max(1, |x|) per output (fleet_gpu.TOL): about six orders above fp64 rounding of the chain, the device's atan2 /
sin / cos / sqrt included, far below any modelling difference.  The closed-loop walk is held to the CPU loop's recorded
statistics (tests/golden/plant_closed_loop_cpu.json) by plant_loop.envelope(); everything else compares two runs of the
library bit for bit.  The helpers (pair, dev, snap, close, compare, ...) and the bodies of the first two tests, which
tests/test_gpu_constants.py runs again at other constants, live in tests/fleet_gpu.py.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from quadruped_ctrl_amd import workloads as W

import fleet_gpu as G
import plant_loop as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANT_KEYS = G.PLANT_KEYS
_pair, _dev, _snap, _walk_setup = G.pair, G.dev, G.snap, G.walk_setup


@pytest.mark.parametrize("substeps", [1, 4])
def test_single_step_parity(substeps):
    """B = 257 (the last block is partial, 1028 lanes are no multiple of 64): random poses and joint states, every old
    and new stance pattern (both edges, all-swing, all-stance), a saturated cone, pulling legs, a near-straight knee, a
    swing command out of reach and a zero one."""
    G.single_step(substeps)


def test_teacher_forced_closed_loop():
    """64 robots, 40 ticks (three solves): at every tick the numpy plant is stepped from the device plant's previous
    state with the device's effort and controller view, and compared with the device's step."""
    G.teacher_forced_closed_loop(64, 40)


@pytest.mark.parametrize("mode", [0, 1])
def test_closed_loop_walk(mode):
    """The CPU yardstick's commands, four robots per command, 650 ticks, device controller + device plant: every robot
    stays safe, no solve reports an error bit, and per robot the height's extremes, the largest |roll| and |pitch| and
    the last second's mean forward speed lie inside the CPU run's recorded value for that command widened by twice the
    CPU run's own spread of the quantity over its 16 robots (plant_loop.envelope: the only source of the bounds)."""
    from quadruped_ctrl_amd.binding import rollout
    reps = 4
    B = L.N_CMD * reps
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_closed_loop_cpu.json")))
    rec = gold[f"mode{mode}"]
    gait, vel, xyyaw = _walk_setup(mode, reps)
    assert np.array_equal(rec["vel"], vel[:L.N_CMD]) and np.array_equal(rec["gait"], gait[:L.N_CMD])
    c, plant = _pair(B, "per_robot" if mode == 1 else "lockstep", mode if mode == 1 else None, xyyaw=xyyaw)
    c.set_gait(_dev(c, gait))
    c.set_vel(_dev(c, vel))
    r = L.Recorder(B, L.TICKS)
    r.add(plant.state.cpu().numpy(), initial=True)
    for t in range(L.TICKS):
        rollout(c, plant, 1)
        r.add(plant.state.cpu().numpy())
        assert (c.read("status")[:, 0] & 47 == 0).all(), t
    assert (c.read("safe") == 1).all()
    G.assert_inside_envelope(r.stats(), rec, reps, f"mode {mode}")
    c.close()


@pytest.mark.parametrize("schedule,ticks", [("lockstep", 26), ("per_robot", 5)])
def test_graph_capture_matches_eager(schedule, ticks):
    from quadruped_ctrl_amd.binding import QmpcError, rollout
    B = 64
    gait, vel, xyyaw = _walk_setup(0, 4)
    out = []
    for graph in (False, True):
        c, plant = _pair(B, schedule, xyyaw=xyyaw)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        rollout(c, plant, 13)                                        # an eager start: past the first solve
        if graph and schedule == "lockstep":
            with pytest.raises(QmpcError):
                rollout(c, plant, 5, graph=True)
        res = rollout(c, plant, ticks, graph=graph)
        assert (res["graph"] is not None) == graph
        snap = _snap(plant)
        snap["effort"] = res["effort"].cpu().numpy().copy()
        v = c.view()
        snap.update({"ctrl_" + k: v[k].cpu().numpy().copy() for k in v if k not in ("batch", "ticks")})
        out.append(snap)
        assert v["ticks"] == 13 + ticks
        c.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(out[0]["effort"]).max() > 1.0


def test_reset_masked_robots_only():
    from quadruped_ctrl_amd.binding import rollout
    B = 64
    gait, vel, xyyaw = _walk_setup(0, 4)
    mask = (np.arange(B) % 3 == 0)
    runs = []
    for do_reset in (False, True):
        c, plant = _pair(B, "per_robot", xyyaw=xyyaw)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        first = _snap(plant)
        rollout(c, plant, 20)
        if do_reset:
            plant.reset(_dev(c, mask), _dev(c, xyyaw))
            after = _snap(plant)
            c.reset(_dev(c, mask))
            c.set_gait(_dev(c, gait))
            c.set_vel(_dev(c, vel))
        else:
            before = _snap(plant)
        rollout(c, plant, 15)
        end = _snap(plant)
        end["effort"] = plant.effort.cpu().numpy().copy()
        runs.append(end)
        c.close()
    for k in PLANT_KEYS:
        assert np.array_equal(after[k][mask], first[k][mask]), k         # the initial state, bit for bit
        assert np.array_equal(after[k][~mask], before[k][~mask]), k      # the others: untouched
    assert not np.array_equal(before["p"][mask], first["p"][mask])
    for k in runs[0]:
        assert np.array_equal(runs[0][k][~mask], runs[1][k][~mask]), k   # ... and they go on as if nothing happened
    assert not np.array_equal(runs[0]["state"][mask], runs[1]["state"][mask])


def test_argument_and_state_errors():
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant, PlantView, QmpcError
    OK, ARG, STATE = 0, 1, 3
    B = 8
    c = BatchedController(0, max_batch=16)
    lib, h = c.lib, c.mpc.h
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device=c.device)
    eff, st, mo = d(B, 12), d(B, 16), d(B, 24)
    mask = torch.zeros(B, dtype=torch.uint8, device=c.device)
    v = PlantView()
    assert lib.qmpc_plant_init(h, B, 0.4, 1, None, None) == STATE            # before qmpc_ctrl_init
    with pytest.raises(QmpcError):
        BatchedPlant(c).init()
    c.init(B, 500.0, L.PID)
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == STATE   # before plant_init
    assert lib.qmpc_plant_reset(h, B, mask.data_ptr(), None, None) == STATE
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == STATE
    assert lib.qmpc_plant_init(None, B, 0.4, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B + 1, 0.4, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, 0.4, 0, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, -0.1, 1, None, None) == ARG
    assert lib.qmpc_plant_init(h, B, float("nan"), 1, None, None) == ARG
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == STATE                   # a refused init initialises nothing
    assert lib.qmpc_plant_init(h, B, 0.4, 2, None, None) == OK
    assert lib.qmpc_plant_view_get(h, None) == ARG
    assert lib.qmpc_plant_view_get(h, C.byref(v)) == OK and (v.batch, v.substeps, v.mu_plant) == (B, 2, 0.4)
    assert lib.qmpc_plant_step(h, B - 1, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, None, st.data_ptr(), mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), None, mo.data_ptr(), None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), None, None) == ARG
    assert lib.qmpc_plant_reset(h, B, None, None, None) == ARG
    assert lib.qmpc_plant_reset(h, B + 1, mask.data_ptr(), None, None) == ARG
    assert lib.qmpc_plant_step(h, B, eff.data_ptr(), st.data_ptr(), mo.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(st).all() and torch.isfinite(mo).all()
    c.close()


def test_plant_touches_no_controller_state():
    """After a closed-loop run and a controller re-init, the controller fed make_state_stream produces the efforts of
    a handle that never had a plant."""
    from quadruped_ctrl_amd.binding import rollout
    B, ticks = 64, 27
    gait, vel, xyyaw = _walk_setup(0, 4)
    state, motor = W.make_state_stream(B, ticks, 64)
    effs = []
    for with_plant in (True, False):
        c, plant = _pair(B, xyyaw=xyyaw) if with_plant else (None, None)
        if not with_plant:
            from quadruped_ctrl_amd.binding import BatchedController
            c = BatchedController(0, max_batch=B)
        else:
            c.set_gait(_dev(c, gait))
            c.set_vel(_dev(c, vel))
            rollout(c, plant, 26)
        c.init(B, L.FREQ, L.PID)
        c.set_gait(_dev(c, gait))
        c.set_vel(_dev(c, vel))
        out = []
        for t in range(ticks):
            out.append(c.tick_state(_dev(c, state[t]), _dev(c, motor[t])).cpu().numpy().copy())
            if with_plant and t % 2:
                plant.step(plant.effort)                                 # the plant running beside it changes nothing
        effs.append(np.stack(out))
        c.close()
    assert np.array_equal(effs[0], effs[1]) and np.abs(effs[0]).max() > 1.0
