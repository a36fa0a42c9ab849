"""GPU suite (-m gpu): the life cycle of a handle that holds every fleet allocation -- controller, plant, the plant's
statistics, sensors.  Three handles are made, used and closed in turn, and the last one is initialised a second time before
it is closed: the results of every round are those of the first, bit for bit.  No memory-size assertions: free-memory
readings on a shared device include other tenants.
"""
import numpy as np
import pytest

import fleet_gpu as G
import plant_loop as L
import sense_loop as SL

pytestmark = pytest.mark.gpu

MAX_BATCH, B, SEED, SETTLE, TICKS = 8, 4, 0x9E3779B97F4A7C15, 50, 13   # (13 ticks in lockstep: one MPC solve, on the last)


def _init_and_run(c, plant, sensors):
    """init of all three with fixed arguments, statistics on, noise bound, the warm-up, 13 closed-loop ticks -> numpy
    copies of what they left.  Every call raises unless it succeeds."""
    import torch
    from quadruped_ctrl_amd.binding import rollout_sensed
    gait, vel, xyyaw = (a[:B] for a in L.commands(0))
    c.init(B, G.DEFAULTS["freq"], L.PID)
    c.set_gait(G.dev(c, gait))
    c.set_vel(G.dev(c, vel))
    plant.init(G.DEFAULTS["mu"], 1, G.dev(c, xyyaw))
    plant.enable_stats()
    plant.reset_stats()
    sensors.init(SEED)
    keep = {k: G.dev(c, v) for k, v in SL.noise(B).items()}
    sensors.set_params(**keep)
    sensors.settle(SETTLE)
    res = rollout_sensed(c, plant, sensors, TICKS)
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy().copy() for k in ("effort", "state", "imu")}
    out["status"], out["safe"] = c.read("status"), c.view()["safe"].cpu().numpy().copy()
    out["stats_n"] = plant.stats()["n"].cpu().numpy().copy()
    out["sense_n"] = sensors.view()["n"].cpu().numpy().copy()
    out["ticks"] = c.view()["ticks"]
    return out


def _check(out, first, what):
    assert (out["status"] == 0).all() and (out["safe"] == 1).all(), (what, out["status"], out["safe"])
    assert (out["stats_n"] == TICKS).all() and (out["sense_n"] == SETTLE + TICKS).all() and out["ticks"] == TICKS, what
    assert np.isfinite(out["effort"]).all() and np.abs(out["effort"]).max() > 1.0, what
    for k in ("effort", "state", "imu"):
        assert np.array_equal(out[k], first[k]), (what, k, np.abs(out[k] - first[k]).max())


def test_three_handles_in_turn_and_a_second_init_repeat_the_first_round():
    """max_batch 8, 4 robots, lockstep, robot mode 0, plant_loop's first four commands, sense_loop's noise on a fixed seed.
    Per handle: init, BatchedPlant.init, enable_stats, BatchedSensors.init + set_params, settle(50), 13 ticks of
    rollout_sensed, close().  All solve statuses 0, all robots safe, the statistics' n = 13; effort, state and imu of
    rounds 2 and 3 equal round 1 bit for bit.  On the last handle, before close(): init again on all three with the same
    arguments -- the blocks are reused and fully re-initialised, so the tick count restarts and the same 13 ticks give
    round 1's outputs again.  (reset_stats() after enable_stats(): the statistics outlive a qmpc_plant_init by design.)"""
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant, BatchedSensors
    first = None
    for rnd in (1, 2, 3):
        c = BatchedController(0, max_batch=MAX_BATCH)
        plant = BatchedPlant(c)
        sensors = BatchedSensors(plant)
        out = _init_and_run(c, plant, sensors)
        first = first or out
        _check(out, first, f"round {rnd}")
        if rnd == 3:
            _check(_init_and_run(c, plant, sensors), first, "second init of round 3's handle")
        c.close()
