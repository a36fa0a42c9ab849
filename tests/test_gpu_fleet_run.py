"""GPU suite (-m gpu) for the fleet run (include/qmpc_fleet.h; rollout(..., fused=True), BatchedController.fleet_info).

Every test feeds two handles identically, advances one by the per-tick path (rollout(): qmpc_ctrl_tick_state ->
qmpc_plant_step) and the other through qmpc_fleet_run, and compares RAW BITS: effort, state, motor, every controller array
qmpc_debug_ctrl_read knows, every array of the plant's view, T and the counters, and where they are on the plant's
statistics.  Two things are compared per robot and not as stored: the due list, whose order neither path defines (one
atomic per wave), and nothing else.

Fleet sizes: 1 robot; 17, which fills neither a wave's 16 robots nor a workgroup; 150, which spans three workgroups of the
span kernel at 64 robots per workgroup and ten at 16, with a ragged last one either way.  Commands: the plant source's
(tools/ctrl_bench.py --source plant): gaits 0, 4, 5, 10, x commands over [0, 0.5] m/s, gains (100, 1, 0, 0.05).
"""
import os
import re

import numpy as np
import pytest

import fleet_gpu as G
import plant_loop as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 17, 150)
assert L.PID == (100.0, 1.0, 0.0, 0.05)


def ctrl_arrays():
    src = open(os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_glue.h")).read()
    body = re.search(r"#define QMPC_CTRL_ARRAYS\(X\)((?:.*\\\n)*.*)", src).group(1)
    return [n for _, n, _ in re.findall(r"X\((\w+), (\w+), (\d+)\)", body)]


CTRL = ctrl_arrays()
assert len(CTRL) > 50 and "due_list" in CTRL


def commands(B, mode):
    k = np.arange(B)
    gait = np.array([0, 4, 5, 10], np.int32)[k % 4] if mode == 0 else np.full(B, 9, np.int32)
    vel = np.zeros((B, 3))
    vel[:, 0] = 0.5 * ((k * 7) % 16) / 15.0                   # x commands over [0, 0.5] m/s, both ends taken from B = 16 on
    vel[:, 2] = 0.1 * ((k % 3) - 1)
    if mode == 0:
        vel[gait == 4] = 0.0                                   # (gait 4 stands)
    xyyaw = np.stack([0.5 * (k % 16), 0.5 * (k // 16), 0.05 * ((k % 5) - 2)], 1).astype(np.float64)
    return gait, vel, xyyaw


class Twin:
    """Two handles fed identically: `a` walks by the per-tick path, `b` by the fleet run."""

    def __init__(self, B, schedule="lockstep", mode=None):
        self.B = B
        self.gait, self.vel, self.xyyaw = commands(B, mode or 0)
        self.h = []
        for _ in range(2):
            c, p = G.pair(B, schedule, mode, xyyaw=self.xyyaw)
            keep = [G.dev(c, self.gait), G.dev(c, self.vel)]
            c.set_gait(keep[0])
            c.set_vel(keep[1])
            self.h.append((c, p, keep))
        (self.ca, self.pa, _), (self.cb, self.pb, _) = self.h

    def both(self, f):
        for c, p, keep in self.h:
            f(c, p, keep)

    def old(self, ticks):
        """`ticks` per-tick ticks on BOTH handles (a common prefix)."""
        from quadruped_ctrl_amd.binding import rollout
        self.both(lambda c, p, keep: rollout(c, p, ticks))

    def run(self, ticks, calls=None):
        """`ticks` on a by the per-tick path; on b through qmpc_fleet_run, in one call or in `calls`."""
        from quadruped_ctrl_amd.binding import rollout
        rollout(self.ca, self.pa, ticks)
        for n in calls or (ticks,):
            rollout(self.cb, self.pb, n, fused=True)

    def close(self):
        self.both(lambda c, p, keep: c.close())


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b, what):
    G.equal(raw(a), raw(b), what)


def compare(t, what, ticks_too=True):
    import torch
    torch.cuda.synchronize()
    ca, pa, cb, pb = t.ca, t.pa, t.cb, t.pb
    for k, ta, tb in (("effort", pa.effort, pb.effort), ("state", pa.state, pb.state), ("motor", pa.motor, pb.motor)):
        same_bits(ta.cpu().numpy(), tb.cpu().numpy(), f"{what}: {k}")
    sa, sb = G.snap(pa), G.snap(pb)
    for k in G.PLANT_KEYS:
        same_bits(sa[k], sb[k], f"{what}: plant view {k}")
    ra, rb = ({n: c.read(n) for n in CTRL} for c in (ca, cb))
    for n in CTRL:
        if n == "due_list":                                    # the order is undefined on both paths: per robot
            na, nb = int(ra["due_count"][0, 0]), int(rb["due_count"][0, 0])
            G.equal(np.sort(ra[n][:na, 0]), np.sort(rb[n][:nb, 0]), f"{what}: the due robots of the last tick")
            if t.cb.schedule == "per_robot":
                G.equal(np.sort(rb[n][:nb, 0]), np.flatnonzero(rb["due"][:, 0]), f"{what}: the due list against the due flags")
        else:
            same_bits(ra[n], rb[n], f"{what}: controller array {n}")
    va, vb = ca.view(), cb.view()
    if ticks_too:
        assert va["ticks"] == vb["ticks"], f"{what}: T is {va['ticks']} by the per-tick path and {vb['ticks']} fused"
    G.equal(va["counter"].cpu().numpy(), vb["counter"].cpu().numpy(), f"{what}: the counters")


def fused_only(info, ticks, what):
    assert info["reason"] == 0 and info["fused_ticks"] == info["ticks"] == ticks and info["fallback_ticks"] == 0, (what, info)
    assert 0 < info["fused_launches"], (what, info)


@pytest.mark.parametrize("B", SIZES)
def test_mode0_lockstep_across_three_solves(B):
    """Five per-tick ticks on both handles, so that T is mid-period; then 40 ticks, which cross the solves of ticks 13, 26
    and 39.  Four launches of the span kernel serve them (8, 13, 13 and 6 ticks' worth)."""
    t = Twin(B)
    t.old(5)
    compare(t, f"B = {B}, the common prefix")
    t.run(40)
    compare(t, f"B = {B}, 40 ticks from T = 5")
    assert t.cb.view()["ticks"] == 45
    info = t.cb.fleet_info()
    fused_only(info, 40, B)
    assert info["fused_launches"] == 4, info
    assert t.ca.fleet_info() == dict(ticks=0, fused_ticks=0, fused_launches=0, fallback_ticks=0, reason=0)
    moved = float(np.abs(t.pb.effort.cpu().numpy()).max())
    assert moved > 1.0, f"the largest effort is {moved}: the fleet did not move"
    safe = t.cb.read("safe")
    assert (safe == 1).all(), f"robots latched unsafe: {G._where(safe != 1)}"
    t.close()


@pytest.mark.parametrize("B", SIZES)
def test_mode1_per_robot_schedule(B):
    """Robot mode 1 with the per-robot schedule.  Group g = b % 13 is reset before tick g (include/qmpc_ctrl.h), so that
    one thirteenth of the fleet is due on every tick; then 30 ticks: 31 launches of the span kernel and 30 solves over
    the due list."""
    import torch
    t = Twin(B, "per_robot", 1)
    group = np.arange(B) % 13

    def stagger(c, p, keep):
        from quadruped_ctrl_amd.binding import rollout
        for g in range(13):
            c.reset(G.dev(c, group == g))
            c.set_gait(keep[0])                                # (a reset zeroes the robot's commands)
            c.set_vel(keep[1])
            rollout(c, p, 1)
    t.both(stagger)
    compare(t, f"B = {B}, the staggered prefix")
    t.run(30)
    compare(t, f"B = {B}, 30 ticks")
    torch.cuda.synchronize()
    same_bits(t.ca.read("status"), t.cb.read("status"), f"B = {B}: status")
    assert (t.cb.read("status")[:, 0] & 47 == 0).all(), t.cb.read("status")[:, 0]
    info = t.cb.fleet_info()
    fused_only(info, 30, B)
    assert info["fused_launches"] == 31, info
    t.close()


@pytest.mark.parametrize("B", SIZES)
def test_varied_plant_with_statistics(B):
    """qmpc_plant_set_params -- per-robot mass and floor, a 30 N lateral push -- and the statistics on: the span kernel's
    <VARY, STATS> instantiation, over two periods."""
    t = Twin(B)
    k = np.arange(B)
    prm = dict(mass=9.0 * np.array([0.8, 1.0, 1.2, 1.4])[(k // 4) % 4], mu=np.array([0.3, 0.4, 0.6, 0.8])[k % 4],
               force=np.stack([np.zeros(B), np.where(k % 2 == 1, 30.0, -30.0), np.zeros(B)], 1))

    def bind(c, p, keep):
        keep.append({n: G.dev(c, v) for n, v in prm.items()})
        p.set_params(**keep[-1])
        p.enable_stats()
        p.reset_stats()
    t.both(bind)
    t.run(26)
    compare(t, f"B = {B}, varied plant, 26 ticks")
    sa, sb = G.plant_stats(t.pa), G.plant_stats(t.pb)
    for n in sa:
        same_bits(sa[n], sb[n], f"B = {B}: statistic {n}")
    assert (sb["n"] == 26).all(), sb["n"]
    fused_only(t.cb.fleet_info(), 26, B)
    t.close()


@pytest.mark.parametrize("B", SIZES)
def test_statistics_alone_and_params_alone(B):
    """The two mixed instantiations: statistics on a plain plant (<false, true>) on one pair, parameters without
    statistics (<true, false>) on another; 14 ticks, one solve."""
    for stats in (True, False):
        t = Twin(B)

        def bind(c, p, keep):
            if stats:
                p.enable_stats()
                p.reset_stats()
            else:
                keep.append(G.dev(c, np.full(B, 0.5)))
                p.set_params(mu=keep[-1])
        t.both(bind)
        t.run(14)
        compare(t, f"B = {B}, stats {stats}, 14 ticks")
        if stats:
            sa, sb = G.plant_stats(t.pa), G.plant_stats(t.pb)
            for n in sa:
                same_bits(sa[n], sb[n], f"B = {B}: statistic {n}")
        fused_only(t.cb.fleet_info(), 14, B)
        t.close()


@pytest.mark.parametrize("B", SIZES)
def test_call_splitting(B):
    """1 + 12 + 13 + 14 ticks in four calls equal 40 ticks in one call -- and both equal the per-tick path: a call ends on
    a whole tick wherever it ends."""
    t = Twin(B)
    one = Twin(B)
    t.old(5)
    one.old(5)
    t.run(40, calls=(1, 12, 13, 14))
    one.run(40)
    compare(t, f"B = {B}, four calls")
    for k in ("effort", "state", "motor"):
        same_bits(getattr(t.pb, k).cpu().numpy(), getattr(one.pb, k).cpu().numpy(), f"B = {B}: {k}, four calls against one")
    for n in CTRL:
        if n != "due_list":
            same_bits(t.cb.read(n), one.cb.read(n), f"B = {B}: controller array {n}, four calls against one")
    G.same(t.pb, one.pb, f"B = {B}: four calls against one")
    fused_only(t.cb.fleet_info(), 40, B)
    # T = 5: 1 -> one launch; 12 -> E..L of tick 13 | C..P (2); 13 -> up to tick 26 | rest (2); 14 -> up to 39 | rest (2)
    assert t.cb.fleet_info()["fused_launches"] == 7 and one.cb.fleet_info()["fused_launches"] == 4
    t.close()
    one.close()


@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_graph_of_26_ticks_replayed(schedule):
    """A captured block of 26 ticks, replayed twice in all (the capture's own replay and one more), equals 52 eager ticks of
    the per-tick path -- robot mode 0, in lockstep and with the per-robot schedule, where every launch is preceded by the
    reset of the due count and followed by a solve over the due list.  At 150 robots only: what a capture changes is how
    the launches are enqueued, not what a lane does; the lane cases are the eager tests'."""
    from quadruped_ctrl_amd.binding import rollout
    B = 150
    t = Twin(B, schedule)
    rollout(t.ca, t.pa, 52)
    g = rollout(t.cb, t.pb, 26, graph=True, fused=True)["graph"]
    g.replay()
    compare(t, f"{schedule}: 2 x 26 captured ticks against 52 eager", ticks_too=False)
    assert t.cb.view()["ticks"] == 26                           # (a replay does not advance the host's count)
    info = t.cb.fleet_info()
    fused_only(info, 26, schedule)
    assert info["fused_launches"] == (3 if schedule == "lockstep" else 27), info
    t.close()


def test_graph_of_20_ticks_is_refused_in_lockstep():
    from quadruped_ctrl_amd.binding import QmpcError, rollout
    t = Twin(17)
    for fused in (False, True):
        with pytest.raises(QmpcError, match="multiple of 13"):
            rollout(t.cb, t.pb, 20, graph=True, fused=fused)
    assert t.cb.view()["ticks"] == 0 and t.cb.fleet_info()["ticks"] == 0
    t.close()


def test_fallback_on_terrain():
    """Terrain rows bound: the call enqueues the per-tick launches -- the terrain kernels -- and says why."""
    import plant_loop_terrain as LT
    from quadruped_ctrl_amd.binding import FLEET_REASONS
    B = 17
    t = Twin(B)
    rows = LT.terrain(16)[np.arange(B) % 16]
    t.both(lambda c, p, keep: keep.append(G.stand_on(c, p, rows, t.xyyaw, clamp_swing=True, rebase_z=True)))
    t.run(15)
    compare(t, "terrain bound, 15 ticks")
    ta, tb = t.pa.terrain(), t.pb.terrain()
    for k in ("ground", "support"):
        same_bits(ta[k].cpu().numpy(), tb[k].cpu().numpy(), f"terrain {k}")
    info = t.cb.fleet_info()
    assert info == dict(ticks=15, fused_ticks=0, fused_launches=0, fallback_ticks=15, reason=FLEET_REASONS["terrain"]), info
    # ... and with the rows unbound again (a new plant) the next call runs fused
    t.both(lambda c, p, keep: p.init(0.4, 1, G.dev(c, t.xyyaw)))
    t.run(3)
    compare(t, "flat again, 3 ticks")
    info = t.cb.fleet_info()
    assert info["reason"] == 0 and info["fused_ticks"] == 3 and info["fallback_ticks"] == 15, info
    t.close()


def test_fallback_on_contact_and_actuators_refused():
    from quadruped_ctrl_amd.binding import FLEET_REASONS, BatchedActuators, QmpcError, rollout
    t = Twin(17)
    t.both(lambda c, p, keep: p.set_contact(**G.ON))
    t.run(14)
    compare(t, "contact decided by the ground, 14 ticks")
    info = t.cb.fleet_info()
    assert info["reason"] == FLEET_REASONS["contact"] and info["fused_ticks"] == 0 and info["fallback_ticks"] == 14, info
    act = BatchedActuators(t.pb)
    act.init()
    with pytest.raises(QmpcError, match="actuators"):
        rollout(t.cb, t.pb, 1, fused=True, actuators=act)
    assert t.cb.fleet_info() == info
    t.close()


def test_errors_enqueue_nothing():
    """Wrong batch, ticks = 0, a null pointer: QMPC_ERR_ARG; before qmpc_plant_init: QMPC_ERR_STATE.  State, T and the
    counts stay as they were."""
    import torch
    from quadruped_ctrl_amd.binding import BatchedController, BatchedPlant, QmpcError, rollout
    B = 17
    t = Twin(B)
    t.run(3)
    torch.cuda.synchronize()
    c, p = t.cb, t.pb
    before = ({n: c.read(n) for n in CTRL}, G.snap(p), p.effort.cpu().numpy().copy(), c.view()["ticks"], c.fleet_info())
    e, s, m, h, lib = p.effort.data_ptr(), p.state.data_ptr(), p.motor.data_ptr(), c.mpc.h, c.lib
    assert lib.qmpc_fleet_run(h, B + 1, 13, e, s, m, None) == 1
    assert lib.qmpc_fleet_run(h, B, 0, e, s, m, None) == 1 and lib.qmpc_fleet_run(h, B, -3, e, s, m, None) == 1
    for args in ((None, s, m), (e, None, m), (e, s, None)):
        assert lib.qmpc_fleet_run(h, B, 13, *args, None) == 1
    assert lib.qmpc_fleet_run_info(h, None) == 1
    with pytest.raises(QmpcError):
        rollout(c, p, 0, fused=True)
    torch.cuda.synchronize()
    after = ({n: c.read(n) for n in CTRL}, G.snap(p), p.effort.cpu().numpy().copy(), c.view()["ticks"], c.fleet_info())
    for n in CTRL:
        same_bits(before[0][n], after[0][n], f"refused calls: controller array {n}")
    for k in G.PLANT_KEYS:
        same_bits(before[1][k], after[1][k], f"refused calls: plant view {k}")
    same_bits(before[2], after[2], "refused calls: effort")
    assert before[3] == after[3] == 3 and before[4] == after[4], (before[3:], after[3:])
    # before qmpc_plant_init, and before qmpc_ctrl_init
    c2 = BatchedController(0, max_batch=B)
    buf = torch.zeros((B, 24), dtype=torch.float64, device=c2.device)
    assert c2.lib.qmpc_fleet_run(c2.mpc.h, B, 13, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == 3
    c2.init(B, L.FREQ, L.PID)
    assert c2.lib.qmpc_fleet_run(c2.mpc.h, B, 13, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == 3
    assert c2.fleet_info()["ticks"] == 0 and c2.view()["ticks"] == 0
    with pytest.raises(QmpcError, match="before init"):
        rollout(c2, BatchedPlant(c2), 13, fused=True)
    c2.close()
    t.close()
