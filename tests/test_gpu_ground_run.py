"""GPU suite (-m gpu) for the ground-run switch (include/qmpc_ground_run.h; BatchedController.set_ground_run): the fleet
run and the loop run on terrain rows and on a height field through the fused launch.

The harness is the twin-handle, raw-bits one of tests/test_gpu_fleet_run.py (Twin, compare) and tests/test_gpu_loop.py
(Twin, Fleets, compare_*), imported as they stand: handle `a` walks by the per-tick path -- rollout(), or
rollout_episodes() with the actuators -- and handle `b`, with the switch on, through rollout(fused=True) / rollout_loop().
Everything those two suites compare is compared, and the `ground` and `support` arrays of the terrain view bit for bit,
and the plant's statistics where they are on.  Every test holds b to reason == 0, fused_ticks == ticks and
fallback_ticks == 0: without the switch a bound ground is the per-tick path.

The ground: rows are plant_loop_terrain.terrain(16)[k % 16] -- stairs up, cross slope, stairs down, uphill by k % 4 -- and
the bank is plant_loop_field.field_for(B, RUNGS["scheduled"]), whose maps lie around plant_loop's start poses: the field
tests stand the robots there.
"""
import numpy as np
import pytest

import episode_gpu as EG
import fleet_gpu as G
import plant_loop as L
import plant_loop_field as LF
import plant_loop_terrain as LT
import test_gpu_fleet_run as TF
import test_gpu_loop as TL

pytestmark = pytest.mark.gpu

SIZES = (1, 17, 150)
_np = EG.to_np


def rows_for(B):
    return LT.terrain(16)[np.arange(B) % 16]


def on_rows(t, clamp=True, rebase=True, xyyaw=None):
    """Terrain rows bound on both handles and the robots stood on them; the switch on, on b alone."""
    rows = rows_for(t.B)
    for h in t.h:
        c, p, keep = h[0], h[1], h[2]
        keep.append(G.stand_on(c, p, rows, t.xyyaw if xyyaw is None else xyyaw, clamp_swing=clamp, rebase_z=rebase))
    t.cb.set_ground_run()
    assert t.cb.ground_run and not t.ca.ground_run
    return rows


def field_poses(B):
    """plant_loop's start poses, which field_for() lays its maps around."""
    return L.commands(0)[2][np.arange(B) % L.N_CMD]


def on_field(t, amp, rows=False, clamp=True, rebase=True, xyyaw=None):
    """The bank bound on both handles (on top of the rows, or alone: rows null) and the robots stood on the surface; the
    switch on, on b alone."""
    z, place, cell = LF.field_for(t.B, amp)
    xyyaw = field_poses(t.B) if xyyaw is None else xyyaw
    for h in t.h:
        c, p, keep = h[0], h[1], h[2]
        if rows:
            keep.append(G.dev(c, rows_for(t.B)))
            p.set_terrain(keep[-1], clamp_swing=clamp, rebase_z=rebase)
        keep += [G.dev(c, z), G.dev(c, place)]
        p.set_field(keep[-2], keep[-1], cell, clamp_swing=clamp, rebase_z=rebase)
        p.reset(G.all_robots(c, t.B), G.dev(c, xyyaw))
    t.cb.set_ground_run()


def same_ground(pa, pb, what):
    ta, tb = pa.terrain(), pb.terrain()
    for k in ("ground", "support"):
        TF.same_bits(_np(ta[k]), _np(tb[k]), f"{what}: terrain {k}")
    return _np(ta["ground"]), _np(ta["support"])


def compare(t, what, ticks_too=True):
    """tests/test_gpu_fleet_run.py's compare, and the terrain view -> a's (ground, support)."""
    TF.compare(t, what, ticks_too)
    return same_ground(t.pa, t.pb, what)


def felt(t, rows, what):
    """Not vacuous, on the per-tick handle: the sloped robots that do not start at height 0 stand on a support that is
    not 0, and some stance foot is off the plane z = 0."""
    _, support = same_ground(t.pa, t.pb, what)
    h0 = rows[:, 1] * t.xyyaw[:, 0] + rows[:, 2] * t.xyyaw[:, 1]
    sloped = np.abs(h0) > 1e-3
    assert sloped.any() and (np.abs(support[sloped]) > 1e-4).all(), (what, support[sloped])
    s = G.snap_legs(t.pa, t.B)
    assert (np.abs(s["foot"][..., 2][s["stance"] != 0]) > 1e-4).any(), f"{what}: every stance foot is at z = 0"


# ---- 1. terrain rows, the fleet run ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,flags", [(1, True), (17, True), (150, True), (17, False)])
def test_rows_mode0_lockstep_across_three_solves(B, flags):
    """Five per-tick ticks on both handles, then 40 ticks, which cross three solves: four fused launches on terrain."""
    t = TF.Twin(B)
    rows = on_rows(t, clamp=flags, rebase=flags)
    t.old(5)
    compare(t, f"B = {B}, the common prefix")
    t.run(40)
    compare(t, f"B = {B}, 40 ticks on rows from T = 5")
    info = t.cb.fleet_info()
    TF.fused_only(info, 40, B)
    assert info["fused_launches"] == 4 and t.cb.view()["ticks"] == 45, info
    if B >= 17:
        felt(t, rows, f"B = {B}")
    assert float(np.abs(_np(t.pb.effort)).max()) > 1.0, "the fleet did not move"
    t.close()


@pytest.mark.parametrize("B", SIZES)
def test_rows_mode1_per_robot_schedule(B):
    """Robot mode 1 with the per-robot schedule, staggered as tests/test_gpu_fleet_run.py staggers it; then 30 ticks on
    terrain: 31 fused launches and 30 solves over the due list."""
    from quadruped_ctrl_amd.binding import rollout
    t = TF.Twin(B, "per_robot", 1)
    rows = on_rows(t)
    group = np.arange(B) % 13

    def stagger(c, p, keep):
        for g in range(13):
            c.reset(G.dev(c, group == g))
            c.set_gait(keep[0])                                # (a reset zeroes the robot's commands)
            c.set_vel(keep[1])
            rollout(c, p, 1)
    t.both(stagger)
    compare(t, f"B = {B}, the staggered prefix")
    t.run(30)
    compare(t, f"B = {B}, 30 ticks on rows")
    TF.same_bits(t.ca.read("status"), t.cb.read("status"), f"B = {B}: status")
    info = t.cb.fleet_info()
    TF.fused_only(info, 30, B)
    assert info["fused_launches"] == 31, info
    if B >= 17:
        felt(t, rows, f"B = {B}")
    t.close()


# ---- 2. the height field ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("full", [False, True], ids=["plain", "params+stats"])
@pytest.mark.parametrize("rows", [False, True], ids=["bank", "bank+rows"])
@pytest.mark.parametrize("B", SIZES)
def test_field_26_ticks(B, rows, full):
    """The scheduled-contact field, alone (rows null) and on top of the terrain rows, in the kernel's two <VARY, STATS>
    extremes: nothing bound, and per-robot mass, floor and a lateral push with the statistics on.  26 ticks, two solves."""
    t = TF.Twin(B)
    on_field(t, LF.RUNGS["scheduled"], rows=rows)
    if full:
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
    what = f"B = {B}, field{' on rows' if rows else ''}{', varied' if full else ''}, 26 ticks"
    ground, support = compare(t, what)
    if full:
        sa, sb = G.plant_stats(t.pa), G.plant_stats(t.pb)
        for n in sa:
            TF.same_bits(sa[n], sb[n], f"{what}: statistic {n}")
        assert (sb["n"] == 26).all(), sb["n"]
    info = t.cb.fleet_info()
    TF.fused_only(info, 26, what)
    assert info["fused_launches"] == 3, info
    assert np.abs(support).max() > 1e-3, f"{what}: the ground is not felt"
    t.close()


def test_field_of_zeros_is_the_flat_fused_run():
    """A bank of zeros and no rows, flags 0: include/qmpc_field.h's own contract is the flat plant's bits.  The fused run
    on that bank equals the per-tick run on it AND the flat fused run of a third handle."""
    from quadruped_ctrl_amd.binding import rollout
    B = 17
    t = TF.Twin(B)
    on_field(t, 0.0, clamp=False, rebase=False, xyyaw=t.xyyaw)
    t.run(26)
    compare(t, "a bank of zeros, 26 ticks")
    TF.fused_only(t.cb.fleet_info(), 26, "a bank of zeros")
    flat = TF.Twin(B)                                            # (its b handle alone is used: the flat fused run)
    rollout(flat.cb, flat.pb, 26, fused=True)
    TF.fused_only(flat.cb.fleet_info(), 26, "flat")
    import torch
    torch.cuda.synchronize()
    for k in ("effort", "state", "motor"):
        TF.same_bits(_np(getattr(t.pb, k)), _np(getattr(flat.pb, k)), f"a bank of zeros against flat: {k}")
    G.same(t.pb, flat.pb, "a bank of zeros against flat")
    for n in TF.CTRL:
        if n != "due_list":
            TF.same_bits(t.cb.read(n), flat.cb.read(n), f"a bank of zeros against flat: controller array {n}")
    t.close()
    flat.close()


# ---- 3. the loop run on ground ---------------------------------------------------------------------------------------------

def fleet_on_rows(f):
    f.keep.append(G.stand_on(f.c, f.p, LT.terrain(EG.B), f.xyyaw0, clamp_swing=True, rebase_z=True))


def fleet_on_field(f):
    z, place, cell = LF.field_for(EG.B, LF.RUNGS["scheduled"])
    f.keep += [G.dev(f.c, z), G.dev(f.c, place)]
    f.p.set_field(f.keep[-2], f.keep[-1], cell, clamp_swing=True, rebase_z=True)
    f.p.reset(G.all_robots(f.c, EG.B), G.dev(f.c, f.xyyaw0))


GROUNDS = dict(rows=fleet_on_rows, field=fleet_on_field)


def same_but_nan_signs(a, b, loose, what):
    """Two [B, ...] float arrays, raw bits.  loose [B] bool: in those robots' rows a word may also be a NaN on both sides;
    every other row, and every word there that is not a NaN on both sides, bit for bit."""
    TL.same_bits(a[~loose], b[~loose], what)
    a, b = a[loose], b[loose]
    ok = (TL.raw(a) == TL.raw(b)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), f"{what}: the rows of the NaN-mass robots {np.flatnonzero(loose)} differ in more than a NaN's bits"


def nan_mass_robots(fa, fb, what, on):
    """The robots whose bound mass is not finite (the same on both handles), or none where `on` is false."""
    if not on:
        return np.zeros(EG.B, bool)
    loose = ~np.isfinite(_np(fa.prm["mass"]))
    G.equal(loose, ~np.isfinite(_np(fb.prm["mass"])), f"{what}: the robots with a mass that is not finite")
    return loose


def compare_fleets(fl, what, ticks_too=True, nan_mass_rows=False):
    """tests/test_gpu_loop.py's Fleets.compare, statement for statement, with the leg command taken out of the bitwise
    comparisons and given to same_but_nan_signs: `effort`, and the actuators' `ring`, which is the efforts of the last
    ticks as the leg command wrote them.  Everything else -- state, motor, the plant view, ground, support, the
    statistics, the contact counters, the controller's view and arrays, the manager, the bound commands, the actuators'
    head, age and accumulators -- is compared as raw bits for every robot, the NaN-mass one included.

    Why (nan_mass_rows, the cases with a check on every fifth tick): the episode fleet's robot 5 has a NaN mass
    (Fleet.push) and then walks on NaNs for five ticks.  Where an instruction adds two NaNs the result's sign is its first
    operand's, the compiler may order a sum's operands either way, and the ground compiles of the loop kernel are other
    compilations of the leg command's text than the per-tick kernel.  Measured on rows and on the field, lockstep, every
    5, after 5, 10 and 90 ticks: the ONLY words that differ between the two paths are effort[5][0:12], NaN on both --
    0xfff8000000000000, 0x7ff8000000000000, 0xfff8... per leg on one path and the opposite signs on the other.  Neither
    IEEE 754 nor the source defines that bit."""
    (fa, fb), (ea, eb), (aa, ab) = fl.f, fl.e, fl.a
    sa, sb = fa.snapshot(), fb.snapshot()
    assert set(sa) == set(sb) and {"ctrl.safe", "ctrl.counter", "plant.stance", "effort", "ground", "support"} <= set(sa), sorted(sa)
    for k in sa:
        if k != "effort":
            assert EG.bits(sa[k], sb[k]), (what, k, np.flatnonzero((sa[k] != sb[k]).reshape(EG.B, -1).any(1))[:8])
    loose = nan_mass_robots(fa, fb, what, nan_mass_rows)
    same_but_nan_signs(_np(fa.p.effort), _np(fb.p.effort), loose, f"{what}: effort")
    for k in ("state", "motor"):
        TL.same_bits(_np(getattr(fa.p, k)), _np(getattr(fb.p, k)), f"{what}: {k}")
    pa, pb = G.snap(fa.p), G.snap(fb.p)
    for k in G.PLANT_KEYS:
        TL.same_bits(pa[k], pb[k], f"{what}: plant view {k}")
    va, vb = ea.view(), eb.view()
    for k in TL.EP_KEYS:
        TL.same_bits(_np(va[k]), _np(vb[k]), f"{what}: manager {k}")
    TL.compare_ctrl(fa.c, fb.c, what, ticks_too, _np(va["mask"]) != 0)
    TL.same_bits(_np(fa.vel), _np(fb.vel), f"{what}: the bound velocities")
    TL.same_bits(_np(fa.gait), _np(fb.gait), f"{what}: the bound gaits")
    la, lb = ea.log(), eb.log()                                 # sorted by (robot, episode): the log as a set
    assert la["dropped"] == lb["dropped"] == 0, (what, la["dropped"], lb["dropped"])
    assert len({(r[0], r[1]) for r in lb["rows"]}) == len(lb["rows"]), f"{what}: a (robot, episode) key twice in the fused log"
    assert EG.rows_equal(la["rows"], lb["rows"]), f"{what}: the logs differ as sets ({len(la['rows'])} and {len(lb['rows'])} rows)"
    if aa is not None:
        wa, wb = aa.view(), ab.view()
        for k in TL.ACT_KEYS:
            if k == "ring":                                      # [max_delay + 1, B, 12]: the robots' axis first
                same_but_nan_signs(_np(wa[k]).swapaxes(0, 1), _np(wb[k]).swapaxes(0, 1), loose, f"{what}: actuator ring")
            else:
                TL.same_bits(_np(wa[k]), _np(wb[k]), f"{what}: actuator {k}")
    return la["rows"]


def fleets(schedule, act, ground):
    fl = TL.Fleets(schedule, act, ground=GROUNDS[ground])
    fl.f[1].c.set_ground_run()
    return fl


def respawned_on_ground(fl, what):
    """On BOTH handles: some robot the manager reset behind the last tick stands on ground that is not 0,
    p_z - 0.29 == ground != 0."""
    for path, f, e in (("per tick", fl.f[0], fl.e[0]), ("fused", fl.f[1], fl.e[1])):
        hit = _np(e.view()["mask"]) != 0
        p, ground = _np(f.p.view()["p"]), _np(f.p.terrain()["ground"])
        ok = hit & np.isfinite(ground)
        print(f"{what}, {path}: {int(hit.sum())} robots reset behind the last tick, {int((ok & (ground != 0)).sum())} of them on ground != 0")
        G.equal(p[ok, 2], 0.29 + ground[ok], f"{what}, {path}: the reset robots' height above their ground")
        assert (ground[ok] != 0).any(), f"{what}, {path}: no robot was respawned onto non-zero ground"


@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("act", [False, True], ids=["episodes", "episodes+actuators"])
@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
@pytest.mark.parametrize("ground", ["rows", "field"])
def test_episodes_90_ticks_on_ground(ground, schedule, act, every):
    """tests/test_gpu_loop.py's 90 ticks -- pushes on, all six causes, a check on every tick and on every fifth -- on
    terrain rows and on the field: every reset lands inside the launch, the plant's on the robot's own ground.  With a
    check on every tick every bit of every array is compared; on every fifth, every bit but those of a NaN in the effort
    of the NaN-mass robot (compare_fleets)."""
    fl = fleets(schedule, act, ground)
    compare_fleets(fl, "start")
    fl.run(90, every)
    what = f"{ground}, {schedule}, every {every}, 90 ticks"
    rows = compare_fleets(fl, what, nan_mass_rows=every != 1)
    fl.not_vacuous(rows, schedule == "lockstep")
    respawned_on_ground(fl, what)
    info = fl.f[1].c.loop_info()
    TL.fused_only(info, 90, what)
    assert info["fused_launches"] == (7 if schedule == "lockstep" else 91), info
    assert fl.f[0].c.loop_info()["ticks"] == 0 and not fl.f[0].c.ground_run
    fl.close()


# ---- 4. call splitting, and the loop run without options -------------------------------------------------------------------

def test_call_splitting_on_rows():
    """1 + 12 + 13 + 14 ticks in four calls equal 40 per-tick ticks on terrain, a check on every tick, actuators in."""
    fl = fleets("lockstep", True, "rows")
    fl.run(40, 1, calls=(1, 12, 13, 14))
    compare_fleets(fl, "four calls on rows")
    info = fl.f[1].c.loop_info()
    TL.fused_only(info, 40, "four calls on rows")
    assert info["fused_launches"] == 7, info
    fl.close()


@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_no_option_is_the_fleet_run_on_rows(schedule):
    """All three options 0 on terrain: the loop run is the fused fleet run -- the same bits, the same launches."""
    from quadruped_ctrl_amd.binding import rollout, rollout_loop
    t = TL.Twin(150, schedule, act=False)
    on_rows(t)
    t.ca.set_ground_run()                                       # (both handles run fused here)
    t.both(lambda c, p, keep, a: rollout(c, p, 5))
    rollout(t.ca, t.pa, 30, fused=True)
    rollout_loop(t.cb, t.pb, 30)
    t.compare(f"{schedule}: 30 ticks on rows, no option")
    same_ground(t.pa, t.pb, f"{schedule}: no option")
    fi, li = t.ca.fleet_info(), t.cb.loop_info()
    assert fi == li and li["fused_ticks"] == 30 and li["reason"] == 0 and li["fallback_ticks"] == 0, (fi, li)
    t.close()


# ---- 5. graphs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["lockstep", "per_robot"])
def test_graph_of_26_ticks_replayed_on_ground(schedule):
    """A captured block of 26 fused ticks on the field over terrain rows, replayed once more, equals 52 eager per-tick
    ticks; between the two replays the rows (z0 + 0.03 m) and the placement rows (the field at half scale) are rewritten
    in place on both handles, and the second block walks on the new ground."""
    from quadruped_ctrl_amd.binding import rollout
    B = 150
    t = TF.Twin(B, schedule)
    on_field(t, LF.RUNGS["scheduled"], rows=True)
    rollout(t.ca, t.pa, 26)
    g = rollout(t.cb, t.pb, 26, graph=True, fused=True)["graph"]
    before, _ = compare(t, f"{schedule}: 26 captured ticks against 26 eager")
    for c, p, keep in t.h:
        keep[-3][:, 0].add_(0.03)                               # the rows' z0 (keep: ..., rows, z, place)
        keep[-1][:, 3].mul_(0.5)                                # the placements' zs
    rollout(t.ca, t.pa, 26)
    g.replay()
    after, _ = compare(t, f"{schedule}: 2 x 26 captured ticks against 52 eager", ticks_too=False)
    assert t.cb.view()["ticks"] == 26                           # (a replay does not advance the host's count)
    assert np.median(after - before) > 0.015, f"the rewritten ground does not show: {np.median(after - before)}"
    info = t.cb.fleet_info()
    TF.fused_only(info, 26, schedule)
    assert info["fused_launches"] == (3 if schedule == "lockstep" else 27), info
    t.close()


# ---- 6. the switch, and what still falls back --------------------------------------------------------------------------------

def test_switch_and_the_remaining_fallback():
    from quadruped_ctrl_amd.binding import FLEET_REASONS, BatchedController
    B = 17
    t = TF.Twin(B)
    on_rows(t)
    # contact decided by the ground stays a fallback with the switch on: the contact bit alone
    t.both(lambda c, p, keep: p.set_contact(**G.ON))
    t.run(14)
    compare(t, "switch on, contact decided by the ground on rows, 14 ticks")
    info = t.cb.fleet_info()
    assert info == dict(ticks=14, fused_ticks=0, fused_launches=0, fallback_ticks=14, reason=FLEET_REASONS["contact"]), info
    # scheduled contact again: fused
    t.both(lambda c, p, keep: p.set_contact(None))
    t.run(3)
    compare(t, "switch on, scheduled contact again, 3 ticks")
    info = t.cb.fleet_info()
    assert info["reason"] == 0 and info["fused_ticks"] == 3 and info["fallback_ticks"] == 14, info
    # the switch off again: the terrain bit, as without this header
    t.cb.set_ground_run(False)
    assert not t.cb.ground_run
    t.run(15)
    compare(t, "switch off again, 15 ticks")
    info = t.cb.fleet_info()
    assert info == dict(ticks=32, fused_ticks=3, fused_launches=info["fused_launches"], fallback_ticks=29,
                        reason=FLEET_REASONS["terrain"]), info
    # qmpc_ctrl_init clears the switch; before it the switch is refused
    t.cb.set_ground_run()
    assert t.cb.ground_run
    t.cb.init(B, L.FREQ, L.PID)
    assert not t.cb.ground_run
    c2 = BatchedController(0, max_batch=B)
    import ctypes as C
    on = C.c_int(5)
    assert c2.lib.qmpc_ground_run_enable(c2.mpc.h, 1) == 3 and c2.lib.qmpc_ground_run_enabled(c2.mpc.h, C.byref(on)) == 3
    assert on.value == 5
    c2.init(B, L.FREQ, L.PID)
    assert c2.lib.qmpc_ground_run_enabled(c2.mpc.h, None) == 1
    assert c2.lib.qmpc_ground_run_enabled(c2.mpc.h, C.byref(on)) == 0 and on.value == 0
    c2.close()
    t.close()
