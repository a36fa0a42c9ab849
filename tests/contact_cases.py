"""The single-step case of the plant with contact decided by the ground, built on tests/plant_model_contact.py alone --
TEST SIDE ONLY.

Shared by tests/test_contact_cpu.py, which checks here on the CPU that the case holds what it promises, and
tests/test_gpu_contact.py, which holds the kernels of csrc/qmpc_contact.hip to the model on it."""
import numpy as np

from quadruped_ctrl_amd import workloads as W

import plant_model as PM
import plant_model_contact as PCM
import terrain_cases as TC
from plant_cases import DEFAULTS, STAND, hold

f32 = np.float32
B = TC.B                     # 37: 148 lanes, a partial last wave, an odd number of quads
EDGE = 1e-6                  # every comparison the step branches on is at least this far (relative) from a tie
PARAMS = dict(drop_speed=0.7, slip_gain=0.013, slip_vmax=0.35)       # none at its default, the cap within reach
STATE = ("p", "v", "q", "w", "foot", "stance", "support", "ground", "drop", "slip", "early", "late")
values = TC.values


def model(substeps, rows, vals=None, flags=(True, True, True), src=None, tflags=(True, True), **params):
    """A ContactPlantModel on rows with the contact flags (early, late, slip); src: take the state of that model."""
    vals = vals or {}
    m = PCM.ContactPlantModel(B, DEFAULTS["freq"], DEFAULTS["mu"], substeps, rows=rows, clamp_swing=tflags[0],
                              rebase_z=tflags[1], mass_b=vals.get("mass"), ibody_b=vals.get("ibody"),
                              mu_b=vals.get("mu"), force=vals.get("force"), torque=vals.get("torque"))
    m.set_contact(*flags, **{**PARAMS, **params})
    if src is not None:
        for k in STATE:
            setattr(m, k, getattr(src, k).copy())
    return m


def _build(substeps, rows, xy, seed):
    """The state and the controller's outputs on `rows` with the bodies over xy [B,2]; every random number is drawn in
    the same order whatever the rows are."""
    rng = np.random.default_rng(seed)
    k = np.arange(B)
    rpy = np.stack([rng.uniform(-0.15, 0.15, B), rng.uniform(-0.15, 0.15, B), rng.uniform(-3.1, 3.1, B)], 1)
    q = np.asarray(W._quat_from_rpy(rpy), np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    m = model(substeps, rows)
    m.q = q
    m.p = np.concatenate([xy, (m.height(xy[:, 0], xy[:, 1]) + rng.uniform(0.24, 0.30, B))[:, None]], 1)
    m.v = rng.uniform(-0.6, 0.6, (B, 3))
    m.w = rng.uniform(-1.5, 1.5, (B, 3))
    R = PM.rot(m.q)
    body_foot = PM.HIP + STAND + rng.uniform(-0.05, 0.05, (B, 4, 3))
    m.foot = m.p[:, None, :] + PM.mul(R[:, None, :], body_foot)
    old = ((k[:, None] >> np.arange(4)) & 1).astype(bool)                  # every pinned pattern, twice ...
    new = ((((k * 7 + 3) % 16)[:, None] >> np.arange(4)) & 1).astype(bool)  # ... against the schedules in another order
    surf = m.height(m.foot[..., 0], m.foot[..., 1])
    up = rng.uniform(0.02, 0.06, (B, 4))
    up[2::6] = -rng.uniform(0.002, 0.02, (len(k[2::6]), 4))                # unpinned feet below the surface: they land at the edge
    m.foot[..., 2] = np.where(old, surf, surf + up)
    m.stance = old.copy()
    m.support = rng.uniform(-0.1, 0.1, B)                                  # (kept by the robots with no foot pinned)
    m.drop = np.where(new & ~old, rng.uniform(0.0, 0.02, (B, 4)), 0.0)
    m.slip = rng.uniform(0.0, 0.5, B)
    m.early, m.late = rng.integers(0, 50, B).astype(np.int32), rng.integers(0, 50, B).astype(np.int32)
    f = np.zeros((B, 4, 3))
    f[..., 2] = rng.uniform(5, 40, (B, 4))
    f[..., :2] = rng.uniform(-0.3, 0.3, (B, 4, 2)) * f[..., 2:3]
    f[0::7, :, 2] *= -1                                                    # pulling legs
    f[3::7, :, 0] = 2 * m.mu * f[3::7, :, 2]                               # demand outside the cone
    f[5::7, :, 1] = -8 * m.mu * f[5::7, :, 2]                              # ... and far outside: the sliding speed's cap
    tau = hold(m, f) + rng.uniform(-0.5, 0.5, (B, 4, 3))
    cs = np.where(new, rng.uniform(0.05, 1.0, (B, 4)), 0.0).astype(f32)
    pd = (STAND[None] + rng.uniform(-0.06, 0.06, (B, 4, 3))).astype(f32)
    pd[..., 2] += f32(0.03)                                                # (most commands end above the surface ...)
    pd[1::4, :, 2] -= f32(0.08)                                            # ... these are aimed below it
    pd[5] = [0.0, -0.065, -0.6]                                            # out of reach
    vd = rng.uniform(-1.0, 1.0, (B, 4, 3)).astype(f32)
    return m, old, new, tau, cs, pd, vd


def parity_case(substeps):
    """-> (m, rows, old, new, tau, cs, pd, vd): a ContactPlantModel with all three flags and PARAMS in a random state on
    slope plus stairs (terrain_cases.rows_for, both terrain flags), every old pinned pattern against a shuffled schedule,
    unpinned feet above and below the surface, late feet with some drop already, commands above and below the surface,
    demands inside, outside and far outside the cone.  One robot's flight is then shifted along its heading so that a
    tread edge lies under the middle of one foot's slide.  check() says what the case holds."""
    seed = 4100 + substeps
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2, 2, (B, 2))
    rows = TC.rows_for(np.concatenate([xy, np.zeros((B, 1))], 1), rng)
    m0, old, new, tau, cs, pd, vd = _build(substeps, rows, xy, seed + 50)
    after = model(substeps, rows, src=m0)
    after.step(tau.reshape(B, 12), cs, pd, vd)
    # the longest slide inside the flight: its nearest tread edge goes under its middle
    u0, u1 = m0.tread(m0.foot[..., 0], m0.foot[..., 1]), after.tread(after.foot[..., 0], after.foot[..., 1])
    tr = after.trace
    ok = tr["slid"] & tr["pin2"] & tr["s"] & (np.minimum(u0, u1) > 0.3) & (np.maximum(u0, u1) < 2.7)
    du = np.where(ok, np.abs(u1 - u0), 0.0)
    b, i = np.unravel_index(np.argmax(du), du.shape)
    assert du[b, i] > 1e-4, du.max()
    mid = 0.5 * (u0[b, i] + u1[b, i])
    rows = rows.copy()
    rows[b, 6] += (mid - np.round(mid)) * rows[b, 4]
    m0, old, new, tau, cs, pd, vd = _build(substeps, rows, xy, seed + 50)
    return m0, rows, old, new, tau, cs, pd, vd


def stepped(case, substeps, vals=None, **kw):
    """The case's model after its step, with the comparisons and floor() arguments it went through on record."""
    m0, rows, old, new, tau, cs, pd, vd = case
    m = model(substeps, rows, vals, src=m0, **kw)
    m.floors = []
    m.step(tau.reshape(B, 12), cs, pd, vd)
    return m


def check(case, after):
    """What the case promises, on the model's own values: `case` as parity_case() returned it, `after` = stepped(case).
    Every branch of include/qmpc_contact.h is taken by some foot, and no comparison the step branched on is within EDGE
    (relative to its operands) of a tie: c_z against height at the edges, c*_z against height at the command, |t| against
    mu fn in every substep, and every argument of floor() against the integers."""
    m0, rows, old, new, tau, cs, pd, vd = case
    tr = after.trace
    s, pin0, pin1, pin2 = tr["s"], tr["pin0"], tr["pin1"], tr["pin2"]
    assert np.array_equal(s, new) and np.array_equal(pin0, old)
    sw = ~s
    # early: pinned by the command, kept pinned, released
    assert (sw & ~pin0 & pin2).sum() >= 3 and (sw & pin0 & pin2).sum() >= 3 and (sw & pin0 & ~pin2).sum() >= 3
    assert (sw & ~pin0 & ~pin2).sum() >= 3                                   # ... and plain swing
    # late: landed at the edge (from below), still in the air, landing on this tick's command
    edge = s & ~pin0
    assert (edge & pin1).sum() >= 3 and (edge & ~pin1 & ~pin2).sum() >= 3 and (edge & ~pin1 & pin2).sum() >= 3
    assert (after.drop[edge & ~pin1 & ~pin2] > 0).all() and (after.drop[pin2 | sw] == 0).all()
    assert (after.grf[~pin1] == 0).all()                                     # no load before landing
    # sliding, one slide over a tread edge, unsaturated feet that do not move a bit, the speed's cap
    slid = tr["slid"]
    held = pin1 & pin2 & ~slid
    assert slid.sum() >= 6 and held.sum() >= 10 and np.array_equal(after.foot[held], np.where(tr["land"][..., None], after.foot, m0.foot)[held])
    moved = np.linalg.norm(after.foot[..., :2] - m0.foot[..., :2], axis=-1)
    kept = slid & pin2 & s
    assert (moved[kept] > 0).all()
    if after.mu_b is None and after.force is None:                           # (the edge was placed for the plain robots)
        k0 = np.floor(m0.tread(m0.foot[..., 0], m0.foot[..., 1]))
        k1 = np.floor(after.tread(after.foot[..., 0], after.foot[..., 1]))
        inside = (np.minimum(k0, k1) >= -1) & (np.maximum(k0, k1) <= 3)
        assert (kept & (k0 != k1) & inside).any()
        assert (after.slip - m0.slip).max() >= 0.9 * after.h * after.substeps * after.slip_vmax      # somebody is capped
    assert ((after.slip - m0.slip)[slid.any(1)] > 0).all() and np.array_equal(after.slip[~slid.any(1)], m0.slip[~slid.any(1)])
    # all four feet unpinned through the substeps: support is kept
    none = ~pin1.any(1)
    assert none.sum() >= 2 and np.array_equal(after.support[none], m0.support[none])
    assert np.array_equal(after.early - m0.early, (sw & pin2).sum(1)) and np.array_equal(after.late - m0.late, (edge & ~pin1).sum(1))
    assert {n for n, *_ in after.ties} == {"edge", "cone", "touch"}
    check_ties(after)


def check_ties(after):
    """No comparison the step branched on is within EDGE (relative to its operands) of a tie."""
    for name, a, b, where in after.ties:
        if where.any():
            gap = (np.abs(a - b) / np.maximum(np.abs(a), np.abs(b)))[where]
            assert gap.min() >= EDGE, (name, float(gap.min()))
    if after.rows is None:
        return
    u = np.concatenate(after.floors)
    assert len(u) >= 2 * B * 4 and (np.abs(u - np.round(u)) >= EDGE * np.maximum(1.0, np.abs(u))).all()


def result(m):
    """Everything a step writes, one row per robot."""
    return np.concatenate([m.state, m.foot.reshape(B, 12), m.motor, m.grf.reshape(B, 12), m.support[:, None],
                           m.ground[:, None], m.drop, m.slip[:, None], m.stance.astype(float),
                           m.early[:, None].astype(float), m.late[:, None].astype(float)], 1)


def sensitivity(substeps=1):
    """-> {what: how far the case's result moves} for each contact flag dropped and each parameter changed, on the model:
    the parity on this case cannot pass on a kernel that ignores one of them."""
    case = parity_case(substeps)
    base = result(stepped(case, substeps))
    out = {}
    for k, name in enumerate(("early", "late", "slip")):
        flags = tuple(j != k for j in range(3))
        out[f"flag {name} dropped"] = float(np.abs(result(stepped(case, substeps, flags=flags)) - base).max())
    for name, val in PARAMS.items():
        out[f"{name} doubled"] = float(np.abs(result(stepped(case, substeps, **{name: 2 * val})) - base).max())
    out["terrain flag rebase_z dropped"] = float(np.abs(result(stepped(case, substeps, tflags=(True, False))) - base).max())
    # (with `early` a swing foot below the surface is pinned, so the terrain's swing clamp has nothing left to lift:
    #  it is felt without `early`)
    no_early = (False, True, True)
    out["terrain flag clamp_swing dropped (without early)"] = float(np.abs(
        result(stepped(case, substeps, flags=no_early, tflags=(False, True))) - result(stepped(case, substeps, flags=no_early))).max())
    return out
