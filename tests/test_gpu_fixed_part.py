"""GPU suite (-m gpu): the fixed part of the solve in front of the sweep -- stage 0's float transcendentals (cos / sin of the
yaw, roll, pitch, yaw from the quaternion), the tracking-error rows built from them, M_b / N_b and the coefficient tables --
at the shapes where that code changes path, in every instantiation that shares it.  A rearrangement of these stages
(which wave evaluates what, what is handed on through LDS) must leave every figure below where it is.

Shapes: the smallest at which that code takes another path.
  * horizons 1, 10, 15, 16 ((h + 1)^2 crosses the 256 threads of the 64-row class at h = 16 -- a second table entry per
    thread --, 12 h crosses a wave at 6, 11 and 16; h = 1 leaves most scan lanes empty), and 5, the longest horizon whose
    ALL-STANCE table (60 rows) still fits the 64-row class;
  * batches 1 and 65;
  * contact tables: random (at most 21 stance foot-steps, so that the 64-row instantiations take them), all-swing, one
    foot on the last step only, and all four feet down at h = 5;
  * x_drag zero and non-zero.

Bounds.
  (a) cos / sin of the yaw and roll, pitch, yaw as the kernel evaluated them (dbg_aux) against numpy float32 evaluations
      of the same float expressions: 3e-7 for cos / sin and 1e-6 for the angles, the figures solve_gpu.py
      (dump_model_compare) uses -- two float ulps of the device's routine plus the same of numpy's at |cos| <= 1
      (ulp 6e-8) and at |angle| < 4 (ulp 2.4e-7).
  (b) the same robots through the 64-row class four per CU, five per CU (qmpc_set_dense) and through the 96-row class
      (solve_gpu.route c1, c6, c4: stance hint raised; at h = 1 and 5 the chain has no such class, 12 h <= 64, and the third run is the 64-row class
      again): identical dbg_aux bits; forces within 1e-9 of the largest force, the bound test_size_hint
      uses between instantiations.
  (c) forces against the oracle pipeline, per robot, max(1e-4, 1.5 x the reference's float-order spread) (bound_for).
"""
import numpy as np
import pytest

from oracle import oracle as O
from quadruped_ctrl_amd import workloads as W
from solve_gpu import bound_for, rel_f0, report, route

pytestmark = pytest.mark.gpu
MAX_ST = 21  # stance foot-steps the 64-row class holds (3 x 21 = 63 rows)


def make_case(h, B, drag):
    rng = np.random.default_rng(4200 + 10 * h + B)
    b = W.make_standing(B, h, seed=300 + h)
    g = np.zeros((B, 4 * h), np.uint8)
    for i in range(B):
        kind = i % 4
        if kind == 0 or kind == 3:  # random table, thinned to what the 64-row class takes
            t = (rng.random(4 * h) < 0.5).astype(np.uint8)
            on = np.flatnonzero(t)
            if on.size > MAX_ST:
                t[rng.choice(on, on.size - MAX_ST, replace=False)] = 0
            if h == 5 and kind == 3:
                t[:] = 1  # all four feet down on every step: 60 rows
            g[i] = t
        elif kind == 2:
            g[i, 4 * (h - 1) + int(rng.integers(0, 4))] = 1  # one foot, last step only
        # kind == 1: all swing
    b["gait"] = g
    # attitudes away from zero, a yaw of either sign and beyond pi / 2 (every quadrant of atan2f)
    rpy = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-3.0, 3.0, B)], 1)
    b["q"] = W._quat_from_rpy(rpy).astype(np.float32)
    b["yaw"] = rpy[:, 2].astype(np.float32)
    b["traj"].reshape(B, h, 12)[:, :, 2] = b["yaw"][:, None]
    b["x_drag"] = rng.normal(0, 0.7, B).astype(np.float32) if drag else np.zeros(B, np.float32)
    return b


def angles_f32(b):
    """cos yaw, sin yaw, roll, pitch, yaw: the kernel's float expressions (products and sums one by one) in numpy float32."""
    f = np.float32
    w, x, y, z = (b["q"][:, k].astype(f) for k in range(4))
    roll = np.arctan2(f(2) * (y * z + w * x), w * w - x * x - y * y + z * z)
    yaw = np.arctan2(f(2) * (x * y + w * z), w * w + x * x - y * y - z * z)
    asd = np.minimum(-2.0 * (x * z - w * y).astype(np.float64), .99999)
    pitch = np.arcsin(asd.astype(f))
    for a in (roll, yaw, pitch):
        assert a.dtype == f
    return np.stack([np.cos(b["yaw"].astype(f)), np.sin(b["yaw"].astype(f)), roll, pitch, yaw], 1).astype(np.float64)


def run(m, b):
    aux = m.debug_aux(b["batch"])
    res = m.solve(b, full=True)
    a = aux.cpu().numpy()[:, :5].copy()
    m.debug_off()
    assert ((res["status"] & 47) == 0).all(), np.unique(res["status"])
    return res, a


@pytest.mark.parametrize("h", [1, 5, 10, 15, 16])
def test_fixed_part(h, mpc_factory):
    m = None
    for B in (1, 65):
        for drag in (False, True):
            b = make_case(h, B, drag)
            nst = (b["gait"] != 0).sum(1)
            assert nst.max() <= MAX_ST
            if m is None:
                m = mpc_factory(b, max_batch=65)
            # the 64-row class, four workgroups per CU
            route(m, "c1")
            r1, a1 = run(m, b)
            # (a) the transcendentals as evaluated
            ref = angles_f32(b)
            d = np.abs(a1 - ref)
            print(f"h={h} B={B} drag={drag}: cos/sin diff max {d[:, :2].max():.2e}, angles diff max {d[:, 2:].max():.2e}")
            assert d[:, :2].max() < 3e-7 and d[:, 2:].max() < 1e-6
            # (b) five per CU, and the 96-row class
            route(m, "c6")
            r6, a6 = run(m, b)
            route(m, "c4")
            r4, a4 = run(m, b)
            assert np.array_equal(a1.view(np.int64), a6.view(np.int64))
            assert np.array_equal(a1.view(np.int64), a4.view(np.int64))
            tol = 1e-9 * np.abs(r1["grf"]).max()
            d6, d4 = np.abs(r6["grf"] - r1["grf"]).max(), np.abs(r4["grf"] - r1["grf"]).max()
            print(f"   instantiations: five per CU {d6:.2e}, 96-row class {d4:.2e} (bound {tol:.2e})")
            assert d6 <= tol and d4 <= tol
            assert np.all(r1["grf"][nst == 0] == 0) and np.all(r1["iters"][nst == 0] == 0)
            # (c) the oracle pipeline
            oref, nwsr, rc = O.solve_batch(b)
            assert (rc == 0).all()
            err = rel_f0(r1["grf"], oref)
            bd = bound_for(b, err=err)
            report(f"fixed part h={h} B={B} drag={drag}", err, bd)
            assert (err < bd).all()
