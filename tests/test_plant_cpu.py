"""CPU suite for the reduced-order plant (include/qmpc_plant.h): the exported surface, and the numpy restatement
tests/plant_model.py on the closed forms it must reproduce -- the same model the GPU suite (tests/test_gpu_plant.py)
holds the kernel to; the closed forms themselves are functions of the model's constructor arguments in
tests/plant_cases.py, run here at the handle's defaults -- and the CPU closed loop against the reference pipeline that
the GPU walk is measured by."""
import json
import os
import re

import numpy as np

import plant_cases as PC
import plant_loop as L
import plant_model as PM
from plant_cases import STAND, none as _none

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plant_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_plant.h")).read()
    decl = set(re.findall(r"^int (qmpc_\w+)\(", hdr, re.M))
    want = {"qmpc_plant_init", "qmpc_plant_reset", "qmpc_plant_step", "qmpc_plant_view_get"}
    assert decl == want == set(binding.PLANT_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the view structure of the binding follows the header's member order
    body = re.search(r"typedef struct \{(.*?)\} qmpc_plant_view;", hdr, re.S).group(1)
    members = re.findall(r"(\w+);", body)
    assert members == [n for n, _ in binding.PlantView._fields_]


def test_fk_ik_round_trip():
    """FK(IK(p)) = p over a box around the stand pose and IK(FK(q)) = q over a box of angles with the knee bent
    forwards (knee > 0), all four legs; fp64 rounding of a dozen operations on O(1) values: 1e-12."""
    g = np.linspace(-0.08, 0.08, 9)
    box = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 3)
    p = STAND[None] + box
    ang = PM.leg_ik(p)
    assert (ang[..., 2] > 0).all()
    _, back = PM.leg_fk(ang)
    assert np.abs(back - p).max() < 1e-12
    a, h, k = np.meshgrid(np.linspace(-0.5, 0.5, 7), np.linspace(-1.4, -0.2, 9), np.linspace(0.5, 2.2, 9), indexing="ij")
    q = np.broadcast_to(np.stack([a, h, k], -1).reshape(-1, 1, 3), (a.size, 4, 3))
    _, pq = PM.leg_fk(q)
    assert np.abs(PM.leg_ik(pq) - q).max() < 1e-12
    # the stand pose itself is on qmpc_leg_fk's branch: hip back, knee forwards, inside checkJointLimit's box
    s = PM.leg_ik(STAND)
    assert (np.abs(s[:, 0]) < 0.02).all() and (s[:, 1] < -0.5).all() and (s[:, 2] > 1.0).all()


def test_free_fall_matches_the_recurrence_exactly():
    PC.free_fall()


def test_symmetric_stance_is_an_equilibrium():
    PC.hover()


def test_quaternion_stays_normalised_and_principal_axis_rotation_keeps_omega():
    PC.spin()


def test_unilateral_friction_and_straight_knee():
    PC.friction_and_straight_knee()


def test_joint_rates_against_a_finite_difference_of_the_angles():
    """A pinned foot's joint rates: the plant's formula (rdot = -rBody v - w x (rBody (c - p)), qd = J^-1 rdot) against
    a central difference of the model's own angles along the exact rigid motion p + t v, q (x) exp(t w).  Step 1e-6 s:
    truncation ~ t^2 |q'''| / 6 ~ 1e-10 at these rates, rounding ~ 1e-16 / 1e-6 = 1e-10; the bound is 1e-7, and dropping
    or misplacing the hip offset in the lever arm is an error of |w| |hip| / l ~ 1 rad/s."""
    B = 5
    rng = np.random.default_rng(7)
    pl = PM.PlantModel(B, 500.0, 0.4, 1, rng.uniform(-1, 1, (B, 3)))
    pl.v[:] = rng.uniform(-0.5, 0.5, (B, 3))
    pl.w[:] = rng.uniform(-2, 2, (B, 3))
    ones = np.ones((B, 4), bool)
    z3 = np.zeros((B, 3))
    _, motor, _ = pl._readout(pl.p, pl.v, pl.q, pl.w, pl.foot, ones, z3, None, None)

    def angles(t):
        a = np.linalg.norm(pl.w, axis=1) * t
        dq = np.concatenate([np.cos(a / 2)[:, None], np.sin(a / 2)[:, None] * pl.w / np.linalg.norm(pl.w, axis=1)[:, None]], 1)
        q0, q1, q2, q3 = (pl.q[:, k] for k in range(4))
        d0, d1, d2, d3 = (dq[:, k] for k in range(4))
        q = np.stack([q0 * d0 - q1 * d1 - q2 * d2 - q3 * d3, q0 * d1 + q1 * d0 + q2 * d3 - q3 * d2,
                      q0 * d2 - q1 * d3 + q2 * d0 + q3 * d1, q0 * d3 + q1 * d2 - q2 * d1 + q3 * d0], 1)
        return pl._readout(pl.p + t * pl.v, pl.v, q, pl.w, pl.foot, ones, z3, None, None)[1][:, :12]

    t = 1e-6
    fd = (angles(t) - angles(-t)) / (2 * t)
    assert np.abs(motor[:, 12:]).max() > 0.5
    assert np.abs(fd - motor[:, 12:]).max() < 1e-7


def test_swing_foot_tracks_its_command_and_is_clamped_to_the_shell():
    B = 2
    pl = PM.PlantModel(B, 500.0, 0.4, 1, np.array([[0, 0, 0.5], [1, 1, -0.5]]))
    cs = np.zeros((B, 4), np.float32)
    pd = np.tile(STAND.reshape(1, 12), (B, 1)).astype(np.float32)
    pd[0, 0:3] = [0.05, -0.07, -0.2]
    pd[1, 0:3] = [0.0, -0.065, -0.6]                              # out of reach: scaled back to knee angle 0.05
    vd = np.zeros((B, 12), np.float32)
    vd[0, 0:3] = [0.4, 0.0, -0.2]
    st, mo = pl.step(np.zeros((B, 12)), cs, pd, vd)
    J, p = PM.leg_fk(mo[:, :12].reshape(B, 4, 3))
    assert np.abs(p[0, 0] - pd[0, 0:3].astype(np.float64)).max() < 1e-12
    v = np.stack([(J[0, 0, 3 * k] * mo[0, 12] + J[0, 0, 3 * k + 1] * mo[0, 13]) + J[0, 0, 3 * k + 2] * mo[0, 14] for k in range(3)])
    assert np.abs(v - vd[0, 0:3]).max() < 1e-12
    assert abs(mo[1, 2] - PM.KNEE_MIN) < 1e-9 and np.abs(p[1, 0] / np.linalg.norm(p[1, 0]) - pd[1, 0:3] / np.linalg.norm(pd[1, 0:3])).max() < 1e-7
    # the world position follows the body: c = p + R (hip + r)
    R = PM.rot(pl.q)
    assert np.abs(pl.foot - (pl.p[:, None, :] + PM.mul(R[:, None, :], PM.HIP + p))).max() < 1e-12
    # touch-down pins it on the ground, where it stays
    c = pl.foot.copy()
    pl.step(np.zeros((B, 12)), np.ones((B, 4), np.float32), pd, vd)
    assert np.array_equal(pl.foot[..., :2], c[..., :2]) and (pl.foot[..., 2] == 0).all() and pl.stance.all()


def test_reset_restores_masked_robots_only():
    B = 4
    xy = np.array([[0, 0, 0], [1, 0, 0.2], [2, 0, -0.2], [3, 0, 0.1]], np.float64)
    pl, fresh = PM.PlantModel(B, 500.0, 0.4, 1, xy), PM.PlantModel(B, 500.0, 0.4, 1, xy)
    cs, pd, vd = _none(B)
    for _ in range(5):
        pl.step(np.zeros((B, 12)), cs, pd, vd)
    keep = {k: getattr(pl, k).copy() for k in ("p", "v", "q", "w", "foot", "stance", "state", "motor")}
    mask = np.array([1, 0, 1, 0], bool)
    pl.reset(mask, xy)
    for k, old in keep.items():
        assert np.array_equal(getattr(pl, k)[mask], getattr(fresh, k)[mask]), k
        assert np.array_equal(getattr(pl, k)[~mask], old[~mask]), k


def test_cpu_closed_loop_is_safe_and_is_what_the_fixture_records():
    """The yardstick of the GPU walk: plant_model + the controller's restatements + the reference's qpOASES, 16 robots,
    650 ticks, modes 0 and 1.  The reference pipeline alone keeps every robot safe on the command set (safe == 1 covers
    the orientation and joint-limit latches; every solve returns 0 below the nWSR cap of 100), and the statistics are
    those of tests/golden/plant_closed_loop_cpu.json (another libm may move them in the last digits: the loop is not
    chaotic over 1.3 s on these commands, 1e-6 holds a last-bit difference amplified a billion times)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plant_closed_loop_cpu.json")))
    assert gold["ticks"] == L.TICKS == 650 and tuple(gold["pid"]) == L.PID
    for mode in (0, 1):
        stats, info = L.cpu_loop(mode)
        rec = gold[f"mode{mode}"]
        gait, vel, xyyaw = L.commands(mode)
        assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
        assert (info["safe"] == 1).all() and info["rc_bad"] == 0 and info["nwsr_max"] < 100, (mode, info)
        assert info["n_solves"] >= 16 * 45
        assert vel[:, 0].min() == 0 and vel[:, 0].max() <= 0.5 and np.abs(vel[:, 2]).max() <= 0.1
        if mode == 0:
            assert set(gait) == {0, 4, 5, 10}
        for k in L.STATS:
            print(mode, k, np.abs(stats[k] - np.asarray(rec[k])).max())
            assert np.abs(stats[k] - np.asarray(rec[k])).max() < 1e-6, (mode, k)
        # the robots walk: the height settles near the controller's 0.25, the speed follows the command
        assert (stats["z_min"] > 0.2).all() and (stats["roll_max"] < 0.1).all() and (stats["pitch_max"] < 0.1).all()
        assert np.abs(stats["vx_mean"] - vel[:, 0]).max() < 0.05
        lo_hi = L.envelope(rec)
        for k in L.STATS:
            assert (stats[k] >= lo_hi[k][0]).all() and (stats[k] <= lo_hi[k][1]).all(), (mode, k)
