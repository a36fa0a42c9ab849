"""CPU suite for the batched controller's ticks driven by simulator ground truth (qmpc_ctrl_prework_state /
qmpc_ctrl_tick_state, include/qmpc_ctrl.h): the restatement of the cheater estimators in tests/ctrl_model_state.py on
hand cases and against fp64, workloads.make_state_stream, and the library's exports."""
import ctypes as C
import os
import re

import numpy as np

from quadruped_ctrl_amd import binding, workloads as W

import ctrl_model as M
from ctrl_model_state import ACC, OMEGA, ORI, POS, VBODY, as_imu, estimate_state, rebase_yaw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
MOTOR = np.tile(np.concatenate([np.tile([0.0, -0.8, 1.6], 4), np.zeros(12)]), (1, 1))


def _row(q, pos=(0.1, -0.2, 0.29), w=(0.3, -0.1, 0.2), vb=(1.0, 2.0, 3.0), acc=(0.5, -0.25, 9.81)):
    return np.array([list(q) + list(pos) + list(w) + list(vb) + list(acc)], f64)


def test_identity_quaternion():
    st = _row((1, 0, 0, 0))
    m = M.CtrlModel(1)
    before = {k: getattr(m, k).copy() for k in ("xhat", "P", "first_visit", "ori_ini_inv")}
    e = estimate_state(m, st, MOTOR)
    assert np.array_equal(e["r_body"], np.eye(3, dtype=f32).reshape(1, 9))
    assert np.array_equal(e["orientation"], np.array([[1, 0, 0, 0]], f32)) and (e["rpy"] == 0).all()
    assert np.array_equal(e["v_world"], st[:, VBODY].astype(f32)) and np.array_equal(e["v_body"], e["v_world"])
    assert np.array_equal(e["omega_world"], st[:, OMEGA].astype(f32)) and np.array_equal(e["omega_body"], e["omega_world"])
    assert np.array_equal(e["a_world"], st[:, ACC].astype(f32))
    assert np.array_equal(e["position"], st[:, POS].astype(f32))     # rounded to float once: 0.1 is not a float
    assert e["position"].dtype == f32 and float(e["position"][0, 0]) != 0.1
    for k, v in before.items():                                       # no filter, no first visit
        assert np.array_equal(getattr(m, k), v), k
    assert set(e) == {"orientation", "rpy", "r_body", "omega_body", "omega_world", "a_world", "position", "v_world",
                      "v_body", "leg_q", "qd", "leg_J", "leg_p", "leg_v"}     # CtrlModel.estimate's keys and v_body


def test_quarter_turn_from_the_rounded_floats():
    """q = (s, 0, 0, s) with s = float(sqrt(1/2)) = 0.70710677: s * s rounds to 1/2 - 2^-25, so 2 s s = 1 - 2^-24 and
    1 - 2 s s = 2^-24 -- R = [[2^-24, -(1 - 2^-24), 0], [1 - 2^-24, 2^-24, 0], [0, 0, 1]], rBody its transpose; the
    quaternion is used as given (its norm is not 1 in float)."""
    s = f32(np.sqrt(0.5))
    assert s == f32(0.70710677) and f32(s * s) == f32(0.5 - 2.0 ** -25)
    c, d = f32(2.0 ** -24), f32(1 - 2.0 ** -24)
    vb, w, acc = (f32(1), f32(2), f32(3)), (f32(0.3), f32(-0.1), f32(0.2)), (f32(0.5), f32(-0.25), f32(9.81))
    e = estimate_state(M.CtrlModel(1), _row((s, 0, 0, s)), MOTOR)
    assert np.array_equal(e["orientation"][0], np.array([s, 0, 0, s], f32))
    assert np.array_equal(e["r_body"][0], np.array([c, d, 0, -d, c, 0, 0, 0, 1], f32))
    for name, x in (("v_world", vb), ("omega_world", w), ("a_world", acc)):
        want = [f32(f32(f32(c * x[0]) + f32(-d * x[1])) + f32(f32(0) * x[2])),
                f32(f32(f32(d * x[0]) + f32(c * x[1])) + f32(f32(0) * x[2])),
                f32(f32(f32(f32(0) * x[0]) + f32(f32(0) * x[1])) + f32(f32(1) * x[2]))]
        assert np.array_equal(e[name][0], np.array(want, f32)), name
    # vBody (1, 2, 3) turned by a quarter: (-2, 1, 3) up to the two roundings above
    assert np.abs(e["v_world"][0] - np.array([-2, 1, 3], f32)).max() <= 2.0 ** -22
    assert abs(float(e["rpy"][0, 2]) - np.pi / 2) < 1e-6 and (e["rpy"][0, :2] == 0).all()


def test_products_against_fp64_of_the_same_floats():
    """omega_world, a_world and v_world are length-3 dot products in float: each component lies within
    gamma_3 sum |r_ik| |x_k| of the fp64 value of the same float operands, gamma_3 = 3 u / (1 - 3 u), u = 2^-24."""
    state, motor = W.make_state_stream(300, 3, 17)
    u = 2.0 ** -24
    gamma3 = 3 * u / (1 - 3 * u)
    for t in range(3):
        e = estimate_state(M.CtrlModel(300), state[t], motor[t])
        rB = e["r_body"].reshape(-1, 3, 3).astype(f64)
        for name, x in (("omega_world", e["omega_body"]), ("a_world", state[t][:, ACC].astype(f32)), ("v_world", e["v_body"])):
            x = x.astype(f64)
            exact = np.einsum("bki,bk->bi", rB, x)                         # rBody^T x
            bound = gamma3 * np.einsum("bki,bk->bi", np.abs(rB), np.abs(x))
            err = np.abs(e[name].astype(f64) - exact)
            assert (err <= bound).all(), (name, t, (err / bound).max())
            assert err.max() > 0                                            # (the float result is not the fp64 one)


def test_make_state_stream():
    B, T = 9, 50
    state, motor = W.make_state_stream(B, T, 5)
    assert state.shape == (T, B, 16) and motor.shape == (T, B, 24) and state.dtype == f64 and motor.dtype == f64
    s2, m2 = W.make_state_stream(B, T, 5)
    assert np.array_equal(state, s2) and np.array_equal(motor, m2)
    s3, _ = W.make_state_stream(B, T, 6)
    assert not np.array_equal(state, s3)
    assert np.abs(np.linalg.norm(state[..., ORI], axis=-1) - 1).max() < 1e-12
    imu, motor_i = W.make_tick_stream(B, T, 5)
    assert np.array_equal(motor, motor_i)
    assert np.array_equal(as_imu(state), imu)                                # quaternion, gyro, accelerometer
    assert np.array_equal(state[..., 0], imu[..., 6]) and np.array_equal(state[..., 1:4], imu[..., 3:6])
    assert np.array_equal(state[..., OMEGA], imu[..., 7:10]) and np.array_equal(state[..., ACC], imu[..., 0:3])
    # position near (0, 0, 0.29), drifting smoothly by centimetres; vBody inside the tests' velocity commands
    pos, vb = state[..., POS], state[..., VBODY]
    assert np.abs(pos - np.array([0, 0, 0.29])).max() < 0.05 and np.ptp(pos[..., 0], axis=0).max() > 1e-3
    assert np.abs(np.diff(pos, axis=0)).max() < 1e-3
    assert (vb[..., 0] > -0.8).all() and (vb[..., 0] < 1.5).all() and np.abs(vb[..., 1]).max() < 0.4   # ctrl_model.command_vel
    assert np.abs(vb).max() > 0.05
    # roll / joint as in make_tick_stream
    sr, mr = W.make_state_stream(B, T, 5, roll=(2, 0.7, 10), joint=(3, 4, 0.5, 7))
    ir, mi = W.make_tick_stream(B, T, 5, roll=(2, 0.7, 10), joint=(3, 4, 0.5, 7))
    assert np.array_equal(mr, mi) and (mr[7:, 3, 4] == 0.5).all() and np.array_equal(mr[:7], motor[:7])
    assert np.array_equal(sr[..., 1:4], ir[..., 3:6]) and np.array_equal(sr[:10], state[:10])
    rpy = M.quat_to_rpy(sr[:, 2, ORI].astype(f32))
    assert np.abs(rpy[10:, 0] - 0.7).max() < 1e-6 and np.abs(rpy[:10, 0]).max() < 0.05
    keep = np.arange(B) != 2
    assert np.array_equal(sr[:, keep], state[:, keep])


def test_rebase_yaw_turns_about_the_world_z_axis_only():
    state, _ = W.make_state_stream(40, 30, 9)
    r = rebase_yaw(state)
    assert np.abs(np.linalg.norm(r[..., ORI], axis=-1) - 1).max() < 1e-12
    a = M.quat_to_rpy(state[..., ORI].reshape(-1, 4).astype(f32)).reshape(30, 40, 3).astype(f64)
    b = M.quat_to_rpy(r[..., ORI].reshape(-1, 4).astype(f32)).reshape(30, 40, 3).astype(f64)
    assert np.abs(b[0, :, 2]).max() < 1e-6 and np.abs(a[0, :, 2]).max() > 2.5        # every robot starts at yaw 0
    assert np.abs(a[..., :2] - b[..., :2]).max() < 1e-6                                # roll and pitch are kept
    d = (a[..., 2] - a[0, :, 2]) - b[..., 2]
    assert np.abs((d + np.pi) % (2 * np.pi) - np.pi).max() < 1e-6                     # yaw is shifted by the tick-0 yaw
    keep = np.ones(16, bool)
    keep[ORI] = False
    assert np.array_equal(r[..., keep], state[..., keep])


def test_state_symbols_exported():
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "qmpc_ctrl.h")).read()
    decl = set(re.findall(r"^int (qmpc_[a-z_]+)\s*\(", hdr, re.M))
    lib = C.CDLL(binding.LIB_PATH)
    for name in ("qmpc_ctrl_prework_state", "qmpc_ctrl_tick_state"):
        assert name in decl and name in binding.CTRL_EXPORTS and hasattr(lib, name), name
    assert binding.CTRL_SIGNATURES["qmpc_ctrl_prework_state"] == [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    assert binding.CTRL_SIGNATURES["qmpc_ctrl_tick_state"] == [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    lib = binding.load_library()
    assert lib.qmpc_ctrl_prework_state(None, 1, None, None, None) == 1       # QMPC_ERR_ARG: a null handle
    assert lib.qmpc_ctrl_tick_state(None, 1, None, None, None, None) == 1
    for m in ("prework_state", "tick_state"):
        assert callable(getattr(binding.BatchedController, m))
