"""The estimator stage of a tick driven by simulator ground truth (qmpc_ctrl_tick_state) -- TEST SIDE ONLY.

estimate_state() restates in numpy float32, operation by operation, what qmpc_glue.hip's qmpc_ctrl_est_state_kernel
computes: CheaterOrientationEstimator::run (src/Controllers/OrientationEstimator.cpp:21-39),
CheaterPositionVelocityEstimator::run (src/Controllers/PositionVelocityEstimator.cpp:229-238) and
LegController::updateData (oracle.glue.leg_update), on tests/ctrl_model.py's own pieces: CtrlModel.derived for the
rotation matrix and rpy, rowT for the three rBody^T products.  The model's filter and first-visit state are not touched.
"""
import numpy as np

from oracle import glue as G

import ctrl_model as M

f32, f64 = np.float32, np.float64

# CheaterState<double> member order (src/Utilities/IMUTypes.h:25-32): columns of state[B][16]
ORI, POS, OMEGA, VBODY, ACC = slice(0, 4), slice(4, 7), slice(7, 10), slice(10, 13), slice(13, 16)


def as_imu(state):
    """The imu[B][10] row (accelerometer, quaternion x y z w, gyro) that carries the same quaternion, omegaBody and
    acceleration as state[B][16]."""
    state = np.asarray(state, f64)
    imu = np.zeros(state.shape[:-1] + (10,))
    imu[..., 0:3] = state[..., ACC]
    imu[..., 3:6] = state[..., 1:4]
    imu[..., 6] = state[..., 0]
    imu[..., 7:10] = state[..., OMEGA]
    return imu


def estimate_state(model, state, motor):
    """-> the dict of CtrlModel.estimate, with position, v_world and v_body from the state; updates the model's leg
    data in place (as estimate does) and nothing else of it."""
    state = np.asarray(state, f64)
    q = state[:, ORI].astype(f32)                       # .template cast<float>(): used as given, not normalised
    est = M.CtrlModel.derived(q, as_imu(state))         # rpy, r_body = R^T, omega_body
    rB = est["r_body"]
    w, a, vb = est["omega_body"], state[:, ACC].astype(f32), state[:, VBODY].astype(f32)
    est["omega_world"] = np.stack([M.rowT(rB, k, w[:, 0], w[:, 1], w[:, 2]) for k in range(3)], 1)
    est["a_world"] = np.stack([M.rowT(rB, k, a[:, 0], a[:, 1], a[:, 2]) for k in range(3)], 1)
    motor = np.asarray(motor, f64)
    qj, qd = motor[:, :12].astype(f32), motor[:, 12:].astype(f32)
    J, p, v = G.leg_update(qj, qd, model.geom)
    model.leg_p, model.leg_v = p, v
    est.update(position=state[:, POS].astype(f32),
               v_world=np.stack([M.rowT(rB, k, vb[:, 0], vb[:, 1], vb[:, 2]) for k in range(3)], 1), v_body=vb,
               leg_q=qj, qd=qd, leg_J=J.reshape(len(state), 36), leg_p=p, leg_v=v)
    return est


def rebase_yaw(state):
    """state[T,B,16] with every robot's yaw reported relative to its yaw at tick 0: orientation <- qz(-yaw_0) (x) orientation
    in float64 -- a simulator whose world frame is the robot's start heading, which is what the sensor path's
    VectorNavOrientationEstimator makes of its quaternion (_ori_ini_inv).  The controller starts with _yaw_des_true = 0
    and re-anchors it only beyond 5 rad (ConvexMPCLocomotion.cpp:106), so only such a start is the situation the
    sensor-path tests put it in; roll, pitch, body-frame rates and everything else are unchanged."""
    state = np.array(state, f64)
    w, x, y, z = (state[0][:, k] for k in range(4))
    yaw0 = np.arctan2(2 * (x * y + w * z), ((w * w + x * x) - y * y) - z * z)
    c, s = np.cos(yaw0 / 2), -np.sin(yaw0 / 2)          # qz(-yaw0) = (c, 0, 0, s)
    w, x, y, z = (state[..., k].copy() for k in range(4))
    state[..., 0], state[..., 1], state[..., 2], state[..., 3] = c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w
    return state
