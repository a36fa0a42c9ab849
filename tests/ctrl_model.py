"""numpy float32 restatement of the batched locomotion controller (include/qmpc_ctrl.h) -- TEST SIDE ONLY.

Restates, operation by operation and vectorised over robots, what qmpc_glue.hip's controller kernels compute:
  estimate()   VectorNavOrientationEstimator::run (src/Controllers/OrientationEstimator.cpp:46-110,
               src/Utilities/orientation_tools.h:129-211,272-285) + LegController::updateData (oracle.glue.leg_update)
               + the Kalman filter (oracle.glue.kf_step) on the previous tick's leg data
  loco()       the safety checks (src/GaitCtrller.cpp:108-123, src/Controllers/SafetyChecker.cpp) and
               ConvexMPCLocomotion::run (src/MPC_Ctrl/ConvexMPCLocomotion.cpp:116-496) up to updateMPCIfNeeded
  command()    the qmpc_command rows of an MPC tick, for oracle.oracle.pack_commands -> solve_batch -> forces_to_body
  legcmd()     the gains of :378-382 and LegController::updateCommand (oracle.glue.leg_command), then the latch

The decisions written down in qmpc_glue.hip (abs(float) = the float overload, double sqrt, double promotion of pfx_rel / pfy_rel, truncated
walking integers, counter timing, setInitialPosition's _p) are restated here the same way; `float_sqrt=True` gives
the other overload binding, for the test that shows the choice is observable.
"""
import numpy as np

from oracle import glue as G

f32, f64 = np.float32, np.float64
NSEG, IBM = 14, 13           # horizonLength, iterationsBetweenMPC
HIP = np.array([[0.19, -0.049, 0], [0.19, 0.049, 0], [-0.19, -0.049, 0], [-0.19, 0.049, 0]], f32)  # getHipLocation

# ConvexMPCLocomotion.cpp:27-41 at horizonLength 14; Vec4<int>(double) truncates (walking :37-38)
GAITS = {
    "trotting": ((0, 7, 7, 0), (7, 7, 7, 7)),
    "bounding": ((7, 7, 0, 0), (6, 6, 6, 6)),
    "pronking": ((0, 0, 0, 0), (6, 6, 6, 6)),
    "jumping": ((0, 0, 0, 0), (3, 3, 3, 3)),
    "galloping": ((0, 4, 7, 11), (7, 7, 7, 7)),
    "standing": ((0, 0, 0, 0), (14, 14, 14, 14)),
    "trotRunning": ((0, 7, 7, 0), (6, 6, 6, 6)),
    "walking": ((0, int(14 / 2.0), int(14 / 4.0), int(3.0 * 14 / 4.0)), (int(3.0 * 14 / 4.0),) * 4),
    "walking2": ((0, 7, 7, 0), (10, 10, 10, 10)),
    "pacing": ((7, 0, 7, 0), (7, 7, 7, 7)),
}
# robot mode 0 (:149-172)
GAIT_OF_NUMBER = {1: "bounding", 2: "pronking", 4: "standing", 5: "trotRunning", 7: "galloping", 8: "pacing",
                  9: "trotting", 10: "walking", 11: "walking2"}


def gait_name(gn):
    return GAIT_OF_NUMBER.get(int(gn), "trotting")


def split_gait(g):
    """set_gait_type's number -> (gait number, omni mode) (:127-132): 20 and above is omni, 20 subtracted."""
    g = np.asarray(g, np.int32)
    omni = g >= 20
    return np.where(omni, g - 20, g).astype(np.int32), omni


def mpc_table(offsets, durations, iteration, n=NSEG):
    """OffsetDurationGait::getMpcTable (Gait.cpp:142-166)."""
    t = np.zeros(4 * n, np.int32)
    for i in range(n):
        it = (i + iteration + 1) % n
        for j in range(4):
            pr = it - offsets[j]
            if pr < 0:
                pr += n
            t[i * 4 + j] = 1 if pr < durations[j] else 0
    return t


def gait_states(phase, off, dur, n=NSEG):
    """getContactState / getSwingState (Gait.cpp:61-123), vectorised: phase [B] f32, off / dur [B,4] int -> [B,4] x 2."""
    offF = off.astype(f32) / f32(n)
    durF = dur.astype(f32) / f32(n)
    pr = phase[:, None] - offF
    pr = np.where(pr < 0, pr + f32(1), pr)
    contact = np.where(pr > durF, f32(0), pr / durF).astype(f32)
    so = offF + durF
    so = np.where(so > 1, so - f32(1), so)
    sd = f32(1) - durF
    pr = phase[:, None] - so
    pr = np.where(pr < 0, pr + f32(1), pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        swing = np.where(pr > sd, f32(0), np.where(sd.astype(f64) < 1e-10, f32(0), pr / sd)).astype(f32)
    return contact, swing


def row3(R, k, x0, x1, x2):
    """row k of a [B,9] row-major matrix times (x0, x1, x2), ((a0 b0 + a1 b1) + a2 b2)."""
    return (R[:, 3 * k] * x0 + R[:, 3 * k + 1] * x1) + R[:, 3 * k + 2] * x2


def rowT(R, k, x0, x1, x2):
    """row k of R^T (column k of R) times x."""
    return (R[:, k] * x0 + R[:, 3 + k] * x1) + R[:, 6 + k] * x2


def bezier_axis(axis, p0, pf, p0z, pfz, h, ph, st):
    """computeSwingTrajectoryBezier (FootSwingTrajectory.cpp:17-37) for one axis (p, v)."""
    def bez(y0, yf, x):
        return y0 + (x * x * x + f32(3) * (x * x * (f32(1) - x))) * (yf - y0)

    def d1(y0, yf, x):
        return (f32(6) * x * (f32(1) - x)) * (yf - y0)
    if axis < 2:
        return bez(p0, pf, ph), d1(p0, pf, ph) / st
    lo = ph < f32(0.5)
    x_lo, x_hi = ph * f32(2), ph * f32(2) - f32(1)
    p = np.where(lo, bez(p0z, p0z + h, x_lo), bez(p0z + h, pfz, x_hi))
    v = np.where(lo, d1(p0z, p0z + h, x_lo) * f32(2) / st, d1(p0z + h, pfz, x_hi) * f32(2) / st)
    return p.astype(f32), v.astype(f32)


def quat_to_rpy(q):
    """ori::quatToRPY (orientation_tools.h:195-208); q [B,4] f32."""
    m = f64(-2.0) * (q[:, 1] * q[:, 3] - q[:, 0] * q[:, 2]).astype(f64)
    as_ = np.minimum(m, 0.99999).astype(f32)
    two = f32(2)
    r2 = np.arctan2(two * (q[:, 1] * q[:, 2] + q[:, 0] * q[:, 3]), ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) - q[:, 2] * q[:, 2]) - q[:, 3] * q[:, 3])
    with np.errstate(invalid="ignore"):
        r1 = np.arcsin(as_)
    r0 = np.arctan2(two * (q[:, 2] * q[:, 3] + q[:, 0] * q[:, 1]), ((q[:, 0] * q[:, 0] - q[:, 1] * q[:, 1]) - q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return np.stack([r0, r1, r2], 1).astype(f32)


def yaw_inverse_quat(yaw):
    """rpyToQuat((-0, -0, -yaw)) (orientation_tools.h:93-100, :129-162): Rz(-yaw) through coordinateRotation, then
    rotationMatrixToQuaternion; the X / Y factors are identities (sin(-0) = -0, cos = 1)."""
    th = -yaw
    s, c = np.sin(th).astype(f32), np.cos(th).astype(f32)
    z = np.zeros_like(s)
    one = np.ones_like(s)
    # R = Rz rows: (c, s, 0), (-s, c, 0), (0, 0, 1);  r = R^T
    r00, r01, r02 = c, -s, z
    r10, r11, r12 = s, c, z
    r20, r21, r22 = z, z, one
    tr = (r00 + r11) + r22
    q = np.zeros((len(yaw), 4), f32)
    a = tr > 0.0
    S = (np.sqrt(tr.astype(f64) + 1.0) * 2.0).astype(f32)
    qa = [(0.25 * S.astype(f64)).astype(f32), (r21 - r12) / S, (r02 - r20) / S, (r10 - r01) / S]
    b_ = (~a) & (r00 > r11) & (r00 > r22)
    Sb = (np.sqrt(((1.0 + r00.astype(f64)) - r11) - r22) * 2.0).astype(f32)
    qb = [(r21 - r12) / Sb, (0.25 * Sb.astype(f64)).astype(f32), (r01 + r10) / Sb, (r02 + r20) / Sb]
    c_ = (~a) & (~b_) & (r11 > r22)
    with np.errstate(invalid="ignore", divide="ignore"):
        Sc = (np.sqrt(((1.0 + r11.astype(f64)) - r00) - r22) * 2.0).astype(f32)
        qc = [(r02 - r20) / Sc, (r01 + r10) / Sc, (0.25 * Sc.astype(f64)).astype(f32), (r12 + r21) / Sc]
        Sd = (np.sqrt(((1.0 + r22.astype(f64)) - r00) - r11) * 2.0).astype(f32)
        qd = [(r10 - r01) / Sd, (r02 + r20) / Sd, (r12 + r21) / Sd, (0.25 * Sd.astype(f64)).astype(f32)]
    for k in range(4):
        q[:, k] = np.where(a, qa[k], np.where(b_, qb[k], np.where(c_, qc[k], qd[k])))
    return q


def fk64(q, leg, g=G.GEOM.astype(np.float64)):
    """Independent fp64 forward kinematics from the leg geometry: abad rotation about x, hip and knee
    about y (Mini Cheetah convention of computeLegJacobianAndPosition)."""
    l1, l2, l3, l4 = g
    side = -1.0 if leg % 2 == 0 else 1.0
    s1, c1 = np.sin(q[0]), np.cos(q[0])
    s2, c2 = np.sin(q[1]), np.cos(q[1])
    s23, c23 = np.sin(q[1] + q[2]), np.cos(q[1] + q[2])
    x = l3 * s23 + l2 * s2
    zz = -(l3 * c23 + l2 * c2)          # leg-plane "down" before the abad rotation
    yy = (l1 + l4) * side
    return np.array([x, yy * c1 - zz * s1, yy * s1 + zz * c1])


def calm_est(B, rng, roll=0.0):
    """An estimator read-out of B robots standing calmly: what loco() takes where no estimator runs."""
    return dict(position=np.stack([rng.normal(0, .1, B), rng.normal(0, .1, B), rng.uniform(.2, .3, B)], 1).astype(f32),
                v_world=rng.normal(0, .5, (B, 3)).astype(f32),
                rpy=np.stack([np.full(B, roll), rng.normal(0, .02, B), rng.normal(0, 1, B)], 1).astype(f32),
                r_body=np.tile(np.eye(3, dtype=f32).reshape(1, 9), (B, 1)),
                leg_p=np.tile(np.array([0, 0, -.28], f32), (B, 4)), leg_q=np.tile(np.array([0, -.8, 1.6], f32), (B, 4)))


# the commands of the GPU suites' runs (tests/test_gpu_controller.py and the files that follow it)
def command_gaits(B, t, switch_at):
    """Every gait number 0 .. 11 and its omni variant, switched part-way (into and out of standing)."""
    g = (np.arange(B) % 12).astype(np.int32)
    g = np.where(np.arange(B) % 24 >= 12, g + 20, g)
    if t >= switch_at:
        g = np.where(np.arange(B) % 3 == 0, 4, np.where(g % 20 == 4, 9 + 20 * (g >= 20), (g + 5) % 12)).astype(np.int32)
    return g


def command_vel(B, seed):
    rng = np.random.default_rng(seed)
    v = np.stack([rng.uniform(-0.8, 1.5, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-0.6, 0.6, B)], 1)
    v[::7] = 0.0           # robots standing still in command (yaw rate 0: coordinateRotation is exact there)
    v[1::11, 0] = 0.02     # inside the 0.03 dead band
    return v


class CtrlModel:
    """State of GaitCtrller / ConvexMPCLocomotion for B robots (numpy), same names as QmpcCtrlDev."""

    def __init__(self, B, freq=500.0, pid=(0.0, 0.0, 0.0, 0.0), float_sqrt=False, geom=G.GEOM):
        self.B = B
        self.geom = np.asarray(geom, f32)        # qmpc_set_leg_geometry's four lengths (the handle's floats)
        self.dt = f32(1.0 / freq)
        self.dt_mpc = self.dt * f32(13)
        self.kp_joint, self.kd_joint = f32(pid[2]), f32(pid[3])
        self.float_sqrt = float_sqrt
        self.reset(np.ones(B, bool), 0)

    def reset(self, mask, counter0):
        B = self.B
        m = np.asarray(mask, bool)
        z = lambda *s: np.zeros((B,) + s, f32)
        fresh = dict(
            xhat=z(18), P=np.tile((100 * np.eye(18, dtype=f32)).reshape(1, 324), (B, 1)), leg_p=z(12), leg_v=z(12),
            contact_phase=np.full((B, 4), 0.5, f32), ori_ini_inv=z(4), first_visit=np.ones(B, np.int32),
            vel_cmd=z(3), vel_des=z(3), yaw_des=z(), yaw_des_true=z(), rpy_int=z(2), rpy_comp=z(2), stand_traj=z(6),
            wpd=z(2), xci=z(), p_foot=z(12), sw_p0=z(12), sw_pf=z(12), sw_p=z(12), sw_v=z(12), swing_time=z(4),
            swing_rem=z(4), contact_state=z(4), swing_state=z(4), p_des=z(12), v_des=z(12), f_ff=z(12), pf_rel=z(8),
            counter=np.full(B, counter0, np.int32), first_run=np.ones(B, np.int32), first_swing=np.ones((B, 4), np.int32),
            gait_num=np.zeros(B, np.int32), current_gait=np.full(B, -1, np.int32), offsets=np.zeros((B, 4), np.int32),
            durations=np.zeros((B, 4), np.int32), iteration=np.zeros(B, np.int32), safe=np.ones(B, np.int32))
        for k, v in fresh.items():
            if not hasattr(self, k):
                setattr(self, k, v.copy())
            else:
                getattr(self, k)[m] = v[m]

    # ---- set_gait_type / SetRobotVel (GaitCtrller.cpp:75-93: abs(double) is the double overload there)
    def set_gait(self, g):
        self.gait_num[:] = np.asarray(g, np.int32)

    def set_vel(self, vel):
        vel = np.asarray(vel, f64)
        self.vel_cmd[:] = np.where(np.abs(vel) < 0.03, 0.0, vel * 1.0).astype(f32)

    # ---- pre_work: the estimators, then updateData
    def estimate(self, imu, motor):
        """-> dict of this tick's estimator outputs (float32); updates the filter and leg data in place."""
        imu = np.asarray(imu, f64)
        o = np.stack([imu[:, 6], imu[:, 3], imu[:, 4], imu[:, 5]], 1).astype(f32)
        fv = self.first_visit != 0
        if fv.any():
            rpy_ini = quat_to_rpy(o[fv])
            self.ori_ini_inv[fv] = yaw_inverse_quat(rpy_ini[:, 2])
            self.first_visit[fv] = 0
        inv = self.ori_ini_inv
        r1, r2 = inv[:, 0], o[:, 0]
        a0, a1, a2, b0, b1, b2 = inv[:, 1], inv[:, 2], inv[:, 3], o[:, 1], o[:, 2], o[:, 3]
        dot = (a0 * b0 + a1 * b1) + a2 * b2
        q = np.stack([r1 * r2 - dot, (r1 * b0 + r2 * a0) + (a1 * b2 - a2 * b1), (r1 * b1 + r2 * a1) + (a2 * b0 - a0 * b2),
                      (r1 * b2 + r2 * a2) + (a0 * b1 - a1 * b0)], 1).astype(f32)
        est = self.derived(q, imu)
        self.kf_leg_p, self.kf_leg_v = self.leg_p.copy(), self.leg_v.copy()
        motor = np.asarray(motor, f64)
        qj, qd = motor[:, :12].astype(f32), motor[:, 12:].astype(f32)
        J, p, v = G.leg_update(qj, qd, self.geom)
        self.leg_p, self.leg_v = p, v
        pos, vw, _ = G.kf_step(self.xhat, self.P, est["r_body"], est["a_world"], est["omega_body"], self.contact_phase,
                               self.kf_leg_p, self.kf_leg_v)
        est.update(position=pos, v_world=vw, leg_q=qj, qd=qd, leg_J=J.reshape(self.B, 36), leg_p=p, leg_v=v)
        return est

    @staticmethod
    def derived(q, imu):
        """rpy, rBody, omegaWorld, aWorld of orientation q (quaternionToRotationMatrix, :170-189)."""
        e0, e1, e2, e3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, two = f32(1), f32(2)
        R = np.stack([one - two * (e2 * e2 + e3 * e3), two * (e1 * e2 - e0 * e3), two * (e1 * e3 + e0 * e2),
                      two * (e1 * e2 + e0 * e3), one - two * (e1 * e1 + e3 * e3), two * (e2 * e3 - e0 * e1),
                      two * (e1 * e3 - e0 * e2), two * (e2 * e3 + e0 * e1), one - two * (e1 * e1 + e2 * e2)], 1).astype(f32)
        rB = R.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9).copy()
        w = imu[:, 7:10].astype(f32)
        a = imu[:, 0:3].astype(f32)
        ow = np.stack([row3(R, k, w[:, 0], w[:, 1], w[:, 2]) for k in range(3)], 1)
        aw = np.stack([row3(R, k, a[:, 0], a[:, 1], a[:, 2]) for k in range(3)], 1)
        return dict(orientation=q, rpy=quat_to_rpy(q), r_body=rB, omega_body=w, omega_world=ow, a_world=aw)

    # ---- safety + ConvexMPCLocomotion::run up to updateMPCIfNeeded
    def loco(self, est, pf_override=None):
        """est: position, v_world, rpy, r_body [B,9], leg_p [B,12], leg_q [B,12] (unclamped).  pf_override: the
        landing points to continue with (teacher forcing past coordinateRotation's sin / cos).  -> dict."""
        B, dt, dtm = self.B, self.dt, self.dt_mpc
        pos, vW, rpy, rB = est["position"], est["v_world"], est["rpy"], est["r_body"]
        # safety: abs(float) is the float overload (Eigen's SSE headers reach libstdc++'s <stdlib.h>); checkJointLimit
        # only when the orientation check passed (else-if chain)
        bad_ori = (np.abs(rpy[:, 0]).astype(f64) >= 0.5) | (np.abs(rpy[:, 1]).astype(f64) >= 0.5)
        q = est["leg_q"].copy().reshape(B, 4, 3)
        lim = [(0, "lt", -f32(1.0472)), (0, "gt", f32(1.0472)), (1, "lt", f32(-1.8)), (1, "gt", f32(0.174533)),
               (2, "gt", f32(2.79253)), (2, "lt", f32(-0.174533))]
        hit = np.zeros(B, bool)
        for j, op, v in lim:
            x = q[:, :, j]
            m = (x < v) if op == "lt" else (x > v)
            m &= ~bad_ori[:, None]
            hit |= m.any(1)
            x[m] = v
        self.q = q.reshape(B, 12)
        self.safe[bad_ori | hit] = 0
        # _SetupCommand (:76-114)
        vd = self.vel_des
        xc, yc, wc = self.vel_cmd[:, 0], self.vel_cmd[:, 1], self.vel_cmd[:, 2]
        xv = vd[:, 0] * (f32(1) - f32(0.01)) + xc * f32(0.01)
        yv = vd[:, 1] * (f32(1) - f32(0.006)) + yc * f32(0.006)
        yr = vd[:, 2] * (f32(1) - f32(0.03)) + wc * f32(0.03)
        xv = np.where(xv.astype(f64) > 2.0, f32(2), np.where(xv.astype(f64) < -1.0, f32(-1), xv)).astype(f32)
        yv = np.where(yv.astype(f64) > 0.6, f32(0.6), np.where(yv.astype(f64) < -0.6, f32(-0.6), yv)).astype(f32)
        vd[:, 0], vd[:, 1], vd[:, 2] = xv, yv, yr
        self.yaw_des[:] = rpy[:, 2] + dt * yr
        ydt = self.yaw_des_true.copy()
        ydt = np.where(np.abs(rpy[:, 2] - ydt).astype(f64) > 5.0, rpy[:, 2], ydt)   # abs(float) (:106)
        self.yaw_des_true[:] = ydt + dt * yr
        # run
        gn, omni = split_gait(self.gait_num)
        first = self.first_run != 0
        st = (gn == 4) & (self.current_gait != 4) | first
        self.stand_traj[st] = np.stack([pos[:, 0], pos[:, 1], np.full(B, 0.21, f32), np.zeros(B, f32), np.zeros(B, f32),
                                        rpy[:, 2]], 1)[st]
        self.wpd[st] = pos[st, :2]
        for b in range(B):
            o, d = GAITS[gait_name(gn[b])]
            self.offsets[b], self.durations[b] = o, d
        standing = gn == 4
        self.current_gait[:] = gn
        cnt = self.counter.copy()
        self.iteration[:] = (cnt // IBM) % NSEG
        phase = (cnt % (IBM * NSEG)).astype(f32) / f32(IBM * NSEG)
        vw0 = np.where(omni, xv, ((rB[:, 0] * xv) + (rB[:, 3] * yv)) + (rB[:, 6] * f32(0)))
        vw1 = np.where(omni, yv, ((rB[:, 1] * xv) + (rB[:, 4] * yv)) + (rB[:, 7] * f32(0)))
        ri, rc = self.rpy_int, self.rpy_comp
        m = np.abs(vW[:, 0]).astype(f64) > 0.2
        with np.errstate(divide="ignore", invalid="ignore"):
            ri[m, 1] = ri[m, 1] + (dt * (f32(0) - rpy[m, 1])) / vW[m, 0]
            m = np.abs(vW[:, 1]).astype(f64) > 0.1
            ri[m, 0] = ri[m, 0] + (dt * (f32(0) - rpy[m, 0])) / vW[m, 1]
        ri[:] = np.fmin(np.fmax(ri, f32(-0.25)), f32(0.25))   # fminf / fmaxf: a NaN operand loses
        rc[:, 1] = vW[:, 0] * ri[:, 1]
        rc[:, 0] = vW[:, 1] * ri[:, 0]
        lp = est["leg_p"]
        pF = np.zeros((B, 12), f32)
        for i in range(4):
            x = [HIP[i, k] + lp[:, 3 * i + k] for k in range(3)]
            for k in range(3):
                pF[:, 3 * i + k] = pos[:, k] + rowT(rB, k, *x)
        self.p_foot[:] = pF
        ns = ~standing
        self.wpd[ns, 0] = self.wpd[ns, 0] + dt * vw0[ns]
        self.wpd[ns, 1] = self.wpd[ns, 1] + dt * vw1[ns]
        if first.any():
            self.wpd[first] = pos[first, :2]
            self.sw_p0[first] = pF[first]
            self.sw_p[first] = pF[first]
            self.sw_pf[first] = pF[first]
            self.first_run[first] = 0
        # foot placement (:297-372)
        dur = self.durations
        self.swing_time[:] = dtm * (NSEG - dur).astype(f32)
        iy = np.array([-0.08, 0.08, 0.02, -0.02], f32)
        v_abs = np.abs(xv)
        with np.errstate(invalid="ignore"):
            if self.float_sqrt:
                sq = (f32(0.5) * np.sqrt(pos[:, 2] / f32(9.81))).astype(f32)
            else:
                sq = f64(0.5) * np.sqrt((pos[:, 2] / f32(9.81)).astype(f64))
        pf_calc = np.zeros((B, 12), f32)
        for i in range(4):
            fs = self.first_swing[:, i] != 0
            self.swing_rem[:, i] = np.where(fs, self.swing_time[:, i], self.swing_rem[:, i] - dt)
            side = f32(-1) if i % 2 == 0 else f32(1)
            pr = [np.full(B, HIP[i, 0], f32), np.full(B, HIP[i, 1] + f32(f64(side) * 0.065), f32), np.full(B, HIP[i, 2], f32)]
            pr[1] = pr[1] + (iy[i] * v_abs) * f32(-0.2)
            stt = dtm * dur[:, i].astype(f32)
            th = ((-yr) * stt) / f32(2)
            s, c = np.sin(th).astype(f32), np.cos(th).astype(f32)
            py = [(c * pr[0] + s * pr[1]) + f32(0) * pr[2], (-s * pr[0] + c * pr[1]) + f32(0) * pr[2],
                  (f32(0) * pr[0] + f32(0) * pr[1]) + f32(1) * pr[2]]
            dv = [xv, yv, np.zeros(B, f32)]
            x = [py[k] + dv[k] * self.swing_rem[:, i] for k in range(3)]
            P = [pos[:, k] + rowT(rB, k, *x) for k in range(3)]
            if self.float_sqrt:
                cx = (sq * (vW[:, 1] * yr)).astype(f64)
                cy = (sq * ((-vW[:, 0]) * yr)).astype(f64)
            else:
                cx = sq * (vW[:, 1] * yr).astype(f64)
                cy = sq * ((-vW[:, 0]) * yr).astype(f64)
            pfx = (((vW[:, 0].astype(f64) * (0.5 + 0.0)) * stt.astype(f64) + (f32(0.03) * (vW[:, 0] - vw0)).astype(f64)) + cx).astype(f32)
            pfy = ((((vW[:, 1].astype(f64) * 0.5) * stt.astype(f64)) * 1.0 + (f32(0.03) * (vW[:, 1] - vw1)).astype(f64)) + cy).astype(f32)
            pfx = np.fmin(np.fmax(pfx, f32(-0.3)), f32(0.3))   # (a NaN pfx_rel -- sqrt of a negative height -- becomes -0.3)
            pfy = np.fmin(np.fmax(pfy, f32(-0.3)), f32(0.3))
            self.pf_rel[:, 2 * i], self.pf_rel[:, 2 * i + 1] = pfx, pfy
            pf_calc[:, 3 * i + 0] = P[0] + pfx
            pf_calc[:, 3 * i + 1] = P[1] + pfy
            pf_calc[:, 3 * i + 2] = 0
        self.sw_pf[:] = pf_calc if pf_override is None else pf_override
        self.counter += 1
        contact, swing = gait_states(phase, self.offsets, dur)
        self.contact_state[:], self.swing_state[:] = contact, swing
        h = f32(0.06)
        for foot in range(4):
            sw = swing[:, foot] > 0
            sl = slice(3 * foot, 3 * foot + 3)
            newsw = sw & (self.first_swing[:, foot] != 0)
            self.sw_p0[newsw, sl] = pF[newsw, sl]
            self.sw_p[newsw, sl] = pF[newsw, sl]
            self.first_swing[sw, foot] = 0
            self.first_swing[~sw, foot] = 1
            p0, pfv = self.sw_p0[:, sl], self.sw_pf[:, sl]
            with np.errstate(divide="ignore", invalid="ignore"):
                for ax in range(3):
                    pp, vv = bezier_axis(ax, p0[:, ax], pfv[:, ax], p0[:, 2], pfv[:, 2], h, swing[:, foot],
                                         self.swing_time[:, foot])
                    self.sw_p[sw, 3 * foot + ax] = pp[sw]
                    self.sw_v[sw, 3 * foot + ax] = vv[sw]
            self.contact_phase[:, foot] = np.where(sw, f32(0), contact[:, foot])
            dp = [self.sw_p[:, 3 * foot + k] - pos[:, k] for k in range(3)]
            dvv = [self.sw_v[:, 3 * foot + k] - vW[:, k] for k in range(3)]
            for k in range(3):
                self.p_des[:, 3 * foot + k] = row3(rB, k, *dp) - HIP[foot, k]
                self.v_des[:, 3 * foot + k] = row3(rB, k, *dvv)
        self.omni = omni
        return dict(pf=pf_calc, vw0=vw0, vw1=vw1)

    def command(self, est):
        """The qmpc_command rows of this tick in oracle.oracle.pack_commands' layout (omni per robot through rBody)."""
        B = self.B
        eye = np.tile(np.eye(3, dtype=f32).reshape(1, 9), (B, 1))
        return dict(batch=B, horizon=NSEG, position=est["position"], v_world=est["v_world"],
                    omega_world=est["omega_world"], orientation=est["orientation"], rpy=est["rpy"],
                    r_body=np.where(self.omni[:, None], eye, est["r_body"]), p_foot=self.p_foot, vel_des=self.vel_des,
                    yaw_des_true=self.yaw_des_true, rpy_comp=self.rpy_comp, stand_traj=self.stand_traj,
                    rp_des=np.zeros((B, 2), f32), gait_type=self.current_gait, gait_offsets=self.offsets,
                    gait_durations=self.durations, gait_iteration=self.iteration, world_position_desired=self.wpd,
                    x_comp_integral=self.xci, body_height=f32(0.25), omni_mode=0)

    def legcmd(self, est, f_ff):
        """Gains, LegController::updateCommand, latch -> effort [B,12] float64 (oracle.glue.leg_command)."""
        B = self.B
        swing = self.swing_state > 0                                           # [B,4]
        force = np.where(np.repeat(swing, 3, 1), f32(0), f_ff).astype(f32)
        kp = np.zeros((B, 4, 9), f32)
        kd = np.zeros((B, 4, 9), f32)
        for k, v in ((0, 700), (4, 700), (8, 200)):
            kp[:, :, k] = np.where(swing, f32(v), f32(0))
        kd[:, :, 0] = kd[:, :, 4] = kd[:, :, 8] = 10
        tau, _ = G.leg_command(dict(tau_ff=np.zeros((B, 12), f32), force_ff=force, kp_cart=kp, kd_cart=kd, p_des=self.p_des,
                                    v_des=self.v_des, q=self.q, qd=est["qd"], J=est["leg_J"].reshape(B, 4, 9),
                                    p=est["leg_p"], v=est["leg_v"], kp_joint=self.kp_joint, kd_joint=self.kd_joint), self.geom)
        return np.where(self.safe[:, None] != 0, tau.astype(f64), 0.0)
