"""Robot mode 1 of the batched locomotion controller on top of tests/ctrl_model.py -- TEST SIDE ONLY.

CtrlModelMode1 restates, in numpy and vectorised over robots, ConvexMPCLocomotion::run with robotMode == 1
(src/MPC_Ctrl/ConvexMPCLocomotion.cpp:173-233): the `aio` gait, whose segment count, offsets and durations are
re-selected from the filtered velocity command on the ticks where the phase the previous tick's setIterations left is 0,
and whose iterationCounter restarts when the segment count changes.  Everything after the gait selection is the mode-0
tick of CtrlModel.loco with the robot's own segment count where that has the literal 14 (setIterations, the contact
and swing states, getCurrentSwingTime; getCurrentStanceTime reads the durations).

What differs from mode 0, line by line:
  :175      vBody = sqrt(x*x) + (y*y): float products, the double sqrt (the overload decision of qmpc_glue.hip), a
            double sum -- the reference's expression, not a norm
  :176-177  gait = &aio, gaitNumber = 9: the caller's gait number keeps its omni flag (:129-132) and the :137 test only
  :178      the phase tested is OffsetDurationGait::_phase as the PREVIOUS tick left it; a fresh robot's is 0 here (the
            reference reads an uninitialised float), so the first tick selects
  :179-231  aio_select(): integer h / 2, h / 4, 3 * h / 4; the walk-to-trot case and h = -20.0 * vBody + 42.0 in double,
            truncated by the conversion to int; abs(_yaw_turn_rate) is the float overload against the double 0.01;
            iterationCounter = 0 where getGaitHorizon() != h
  :233      horizonLength = h: the local `int h = 10` unless this tick took the phase-0 branch (recorded in .horizon)
  :238      current_gait = gaitNumber: 4 only on a phase-0 tick of the standing case
  :277      gait != &standing holds for &aio always: world_position_desired is integrated in the standing case too
The solve of a due robot (command_mode1) runs at horizon 10 on rows 0 .. 9 of the robot's n-row table
(getMpcTable, Gait.cpp:142-166; mpc_rows).
"""
import numpy as np

import ctrl_model as M
from ctrl_model import HIP, IBM, f32, f64, row3, rowT

MPC_HORIZON = 10          # `int h = 10` (:174): horizonLength of every tick that is not a phase-0 tick
NSEG_AIO = 14             # the aio gait's constructor (:41)


NSEGS = {10, 11, 12, 13, 14, 16}   # the segment counts the six cases reach

# x commands of the six cases (:179-231): standing, turning on the spot (yaw 0.5), walking, walk-to-trot, trot, and
# the fast trot's four segment counts 13 (42 - 28.4 = 13.6), 12 (42 - 29.6 = 12.4), 11 (42 - 30.4 = 11.6), 10 (42 - 35 < 10)
SWEEP_X = (0.0, 0.0, 0.1, 0.32, 0.8, 1.42, 1.48, 1.52, 1.75)
SWEEP_YAW = (0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def sweep_vel(B, segment):
    """Robot b's command in segment `segment`: case (b + 2 * segment) % 9; every fourth robot adds a y command."""
    k = (np.arange(B) + 2 * segment) % len(SWEEP_X)
    v = np.zeros((B, 3))
    v[:, 0] = np.array(SWEEP_X)[k]
    v[:, 2] = np.array(SWEEP_YAW)[k]
    v[(np.arange(B) % 4 == 3) & (v[:, 0] > 0), 1] = 0.25       # vBody = |x| + y * y: + 0.0625
    return v


def aio_select(xv, yv, yr):
    """The phase-0 branch (:179-231) for scalars float32 -> (h, offsets, durations, gaitNumber)."""
    xv, yv, yr = f32(xv), f32(yv), f32(yr)
    vBody = float(np.sqrt(f64(xv * xv))) + float(f64(yv * yv))
    gn = 9
    h = 10
    if vBody < 0.002:
        if float(np.abs(yr)) < 0.01:
            gn = 4
            off, dur = (0, 0, 0, 0), (h,) * 4
        else:
            h = 10
            off, dur = (0, h // 2, h // 2, 0), (h // 2,) * 4
    elif vBody <= 0.2:
        h = 16
        off, dur = (0, 1 * h // 2, 1 * h // 4, 3 * h // 4), (3 * h // 4,) * 4
    elif 0.2 < vBody <= 0.4:
        h = 16
        off = (0, 1 * h // 2, int(h * ((5.0 / 4.0) * vBody)), int(h * ((5.0 / 4.0) * vBody + (1.0 / 2.0))))
        dur = (int(h * ((-5.0 / 4.0) * vBody + 1.0)),) * 4
    elif 0.4 < vBody <= 1.4:
        h = 14
        off, dur = (0, h // 2, h // 2, 0), (h // 2,) * 4
    else:
        h = int(-20.0 * vBody + 42.0)
        if h < 10:
            h = 10
        off, dur = (0, h // 2, h // 2, 0), (h // 2,) * 4
    return h, off, dur, gn


def mpc_rows(offsets, durations, iteration, n, rows=MPC_HORIZON):
    """Rows 0 .. rows-1 of the n-row contact table (what a horizon-`rows` solve reads of getMpcTable's output)."""
    return M.mpc_table(offsets, durations, int(iteration), n=int(n))[:4 * rows]


def gait_states_n(phase, off, dur, n):
    """ctrl_model.gait_states with a segment count per robot (n [B] int)."""
    nf = n.astype(f32)[:, None]
    offF = off.astype(f32) / nf
    durF = dur.astype(f32) / nf
    pr = phase[:, None] - offF
    pr = np.where(pr < 0, pr + f32(1), pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        contact = np.where(pr > durF, f32(0), pr / durF).astype(f32)
    so = offF + durF
    so = np.where(so > 1, so - f32(1), so)
    sd = f32(1) - durF
    pr = phase[:, None] - so
    pr = np.where(pr < 0, pr + f32(1), pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        swing = np.where(pr > sd, f32(0), np.where(sd.astype(f64) < 1e-10, f32(0), pr / sd)).astype(f32)
    return contact, swing


class CtrlModelMode1(M.CtrlModel):
    """CtrlModel in robot mode 1.  Extra state: nseg [B], gait_phase [B]; per tick: due [B], horizon [B], phase0 [B],
    restarted [B] (what the tick did, for the tests)."""

    def reset(self, mask, counter0=0):
        super().reset(mask, counter0)
        B = self.B
        m = np.asarray(mask, bool)
        for k, v in (("nseg", np.full(B, NSEG_AIO, np.int32)), ("gait_phase", np.zeros(B, f32))):
            if not hasattr(self, k):
                setattr(self, k, v.copy())
            else:
                getattr(self, k)[m] = v[m]

    def loco(self, est, pf_override=None):
        B, dt, dtm = self.B, self.dt, self.dt_mpc
        pos, vW, rpy, rB = est["position"], est["v_world"], est["rpy"], est["r_body"]
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
        ydt = np.where(np.abs(rpy[:, 2] - ydt).astype(f64) > 5.0, rpy[:, 2], ydt)
        self.yaw_des_true[:] = ydt + dt * yr
        # run: :127-146 with the caller's gait number
        gn, omni = M.split_gait(self.gait_num)
        first = self.first_run != 0
        st = (gn == 4) & (self.current_gait != 4) | first
        self.stand_traj[st] = np.stack([pos[:, 0], pos[:, 1], np.full(B, 0.21, f32), np.zeros(B, f32), np.zeros(B, f32),
                                        rpy[:, 2]], 1)[st]
        self.wpd[st] = pos[st, :2]
        # robot mode 1 (:173-233)
        cnt = self.counter.copy()
        self.phase0 = self.gait_phase == 0
        self.restarted = np.zeros(B, bool)
        self.horizon = np.full(B, MPC_HORIZON, np.int32)
        cg = np.full(B, 9, np.int32)
        for b in np.flatnonzero(self.phase0):
            h, o, d, g = aio_select(xv[b], yv[b], yr[b])
            cg[b] = g
            if self.nseg[b] != h:
                cnt[b] = 0
                self.restarted[b] = True
            self.nseg[b] = h
            self.offsets[b], self.durations[b] = o, d
            self.horizon[b] = h
        self.current_gait[:] = cg
        n = self.nseg
        self.iteration[:] = (cnt // IBM) % n
        phase = (cnt % (IBM * n)).astype(f32) / (IBM * n).astype(f32)
        self.gait_phase[:] = phase
        vw0 = np.where(omni, xv, ((rB[:, 0] * xv) + (rB[:, 3] * yv)) + (rB[:, 6] * f32(0)))
        vw1 = np.where(omni, yv, ((rB[:, 1] * xv) + (rB[:, 4] * yv)) + (rB[:, 7] * f32(0)))
        ri, rc = self.rpy_int, self.rpy_comp
        m = np.abs(vW[:, 0]).astype(f64) > 0.2
        with np.errstate(divide="ignore", invalid="ignore"):
            ri[m, 1] = ri[m, 1] + (dt * (f32(0) - rpy[m, 1])) / vW[m, 0]
            m = np.abs(vW[:, 1]).astype(f64) > 0.1
            ri[m, 0] = ri[m, 0] + (dt * (f32(0) - rpy[m, 0])) / vW[m, 1]
        ri[:] = np.fmin(np.fmax(ri, f32(-0.25)), f32(0.25))
        rc[:, 1] = vW[:, 0] * ri[:, 1]
        rc[:, 0] = vW[:, 1] * ri[:, 0]
        lp = est["leg_p"]
        pF = np.zeros((B, 12), f32)
        for i in range(4):
            x = [HIP[i, k] + lp[:, 3 * i + k] for k in range(3)]
            for k in range(3):
                pF[:, 3 * i + k] = pos[:, k] + rowT(rB, k, *x)
        self.p_foot[:] = pF
        self.wpd[:, 0] = self.wpd[:, 0] + dt * vw0          # gait != &standing (:277): &aio never is
        self.wpd[:, 1] = self.wpd[:, 1] + dt * vw1
        if first.any():
            self.wpd[first] = pos[first, :2]
            self.sw_p0[first] = pF[first]
            self.sw_p[first] = pF[first]
            self.sw_pf[first] = pF[first]
            self.first_run[first] = 0
        dur = self.durations
        self.swing_time[:] = dtm * (n[:, None] - dur).astype(f32)     # getCurrentSwingTime (Gait.cpp:215-219)
        iy = np.array([-0.08, 0.08, 0.02, -0.02], f32)
        v_abs = np.abs(xv)
        with np.errstate(invalid="ignore"):
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
            cx = sq * (vW[:, 1] * yr).astype(f64)
            cy = sq * ((-vW[:, 0]) * yr).astype(f64)
            pfx = (((vW[:, 0].astype(f64) * (0.5 + 0.0)) * stt.astype(f64) + (f32(0.03) * (vW[:, 0] - vw0)).astype(f64)) + cx).astype(f32)
            pfy = ((((vW[:, 1].astype(f64) * 0.5) * stt.astype(f64)) * 1.0 + (f32(0.03) * (vW[:, 1] - vw1)).astype(f64)) + cy).astype(f32)
            pfx = np.fmin(np.fmax(pfx, f32(-0.3)), f32(0.3))
            pfy = np.fmin(np.fmax(pfy, f32(-0.3)), f32(0.3))
            self.pf_rel[:, 2 * i], self.pf_rel[:, 2 * i + 1] = pfx, pfy
            pf_calc[:, 3 * i + 0] = P[0] + pfx
            pf_calc[:, 3 * i + 1] = P[1] + pfy
            pf_calc[:, 3 * i + 2] = 0
        self.sw_pf[:] = pf_calc if pf_override is None else pf_override
        self.counter[:] = cnt + 1
        contact, swing = gait_states_n(phase, self.offsets, dur, n)
        self.contact_state[:], self.swing_state[:] = contact, swing
        hgt = f32(0.06)
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
                    pp, vv = M.bezier_axis(ax, p0[:, ax], pfv[:, ax], p0[:, 2], pfv[:, 2], hgt, swing[:, foot],
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
        self.due = (self.counter % IBM == 0)                 # updateMPCIfNeeded (:502) on the incremented counter
        return dict(pf=pf_calc, vw0=vw0, vw1=vw1)

    def command_mode1(self, est, rows):
        """The qmpc_command rows of robots `rows` (indices) at horizon 10, and their contact tables [len, 40]: rows
        0 .. 9 of each robot's n-row table.  The command's own gait fields describe a 10-segment trot and are NOT what
        the solve reads: the caller puts `tables` into the packed record."""
        rows = np.asarray(rows)
        k = len(rows)
        eye = np.tile(np.eye(3, dtype=f32).reshape(1, 9), (k, 1))
        cmd = dict(batch=k, horizon=MPC_HORIZON, position=est["position"][rows], v_world=est["v_world"][rows],
                   omega_world=est["omega_world"][rows], orientation=est["orientation"][rows], rpy=est["rpy"][rows],
                   r_body=np.where(self.omni[rows, None], eye, est["r_body"][rows]), p_foot=self.p_foot[rows],
                   vel_des=self.vel_des[rows], yaw_des_true=self.yaw_des_true[rows], rpy_comp=self.rpy_comp[rows],
                   stand_traj=self.stand_traj[rows], rp_des=np.zeros((k, 2), f32), gait_type=self.current_gait[rows],
                   gait_offsets=np.tile(np.array([0, 5, 5, 0], np.int32), (k, 1)),
                   gait_durations=np.full((k, 4), 5, np.int32), gait_iteration=np.zeros(k, np.int32),
                   world_position_desired=self.wpd[rows], x_comp_integral=self.xci[rows], body_height=f32(0.25),
                   omni_mode=0)
        tables = np.stack([mpc_rows(self.offsets[b], self.durations[b], self.iteration[b], self.nseg[b]) for b in rows]) \
            if k else np.zeros((0, 4 * MPC_HORIZON), np.int32)
        return cmd, tables.astype(np.uint8)
