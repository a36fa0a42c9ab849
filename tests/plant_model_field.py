"""The plant of include/qmpc_field.h in numpy float64 -- TEST SIDE ONLY.

FieldPlantModel is tests/plant_model_contact.py's ContactPlantModel on height-field terrain from memory, operation by
operation in the order of the header and of quadruped_ctrl_amd/csrc/qmpc_plant_dev.h's plant_field_*: the bilinear field
f and its gradient (fx, fy) from one set of four taps, height() = the analytic height + f, and the contact normal per
FOOT, evaluated after the edges and again after each slide move.  height() is overridden, so every place the parents say
height(...) sees the summed surface; the per-foot normal needs steps of its own, because the parents' normal() is per
robot.  With no bank bound it IS its parent: step() and reset() hand over.
"""
import numpy as np

import plant_model as PM
import plant_model_contact as PCM
import plant_model_terrain as PT

f64 = np.float64


class FieldPlantModel(PCM.ContactPlantModel):
    def __init__(self, B, *a, **kw):
        self.z, self.place, self.cell, self.fflags = None, None, None, 0
        self.cells = None                                   # a list while a test records every (u, v) that went through floor()
        super().__init__(B, *a, **kw)                       # qmpc_plant_init: no field

    def set_field(self, z, place=None, cell=None, clamp_swing=False, rebase_z=False):
        """z [M, ny, nx] float32 and place [B, 4] = (map, ox, oy, zs), kept by reference like the device's pointers; None
        unbinds."""
        if z is None:
            self.z, self.place, self.cell, self.fflags = None, None, None, 0
            return
        assert z.dtype == np.float32 and z.ndim == 3 and place.shape == (self.B, 4) and place.dtype == f64
        self.z, self.place, self.cell = z, place, float(cell)
        self.fflags = (PT.CLAMP_SWING if clamp_swing else 0) | (PT.REBASE_Z if rebase_z else 0)

    # ---- the field -------------------------------------------------------------------------------------------------------
    @staticmethod
    def axis(u, n):
        """-> i (int), a, inside: the header's clamp, floor and cap along one axis of n samples."""
        top = f64(n - 1)
        inside = (u >= 0.0) & (u <= top)
        u = np.where(~(u >= 0.0), 0.0, u)
        u = np.where(u > top, top, u)
        fi = np.floor(u)
        fi = np.where(fi > f64(n - 2), f64(n - 2), fi)
        return fi.astype(np.int64), u - fi, inside

    def sample(self, x, y):
        """-> f, fx, fy at (x, y) of every robot's own placement; x, y [B] or [B, 4]."""
        x, y = np.asarray(x, f64), np.asarray(y, f64)
        ex = (slice(None),) + (None,) * (x.ndim - 1)
        M, ny, nx = self.z.shape
        mp, ox, oy, zs = (self.place[:, k][ex] for k in range(4))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            m = np.where(~(mp >= 0.0), 0.0, mp)
            m = np.where(m > f64(M - 1), f64(M - 1), m).astype(np.int64)
            u, v = (x - ox) / self.cell, (y - oy) / self.cell
            if self.cells is not None:
                self.cells.append((np.array(u).reshape(-1), np.array(v).reshape(-1)))
            i, a, in_x = self.axis(u, nx)
            j, b, in_y = self.axis(v, ny)
            m = np.broadcast_to(m, i.shape)
            z00, z10 = self.z[m, j, i].astype(f64), self.z[m, j, i + 1].astype(f64)
            z01, z11 = self.z[m, j + 1, i].astype(f64), self.z[m, j + 1, i + 1].astype(f64)
            d0, d1 = z10 - z00, z11 - z01
            e0, e1 = z00 + a * d0, z01 + a * d1
            e = e1 - e0
            f = zs * (e0 + b * e)
            fx = np.where(in_x, zs * ((d0 + b * (d1 - d0)) / self.cell), 0.0)
            fy = np.where(in_y, zs * (e / self.cell), 0.0)
        return f, fx, fy

    def height(self, x, y):
        if self.z is None:
            return super().height(x, y)
        if self.rows is None:                                  # the field alone: over an all-zero row
            return self._bound(self.height, x, y)
        h = super().height(x, y)
        f, _, _ = self.sample(x, y)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(f == 0.0, h, h + f)

    def foot_surface(self, x, y):
        """-> height [B, 4] and the contact normal n [B, 4, 3] under feet at (x, y) [B, 4], from one set of taps."""
        h = PCM.ContactPlantModel.height(self, x, y)
        f, fx, fy = self.sample(x, y)
        gx0, gy0 = self.rows[:, 1][:, None], self.rows[:, 2][:, None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            gx = np.where(fx == 0.0, gx0, gx0 + fx)
            gy = np.where(fy == 0.0, gy0, gy0 + fy)
            norm = np.sqrt((gx * gx + gy * gy) + 1)
            n = np.stack([-gx / norm, -gy / norm, 1 / norm], -1)
            return np.where(f == 0.0, h, h + f), n

    # ---- reset and step ----------------------------------------------------------------------------------------------------
    def _bound(self, fn, *a):
        """fn(*a) with the rows an all-zero row where none are bound and the flags the OR of both bindings'."""
        rows, flags = self.rows, self.flags
        if rows is None:
            self.rows = np.zeros((self.B, 8))
        self.flags = flags | self.fflags
        try:
            return fn(*a)
        finally:
            self.rows, self.flags = rows, flags

    def reset(self, mask, init_xyyaw=None):
        if self.z is None:
            return super().reset(mask, init_xyyaw)
        mask = np.asarray(mask).astype(bool)
        if self.cflags:                                       # (the counters; support and ground are the field reset's)
            self.early[mask], self.late[mask], self.slip[mask], self.drop[mask] = 0, 0, 0.0, 0.0
        self._bound(PT.TerrainPlantModel.reset, self, mask, init_xyyaw)

    def step(self, effort, contact_state, p_des, v_des):
        if self.z is None:
            return super().step(effort, contact_state, p_des, v_des)
        return self._bound(self._step_field_contact if self.cflags else self._step_field, effort, contact_state, p_des,
                           v_des)

    def _step_field(self, effort, contact_state, p_des, v_des):
        """TerrainPlantModel.step with the summed surface and the normal per foot."""
        B, h = self.B, self.h
        mass = np.full(B, self.mass) if self.mass_b is None else self.mass_b
        ibody = np.broadcast_to(self.ibody, (B, 3)) if self.ibody_b is None else self.ibody_b
        mu = np.full(B, self.mu) if self.mu_b is None else self.mu_b
        tau = np.asarray(effort, f64).reshape(B, 4, 3)
        stance = np.asarray(contact_state).reshape(B, 4) > 0
        p, v, q, w, c = self.p.copy(), self.v.copy(), self.q.copy(), self.w.copy(), self.foot.copy()
        f, vdot = np.zeros((B, 4, 3)), np.zeros((B, 3))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            hz, n = self.foot_surface(c[..., 0], c[..., 1])                                                  # 1 + normal
            c[..., 2] = np.where(stance & ~self.stance, hz, c[..., 2])
            one, sz = np.where(stance, 1.0, 0.0), np.where(stance, c[..., 2], 0.0)
            cnt = (one[:, 0] + one[:, 1]) + (one[:, 2] + one[:, 3])
            ssum = (sz[:, 0] + sz[:, 1]) + (sz[:, 2] + sz[:, 3])
            support = np.where(cnt > 0.0, ssum / np.where(cnt > 0.0, cnt, 1.0), self.support)
            for _ in range(self.substeps):
                R = PM.rot(q)
                rb = PM.mulT(R[:, None, :], c - p[:, None, :])
                f = np.where(stance[..., None], PT.stance_force_terrain(R, rb, tau, mu[:, None], n, self.geom), 0.0)   # 2a
                fb = PM.mulT(R[:, None, :], f)
                m = PM.cross(rb, fb)
                F = (f[:, 0] + f[:, 1]) + (f[:, 2] + f[:, 3])
                N = (m[:, 0] + m[:, 1]) + (m[:, 2] + m[:, 3])
                if self.force is not None:
                    F = F + self.force
                if self.torque is not None:
                    N = N + self.torque
                vdot = np.stack([F[:, 0] / mass, F[:, 1] / mass, F[:, 2] / mass - PM.GRAVITY], 1)
                Iw = ibody * w
                wIw = PM.cross(w, Iw)
                v = v + h * vdot
                w = w + h * ((N - wIw) / ibody)
                p = p + h * v
                q = self._quat_step(q, w, h)
            state, motor, c = self._readout_terrain(p, v, q, w, c, stance, vdot, np.asarray(p_des).reshape(B, 4, 3),
                                                    np.asarray(v_des).reshape(B, 4, 3), support)
            self.ground = self.height(p[:, 0], p[:, 1])
        self.support = support
        self.p, self.v, self.q, self.w, self.foot, self.grf, self.stance = p, v, q, w, c, f, stance
        self.state, self.motor = state, motor
        if self.stats_on:
            self._accumulate(state)
        return state, motor

    @staticmethod
    def _quat_step(q, w, h):
        wn = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        a = wn * h
        small = a < 1e-12
        d0 = np.where(small, 1.0, np.cos(0.5 * a))
        ds = np.where(small, 0.5 * h, np.sin(0.5 * a) / wn)
        d1, d2, d3 = ds * w[:, 0], ds * w[:, 1], ds * w[:, 2]
        q0, q1, q2, q3 = (q[:, k] for k in range(4))
        n0 = ((q0 * d0 - q1 * d1) - q2 * d2) - q3 * d3
        n1 = ((q0 * d1 + q1 * d0) + q2 * d3) - q3 * d2
        n2 = ((q0 * d2 - q1 * d3) + q2 * d0) + q3 * d1
        n3 = ((q0 * d3 + q1 * d2) - q2 * d1) + q3 * d0
        nn = np.sqrt(((n0 * n0 + n1 * n1) + n2 * n2) + n3 * n3)
        return np.stack([n0 / nn, n1 / nn, n2 / nn, n3 / nn], 1)

    def _step_field_contact(self, effort, contact_state, p_des, v_des):
        """ContactPlantModel._step_contact with the summed surface and the normal per foot."""
        B, h, fl = self.B, self.h, self.cflags
        EARLY, LATE, SLIP = PCM.EARLY, PCM.LATE, PCM.SLIP
        mass = np.full(B, self.mass) if self.mass_b is None else self.mass_b
        ibody = np.broadcast_to(self.ibody, (B, 3)) if self.ibody_b is None else self.ibody_b
        mu = (np.full(B, self.mu) if self.mu_b is None else self.mu_b)[:, None]
        tau = np.asarray(effort, f64).reshape(B, 4, 3)
        s = np.asarray(contact_state).reshape(B, 4) > 0
        pd, vd = np.asarray(p_des, f64).reshape(B, 4, 3), np.asarray(v_des, f64).reshape(B, 4, 3)
        p, v, q, w, c = self.p.copy(), self.v.copy(), self.q.copy(), self.w.copy(), self.foot.copy()
        pin, drop, slip = self.stance.copy(), self.drop.copy(), self.slip.copy()
        f, vdot, cd = np.zeros((B, 4, 3)), np.zeros((B, 3)), np.zeros((B, 4, 3))
        pin0, slid_any, self.ties = pin.copy(), np.zeros((B, 4), bool), []
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            # 1. edges; the surface and the normal under every foot from one set of taps (c_x, c_y do not move here)
            hz, n = self.foot_surface(c[..., 0], c[..., 1])
            land = s & ~pin & ((c[..., 2] <= hz) if fl & LATE else True)
            self.ties.append(("edge", c[..., 2].copy(), hz, s & ~pin & bool(fl & LATE)))
            c[..., 2] = np.where(land, hz, c[..., 2])
            pin = (s & (pin | land)) | (~s & pin & bool(fl & EARLY))
            one, sz = np.where(pin, 1.0, 0.0), np.where(pin, c[..., 2], 0.0)
            cnt = (one[:, 0] + one[:, 1]) + (one[:, 2] + one[:, 3])
            ssum = (sz[:, 0] + sz[:, 1]) + (sz[:, 2] + sz[:, 3])
            support = np.where(cnt > 0.0, ssum / np.where(cnt > 0.0, cnt, 1.0), self.support)
            pin1 = pin.copy()
            # 2. substeps
            for _ in range(self.substeps):
                R = PM.rot(q)
                rb = PM.mulT(R[:, None, :], c - p[:, None, :])
                f, slid, sv, t, ft = self._force(R, rb, tau, mu, n, pin)
                slid_any |= slid
                cd = np.where(slid[..., None], -(sv[..., None] * (t / ft[..., None])), 0.0)
                fb = PM.mulT(R[:, None, :], f)
                m = PM.cross(rb, fb)
                F = (f[:, 0] + f[:, 1]) + (f[:, 2] + f[:, 3])
                N = (m[:, 0] + m[:, 1]) + (m[:, 2] + m[:, 3])
                if self.force is not None:
                    F = F + self.force
                if self.torque is not None:
                    N = N + self.torque
                vdot = np.stack([F[:, 0] / mass, F[:, 1] / mass, F[:, 2] / mass - PM.GRAVITY], 1)
                Iw = ibody * w
                wIw = PM.cross(w, Iw)
                v = v + h * vdot
                w = w + h * ((N - wIw) / ibody)
                p = p + h * v
                if fl & SLIP:
                    cx = np.where(slid, c[..., 0] + h * cd[..., 0], c[..., 0])
                    cy = np.where(slid, c[..., 1] + h * cd[..., 1], c[..., 1])
                    hs_, ns_ = self.foot_surface(cx, cy)          # the re-projection's taps give the new normal too
                    cz = np.where(slid, hs_, c[..., 2])
                    n = np.where(slid[..., None], ns_, n)
                    c = np.stack([cx, cy, cz], -1)
                    d = np.where(slid, h * sv, 0.0)
                    slip = slip + ((d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3]))
                q = self._quat_step(q, w, h)
            # 3. unpinned feet and release, at the new pose
            R = PM.rot(q)
            vb = PM.mulT(R, v)
            cmd = ~(s & pin)
            lateft = s & ~pin
            drop = np.where(lateft, drop + self.drop_speed * self.dt, drop)
            ez = R[:, None, 6:9]
            rs = self.clamp(np.where(lateft[..., None], pd - drop[..., None] * ez, pd))
            cs = p[:, None, :] + PM.mul(R[:, None, :], PM.HIP + rs)
            hs = self.height(cs[..., 0], cs[..., 1])
            touching = cs[..., 2] <= hs
            test = s | bool(fl & EARLY)
            hit = cmd & test & touching
            self.ties.append(("touch", cs[..., 2], hs, cmd & test))
            newpin = hit & ~pin
            free = cmd & ~hit
            on = np.stack([cs[..., 0], cs[..., 1], hs], -1)
            c = np.where(newpin[..., None], on, np.where(free[..., None], cs, c))
            pin = np.where(cmd, hit, pin)
            low = np.zeros((B, 4), bool)
            if self.flags & PT.CLAMP_SWING:
                low = free & (c[..., 2] < hs)
                c[..., 2] = np.where(low, hs, c[..., 2])
            self.trace = dict(s=s, pin0=pin0, land=land, pin1=pin1, slid=slid_any, late=lateft, hit=hit, newpin=newpin,
                              free=free, pin2=pin.copy(), foot1=c.copy())
            self.early = self.early + (~s & pin).sum(1).astype(np.int32)
            self.late = self.late + lateft.sum(1).astype(np.int32)
            drop = np.where(pin | ~s, 0.0, drop)
            # 4. read-out
            rb = PM.mulT(R[:, None, :], c - p[:, None, :])
            r = np.where((pin | low)[..., None], rb - PM.HIP, rs)
            rdot = np.where(pin[..., None], (-vb[:, None, :] - PM.cross(w[:, None, :], rb)) + PM.mulT(R[:, None, :], cd), vd)
            ang, C, det = PM.leg(r, self.geom)
            ok = np.abs(det) >= PM.DET_MIN
            sdet = np.where(ok, det, 1.0)
            qd = np.stack([((C[..., k] * rdot[..., 0] + C[..., 3 + k] * rdot[..., 1]) + C[..., 6 + k] * rdot[..., 2]) / sdet
                           for k in range(3)], -1)
            qd = np.where(ok[..., None], qd, 0.0)
            sf = np.stack([vdot[:, 0], vdot[:, 1], vdot[:, 2] + PM.GRAVITY], 1)
            row_p = p.copy()
            if self.flags & PT.REBASE_Z:
                row_p[:, 2] = p[:, 2] - support
            state = np.concatenate([q, row_p, w, vb, PM.mulT(R, sf)], 1)
            motor = np.concatenate([ang.reshape(B, 12), qd.reshape(B, 12)], 1)
            self.ground = self.height(p[:, 0], p[:, 1])
        self.support, self.drop, self.slip = support, drop, slip
        self.p, self.v, self.q, self.w, self.foot, self.grf, self.stance = p, v, q, w, c, f, pin
        self.state, self.motor = state, motor
        if self.stats_on:
            self._accumulate(state)
        return state, motor
