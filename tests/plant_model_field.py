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
        mass, ibody, mu = self.own()
        tau = np.asarray(effort, f64).reshape(B, 4, 3)
        stance = np.asarray(contact_state).reshape(B, 4) > 0
        p, v, q, w, c = self.p.copy(), self.v.copy(), self.q.copy(), self.w.copy(), self.foot.copy()
        f, vdot = np.zeros((B, 4, 3)), np.zeros((B, 3))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            hz, n = self.foot_surface(c[..., 0], c[..., 1])                                                  # 1 + normal
            c[..., 2] = np.where(stance & ~self.stance, hz, c[..., 2])
            support = PT.support_height(stance, c[..., 2], self.support)
            for _ in range(self.substeps):
                R = PM.rot(q)
                rb = PM.mulT(R[:, None, :], c - p[:, None, :])
                f = np.where(stance[..., None], PT.stance_force_terrain(R, rb, tau, mu[:, None], n, self.geom), 0.0)   # 2a
                fb = PM.mulT(R[:, None, :], f)
                m = PM.cross(rb, fb)
                F, N = PM.add_wrench(PM.quad_sum(f), PM.quad_sum(m), self.force, self.torque)
                p, v, w, vdot = PM.body_update(p, v, w, F, N, mass, ibody, h)
                q = PM.quat_step(q, w, h)
            state, motor, c = self._readout_terrain(p, v, q, w, c, stance, vdot, np.asarray(p_des).reshape(B, 4, 3),
                                                    np.asarray(v_des).reshape(B, 4, 3), support)
            self.ground = self.height(p[:, 0], p[:, 1])
        self.support = support
        self.p, self.v, self.q, self.w, self.foot, self.grf, self.stance = p, v, q, w, c, f, stance
        self.state, self.motor = state, motor
        if self.stats_on:
            self._accumulate(state)
        return state, motor

    def _step_field_contact(self, effort, contact_state, p_des, v_des):
        """ContactPlantModel._step_contact with the summed surface and the normal per foot."""
        B, h, fl = self.B, self.h, self.cflags
        EARLY, LATE, SLIP = PCM.EARLY, PCM.LATE, PCM.SLIP
        mass, ibody, mu = self.own()
        mu = mu[:, None]
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
            support = PT.support_height(pin, c[..., 2], self.support)
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
                F, N = PM.add_wrench(PM.quad_sum(f), PM.quad_sum(m), self.force, self.torque)
                p, v, w, vdot = PM.body_update(p, v, w, F, N, mass, ibody, h)
                if fl & SLIP:
                    cx = np.where(slid, c[..., 0] + h * cd[..., 0], c[..., 0])
                    cy = np.where(slid, c[..., 1] + h * cd[..., 1], c[..., 1])
                    hs_, ns_ = self.foot_surface(cx, cy)          # the re-projection's taps give the new normal too
                    cz = np.where(slid, hs_, c[..., 2])
                    n = np.where(slid[..., None], ns_, n)
                    c = np.stack([cx, cy, cz], -1)
                    slip = slip + PM.quad_sum(np.where(slid, h * sv, 0.0))
                q = PM.quat_step(q, w, h)
            # 3. unpinned feet and release, 4. read-out
            self.trace = dict(s=s, pin0=pin0, land=land, pin1=pin1, slid=slid_any)
            pin, c, drop, state, motor = self._release_and_readout(s, pin, p, v, q, w, c, cd, drop, vdot, pd, vd, support)
        self.support, self.drop, self.slip = support, drop, slip
        self.p, self.v, self.q, self.w, self.foot, self.grf, self.stance = p, v, q, w, c, f, pin
        self.state, self.motor = state, motor
        if self.stats_on:
            self._accumulate(state)
        return state, motor
