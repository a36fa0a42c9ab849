"""The plant of include/qmpc_terrain.h in numpy float64 -- TEST SIDE ONLY.

TerrainPlantModel is tests/plant_model_varied.py's VariedPlantModel with the header's changes, operation by operation in
the order of quadruped_ctrl_amd/csrc/qmpc_plant_step_body.h with TERRAIN: touch-down on height(c_x, c_y), the stance
feet's mean height `support`, the friction cone about the contact normal, the swing foot lifted onto the surface
(clamp_swing), `ground` under the body, column 6 of the state row above the stance feet (rebase_z), the statistics over
that column, and the reset that stands the robots on their terrain.  With no rows bound it is VariedPlantModel.
"""
import numpy as np

import plant_model as PM
import plant_model_varied as PV

f64 = np.float64
CLAMP_SWING, REBASE_Z = 1, 2
COLUMNS = ("z0", "gx", "gy", "rise", "run", "count", "s0", "psi")


def stance_force_terrain(R, rb, tau, mu, n, geom=PM.GEOM):
    """plant_model.stance_force with the cone about the normal n [B,1,3]."""
    g, ok = PM.leg_force(R, rb, tau, geom)
    fn = (g[..., 0] * n[..., 0] + g[..., 1] * n[..., 1]) + g[..., 2] * n[..., 2]
    ok = ok & (fn > 0.0)
    t = g - fn[..., None] * n
    ft = np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
    cap = mu * fn
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = cap / ft
        f = np.where((ft > cap)[..., None], fn[..., None] * n + t * sc[..., None], g)
    return np.where(ok[..., None], f, 0.0)


def support_height(pinned, cz, previous):
    """The pinned feet's mean height [B] (pinned, cz [B,4]); `previous` through a flight phase."""
    cnt = PM.quad_sum(np.where(pinned, 1.0, 0.0))
    ssum = PM.quad_sum(np.where(pinned, cz, 0.0))
    return np.where(cnt > 0.0, ssum / np.where(cnt > 0.0, cnt, 1.0), previous)


class TerrainPlantModel(PV.VariedPlantModel):
    """rows [B,8] = (z0, gx, gy, rise, run, count, s0, psi) per robot, or None: flat ground (VariedPlantModel)."""

    def __init__(self, B, freq=500.0, mu=0.4, substeps=1, init_xyyaw=None, rows=None, clamp_swing=False, rebase_z=False,
                 **kw):
        self.rows, self.flags = None, 0
        super().__init__(B, freq, mu, substeps, init_xyyaw, **kw)          # qmpc_plant_init: the flat plant
        self.ground, self.support = np.zeros(B), np.zeros(B)
        self.set_terrain(rows, clamp_swing, rebase_z)

    def set_terrain(self, rows, clamp_swing=False, rebase_z=False):
        self.rows = None if rows is None else np.array(rows, f64).reshape(self.B, 8)
        self.flags = 0 if rows is None else (CLAMP_SWING if clamp_swing else 0) | (REBASE_Z if rebase_z else 0)

    def normal(self):
        gx, gy = self.rows[:, 1], self.rows[:, 2]
        norm = np.sqrt((gx * gx + gy * gy) + 1)
        return np.stack([-gx / norm, -gy / norm, 1 / norm], -1)

    def height(self, x, y):
        """height(x, y) of every robot's own terrain; x, y [B] or [B, 4]."""
        x, y = np.asarray(x, f64), np.asarray(y, f64)
        ex = (slice(None),) + (None,) * (x.ndim - 1)
        z0, gx, gy, rise, run, count, s0, psi = (self.rows[:, k][ex] for k in range(8))
        flight = ~(count <= 0.0) & (run > 0.0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            k = np.floor(((x * np.cos(psi) + y * np.sin(psi)) - s0) / run) + 1
            k = np.where(k < 0.0, 0.0, k)
            k = np.where(k > count, count, k)
            k = np.where(flight, k, 0.0)
            return ((z0 + gx * x) + gy * y) + rise * k

    def tread(self, x, y):
        """Test helper: the abscissa along the flight in tread depths, ((x cos psi + y sin psi) - s0) / run."""
        x = np.asarray(x, f64)
        ex = (slice(None),) + (None,) * (x.ndim - 1)
        run, s0, psi = (self.rows[:, k][ex] for k in (4, 6, 7))
        return ((x * np.cos(psi) + y * np.sin(psi)) - s0) / run

    def reset(self, mask, init_xyyaw=None):
        if self.rows is None:
            return super().reset(mask, init_xyyaw)
        mask = np.asarray(mask).astype(bool)
        B = self.B
        xy = np.zeros((B, 3)) if init_xyyaw is None else np.asarray(init_xyyaw, f64)
        with np.errstate(invalid="ignore", over="ignore"):
            ground = self.height(xy[:, 0], xy[:, 1])
            p = np.stack([xy[:, 0], xy[:, 1], PM.HEIGHT + ground], 1)
            q = np.stack([np.cos(xy[:, 2] / 2), np.zeros(B), np.zeros(B), np.sin(xy[:, 2] / 2)], 1)
            R = PM.rot(q)
            fb = np.stack([np.broadcast_to(PM.HIP[:, 0], (B, 4)), np.broadcast_to(PM.HIP[:, 1] + PM.SIDE * PM.SIDE_OFFSET, (B, 4)),
                           np.full((B, 4), -PM.HEIGHT)], -1)
            fw = PM.mul(R[:, None, :], fb)
            cx, cy = p[:, None, 0] + fw[..., 0], p[:, None, 1] + fw[..., 1]
            c = np.stack([cx, cy, self.height(cx, cy)], -1)
            support = ((c[:, 0, 2] + c[:, 1, 2]) + (c[:, 2, 2] + c[:, 3, 2])) / 4.0
            z3 = np.zeros((B, 3))
            state, motor, _ = self._readout_terrain(p, z3, q, z3, c, np.ones((B, 4), bool), z3, None, None, support)
        for name, new in (("p", p), ("v", z3), ("q", q), ("w", z3), ("foot", c), ("grf", np.zeros((B, 4, 3))),
                          ("stance", np.ones((B, 4), bool)), ("state", state), ("motor", motor), ("ground", ground),
                          ("support", support)):
            getattr(self, name)[mask] = new[mask]

    def step(self, effort, contact_state, p_des, v_des):
        if self.rows is None:
            return super().step(effort, contact_state, p_des, v_des)
        B, h = self.B, self.h
        mass, ibody, mu = self.own()
        tau = np.asarray(effort, f64).reshape(B, 4, 3)
        stance = np.asarray(contact_state).reshape(B, 4) > 0
        p, v, q, w, c = self.p.copy(), self.v.copy(), self.q.copy(), self.w.copy(), self.foot.copy()
        f, vdot = np.zeros((B, 4, 3)), np.zeros((B, 3))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # (a robot's own bad values are its own)
            n = self.normal()[:, None, :]
            c[..., 2] = np.where(stance & ~self.stance, self.height(c[..., 0], c[..., 1]), c[..., 2])          # 1
            support = support_height(stance, c[..., 2], self.support)
            for _ in range(self.substeps):
                R = PM.rot(q)
                rb = PM.mulT(R[:, None, :], c - p[:, None, :])
                f = np.where(stance[..., None], stance_force_terrain(R, rb, tau, mu[:, None], n, self.geom), 0.0)   # 2a
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
            self._accumulate(state)               # z_min / z_max fold the state row's column 6
        return state, motor

    def _readout_terrain(self, p, v, q, w, c, stance, vdot, p_des, v_des, support):
        R = PM.rot(q)
        vb = PM.mulT(R, v)
        rb = PM.mulT(R[:, None, :], c - p[:, None, :])
        r = rb - PM.HIP
        rdot = -vb[:, None, :] - PM.cross(w[:, None, :], rb)
        if p_des is not None:
            rs = self.clamp(np.asarray(p_des, f64))
            cs = p[:, None, :] + PM.mul(R[:, None, :], PM.HIP + rs)
            if self.flags & CLAMP_SWING:                                                                     # 3
                hz = self.height(cs[..., 0], cs[..., 1])
                low = cs[..., 2] < hz
                cs = np.stack([cs[..., 0], cs[..., 1], np.where(low, hz, cs[..., 2])], -1)
                rs = np.where(low[..., None], PM.mulT(R[:, None, :], cs - p[:, None, :]) - PM.HIP, rs)
            sw = ~stance[..., None]
            r = np.where(sw, rs, r)
            rdot = np.where(sw, np.asarray(v_des, f64), rdot)
            c = np.where(sw, cs, c)
        return self._rows(R, q, self._row_p(p, support), w, vb, r, rdot, vdot) + (c,)

    def _row_p(self, p, support):
        """Columns 4:7 of the state row: p, with REBASE_Z its height above the stance feet."""
        row_p = p.copy()
        if self.flags & REBASE_Z:                                                                            # 4
            row_p[:, 2] = p[:, 2] - support
        return row_p
