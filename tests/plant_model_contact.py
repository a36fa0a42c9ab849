"""The plant of include/qmpc_contact.h in numpy float64 -- TEST SIDE ONLY.

ContactPlantModel is tests/plant_model_terrain.py's TerrainPlantModel with contact decided by the ground, operation by
operation in the order of quadruped_ctrl_amd/csrc/qmpc_contact.hip: `stance` is the physical pinned flag pi, the gait's
schedule s only proposes; a scheduled foot that is still in the air is late and is lowered until it lands, a swing foot
that meets the surface is pinned early, and a foot whose force leaves the friction cone slides.  With flags = 0 it is
TerrainPlantModel: step() hands over to it.  With no rows bound the ground is an all-zero row (height 0, normal
(-0, -0, 1)).
"""
import numpy as np

import plant_model as PM
import plant_model_terrain as PT

f64 = np.float64
EARLY, LATE, SLIP = 1, 2, 4
DROP_SPEED, SLIP_GAIN, SLIP_VMAX = 1.0, 0.01, 1.0


class ContactPlantModel(PT.TerrainPlantModel):
    def __init__(self, B, *a, **kw):
        self.cflags, self.drop_speed, self.slip_gain, self.slip_vmax = 0, DROP_SPEED, SLIP_GAIN, SLIP_VMAX
        self.early, self.late = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.slip, self.drop = np.zeros(B), np.zeros((B, 4))
        # what the last contact step decided (trace) and every comparison it branched on (ties: name, a, b, where it
        # counted; floors: the tread abscissae that went through floor()) -- for tests/contact_cases.py
        self.trace, self.ties, self.floors = {}, [], None
        super().__init__(B, *a, **kw)                       # qmpc_plant_init: contact off

    def set_contact(self, early=False, late=False, slip=False, drop_speed=DROP_SPEED, slip_gain=SLIP_GAIN,
                    slip_vmax=SLIP_VMAX):
        self.cflags = (EARLY if early else 0) | (LATE if late else 0) | (SLIP if slip else 0)
        self.drop_speed, self.slip_gain, self.slip_vmax = float(drop_speed), float(slip_gain), float(slip_vmax)

    def height(self, x, y):
        if self.floors is not None:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                self.floors.append(np.asarray(self.tread(x, y)).reshape(-1))
        return super().height(x, y)

    def reset(self, mask, init_xyyaw=None):
        super().reset(mask, init_xyyaw)
        mask = np.asarray(mask).astype(bool)
        if self.cflags:
            self.early[mask], self.late[mask], self.slip[mask], self.drop[mask] = 0, 0, 0.0, 0.0
            if self.rows is None:
                self.support[mask], self.ground[mask] = 0.0, 0.0

    def step(self, effort, contact_state, p_des, v_des):
        if not self.cflags:
            return super().step(effort, contact_state, p_des, v_des)
        unbound = self.rows is None
        if unbound:
            self.rows = np.zeros((self.B, 8))               # (the terrain flags are 0 while nothing is bound)
        try:
            return self._step_contact(effort, contact_state, p_des, v_des)
        finally:
            if unbound:
                self.rows = None

    def _step_contact(self, effort, contact_state, p_des, v_des):
        B, h, fl = self.B, self.h, self.cflags
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
            n = self.normal()[:, None, :]
            # 1. edges
            hz = self.height(c[..., 0], c[..., 1])
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
                    cz = np.where(slid, self.height(cx, cy), c[..., 2])
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

    def _release_and_readout(self, s, pin, p, v, q, w, c, cd, drop, vdot, pd, vd, support):
        """Steps 3 and 4 of include/qmpc_contact.h at the new pose, inside the caller's np.errstate: the commands of the feet
        that are not both scheduled and pinned, their touch-down or release, then the read-out.  -> pin, c, drop, state,
        motor; the decisions go to self.trace and self.ties, the counters to self.early / self.late, the ground under the
        body to self.ground.  Every height is self.height(): the summed surface in tests/plant_model_field.py."""
        B, fl = self.B, self.cflags
        # 3. unpinned feet and release, at the new pose
        R = PM.rot(q)
        vb = PM.mulT(R, v)
        cmd = ~(s & pin)                                      # feet whose command is evaluated
        lateft = s & ~pin
        drop = np.where(lateft, drop + self.drop_speed * self.dt, drop)
        ez = R[:, None, 6:9]                                   # rBody e_z
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
        self.trace.update(late=lateft, hit=hit, newpin=newpin, free=free, pin2=pin.copy(), foot1=c.copy())
        self.early = self.early + (~s & pin).sum(1).astype(np.int32)
        self.late = self.late + lateft.sum(1).astype(np.int32)
        drop = np.where(pin | ~s, 0.0, drop)
        # 4. read-out
        rb = PM.mulT(R[:, None, :], c - p[:, None, :])
        r = np.where((pin | low)[..., None], rb - PM.HIP, rs)
        rdot = np.where(pin[..., None], (-vb[:, None, :] - PM.cross(w[:, None, :], rb)) + PM.mulT(R[:, None, :], cd), vd)
        state, motor = self._rows(R, q, self._row_p(p, support), w, vb, r, rdot, vdot)
        self.ground = self.height(p[:, 0], p[:, 1])
        return pin, c, drop, state, motor

    def _force(self, R, rb, tau, mu, n, pin):
        """-> f [B,4,3], slid [B,4], sv [B,4] (the sliding speed), t, ft: plant_model_terrain.stance_force_terrain on the
        pinned feet, with the saturation it found."""
        g, ok = PM.leg_force(R, rb, tau, self.geom)
        fn = (g[..., 0] * n[..., 0] + g[..., 1] * n[..., 1]) + g[..., 2] * n[..., 2]
        ok = ok & (fn > 0.0) & pin
        t = g - fn[..., None] * n
        ft = np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
        cap = mu * fn
        sat = ok & (ft > cap)
        sc = cap / ft
        f = np.where(sat[..., None], fn[..., None] * n + t * sc[..., None], g)
        f = np.where(ok[..., None], f, 0.0)
        sv = self.slip_gain * (ft - cap)
        sv = np.where(sv > self.slip_vmax, self.slip_vmax, sv)
        slid = sat & bool(self.cflags & SLIP)
        self.ties.append(("cone", ft, cap, ok))
        return f, slid, sv, t, ft
