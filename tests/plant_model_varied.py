"""The plant of include/qmpc_plant_vary.h in numpy float64 -- TEST SIDE ONLY.

VariedPlantModel is tests/plant_model.py's PlantModel with the three changes of the header, in its order: the cone of the
robot's own mu_b (2a), the external force and moment added to the quad sums component by component, only when bound
(2b), and the robot's own mass and inertia in vdot / wdot (2c).  It also holds the per-robot statistics of the header
with their initial values, updated at the new pose by every step while `stats_on`.
"""
import numpy as np

import plant_model as PM
from plant_loop import rpy_of

f64 = np.float64
STAT_KEYS = ("n", "z_min", "z_max", "roll_max", "pitch_max", "vx_sum", "vy_sum")


def stats_initial(B):
    return dict(n=np.zeros(B, np.int32), z_min=np.full(B, np.inf), z_max=np.full(B, -np.inf), roll_max=np.zeros(B),
                pitch_max=np.zeros(B), vx_sum=np.zeros(B), vy_sum=np.zeros(B))


class VariedPlantModel(PM.PlantModel):
    """mass_b [B], ibody_b [B,3], mu_b [B], force [B,3] (world), torque [B,3] (body); None: the parent's value / none
    (an unbound member of qmpc_plant_params)."""

    def __init__(self, B, freq=500.0, mu=0.4, substeps=1, init_xyyaw=None, mass=PM.MASS, ibody=PM.IBODY, geom=PM.GEOM,
                 mass_b=None, ibody_b=None, mu_b=None, force=None, torque=None, stats_on=True):
        super().__init__(B, freq, mu, substeps, init_xyyaw, mass=mass, ibody=ibody, geom=geom)
        self.set_params(mass_b, ibody_b, mu_b, force, torque)
        self.stats_on = stats_on
        self.stats = stats_initial(B)

    def set_params(self, mass_b=None, ibody_b=None, mu_b=None, force=None, torque=None):
        B = self.B
        arr = lambda a, shape: None if a is None else np.array(a, f64).reshape(shape)
        self.mass_b, self.ibody_b, self.mu_b = arr(mass_b, (B,)), arr(ibody_b, (B, 3)), arr(mu_b, (B,))
        self.force, self.torque = arr(force, (B, 3)), arr(torque, (B, 3))

    def reset_stats(self, mask=None):
        mask = np.ones(self.B, bool) if mask is None else np.asarray(mask).astype(bool)
        for k, v in stats_initial(self.B).items():
            self.stats[k][mask] = v[mask]

    def own(self):
        """-> mass [B], ibody [B,3], mu [B]: the robot's own value where an array is bound, else the handle's."""
        B = self.B
        return (np.full(B, self.mass) if self.mass_b is None else self.mass_b,
                np.broadcast_to(self.ibody, (B, 3)) if self.ibody_b is None else self.ibody_b,
                np.full(B, self.mu) if self.mu_b is None else self.mu_b)

    def step(self, effort, contact_state, p_des, v_des):
        B, h = self.B, self.h
        mass, ibody, mu = self.own()
        tau = np.asarray(effort, f64).reshape(B, 4, 3)
        stance = np.asarray(contact_state).reshape(B, 4) > 0
        p, v, q, w, c = self.p.copy(), self.v.copy(), self.q.copy(), self.w.copy(), self.foot.copy()
        c[..., 2] = np.where(stance & ~self.stance, 0.0, c[..., 2])
        f, vdot = np.zeros((B, 4, 3)), np.zeros((B, 3))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # (a robot's own bad values are its own)
            for _ in range(self.substeps):
                R = PM.rot(q)
                rb = PM.mulT(R[:, None, :], c - p[:, None, :])
                f = np.where(stance[..., None], PM.stance_force(R, rb, tau, mu[:, None], self.geom), 0.0)      # 2a
                fb = PM.mulT(R[:, None, :], f)
                m = PM.cross(rb, fb)
                F, N = PM.add_wrench(PM.quad_sum(f), PM.quad_sum(m), self.force, self.torque)                  # 2b
                p, v, w, vdot = PM.body_update(p, v, w, F, N, mass, ibody, h)                                  # 2c
                q = PM.quat_step(q, w, h)
            state, motor, c = self._readout(p, v, q, w, c, stance, vdot, np.asarray(p_des).reshape(B, 4, 3),
                                            np.asarray(v_des).reshape(B, 4, 3))
        self.p, self.v, self.q, self.w, self.foot, self.grf, self.stance = p, v, q, w, c, f, stance
        self.state, self.motor = state, motor
        if self.stats_on:
            self._accumulate(state)
        return state, motor

    def _accumulate(self, state):
        s = self.stats
        with np.errstate(invalid="ignore"):
            rpy = rpy_of(state[:, 0:4])
            s["n"] += 1
            s["z_min"], s["z_max"] = np.minimum(s["z_min"], state[:, 6]), np.maximum(s["z_max"], state[:, 6])
            s["roll_max"] = np.maximum(s["roll_max"], np.abs(rpy[:, 0]))
            s["pitch_max"] = np.maximum(s["pitch_max"], np.abs(rpy[:, 1]))
            s["vx_sum"] = s["vx_sum"] + state[:, 10]
            s["vy_sum"] = s["vy_sum"] + state[:, 11]
