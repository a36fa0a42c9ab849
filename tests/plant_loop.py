"""The closed loop controller <-> plant on the CPU, and the statistics both loops are compared by -- TEST SIDE ONLY.

closed_loop() is the ONLY copy of the reference tick: the controller's restatements (tests/ctrl_model.py,
ctrl_model_mode1.py, the cheater estimators of ctrl_model_state.py or the filter behind a sensor model) with the
reference's own qpOASES for every solve (reference_mpc: oracle.solve_batch), on whatever plant model, sensor model and
actuator model the caller hands it.  cpu_loop() runs it on tests/plant_model.py; plant_loop_varied, plant_loop_terrain,
plant_loop_contact, plant_loop_field, sense_loop and act_loop hold the other scenarios and call it too.
tests/golden/make_plant_closed_loop.py records cpu_loop()'s statistics; tests/test_gpu_plant.py holds the GPU loop (library
controller + device plant) to the recorded envelope by the rule of envelope().  The device side of that comparison --
the walk and the statistics from the device accumulators -- is tests/fleet_gpu.py.
"""
import numpy as np

from oracle import oracle as O

import ctrl_model as M
import ctrl_model_mode1 as M1
import plant_model as PM
from ctrl_model_state import estimate_state

f32 = np.float32
FREQ = 500.0
PID = (100.0, 1.0, 0.0, 0.05)     # the reference's simulation parameters (stand_kp, stand_kd, joint_kp, joint_kd)
TICKS = 650                        # 50 solves at 500 Hz
N_CMD = 16
STATS = ("z_min", "z_max", "roll_max", "pitch_max", "vx_mean")


def commands(mode):
    """The command set of the closed-loop tests: 16 robots.  Mode 0: gait numbers from {0, 4, 5, 10} (standing robots
    are commanded 0); both modes: x commands over [0, 0.5] m/s, small yaw rates, start yaws near 0."""
    k = np.arange(N_CMD)
    gait = np.array([0, 4, 5, 10], np.int32)[k % 4] if mode == 0 else np.full(N_CMD, 9, np.int32)
    vel = np.zeros((N_CMD, 3))
    vel[:, 0] = 0.5 * (k // 4 + (k % 4) / 4.0) / 3.75
    vel[:, 2] = 0.1 * ((k % 3) - 1)
    if mode == 0:
        vel[gait == 4] = 0.0
    xyyaw = np.zeros((N_CMD, 3))
    xyyaw[:, 0], xyyaw[:, 1] = 0.5 * (k % 4), 0.5 * (k // 4)
    xyyaw[:, 2] = 0.05 * ((k % 5) - 2)
    return gait, vel, xyyaw


def rpy_of(q):
    """roll, pitch, yaw [B,3] of quaternions w x y z (float64)."""
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([np.arctan2(2 * (y * z + w * x), 1 - 2 * (x * x + y * y)),
                     np.arcsin(np.clip(2 * (w * y - x * z), -1, 1)),
                     np.arctan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))], -1)


class Recorder:
    """Per robot: min / max body height, max |roll|, |pitch|, mean forward (body x) speed over the last second."""

    def __init__(self, B, ticks, freq=FREQ):
        self.z_min, self.z_max = np.full(B, np.inf), np.full(B, -np.inf)
        self.roll_max, self.pitch_max = np.zeros(B), np.zeros(B)
        self.vx_sum, self.n_vx = np.zeros(B), 0
        self.t, self.last = 0, ticks - int(freq)

    def add(self, state, initial=False):
        """The state after a tick; initial=True: the state before the first tick (extremes only, so that every maximum
        and minimum includes the start -- the height's maximum is the start's 0.29 exactly in both loops)."""
        state = np.asarray(state, np.float64)
        rpy = rpy_of(state[:, 0:4])
        self.z_min, self.z_max = np.minimum(self.z_min, state[:, 6]), np.maximum(self.z_max, state[:, 6])
        self.roll_max = np.maximum(self.roll_max, np.abs(rpy[:, 0]))
        self.pitch_max = np.maximum(self.pitch_max, np.abs(rpy[:, 1]))
        if initial:
            return
        if self.t >= self.last:
            self.vx_sum += state[:, 10]
            self.n_vx += 1
        self.t += 1

    def stats(self):
        return dict(z_min=self.z_min, z_max=self.z_max, roll_max=self.roll_max, pitch_max=self.pitch_max,
                    vx_mean=self.vx_sum / max(self.n_vx, 1))


def envelope(rec):
    """Recorded per-command statistics {name: [16]} -> {name: (lo [16], hi [16])}: a robot's own recorded value, widened
    on both sides by twice the spread (max - min) of that quantity across the CPU run's 16 robots; z_min / the maxima
    are one-sided quantities but are held on both sides all the same."""
    out = {}
    for k in STATS:
        v = np.asarray(rec[k], np.float64)
        s = 2.0 * (v.max() - v.min())
        out[k] = (v - s, v + s)
    return out


def controller_for(mode):
    """-> (the controller's restatement for robot mode `mode` with commands() set, the start poses xyyaw [16, 3])."""
    gait, vel, xyyaw = commands(mode)
    m = (M1.CtrlModelMode1 if mode == 1 else M.CtrlModel)(N_CMD, FREQ, PID)
    m.set_gait(gait)
    m.set_vel(vel)
    return m, xyyaw


def reference_mpc(m, e, due):
    """The reference's MPC for the robots `due` (not empty): command -> oracle.pack_commands (mode 1: with the gait
    tables) -> wpd / xci written back -> the reference's own qpOASES -> the forces in the body frame into m.f_ff[due].
    The MPC's model is the controller's: 9 kg, mu 0.4, flat ground, whatever the plant stands on.  -> (nwsr, rc) [due]."""
    if isinstance(m, M1.CtrlModelMode1):
        cmd, tables = m.command_mode1(e, due)
        r, wpd, xci = O.pack_commands(cmd, float(m.dt_mpc))
        r["gait"] = tables
    else:
        r, wpd, xci = O.pack_commands(m.command(e), float(m.dt_mpc))
    m.wpd[due], m.xci[due] = wpd, xci
    r.update(dt=float(m.dt_mpc), mu=0.4, f_max=120.0)
    soln, nwsr, rc = O.solve_batch(r)
    m.f_ff[due] = O.forces_to_body(e["r_body"][due], soln[:, :12].astype(f32))
    return nwsr, rc


def closed_loop(m, plant, ticks, sensors=None, settle=0, actuators=None, each_tick=None):
    """THE reference closed loop -- every cpu_loop* of the loop modules is this on its own models.  Per tick: estimate ->
    loco -> the robots that are due (mode 0: all, every 13th tick; mode 1: m.due) -> reference_mpc -> legcmd -> plant step
    -> Recorder.  m: a controller's restatement with its commands set; plant: a plant model that the caller has built,
    bound and reset.

    sensors     a sense_model.SenseModel: the controller estimates from its readings (CtrlModel.estimate) in the order of
                binding.rollout_sensed -- `settle` times sense -> estimate on the standing plant first (with settle = 0
                one reading and no estimate), then one reading after every step.  None: the cheater estimators of
                ctrl_model_state.estimate_state on the plant's own rows.
    actuators   an act_model.ActModel, applied to the effort with the motor rates the plant showed before the step.
    each_tick   each_tick(t, plant), called just before the step of tick t.

    -> (stats, info): the Recorder's statistics; info holds safe [B], per robot nwsr_max [B] and rc_bad [B] (the number
    of solves whose return code was not 0), n_solves, the last tick's estimate, and the objects the loop ran (ctrl, plant,
    sensors, actuators)."""
    B = plant.B
    mode1 = isinstance(m, M1.CtrlModelMode1)
    rec = Recorder(B, ticks)
    rec.add(plant.state, initial=True)
    if sensors is not None:
        for _ in range(max(settle, 1)):               # BatchedSensors.settle: sense -> pre_work on the standing plant
            imu, motor = sensors.sense(plant.state, plant.motor)
            if settle:
                m.estimate(imu, motor)
    nwsr_max, rc_bad, n_solves, e = np.zeros(B, int), np.zeros(B, int), 0, None
    for t in range(ticks):
        e = estimate_state(m, plant.state, plant.motor) if sensors is None else m.estimate(imu, motor)
        m.loco(e)
        if mode1:
            due = np.flatnonzero(m.due)
        else:
            due = np.arange(B) if (t + 1) % 13 == 0 else np.zeros(0, int)
        if len(due):
            nwsr, rc = reference_mpc(m, e, due)
            rc_bad[due] += (rc != 0)
            nwsr_max[due] = np.maximum(nwsr_max[due], nwsr)
            n_solves += len(due)
        eff = m.legcmd(e, m.f_ff)
        if actuators is not None:
            eff = actuators.apply(eff, np.asarray(plant.motor, np.float64)[:, 12:24])
        if each_tick is not None:
            each_tick(t, plant)
        plant.step(eff, m.contact_state, m.p_des, m.v_des)
        rec.add(plant.state)
        if sensors is not None:
            imu, motor = sensors.sense(plant.state, plant.motor)
    return rec.stats(), dict(safe=m.safe.copy(), nwsr_max=nwsr_max, rc_bad=rc_bad, n_solves=n_solves, estimate=e, ctrl=m,
                             plant=plant, sensors=sensors, actuators=actuators)


def scalars(info):
    """info of closed_loop -> the fields cpu_loop reports: safe, nwsr_max over everything, rc_bad as a count, n_solves."""
    return dict(safe=info["safe"], nwsr_max=int(info["nwsr_max"].max()), n_solves=info["n_solves"],
                rc_bad=int(info["rc_bad"].sum()))


def cpu_loop(mode, ticks=TICKS, substeps=1, mu=0.4):
    """-> (stats, info): info holds safe [B], the largest reference nWSR, the number of solves."""
    m, xyyaw = controller_for(mode)
    stats, info = closed_loop(m, PM.PlantModel(N_CMD, FREQ, mu, substeps, xyyaw), ticks)
    return stats, scalars(info)


