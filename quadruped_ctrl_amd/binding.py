"""ctypes binding of the C ABI in include/qmpc.h (libqmpc.so).

PyTorch is used only for device memory and streams; every solve goes through
the hand-written HIP kernels in csrc/.  There is no CPU or PyTorch fallback:
if libqmpc.so is missing or no HIP device is present this module raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libqmpc.so")

QMPC_OK = 0
ABI_VERSION = 23              # qmpc_abi_version() this binding was written against
ST_MAXITER, ST_NOT_PD, ST_INFEASIBLE, ST_WS_FULL, ST_FALLBACK = 1, 2, 4, 8, 16
ST_COMPACTED, ST_SPILLED = 64, 128
ST_NONFINITE = 32
ST_ERROR_MASK = 15 | 32
# the int32 arrays among the controller's device state (QMPC_CTRL_ARRAYS in csrc/qmpc_glue.h): what read() returns as int32
CTRL_INT_ARRAYS = ("counter", "first_run", "first_swing", "first_visit", "gait_num", "current_gait", "offsets", "durations",
                   "iteration", "safe", "status", "due", "due_list", "due_count", "nseg", "mpc_offsets", "mpc_durations")
CTRL_SCHEDULES = dict(lockstep=0, per_robot=1)   # QMPC_CTRL_LOCKSTEP / QMPC_CTRL_PER_ROBOT (include/qmpc_ctrl.h)

# qmpc_ctrl_view's float arrays (include/qmpc_ctrl.h) in declaration order, elements per robot
CTRL_VIEW_FIELDS = ("position", "v_world", "orientation", "rpy", "r_body", "omega_world", "leg_q", "leg_p", "leg_v",
                    "leg_J", "contact_state", "swing_state", "p_des", "v_des", "f_ff")
CTRL_VIEW_WIDTH = dict(position=3, v_world=3, orientation=4, rpy=3, r_body=9, omega_world=3, leg_q=12, leg_p=12, leg_v=12,
                       leg_J=36, contact_state=4, swing_state=4, p_des=12, v_des=12, f_ff=12, safe=1, counter=1)

KF_FIELDS = ("xhat", "P", "r_body", "a_world", "omega_body", "contact_phase", "leg_p", "leg_v", "position", "v_world", "v_body")

# qmpc_leg_command fields (include/qmpc.h), in declaration order
LEG_F32 = ("tau_ff", "force_ff", "kp_cart", "kd_cart", "p_des", "v_des", "q", "qd", "J", "p", "v")

# qmpc_command fields (include/qmpc.h), in declaration order
CMD_F32 = ("position", "v_world", "omega_world", "orientation", "rpy", "r_body", "p_foot",
           "vel_des", "yaw_des_true", "rpy_comp", "stand_traj", "rp_des")
CMD_I32 = ("gait_type", "gait_offsets", "gait_durations", "gait_iteration")
CMD_STATE = ("world_position_desired", "x_comp_integral")
REC_FIELDS = ("p", "v", "q", "w", "r", "yaw", "traj", "gait", "x_drag", "weights", "alpha")
# qmpc_inputs arrays (include/qmpc.h), in declaration order
INPUT_FIELDS = ("p", "v", "q", "w", "r", "yaw", "traj", "gait", "weights", "alpha", "x_drag")


class Inputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in INPUT_FIELDS] + [("weights_stride", C.c_int), ("alpha_stride", C.c_int),
                                                          ("x_drag_stride", C.c_int)]


class Outputs(C.Structure):
    _fields_ = [("grf", C.c_void_p), ("soln", C.c_void_p),
                ("status", C.c_void_p), ("iters", C.c_void_p)]


class Command(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in CMD_F32 + CMD_I32 + CMD_STATE] + [
        ("body_height", C.c_float), ("omni_mode", C.c_int)]


class Record(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in REC_FIELDS]


class KfState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("xhat", "P", "r_body", "a_world", "omega_body", "contact_phase", "leg_p", "leg_v",
                                          "position", "v_world", "v_body")]


class CtrlView(C.Structure):
    """qmpc_ctrl_view (include/qmpc_ctrl.h)."""
    _fields_ = [(n, C.c_void_p) for n in CTRL_VIEW_FIELDS] + [("safe", C.c_void_p), ("counter", C.c_void_p),
                                                                ("batch", C.c_int), ("ticks", C.c_int)]


# qmpc_plant_view's arrays (include/qmpc_plant.h) in declaration order: name -> (elements per robot, typestr)
PLANT_VIEW_FIELDS = dict(p=(3, "<f8"), v=(3, "<f8"), q=(4, "<f8"), omega=(3, "<f8"), foot=(12, "<f8"), stance=(4, "<i4"),
                         grf=(12, "<f8"), state=(16, "<f8"), motor=(24, "<f8"))


class PlantView(C.Structure):
    """qmpc_plant_view (include/qmpc_plant.h)."""
    _fields_ = [(n, C.c_void_p) for n in PLANT_VIEW_FIELDS] + [("batch", C.c_int), ("substeps", C.c_int),
                                                               ("mu_plant", C.c_double)]


# qmpc_plant_stats' arrays (include/qmpc_plant_vary.h) in declaration order: name -> typestr, [B] each
PLANT_STATS_FIELDS = dict(n="<i4", z_min="<f8", z_max="<f8", roll_max="<f8", pitch_max="<f8", vx_sum="<f8", vy_sum="<f8")
# qmpc_plant_params' members in declaration order: name -> elements per robot
PLANT_PARAM_FIELDS = dict(mass=1, ibody=3, mu=1, force=3, torque=3)


class PlantParams(C.Structure):
    """qmpc_plant_params (include/qmpc_plant_vary.h)."""
    _fields_ = [(n, C.c_void_p) for n in PLANT_PARAM_FIELDS]


class TerrainView(C.Structure):
    """qmpc_terrain_view (include/qmpc_terrain.h)."""
    _fields_ = [("ground", C.c_void_p), ("support", C.c_void_p), ("terrain", C.c_void_p), ("flags", C.c_int),
                ("batch", C.c_int)]


TERRAIN_CLAMP_SWING, TERRAIN_REBASE_Z = 1, 2


class ContactParams(C.Structure):
    """qmpc_contact_params (include/qmpc_contact.h)."""
    _fields_ = [("flags", C.c_int), ("drop_speed", C.c_double), ("slip_gain", C.c_double), ("slip_vmax", C.c_double)]


class ContactView(C.Structure):
    """qmpc_contact_view (include/qmpc_contact.h)."""
    _fields_ = [("early", C.c_void_p), ("late", C.c_void_p), ("slip", C.c_void_p), ("drop", C.c_void_p),
                ("params", ContactParams), ("batch", C.c_int)]


CONTACT_EARLY, CONTACT_LATE, CONTACT_SLIP = 1, 2, 4


class FieldBank(C.Structure):
    """qmpc_field_bank (include/qmpc_field.h)."""
    _fields_ = [("z", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("count", C.c_int), ("cell", C.c_double)]


class FieldView(C.Structure):
    """qmpc_field_view (include/qmpc_field.h)."""
    _fields_ = [("bank", FieldBank), ("place", C.c_void_p), ("flags", C.c_int), ("batch", C.c_int)]


class PlantStats(C.Structure):
    """qmpc_plant_stats (include/qmpc_plant_vary.h)."""
    _fields_ = [(n, C.c_void_p) for n in PLANT_STATS_FIELDS] + [("batch", C.c_int), ("enabled", C.c_int)]


# qmpc_sense_params' members (include/qmpc_sense.h) in declaration order: name -> elements per robot
SENSE_PARAM_FIELDS = dict(acc_bias=3, gyro_bias=3, acc_sigma=1, gyro_sigma=1, q_sigma=1, qd_sigma=1)


class SenseParams(C.Structure):
    """qmpc_sense_params (include/qmpc_sense.h)."""
    _fields_ = [(n, C.c_void_p) for n in SENSE_PARAM_FIELDS]


class SenseView(C.Structure):
    """qmpc_sense_view (include/qmpc_sense.h)."""
    _fields_ = [("n", C.c_void_p), ("epoch", C.c_void_p), ("batch", C.c_int), ("seed", C.c_uint64)]


# qmpc_episode_view's arrays (include/qmpc_episode.h) in declaration order: name -> (elements per robot or None, typestr)
EPISODE_VIEW_FIELDS = dict(age=(None, "<i4"), episode=(None, "<i4"), start=(2, "<f8"), count=(6, "<i4"),
                           ticks_sum=(None, "<i8"), last_cause=(None, "<i4"), last_ticks=(None, "<i4"), mask=(None, "|u1"),
                           xyyaw=(3, "<f8"))
EP_UNSAFE, EP_NONFINITE, EP_TILT, EP_HEIGHT, EP_RANGE, EP_TIMEOUT = 1, 2, 4, 8, 16, 32
EP_CAUSES = dict(unsafe=EP_UNSAFE, nonfinite=EP_NONFINITE, tilt=EP_TILT, height=EP_HEIGHT, range=EP_RANGE,
                 timeout=EP_TIMEOUT)   # in bit order: the columns of the view's count
EP_SPAWN_PER_ROBOT = 1
EPISODE_LOG_COLUMNS = ("robot", "episode", "cause", "age", "dx", "dy", "height", "tilt")


class EpisodeRule(C.Structure):
    """qmpc_episode_rule (include/qmpc_episode.h)."""
    _fields_ = [("causes", C.c_int), ("max_ticks", C.c_int), ("cos_tilt_min", C.c_double), ("z_min", C.c_double),
                ("range", C.c_double)]


class EpisodeBind(C.Structure):
    """qmpc_episode_bind (include/qmpc_episode.h)."""
    _fields_ = [("vel", C.c_void_p), ("gait", C.c_void_p), ("spawn", C.c_void_p), ("commands", C.c_void_p),
                ("log", C.c_void_p), ("n_spawn", C.c_int), ("n_commands", C.c_int), ("log_rows", C.c_int),
                ("flags", C.c_int)]


class EpisodeView(C.Structure):
    """qmpc_episode_view (include/qmpc_episode.h)."""
    _fields_ = [(n, C.c_void_p) for n in EPISODE_VIEW_FIELDS] + [("log_count", C.c_void_p), ("log_dropped", C.c_void_p),
                                                                 ("batch", C.c_int), ("seed", C.c_uint64)]


# qmpc_act_config's scalar members after gear[3] (include/qmpc_act.h) in declaration order
ACT_CONFIG_FIELDS = dict(kt=C.c_double, R=C.c_double, battery_v=C.c_double, damping=C.c_double, dry_friction=C.c_double,
                         tau_max=C.c_double, friction=C.c_int, max_delay=C.c_int)
# qmpc_act_params' members in declaration order: name -> dtype name (one element per robot)
ACT_PARAM_FIELDS = dict(battery_v="float64", tau_max="float64", strength="float64", damping="float64",
                        dry_friction="float64", delay="int32")
# qmpc_act_view's per-robot arrays in declaration order (after ring): name -> typestr
ACT_VIEW_FIELDS = dict(head="<i4", age="<i4", n="<i4", n_vsat="<i8", n_tsat="<i8", tau_peak="<f8", e_heat="<f8",
                       e_mech="<f8", e_pos="<f8")
ACT_STATS = ("n", "n_vsat", "n_tsat", "tau_peak", "e_heat", "e_mech", "e_pos")
ACT_MAX_DELAY = 64


class ActConfig(C.Structure):
    """qmpc_act_config (include/qmpc_act.h)."""
    _fields_ = [("gear", C.c_double * 3)] + list(ACT_CONFIG_FIELDS.items())


class ActParams(C.Structure):
    """qmpc_act_params (include/qmpc_act.h)."""
    _fields_ = [(n, C.c_void_p) for n in ACT_PARAM_FIELDS]


class ActView(C.Structure):
    """qmpc_act_view (include/qmpc_act.h)."""
    _fields_ = ([("ring", C.c_void_p)] + [(n, C.c_void_p) for n in ACT_VIEW_FIELDS]
                + [("config", ActConfig), ("dt", C.c_double), ("batch", C.c_int)])


class EpisodeSenseView(C.Structure):
    """qmpc_episode_sense_view (include/qmpc_episode_sense.h)."""
    _fields_ = [("warm", C.c_void_p), ("hold", C.c_void_p), ("warm_ticks", C.c_int), ("batch", C.c_int)]


# qmpc_fleet_info's members (include/qmpc_fleet.h) in declaration order, and the bits of its `reason`
FLEET_INFO_FIELDS = ("ticks", "fused_ticks", "fused_launches", "fallback_ticks", "reason")
FLEET_REASONS = dict(terrain=1, contact=2, field=4)


class FleetInfo(C.Structure):
    """qmpc_fleet_info (include/qmpc_fleet.h)."""
    _fields_ = [(n, C.c_int if n == "reason" else C.c_longlong) for n in FLEET_INFO_FIELDS]


# qmpc_loop_opts' and qmpc_loop_info's members (include/qmpc_loop.h) in declaration order; the reason bits are the fleet run's
LOOP_OPTS_FIELDS = ("actuators", "episodes_every", "actuator_stats")
LOOP_INFO_FIELDS = ("ticks", "fused_ticks", "fused_launches", "fallback_ticks", "reason")
LOOP_REASONS = dict(terrain=1, contact=2, field=4)


class LoopOpts(C.Structure):
    """qmpc_loop_opts (include/qmpc_loop.h)."""
    _fields_ = [(n, C.c_int) for n in LOOP_OPTS_FIELDS]


class LoopInfo(C.Structure):
    """qmpc_loop_info (include/qmpc_loop.h)."""
    _fields_ = [(n, C.c_int if n == "reason" else C.c_longlong) for n in LOOP_INFO_FIELDS]


class LegCommand(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LEG_F32] + [("kp_joint", C.c_float), ("kd_joint", C.c_float)]


def make_inputs(arrays, batch):
    """Inputs over the record arrays in `arrays` (INPUT_FIELDS keys; contiguous numpy arrays or torch tensors).  weights,
    alpha and x_drag are per robot when they hold `batch` rows, else one row shared by the batch (stride 0); with
    batch == 1 both readings address the same row."""
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    numel = lambda a: a.numel() if hasattr(a, "numel") else a.size
    inp = Inputs(*(ptr(arrays[k]) for k in INPUT_FIELDS))
    inp.weights_stride = 12 if numel(arrays["weights"]) == 12 * batch else 0
    inp.alpha_stride = 1 if numel(arrays["alpha"]) == batch else 0
    inp.x_drag_stride = 1 if numel(arrays["x_drag"]) == batch else 0
    return inp


def _host_record(b):
    """The record arrays of a numpy batch dict (workloads layout), contiguous, in the kernels' dtypes."""
    rec = {k: np.ascontiguousarray(b[k], np.float32) for k in INPUT_FIELDS if k != "gait"}
    rec["gait"] = np.ascontiguousarray(b["gait"], np.uint8)
    return rec


def _host_outputs(batch, horizon, full):
    """Host result arrays ({grf, status, iters[, soln]}) and the Outputs over them."""
    res = {"grf": np.zeros((batch, 12), np.float32), "status": np.zeros(batch, np.int32),
           "iters": np.zeros(batch, np.int32)}
    if full:
        res["soln"] = np.zeros((batch, 12 * horizon))
    out = Outputs(res["grf"].ctypes.data, res["soln"].ctypes.data if full else None, res["status"].ctypes.data,
                  res["iters"].ctypes.data)
    return res, out


# C signatures: name -> argtypes, or (argtypes, restype) where the result is not int
_P, _I, _D = C.c_void_p, C.c_int, C.c_double
# include/qmpc.h, qmpc_expert.h and qmpc_debug.h
SIGNATURES = {
    "qmpc_abi_version": [],
    "qmpc_last_error": ([_P], C.c_char_p),
    "qmpc_create": [_I, _I, _I, C.POINTER(_P)],
    "qmpc_destroy": [_P],
    "qmpc_setup": [_P, _D, _I, _D, _D],
    "qmpc_set_robot": [_P, _D, C.POINTER(_D), _D],
    "qmpc_settings": [_P, _I, _D],
    "qmpc_solve": [_P, _I, C.POINTER(Inputs), C.POINTER(Outputs), _P],
    "qmpc_solve_host": [_P, _I, C.POINTER(Inputs), C.POINTER(Outputs)],
    "qmpc_set_debug": [_P, _P, _P],
    "qmpc_debug_ld": [_P],
    "qmpc_set_debug_clock": [_P, _P],
    "qmpc_set_max_stance": [_P, _I],
    "qmpc_pack": [_P, _I, C.POINTER(Command), C.POINTER(Record), _P],
    "qmpc_forces_to_body": [_P, _I, _P, _P, _P, _P],
    "qmpc_solve_commands": [_P, _I, C.POINTER(Command), C.POINTER(Outputs), _P, _P],
    "qmpc_set_min_stance": [_P, _I],
    "qmpc_set_debug_aux": [_P, _P],
    "qmpc_set_debug_overflow_slices": [_P, _I],
    "qmpc_solve_sharded": [C.POINTER(_P), _I, _I, C.POINTER(Inputs), C.POINTER(Outputs)],
    "qmpc_set_leg_geometry": [_P] + [_D] * 4,
    "qmpc_leg_kinematics": [_P, _I] + [_P] * 6,
    "qmpc_leg_torques": [_P, _I, C.POINTER(LegCommand), _P, _P, _P],
    "qmpc_swing_trajectory": [_P, _I] + [_P] * 9,
    "qmpc_set_warm_start": [_P, _P, _I],
    "qmpc_settings_jcqp": [_P, _I, _I] + [_D] * 4,
    "qmpc_kf_init": [_P, _I, _P, _P, _P],
    "qmpc_kf_step": [_P, _I, C.POINTER(KfState), _P],
    "qmpc_set_model": [_P, _I],
    "qmpc_max_horizon": [],
    "qmpc_set_debug_pool_busy": [_P, _I],
    "qmpc_set_split": [_P, _I],
    "qmpc_reserve": [_P],
    "qmpc_set_debug_engine_events": [_P, _I],
    "qmpc_set_chunks": [_P, _I],
    "qmpc_debug_read_item": [_P, _I, _I, _P, _P, _P],
    "qmpc_debug_read_counts": [_P, _P],
    "qmpc_set_dense": [_P, _I],
    "qmpc_set_size_order": [_P, _I],
    "qmpc_debug_keys": [_P, _I, C.POINTER(Inputs), _P, _P, _P, _P],
    "qmpc_set_order_hint": [_P, _I],
    "qmpc_set_debug_balance": [_P, _I],
    "qmpc_set_warm_start_min_iters": [_P, _I],
    "qmpc_set_debug_overflow_spin": [_P, _I],
    "qmpc_debug_ctrl_read": [_P, C.c_char_p, _P, C.c_longlong, C.POINTER(_I)],
}
# the batched locomotion controller's own header (include/qmpc_ctrl.h), same library and ABI version
CTRL_SIGNATURES = {
    "qmpc_ctrl_init": [_P, _I, _D, C.POINTER(_D), _P],
    "qmpc_ctrl_set_schedule": [_P, _I],
    "qmpc_ctrl_set_robot_mode": [_P, _I],
    "qmpc_ctrl_reset": [_P, _I, _P, _P],
    "qmpc_ctrl_set_gait": [_P, _I, _P, _P],
    "qmpc_ctrl_set_vel": [_P, _I, _P, _P],
    "qmpc_ctrl_prework": [_P, _I, _P, _P, _P],
    "qmpc_ctrl_tick": [_P, _I, _P, _P, _P, _P],
    "qmpc_ctrl_prework_state": [_P, _I, _P, _P, _P],
    "qmpc_ctrl_tick_state": [_P, _I, _P, _P, _P, _P],
    "qmpc_ctrl_view_get": [_P, C.POINTER(CtrlView)],
}
# the reduced-order plant's header (include/qmpc_plant.h), same library and ABI version
PLANT_SIGNATURES = {
    "qmpc_plant_init": [_P, _I, _D, _I, _P, _P],
    "qmpc_plant_reset": [_P, _I, _P, _P, _P],
    "qmpc_plant_step": [_P, _I, _P, _P, _P, _P],
    "qmpc_plant_view_get": [_P, C.POINTER(PlantView)],
}
# per-robot plant parameters and on-device statistics (include/qmpc_plant_vary.h), same library and ABI version
PLANT_VARY_SIGNATURES = {
    "qmpc_plant_set_params": [_P, _I, C.POINTER(PlantParams)],
    "qmpc_plant_stats_enable": [_P, _I],
    "qmpc_plant_stats_reset": [_P, _I, _P, _P],
    "qmpc_plant_stats_get": [_P, C.POINTER(PlantStats)],
}
# per-robot slopes and stairs under the plant (include/qmpc_terrain.h), same library and ABI version
TERRAIN_SIGNATURES = {
    "qmpc_plant_set_terrain": [_P, _I, _P, _I],
    "qmpc_terrain_view_get": [_P, C.POINTER(TerrainView)],
}
# contact decided by the ground under the plant (include/qmpc_contact.h), same library and ABI version
CONTACT_SIGNATURES = {
    "qmpc_plant_set_contact": [_P, _I, C.POINTER(ContactParams)],
    "qmpc_contact_view_get": [_P, C.POINTER(ContactView)],
}
# height-field terrain from memory under the plant (include/qmpc_field.h), same library and ABI version
FIELD_SIGNATURES = {
    "qmpc_plant_set_field": [_P, _I, C.POINTER(FieldBank), _P, _I],
    "qmpc_field_view_get": [_P, C.POINTER(FieldView)],
}
# the sensor model between the plant and the controller's sensor path (include/qmpc_sense.h), same library and ABI version
SENSE_SIGNATURES = {
    "qmpc_sense_init": [_P, _I, C.c_uint64, _P],
    "qmpc_sense_set_params": [_P, _I, C.POINTER(SenseParams)],
    "qmpc_sense_reset": [_P, _I, _P, _P],
    "qmpc_sense": [_P, _I, _P, _P, _P],
    "qmpc_sense_view_get": [_P, C.POINTER(SenseView)],
}
# episodes on the device: termination, respawn, result log (include/qmpc_episode.h), same library and ABI version
EPISODE_SIGNATURES = {
    "qmpc_episode_init": [_P, _I, C.c_uint64, _P],
    "qmpc_episode_set": [_P, _I, C.POINTER(EpisodeRule), C.POINTER(EpisodeBind)],
    "qmpc_episode_step": [_P, _I, _I, _P],
    "qmpc_episode_log_clear": [_P, _P],
    "qmpc_episode_view_get": [_P, C.POINTER(EpisodeView)],
}
# episodes on the sensor path: per-robot warm-up after a reset (include/qmpc_episode_sense.h), same library and ABI version
EPISODE_SENSE_SIGNATURES = {
    "qmpc_episode_sense_init": [_P, _I, _I, _P],
    "qmpc_episode_sense_hold": [_P, _I, _P, _I, _P],
    "qmpc_episode_sense_step": [_P, _I, _P, _P],
    "qmpc_episode_sense_view_get": [_P, C.POINTER(EpisodeSenseView)],
}
# actuators between the controller's effort and the plant (include/qmpc_act.h), same library and ABI version
ACT_SIGNATURES = {
    "qmpc_act_config_default": [C.POINTER(ActConfig)],
    "qmpc_act_init": [_P, _I, C.POINTER(ActConfig), _P],
    "qmpc_act_set_params": [_P, _I, C.POINTER(ActParams)],
    "qmpc_act_reset": [_P, _I, _P, _P, _I, _P],
    "qmpc_act": [_P, _I, _P, _P, _P],
    "qmpc_act_view_get": [_P, C.POINTER(ActView)],
}
# the closed loop of controller and plant, many ticks in one call (include/qmpc_fleet.h), same library and ABI version
FLEET_SIGNATURES = {
    "qmpc_fleet_run": [_P, _I, _I, _P, _P, _P, _P],
    "qmpc_fleet_run_info": [_P, C.POINTER(FleetInfo)],
}
# the fleet's long-running loop -- actuators and episode resets inside the fused launch (include/qmpc_loop.h), same library
# and ABI version
LOOP_SIGNATURES = {
    "qmpc_loop_run": [_P, _I, _I, C.POINTER(LoopOpts), _P, _P, _P, _P],
    "qmpc_loop_run_info": [_P, C.POINTER(LoopInfo)],
}
LOOP_ENTRY_POINTS = list(LOOP_SIGNATURES)
# the switch that lets both run calls serve terrain rows and height fields fused (include/qmpc_ground_run.h), same
# library and ABI version
GROUND_RUN_SIGNATURES = {
    "qmpc_ground_run_enable": [_P, _I],
    "qmpc_ground_run_enabled": [_P, C.POINTER(C.c_int)],
}
GROUND_RUN_ENTRY_POINTS = list(GROUND_RUN_SIGNATURES)
EXPORTS = list(SIGNATURES)
FLEET_EXPORTS = list(FLEET_SIGNATURES)
CTRL_EXPORTS = list(CTRL_SIGNATURES)
PLANT_EXPORTS = list(PLANT_SIGNATURES)
PLANT_VARY_EXPORTS = list(PLANT_VARY_SIGNATURES)
SENSE_EXPORTS = list(SENSE_SIGNATURES)
TERRAIN_EXPORTS = list(TERRAIN_SIGNATURES)
CONTACT_EXPORTS = list(CONTACT_SIGNATURES)
FIELD_EXPORTS = list(FIELD_SIGNATURES)
EPISODE_EXPORTS = list(EPISODE_SIGNATURES)
EPISODE_SENSE_EXPORTS = list(EPISODE_SENSE_SIGNATURES)
ACT_EXPORTS = list(ACT_SIGNATURES)

_lib = None


def load_library():
    """Load libqmpc.so (built in-tree by __graft_entry__.build()).  Loud
    failure when absent -- the product has no other compute path."""
    global _lib
    if _lib is None:
        # PyTorch ships its own copy of the HIP runtime: it has to be the one this process loads FIRST.  Loaded after
        # libqmpc.so (which would pull /opt/rocm's), the process ends up with two runtimes and the kernels registered with
        # the wrong one -- qmpc_create then fails with QMPC_ERR_DEVICE (build() followed by smoke() in one process did)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # Development only: QMPC_LIB names a VARIANT BUILD of this library made by tools/build_variant.sh.  It is honoured only
        # for a file inside this checkout's own (git-ignored) variants/ directory -- the environment cannot point a production
        # load at an arbitrary shared object -- and anything else is refused loudly
        LIB_PATH = globals()["LIB_PATH"]
        override = os.environ.get("QMPC_LIB")
        if override:
            vdir = os.path.realpath(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "variants"))
            real = os.path.realpath(override)
            if os.path.commonpath([real, vdir]) != vdir or os.path.basename(real) != "libqmpc.so":
                raise RuntimeError(f"QMPC_LIB={override!r} refused: only <checkout>/variants/<name>/libqmpc.so "
                                   "(tools/build_variant.sh) may replace the in-tree library")
            LIB_PATH = real
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()')")
        lib = C.CDLL(LIB_PATH)
        for name, sig in {**SIGNATURES, **CTRL_SIGNATURES, **PLANT_SIGNATURES, **PLANT_VARY_SIGNATURES, **TERRAIN_SIGNATURES,
                          **CONTACT_SIGNATURES, **FIELD_SIGNATURES, **SENSE_SIGNATURES, **EPISODE_SIGNATURES,
                          **EPISODE_SENSE_SIGNATURES, **ACT_SIGNATURES, **FLEET_SIGNATURES, **LOOP_SIGNATURES,
                          **GROUND_RUN_SIGNATURES}.items():
            f = getattr(lib, name)
            f.argtypes, f.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        _lib = lib
    return _lib


class QmpcError(RuntimeError):
    pass


class BatchedConvexMPC:
    """Batched MPC solver on one GPU.

    Host-side mirror of the reference's MPC interface
    (src/MPC_Ctrl/convexMPC_interface.h:40-48) for B robots at once:
    setup_problem -> setup(), update_problem_data_floats -> solve(),
    get_solution(0..11) -> the returned grf[B,12].
    """

    def __init__(self, device=0, max_batch=65536, max_horizon=16):
        import torch
        if not torch.cuda.is_available():
            raise QmpcError("no HIP device visible: quadruped_ctrl_amd has no CPU path")
        self.torch = torch
        self.lib = load_library()
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        rc = self.lib.qmpc_create(device, max_batch, max_horizon, C.byref(self.h))
        if rc != QMPC_OK:
            raise QmpcError(f"qmpc_create failed rc={rc}")
        self.horizon = None
        self._dbg = None

    def close(self):
        if self.h:
            self.lib.qmpc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != QMPC_OK:
            err = self.lib.qmpc_last_error(self.h).decode()
            raise QmpcError(f"{what} failed rc={rc} {err}")

    def setup(self, dt, horizon, mu, f_max):
        self._check(self.lib.qmpc_setup(self.h, dt, horizon, mu, f_max), "qmpc_setup")
        self.horizon = horizon

    def set_robot(self, mass, ibody, gravity):
        arr = (C.c_double * 3)(*ibody)
        self._check(self.lib.qmpc_set_robot(self.h, mass, arr, gravity), "qmpc_set_robot")

    def set_leg_geometry(self, abad, hip, knee, knee_y):
        """Link lengths (m) for the leg kernels, the controller's estimators and the plant; read at every launch."""
        self._check(self.lib.qmpc_set_leg_geometry(self.h, abad, hip, knee, knee_y), "qmpc_set_leg_geometry")

    def set_model(self, model):
        """0 = the dense path's zero-order-hold model, 1 = SparseCMPC's (QMPC_MODEL_SPARSE)."""
        self._check(self.lib.qmpc_set_model(self.h, int(model)), "qmpc_set_model")

    def settings_jcqp(self, use_jcqp, max_iter=10000, rho=1e-7, sigma=1e-8, alpha=1.5, terminate=0.1):
        """The reference's JCQP/ADMM alternate (update_solver_settings' use_jcqp = 1 / 2); 0 = exact solve.
        Defaults are the caller's settings (ConvexMPCLocomotion.cpp:644-648)."""
        self._check(self.lib.qmpc_settings_jcqp(self.h, int(use_jcqp), int(max_iter), rho, sigma, alpha, terminate),
                    "qmpc_settings_jcqp")

    def warm_start(self, batch=None, shift_steps=1):
        """Enable warm starting across MPC cycles; returns the [batch, 64] int32 working-set tensor
        (all -1 = cold).  warm_start(None) switches it off."""
        if batch is None:
            self._check(self.lib.qmpc_set_warm_start(self.h, None, 1), "qmpc_set_warm_start")
            self._ws = None
            return None
        t = self.torch
        ws = t.full((batch, 64), -1, dtype=t.int32, device=self.device)
        self._check(self.lib.qmpc_set_warm_start(self.h, ws.data_ptr(), int(shift_steps)), "qmpc_set_warm_start")
        self._ws = ws
        return ws

    def warm_start_min_iters(self, n):
        """Selective warm start: only robots with at least n iterations in the previous call start warm (0: all)."""
        self._check(self.lib.qmpc_set_warm_start_min_iters(self.h, int(n)), "qmpc_set_warm_start_min_iters")

    def set_max_stance(self, max_stance_footsteps):
        """Caller's bound on stance foot-steps per robot (0 = unknown)."""
        self._check(self.lib.qmpc_set_max_stance(self.h, int(max_stance_footsteps)), "qmpc_set_max_stance")

    def set_min_stance(self, min_stance_footsteps):
        """Caller's lower bound on stance foot-steps per robot (0 = unknown)."""
        self._check(self.lib.qmpc_set_min_stance(self.h, int(min_stance_footsteps)), "qmpc_set_min_stance")

    def settings(self, max_iter=1000, tol=1e-9):
        self._check(self.lib.qmpc_settings(self.h, max_iter, tol), "qmpc_settings")

    # ---- device-resident path -------------------------------------------
    def upload(self, b):
        """numpy batch dict (workloads layout) -> dict of device tensors."""
        d = {k: self.torch.from_numpy(a).to(self.device) for k, a in _host_record(b).items()}
        d["batch"] = int(b["batch"])
        return d

    def alloc_outputs(self, batch, full=False, iters=True):
        t = self.torch
        o = {"grf": t.empty((batch, 12), dtype=t.float32, device=self.device),
             "status": t.empty((batch,), dtype=t.int32, device=self.device)}
        o["soln"] = (t.empty((batch, 12 * self.horizon), dtype=t.float64, device=self.device)
                     if full else None)
        o["iters"] = t.empty((batch,), dtype=t.int32, device=self.device) if iters else None
        return o

    def make_args(self, d, o):
        """Pack ctypes argument structs once (for launch-only timing loops)."""
        inp = make_inputs(d, d["batch"])
        out = Outputs(o["grf"].data_ptr(),
                      o["soln"].data_ptr() if o["soln"] is not None else None,
                      o["status"].data_ptr(),
                      o["iters"].data_ptr() if o["iters"] is not None else None)
        return inp, out

    def solve_async(self, batch, inp, out, stream=None):
        """Enqueue one batched solve on `stream` (torch current stream by default)."""
        self._check(self.lib.qmpc_solve(self.h, batch, C.byref(inp), C.byref(out), self._stream_ptr(stream)), "qmpc_solve")

    def solve(self, b, full=False):
        """Convenience: numpy batch dict in, numpy results out (device path)."""
        d = self.upload(b)
        o = self.alloc_outputs(d["batch"], full=full)
        inp, out = self.make_args(d, o)
        self.solve_async(d["batch"], inp, out)
        self.torch.cuda.synchronize(self.device)
        res = {"grf": o["grf"].cpu().numpy(), "status": o["status"].cpu().numpy(),
               "iters": o["iters"].cpu().numpy()}
        if full:
            res["soln"] = o["soln"].cpu().numpy()
        return res

    # ---- caller side on the GPU (ConvexMPCLocomotion.cpp:498-640, :672-680) --
    def upload_command(self, cmd):
        """numpy command dict (workloads.make_commands layout) -> device tensors."""
        t = self.torch
        d = {}
        for k in CMD_F32 + CMD_STATE:
            d[k] = None if cmd.get(k) is None else t.from_numpy(np.ascontiguousarray(cmd[k], np.float32)).to(self.device)
        for k in CMD_I32:
            d[k] = None if cmd.get(k) is None else t.from_numpy(np.ascontiguousarray(cmd[k], np.int32)).to(self.device)
        d["body_height"] = float(cmd["body_height"])
        d["omni_mode"] = int(cmd["omni_mode"])
        d["batch"] = int(cmd["batch"])
        return d

    def alloc_record(self, batch):
        """Device arrays of the update_data_t record for `batch` robots."""
        t, h = self.torch, self.horizon
        f = lambda *shape: t.empty(shape, dtype=t.float32, device=self.device)
        return {"p": f(batch, 3), "v": f(batch, 3), "q": f(batch, 4), "w": f(batch, 3), "r": f(batch, 12),
                "yaw": f(batch), "traj": f(batch, 12 * h),
                "gait": t.empty((batch, 4 * h), dtype=t.uint8, device=self.device),
                "x_drag": f(batch), "weights": f(batch, 12), "alpha": f(batch), "batch": batch}

    def pack_async(self, dcmd, rec, stream=None):
        """Enqueue the record build (qmpc_pack) for the uploaded command."""
        cs = self.make_command_args(dcmd)
        rs = Record(*(rec[k].data_ptr() for k in REC_FIELDS))
        self._check(self.lib.qmpc_pack(self.h, dcmd["batch"], C.byref(cs), C.byref(rs), self._stream_ptr(stream)),
                    "qmpc_pack")

    def make_command_args(self, dcmd):
        """Command struct over the uploaded command (upload_command)."""
        cs = Command(*(None if dcmd[k] is None else dcmd[k].data_ptr() for k in CMD_F32 + CMD_I32 + CMD_STATE))
        cs.body_height = dcmd["body_height"]
        cs.omni_mode = dcmd["omni_mode"]
        return cs

    def solve_commands_async(self, batch, cs, out, f_ff=None, stream=None):
        """One fused launch: command -> (record in registers) -> solve -> grf (+ body-frame forces)."""
        self._check(self.lib.qmpc_solve_commands(self.h, batch, C.byref(cs), C.byref(out),
                                                 None if f_ff is None else f_ff.data_ptr(), self._stream_ptr(stream)),
                    "qmpc_solve_commands")

    def forces_to_body_async(self, batch, r_body, grf, f_ff, stream=None):
        self._check(self.lib.qmpc_forces_to_body(self.h, batch, r_body.data_ptr(), grf.data_ptr(), f_ff.data_ptr(),
                                                 self._stream_ptr(stream)), "qmpc_forces_to_body")

    # ---- host-pointer path (what the single-robot shim uses) -------------
    def solve_host(self, b, full=False):
        B = int(b["batch"])
        rec = _host_record(b)
        res, out = _host_outputs(B, self.horizon, full)
        self._check(self.lib.qmpc_solve_host(self.h, B, C.byref(make_inputs(rec, B)), C.byref(out)), "qmpc_solve_host")
        return res

    # ---- per-tick glue either side of the solve ---------------------------
    def _dev32(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

    def _stream_ptr(self, stream):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        return C.c_void_p(s.cuda_stream)

    def leg_kinematics(self, q, qd, stream=None):
        """LegController::updateData on device tensors q, qd [B,12] -> J [B,4,9], p [B,12], v [B,12]."""
        t = self.torch
        B = q.shape[0]
        J = t.empty((B, 4, 9), dtype=t.float32, device=self.device)
        p = t.empty((B, 12), dtype=t.float32, device=self.device)
        v = t.empty((B, 12), dtype=t.float32, device=self.device)
        self._check(self.lib.qmpc_leg_kinematics(self.h, B, q.data_ptr(), qd.data_ptr(), J.data_ptr(), p.data_ptr(),
                                                 v.data_ptr(), self._stream_ptr(stream)), "qmpc_leg_kinematics")
        return J, p, v

    def leg_torques(self, c, stream=None):
        """LegController::updateCommand: dict of device tensors (LEG_F32 keys; tau_ff / force_ff may be
        None) + kp_joint, kd_joint -> tau [B,12], q_des [B,12]."""
        t = self.torch
        B = c["q"].shape[0]
        lc = LegCommand()
        for k in LEG_F32:
            setattr(lc, k, None if c.get(k) is None else c[k].data_ptr())
        lc.kp_joint, lc.kd_joint = float(c["kp_joint"]), float(c["kd_joint"])
        tau = t.empty((B, 12), dtype=t.float32, device=self.device)
        qdes = t.empty((B, 12), dtype=t.float32, device=self.device)
        self._check(self.lib.qmpc_leg_torques(self.h, B, C.byref(lc), tau.data_ptr(), qdes.data_ptr(),
                                              self._stream_ptr(stream)), "qmpc_leg_torques")
        return tau, qdes

    def kf_init(self, batch, stream=None):
        """LinearKFPositionVelocityEstimator::setup -> (xhat [B,18], P [B,324]) device tensors."""
        t = self.torch
        xhat = t.empty((batch, 18), dtype=t.float32, device=self.device)
        P = t.empty((batch, 324), dtype=t.float32, device=self.device)
        self._check(self.lib.qmpc_kf_init(self.h, batch, xhat.data_ptr(), P.data_ptr(), self._stream_ptr(stream)), "qmpc_kf_init")
        return xhat, P

    def kf_step(self, xhat, P, r_body, a_world, omega_body, contact_phase, leg_p, leg_v, stream=None):
        """LinearKFPositionVelocityEstimator::run on device tensors; xhat, P are updated in place.
        Returns (position, v_world, v_body) [B,3]."""
        t = self.torch
        B = xhat.shape[0]
        pos, vw, vb = (t.empty((B, 3), dtype=t.float32, device=self.device) for _ in range(3))
        st = KfState(xhat.data_ptr(), P.data_ptr(), r_body.data_ptr(), a_world.data_ptr(), omega_body.data_ptr(),
                     contact_phase.data_ptr(), leg_p.data_ptr(), leg_v.data_ptr(), pos.data_ptr(), vw.data_ptr(), vb.data_ptr())
        self._check(self.lib.qmpc_kf_step(self.h, B, C.byref(st), self._stream_ptr(stream)), "qmpc_kf_step")
        return pos, vw, vb

    def swing_trajectory(self, p0, pf, height, phase, swing_time, stream=None):
        """computeSwingTrajectoryBezier for n feet: device tensors [n,3], [n,3], [n], [n], [n] -> p, v, a."""
        t = self.torch
        n = p0.shape[0]
        p, v, a = (t.empty((n, 3), dtype=t.float32, device=self.device) for _ in range(3))
        self._check(self.lib.qmpc_swing_trajectory(self.h, n, p0.data_ptr(), pf.data_ptr(), height.data_ptr(),
                                                   phase.data_ptr(), swing_time.data_ptr(), p.data_ptr(), v.data_ptr(),
                                                   a.data_ptr(), self._stream_ptr(stream)), "qmpc_swing_trajectory")
        return p, v, a

    @staticmethod
    def solve_sharded(solvers, b, full=False):
        """qmpc_solve_sharded: ONE host thread drives several handles (one per device in
        production; several may share a device): contiguous shards of the host batch `b`, all
        devices busy at once, results collected into one set of host arrays."""
        first = solvers[0]
        B = int(b["batch"])
        rec = _host_record(b)
        res, out = _host_outputs(B, first.horizon, full)
        hs = (C.c_void_p * len(solvers))(*[m.h for m in solvers])
        rc = first.lib.qmpc_solve_sharded(hs, len(solvers), B, C.byref(make_inputs(rec, B)), C.byref(out))
        if rc != QMPC_OK:
            raise QmpcError(f"qmpc_solve_sharded failed rc={rc}: " +
                            "; ".join(m.lib.qmpc_last_error(m.h).decode() for m in solvers))
        return res

    # ---- test hook ---------------------------------------------------------
    def debug_dump(self, batch):
        """Enable the assembled-QP dump; returns (H_dev, g_dev, ld) tensors."""
        t = self.torch
        ld = self.lib.qmpc_debug_ld(self.h)
        H = t.zeros((batch, ld, ld), dtype=t.float64, device=self.device)
        g = t.zeros((batch, ld), dtype=t.float64, device=self.device)
        self._check(self.lib.qmpc_set_debug(self.h, H.data_ptr(), g.data_ptr()), "qmpc_set_debug")
        self._dbg = (H, g)
        return H, g, ld

    def debug_aux(self, batch):
        """Enable the dump of the kernel's float transcendentals; returns the [batch,8] tensor
        (cos yaw, sin yaw, roll, pitch, yaw)."""
        t = self.torch
        aux = t.zeros((batch, 8), dtype=t.float64, device=self.device)
        self._check(self.lib.qmpc_set_debug_aux(self.h, aux.data_ptr()), "qmpc_set_debug_aux")
        self._dbg_aux = aux
        return aux

    def debug_overflow_slices(self, n):
        """Test hook: use only n slices of the overflow event pool (negative: all)."""
        self._check(self.lib.qmpc_set_debug_overflow_slices(self.h, int(n)), "qmpc_set_debug_overflow_slices")

    def debug_overflow_spin(self, probes):
        """Test hook: probes for a free overflow slice before a robot falls back (negative: default)."""
        self._check(self.lib.qmpc_set_debug_overflow_spin(self.h, int(probes)), "qmpc_set_debug_overflow_spin")

    def set_split(self, mode):
        """Decoupled sweep / engine kernels for the 128- and 192-row classes: 0 / False off, 1 automatic by batch
        size (default), 2 / True always."""
        mode = 2 if mode is True else (0 if mode is False else int(mode))
        self._check(self.lib.qmpc_set_split(self.h, mode), "qmpc_set_split")

    def set_dense(self, mode):
        """0 / 1 / 2: the 64-row class's five-workgroups-per-CU instantiation never / automatic (handles of 2048+ robots; see
        include/qmpc.h) / whenever that class is the whole chain."""
        self._check(self.lib.qmpc_set_dense(self.h, int(mode)), "qmpc_set_dense")

    def debug_keys(self, b):
        """The scheduling keys of DESIGN 13 as the kernels evaluate them: (stance foot-steps, score, demand) per robot (numpy)."""
        t = self.torch
        d = self.upload(b)
        B = d["batch"]
        o = self.alloc_outputs(B)
        inp, _ = self.make_args(d, o)
        nst = t.empty((B,), dtype=t.int32, device=self.device)
        score = t.empty((B,), dtype=t.float32, device=self.device)
        demand = t.empty((B,), dtype=t.float32, device=self.device)
        self._check(self.lib.qmpc_debug_keys(self.h, B, C.byref(inp), nst.data_ptr(), score.data_ptr(), demand.data_ptr(),
                                             self._stream_ptr(None)), "qmpc_debug_keys")
        t.cuda.synchronize(self.device)
        return nst.cpu().numpy(), score.cpu().numpy(), demand.cpu().numpy()

    def set_size_order(self, on):
        """0 / 1: without a usable order hint, multi-round launches take the robots in blockIdx order / the robots that fit
        the first class largest first by their contact tables (default; include/qmpc_expert.h)."""
        self._check(self.lib.qmpc_set_size_order(self.h, int(bool(on))), "qmpc_set_size_order")

    def set_order_hint(self, mode):
        """0 / 1: multi-round launches take the robots in blockIdx order / hardest first by the previous call's
        iteration counts (default; include/qmpc.h)."""
        self._check(self.lib.qmpc_set_order_hint(self.h, int(mode)), "qmpc_set_order_hint")

    def set_debug_balance(self, mode):
        self._check(self.lib.qmpc_set_debug_balance(self.h, int(mode)), "qmpc_set_debug_balance")

    def set_chunks(self, n):
        self._check(self.lib.qmpc_set_chunks(self.h, int(n)), "qmpc_set_chunks")

    def set_debug_engine_events(self, n):
        self._check(self.lib.qmpc_set_debug_engine_events(self.h, int(n)), "qmpc_set_debug_engine_events")

    def reserve(self):
        self._check(self.lib.qmpc_reserve(self.h), "qmpc_reserve")

    def debug_read_item(self, which, item):
        """Test hook: (H^-1 [ld, ld], x_u [ld], (rid, n, nst, status)) of a work item of the decoupled path after a solve."""
        ld = (128, 192, 448)[which]
        hinv = np.zeros((ld, ld), np.float64)
        xu = np.zeros(ld, np.float64)
        hdr = np.zeros(4, np.int32)
        self._check(self.lib.qmpc_debug_read_item(self.h, int(which), int(item), hinv.ctypes.data_as(C.c_void_p),
                                                  xu.ctypes.data_as(C.c_void_p), hdr.ctypes.data_as(C.c_void_p)),
                    "qmpc_debug_read_item")
        return hinv, xu, hdr

    def debug_read_counts(self):
        """Test hook: the handle's three per-call counter sets as an int32 [3, 256] array (layout: csrc/qmpc_device.h;
        sets 0 / 1 alternate between consecutive calls, set 2 serves calls captured into a graph).  Synchronises."""
        buf = np.zeros((3, 256), np.int32)
        self._check(self.lib.qmpc_debug_read_counts(self.h, buf.ctypes.data_as(C.c_void_p)), "qmpc_debug_read_counts")
        return buf

    def set_debug_pool_busy(self, on):
        self._check(self.lib.qmpc_set_debug_pool_busy(self.h, int(bool(on))), "qmpc_set_debug_pool_busy")

    def debug_clock(self, batch):
        """Enable per-phase shader-clock stamps; returns the [batch,16] tensor."""
        t = self.torch
        clk = t.zeros((batch, 16), dtype=t.int64, device=self.device)
        self._check(self.lib.qmpc_set_debug_clock(self.h, clk.data_ptr()), "qmpc_set_debug_clock")
        self._clk = clk
        return clk

    def debug_off(self):
        self.lib.qmpc_set_debug_clock(self.h, None)
        self.lib.qmpc_set_debug(self.h, None, None)
        self.lib.qmpc_set_debug_aux(self.h, None)
        self._dbg = None
        self._dbg_aux = None


class BatchedController:
    """GaitCtrller::TorqueCalculator for `batch` robots on one GPU (include/qmpc_ctrl.h); the MPC in lockstep by
    default, per robot after set_schedule("per_robot"); robot mode 0 by default, 1 after set_robot_mode(1).

    The reference's single-robot calls map one to one: init_controller -> init(), set_gait_type -> set_gait(),
    set_robot_vel -> set_vel(), pre_work -> prework(), torque_calculator -> tick(); reset() re-initialises chosen
    robots (RL episode ends); prework_state() / tick_state() take a simulator's ground truth (state [B,16] float64,
    CheaterState's member order) in place of imu and skip the filter.  Arguments are torch tensors on the controller's
    device: imu [B,10] and motor [B,24] float64 in the reference's layouts, gait [B] int32, vel [B,3] float64, mask [B] bool / uint8.  Every call only
    enqueues work on the current stream (or `stream`); view() and read() synchronise.  Owns its BatchedConvexMPC
    (`self.mpc`), whose handle holds the controller state."""

    def __init__(self, device=0, max_batch=4096):
        self.mpc = BatchedConvexMPC(device, max_batch=max_batch, max_horizon=16)
        self.torch, self.lib, self.device = self.mpc.torch, self.mpc.lib, self.mpc.device
        self.batch = None

    def close(self):
        self.mpc.close()

    def _s(self, stream):
        return self.mpc._stream_ptr(stream)

    def _chk(self, t, shape, dtype, what):
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise QmpcError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}")
        return t.data_ptr()

    # ---- what the controller, its plant and its sensors (one handle) all do around a C call ----
    def _call(self, name, *args):
        """The C function `name` on the handle, checked."""
        self.mpc._check(getattr(self.lib, name)(self.mpc.h, *args), name)

    def _mask(self, mask):
        """A [B] bool / uint8 mask -> (its uint8 copy, which the caller keeps alive until its next call: the launch reads
        it asynchronously; the copy's pointer).  None -> (None, None)."""
        if mask is None:
            return None, None
        m = mask.to(self.torch.uint8).contiguous()
        return m, self._chk(m, (self.batch,), self.torch.uint8, "mask")

    def _bind(self, name, batch, struct, fields, given):
        """`name`(handle, batch, &struct) over the float64 tensors in `given` (fields: member -> elements per robot;
        None: the member stays null) -> the tensors bound, for the caller to keep referenced."""
        if batch is None:
            raise QmpcError(f"{name} before init()")
        prm = struct()
        for k, per_robot in fields.items():
            if given[k] is not None:
                shape = (batch,) if per_robot == 1 else (batch, per_robot)
                setattr(prm, k, self._chk(given[k], shape, self.torch.float64, k))
        self._call(name, batch, C.byref(prm))
        return {k: t for k, t in given.items() if t is not None}

    def _views(self, name, struct, fields, scalars):
        """`name`(handle, &struct) as a dict: zero-copy device tensors over the struct's pointers (fields: member ->
        (elements per robot, or None for [B]; typestr)) that keep this controller alive, then the members in `scalars`."""
        v = struct()
        self._call(name, C.byref(v))
        res = {k: self.torch.as_tensor(_DeviceArray(getattr(v, k), (v.batch,) if n is None else (v.batch, n), ts, self),
                                       device=self.device) for k, (n, ts) in fields.items()}
        res.update((k, getattr(v, k)) for k in scalars)
        return res

    def init(self, batch, freq=500.0, pid=(0.0, 0.0, 0.0, 0.0), stream=None):
        """GaitCtrller(freq, PIDParam) for robots 0 .. batch-1; pid[2], pid[3] are the joint PD gains."""
        pid_c = (C.c_double * 4)(*[float(x) for x in pid])
        self._call("qmpc_ctrl_init", int(batch), float(freq), pid_c, self._s(stream))
        self.batch = int(batch)
        self.mpc.horizon = 14
        self.schedule = "lockstep"

    def set_schedule(self, mode):
        """"lockstep" (the default after every init()) or "per_robot": each robot's own counter decides when it solves, and
        reset() is init_controller exactly (counter 0).  Only between init() and the first tick() or reset()."""
        if mode not in CTRL_SCHEDULES:
            raise QmpcError(f"set_schedule: unknown mode {mode!r} (one of {sorted(CTRL_SCHEDULES)})")
        self._call("qmpc_ctrl_set_schedule", CTRL_SCHEDULES[mode])
        self.schedule = mode

    def set_robot_mode(self, mode):
        """set_robot_mode for the whole controller: 0 (the default after every init(): the gait picked by number, MPC
        horizon 14) or 1 (the speed-adaptive `aio` gait, 10 .. 16 segments per robot, MPC horizon 10).  Mode 1 needs
        set_schedule("per_robot") first.  Only between init() and the first tick() or reset(); prework() may come first."""
        self._call("qmpc_ctrl_set_robot_mode", int(mode))
        self.mpc.horizon = 10 if int(mode) == 1 else 14

    def reset(self, mask, stream=None):
        """Re-initialise the robots where mask is set; their iteration counter restarts at T mod 13 in lockstep, at 0
        with the per-robot schedule."""
        self._keep, ptr = self._mask(mask)
        self._call("qmpc_ctrl_reset", self.batch or 0, ptr, self._s(stream))

    def set_gait(self, gait, stream=None):
        """set_gait_type: gait numbers 0 .. 11, +20 for omni mode."""
        ptr = self._chk(gait, (self.batch,), self.torch.int32, "gait")
        self._call("qmpc_ctrl_set_gait", self.batch, ptr, self._s(stream))

    def set_vel(self, vel, stream=None):
        """set_robot_vel: [B,3] float64 (x, y, yaw rate), dead band 0.03."""
        ptr = self._chk(vel, (self.batch, 3), self.torch.float64, "vel")
        self._call("qmpc_ctrl_set_vel", self.batch, ptr, self._s(stream))

    def _tick(self, name, what, width, first, motor, effort, stream, tick=True):
        """prework / tick and their _state pair: `first` is imu [B,10] or state [B,16] (`what`, `width`)."""
        if tick and self.batch is None:
            raise QmpcError(f"{name} before init()")
        args = [self._chk(first, (self.batch, width), self.torch.float64, what),
                self._chk(motor, (self.batch, 24), self.torch.float64, "motor")]
        if tick:
            if effort is None:
                effort = self.torch.empty((self.batch, 12), dtype=self.torch.float64, device=self.device)
            args.append(self._chk(effort, (self.batch, 12), self.torch.float64, "effort"))
        self._call(name, self.batch, *args, self._s(stream))
        return effort

    def prework(self, imu, motor, stream=None):
        """pre_work: the estimators and the leg data, no control."""
        self._tick("qmpc_ctrl_prework", "imu", 10, imu, motor, None, stream, tick=False)

    def tick(self, imu, motor, effort=None, stream=None):
        """torque_calculator for every robot -> effort [B,12] float64 (zeros for a latched robot)."""
        return self._tick("qmpc_ctrl_tick", "imu", 10, imu, motor, effort, stream)

    def prework_state(self, state, motor, stream=None):
        """pre_work from simulator ground truth: state [B,16] float64 in CheaterState's member order (orientation w x y z,
        position, omegaBody, vBody, acceleration) through the cheater estimators -- no Kalman filter -- and the leg data."""
        self._tick("qmpc_ctrl_prework_state", "state", 16, state, motor, None, stream, tick=False)

    def tick_state(self, state, motor, effort=None, stream=None):
        """tick() with prework_state() as its pre_work: the same control tick, driven by the true body state.  The filter
        and the orientation estimator's first-visit state stay where they were; ticks of the two kinds may alternate, but
        only a run of one kind is a state the reference can reach."""
        return self._tick("qmpc_ctrl_tick_state", "state", 16, state, motor, effort, stream)

    def read(self, name):
        """One array of the controller's device state (qmpc_debug_ctrl_read) -> numpy [B, n] (float32 or int32)."""
        per = C.c_int(0)
        self.lib.qmpc_debug_ctrl_read(self.mpc.h, name.encode(), np.zeros(1, np.float32).ctypes.data, 0, C.byref(per))
        if per.value == 0:
            raise QmpcError(f"qmpc_debug_ctrl_read: no controller array {name!r} (or no init())")
        out = np.zeros((self.batch, per.value), np.float32)
        self.mpc._check(self.lib.qmpc_debug_ctrl_read(self.mpc.h, name.encode(), out.ctypes.data, out.nbytes, C.byref(per)),
                        f"qmpc_debug_ctrl_read({name})")
        if name in CTRL_INT_ARRAYS:
            out = out.view(np.int32)
        return out

    def view(self):
        """qmpc_ctrl_view_get as zero-copy torch device tensors ([B, n]; safe / counter int32) that ALIAS the controller's
        state: no copy, no synchronisation; they show what the last enqueued work left once the stream has reached it,
        and are valid until close() or the next init().  Read-only by contract.  Plus batch and ticks (T: the ticks
        enqueued since init, captured ones included)."""
        fields = {k: (n, "<i4" if k in ("safe", "counter") else "<f4") for k, n in CTRL_VIEW_WIDTH.items()}
        return self._views("qmpc_ctrl_view_get", CtrlView, fields, ("batch", "ticks"))

    def fleet_info(self):
        """qmpc_fleet_run_info: how the ticks of rollout(..., fused=True) were served since init() -> dict(ticks,
        fused_ticks, fused_launches, fallback_ticks, reason); reason is 0 when the last call ran fused, otherwise the OR
        of the FLEET_REASONS bits that made it fall back to the per-tick launches.  Host-side counts: no synchronisation."""
        info = FleetInfo()
        self._call("qmpc_fleet_run_info", C.byref(info))
        return {n: int(getattr(info, n)) for n in FLEET_INFO_FIELDS}

    def loop_info(self):
        """qmpc_loop_run_info (include/qmpc_loop.h) as a dict: how rollout_loop()'s ticks were served since init() -- ticks,
        fused_ticks, fused_launches, fallback_ticks -- and the last call's reason: 0 when it ran fused, else the sum of the
        LOOP_REASONS bits that made it fall back to the per-tick launches.  Host-side counts: no synchronisation."""
        info = LoopInfo()
        self._call("qmpc_loop_run_info", C.byref(info))
        return {n: int(getattr(info, n)) for n in LOOP_INFO_FIELDS}

    def set_ground_run(self, on=True):
        """qmpc_ground_run_enable (include/qmpc_ground_run.h): with the switch on, rollout(..., fused=True) and
        rollout_loop() serve a plant on terrain rows and / or a height field (scheduled contact) through the fused launch
        too, with the per-tick bits; off (the default after init()) they fall back there.  Read by the next call; a
        captured graph keeps what it captured.  fleet_info() / loop_info() tell how the ticks were served."""
        self._call("qmpc_ground_run_enable", 1 if on else 0)

    @property
    def ground_run(self):
        """qmpc_ground_run_enabled: whether the next run call serves terrain rows and height fields fused."""
        on = C.c_int(0)
        self._call("qmpc_ground_run_enabled", C.byref(on))
        return bool(on.value)


class _DeviceArray:
    """__cuda_array_interface__ over a device pointer of the controller; keeps its owner alive while a tensor uses it."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2}
        self.owner = owner


class BatchedPlant:
    """The reduced-order plant of include/qmpc_plant.h for a BatchedController's robots: the MPC's single rigid body
    with massless legs, scheduled contact, no slip, flat ground -- fp64 on the device.  step(effort) consumes what
    ctrl.tick_state() produced (and reads the controller's contact_state / p_des / v_des) and returns the next
    (state [B,16], motor [B,24]); tick_state -> step is a closed loop without the host (see rollout()).

    Constructed FROM a controller (the plant lives in the controller's handle and is freed with it), after ctrl.init().
    Every call only enqueues on the current stream (or `stream`).  `state` / `motor` are the plant's own read-out rows
    (zero-copy, rewritten by init / reset / step): feed them to ctrl.tick_state directly."""

    def __init__(self, ctrl):
        self.ctrl, self.torch, self.lib, self.device = ctrl, ctrl.torch, ctrl.lib, ctrl.device
        self.batch = None
        self._params = {}
        self._terrain = None
        self._field = None

    def _xyyaw(self, xyyaw):
        if xyyaw is None:
            return None
        return self.ctrl._chk(xyyaw, (self.ctrl.batch, 3), self.torch.float64, "init_xyyaw")

    def init(self, mu_plant=0.4, substeps=1, init_xyyaw=None, stream=None):
        """All robots of the controller into the initial state: body at (x, y, 0.29) with yaw from init_xyyaw [B,3]
        float64 (zeros without), at rest, four feet under the hips on the ground, in stance."""
        self.ctrl._call("qmpc_plant_init", self.ctrl.batch or 0, float(mu_plant), int(substeps), self._xyyaw(init_xyyaw),
                        self.ctrl._s(stream))
        self.batch = self.ctrl.batch
        self._keep = init_xyyaw
        self._params = {}     # (qmpc_plant_init unbinds: a new plant is the plain plant)
        self._terrain = None  # (... on flat ground)
        self._field = None    # (... with no height field)
        v = self.view()
        self.state, self.motor = v["state"], v["motor"]
        self.effort = self.torch.zeros((self.batch, 12), dtype=self.torch.float64, device=self.device)

    def reset(self, mask, init_xyyaw=None, stream=None):
        """The initial state again for the robots where mask is set; the others keep every bit."""
        m, ptr = self.ctrl._mask(mask)
        self.ctrl._call("qmpc_plant_reset", self.ctrl.batch or 0, ptr, self._xyyaw(init_xyyaw), self.ctrl._s(stream))
        self._keep = (m, init_xyyaw)   # (alive until the next call: the launch reads them asynchronously)

    def step(self, effort, state=None, motor=None, stream=None):
        """One control period -> (state, motor); written into the tensors given, or into the plant's own rows."""
        if self.batch is None:
            raise QmpcError("qmpc_plant_step before init()")
        state = self.state if state is None else state
        motor = self.motor if motor is None else motor
        e = self.ctrl._chk(effort, (self.batch, 12), self.torch.float64, "effort")
        a = self.ctrl._chk(state, (self.batch, 16), self.torch.float64, "state")
        b = self.ctrl._chk(motor, (self.batch, 24), self.torch.float64, "motor")
        self.ctrl._call("qmpc_plant_step", self.batch, e, a, b, self.ctrl._s(stream))
        return state, motor

    def view(self):
        """qmpc_plant_view_get as zero-copy device tensors (p, v, q, omega, foot, stance, grf, state, motor: [B, n],
        float64, stance int32) that alias the plant's state, like BatchedController.view(); plus batch, substeps,
        mu_plant.  Read-only by contract."""
        return self.ctrl._views("qmpc_plant_view_get", PlantView, PLANT_VIEW_FIELDS, ("batch", "substeps", "mu_plant"))

    # -- include/qmpc_plant_vary.h -------------------------------------------------------------------------------------
    def set_params(self, mass=None, ibody=None, mu=None, force=None, torque=None):
        """Per-robot body, floor and pushes of the PLANT (the controller is not told): float64 device tensors mass [B],
        ibody [B,3], mu [B], force [B,3] (world frame, N, on the body origin), torque [B,3] (body frame, N m); None keeps
        the handle's value / none.  The plant reads the tensors at every later step -- write into them in place (on the
        stream) to change a push, also between replays of a captured graph; they are kept referenced here.  All None
        unbinds; init() unbinds, reset() does not."""
        self._params = self.ctrl._bind("qmpc_plant_set_params", self.batch, PlantParams, PLANT_PARAM_FIELDS,
                                       dict(mass=mass, ibody=ibody, mu=mu, force=force, torque=torque))

    def enable_stats(self, on=True):
        """Per-robot statistics on the device, updated by every step while on (see stats()).  The first enable
        allocates and synchronises, once."""
        self.ctrl._call("qmpc_plant_stats_enable", 1 if on else 0)

    def reset_stats(self, mask=None, stream=None):
        """The initial values (n 0, z_min +inf, z_max -inf, the rest 0) for the robots where mask is set; None: all."""
        self._keep, ptr = self.ctrl._mask(mask)
        self.ctrl._call("qmpc_plant_stats_reset", self.ctrl.batch or 0, ptr, self.ctrl._s(stream))

    def stats(self):
        """qmpc_plant_stats_get as zero-copy device tensors [B] that alias the accumulators, like view(): n (int32),
        z_min, z_max, roll_max, pitch_max, vx_sum, vy_sum (float64); plus batch, enabled.  A window's mean velocity is
        the difference of two (copied) reads of a sum over the difference of n.  Read-only by contract."""
        res = self.ctrl._views("qmpc_plant_stats_get", PlantStats, {k: (None, ts) for k, ts in PLANT_STATS_FIELDS.items()},
                               ("batch", "enabled"))
        res["enabled"] = bool(res["enabled"])
        return res


    # -- include/qmpc_terrain.h ----------------------------------------------------------------------------------------
    def set_terrain(self, rows, clamp_swing=False, rebase_z=False):
        """Per-robot slopes and stairs under the PLANT (the controller is not told): rows is a float64 device tensor
        [B, 8] of (z0, gx, gy, rise, run, count, s0, psi) -- height(x, y) = z0 + gx x + gy y + rise k with k the tread
        index along heading psi from abscissa s0 -- or None to unbind (flat ground).  The plant reads the tensor at every
        later step and reset -- write into it in place (on the stream) to change the ground, also between replays of a
        captured graph; it is kept referenced here.  clamp_swing lifts a swing foot commanded below the surface onto
        it; rebase_z makes column 6 of the state row the height above the stance feet.  init() unbinds, reset() does
        not and places the robots on the terrain: init() -> set_terrain() -> reset(all)."""
        if self.batch is None:
            raise QmpcError("qmpc_plant_set_terrain before init()")
        ptr = None if rows is None else self.ctrl._chk(rows, (self.batch, 8), self.torch.float64, "rows")
        flags = (TERRAIN_CLAMP_SWING if clamp_swing else 0) | (TERRAIN_REBASE_Z if rebase_z else 0)
        self.ctrl._call("qmpc_plant_set_terrain", self.batch, ptr, flags)
        self._terrain = rows

    def terrain(self):
        """qmpc_terrain_view_get as zero-copy device tensors [B] that alias the plant's arrays, like view(): ground (the
        height under the body origin at the last pose on terrain), support (the mean height of the stance feet); plus
        flags, batch and bound.  Read-only by contract."""
        res = self.ctrl._views("qmpc_terrain_view_get", TerrainView, dict(ground=(None, "<f8"), support=(None, "<f8")),
                               ("terrain", "flags", "batch"))
        res["bound"] = bool(res.pop("terrain"))
        return res

    # -- include/qmpc_contact.h ----------------------------------------------------------------------------------------
    def set_contact(self, early=False, late=False, slip=False, drop_speed=1.0, slip_gain=0.01, slip_vmax=1.0):
        """Contact decided by the ground under the PLANT (the controller is not told), with or without terrain bound:
        `early` pins a swing foot that meets the surface, `late` leaves a foot scheduled to stand in the air until it
        lands (lowered at drop_speed m/s), `slip` lets a foot whose force leaves the friction cone slide at slip_gain m/s
        per newton of excess, capped at slip_vmax.  The defaults are modelling choices, not measurements.  Host state
        only; all three False, or set_contact(None), switches it off.  init() switches it off, reset() keeps it and
        zeroes the masked robots' counters.  With contact on the plant view's `stance` is the physical pinned flag."""
        if self.batch is None:
            raise QmpcError("qmpc_plant_set_contact before init()")
        if early is None:
            self.ctrl._call("qmpc_plant_set_contact", self.batch, None)
            return
        flags = (CONTACT_EARLY if early else 0) | (CONTACT_LATE if late else 0) | (CONTACT_SLIP if slip else 0)
        prm = ContactParams(flags, float(drop_speed), float(slip_gain), float(slip_vmax))
        self.ctrl._call("qmpc_plant_set_contact", self.batch, C.byref(prm))

    def contact(self):
        """qmpc_contact_view_get as zero-copy device tensors that alias the plant's arrays, like terrain(): early, late
        ([B] int32, foot-ticks), slip ([B] float64, metres), drop ([B, 4] float64); plus flags, drop_speed, slip_gain,
        slip_vmax and batch.  Read-only by contract."""
        res = self.ctrl._views("qmpc_contact_view_get", ContactView,
                               dict(early=(None, "<i4"), late=(None, "<i4"), slip=(None, "<f8"), drop=(4, "<f8")),
                               ("params", "batch"))
        prm = res.pop("params")
        res.update(flags=prm.flags, drop_speed=prm.drop_speed, slip_gain=prm.slip_gain, slip_vmax=prm.slip_vmax)
        return res

    # -- include/qmpc_field.h ------------------------------------------------------------------------------------------
    def set_field(self, z, place=None, cell=None, clamp_swing=False, rebase_z=False):
        """Height-field terrain from memory under the PLANT (the controller is not told), added to the ground of
        set_terrain() where that is bound: z is a contiguous float32 device tensor [M, ny, nx] (a bank of M maps, x
        fastest, `cell` metres between samples), place a float64 device tensor [B, 4] of (map, ox, oy, zs) per robot -- the
        robot stands on map `map`, whose sample (0, 0) lies at world (ox, oy), scaled by zs; heights are bilinear and the
        edge samples extend outward.  The plant reads both tensors at every later step and reset -- write into them in
        place (on the stream) to move a robot or change the ground, also between replays of a captured graph; they are
        kept referenced here.  The flags are set_terrain()'s and are OR-ed with its.  set_field(None) unbinds; init()
        unbinds, reset() does not and places the robots on the surface: init() -> set_field() -> reset(all)."""
        if self.batch is None:
            raise QmpcError("qmpc_plant_set_field before init()")
        if z is None:
            self.ctrl._call("qmpc_plant_set_field", self.batch, None, None, 0)
            self._field = None
            return
        t = self.torch
        if not (isinstance(z, t.Tensor) and z.dim() == 3 and z.dtype == t.float32 and z.is_contiguous()
                and z.device == t.device(self.device)):
            raise QmpcError("z: a contiguous float32 tensor [M, ny, nx] on the plant's device")
        if cell is None:
            raise QmpcError("cell: metres between samples")
        ptr = self.ctrl._chk(place, (self.batch, 4), t.float64, "place")
        bank = FieldBank(z.data_ptr(), int(z.shape[2]), int(z.shape[1]), int(z.shape[0]), float(cell))
        flags = (TERRAIN_CLAMP_SWING if clamp_swing else 0) | (TERRAIN_REBASE_Z if rebase_z else 0)
        self.ctrl._call("qmpc_plant_set_field", self.batch, C.byref(bank), ptr, flags)
        self._field = (z, place)

    def field(self):
        """qmpc_field_view_get: bound, nx, ny, count, cell, flags, batch, and the tensors as bound (z, place; None
        without a field)."""
        v = FieldView()
        self.ctrl._call("qmpc_field_view_get", C.byref(v))
        z, place = self._field if self._field is not None else (None, None)
        return dict(bound=bool(v.bank.z), nx=v.bank.nx, ny=v.bank.ny, count=v.bank.count, cell=v.bank.cell,
                    flags=v.flags, batch=v.batch, z=z, place=place)


class BatchedSensors:
    """The sensor model of include/qmpc_sense.h for a BatchedPlant's robots: sense() turns the plant's last read-out into
    imu [B,10] / motor [B,24] float64 as ctrl.tick() takes them -- exactly (nothing bound) or with per-robot
    accelerometer and gyro bias and white noise on the accelerometer, the gyro and the joint encoders (set_params).
    tick -> plant.step -> sense is a closed loop through the controller's estimators without the host (see
    rollout_sensed()); settle() first, or most of the fleet falls (the Kalman filter starts at height 0).

    Constructed FROM a plant (the sensors live in the same handle), after plant.init().  Every call only enqueues on
    the current stream (or `stream`).  `imu` / `motor` are the sensors' own output tensors, rewritten by sense()."""

    def __init__(self, plant):
        self.plant, self.ctrl = plant, plant.ctrl
        self.torch, self.lib, self.device = plant.torch, plant.lib, plant.device
        self.batch = None
        self._params = {}

    def init(self, seed=0, stream=None):
        """Counters n = 0, epoch = 0 for every robot, the noise stream's 64-bit seed, nothing bound."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.ctrl._call("qmpc_sense_init", self.plant.batch or 0, seed, self.ctrl._s(stream))
        self.batch = self.plant.batch
        self._params = {}
        self.imu = self.torch.zeros((self.batch, 10), dtype=self.torch.float64, device=self.device)
        self.motor = self.torch.zeros((self.batch, 24), dtype=self.torch.float64, device=self.device)

    def set_params(self, acc_bias=None, gyro_bias=None, acc_sigma=None, gyro_sigma=None, q_sigma=None, qd_sigma=None):
        """Per-robot sensor errors: float64 device tensors acc_bias [B,3] (m/s^2, body frame), gyro_bias [B,3] (rad/s),
        acc_sigma, gyro_sigma, q_sigma (rad, all 12 joints), qd_sigma (rad/s) [B]; None: that term is absent.  The
        tensors are read at every later sense() -- write into them in place (on the stream) to change a value, also
        between replays of a captured graph; they are kept referenced here.  All None unbinds; init() unbinds."""
        self._params = self.ctrl._bind("qmpc_sense_set_params", self.batch, SenseParams, SENSE_PARAM_FIELDS,
                                       dict(acc_bias=acc_bias, gyro_bias=gyro_bias, acc_sigma=acc_sigma,
                                            gyro_sigma=gyro_sigma, q_sigma=q_sigma, qd_sigma=qd_sigma))

    def reset(self, mask=None, stream=None):
        """A new noise epoch (epoch += 1, n = 0) for the robots where mask is set; None: all."""
        self._keep, ptr = self.ctrl._mask(mask)
        self.ctrl._call("qmpc_sense_reset", self.batch or 0, ptr, self.ctrl._s(stream))

    def sense(self, imu=None, motor=None, stream=None):
        """One reading of the plant's last read-out -> (imu, motor); written into the tensors given, or into the
        sensors' own."""
        if self.batch is None:
            raise QmpcError("qmpc_sense before init()")
        imu = self.imu if imu is None else imu
        motor = self.motor if motor is None else motor
        a = self.ctrl._chk(imu, (self.batch, 10), self.torch.float64, "imu")
        b = self.ctrl._chk(motor, (self.batch, 24), self.torch.float64, "motor")
        self.ctrl._call("qmpc_sense", self.batch, a, b, self.ctrl._s(stream))
        return imu, motor

    def settle(self, n=50, stream=None):
        """n x (sense -> ctrl.prework) with the plant not stepping: the reference's warm-up (init_controller, pre_work
        ..., then torques), which lets the Kalman filter find the standing body before the first tick."""
        for _ in range(int(n)):
            self.sense(stream=stream)
            self.ctrl.prework(self.imu, self.motor, stream=stream)

    def view(self):
        """qmpc_sense_view_get as zero-copy device tensors n, epoch ([B] int32) that alias the counters, like
        BatchedPlant.view(); plus batch, seed.  Read-only by contract."""
        return self.ctrl._views("qmpc_sense_view_get", SenseView, dict(n=(None, "<i4"), epoch=(None, "<i4")),
                                ("batch", "seed"))


class BatchedActuators:
    """The actuator stage of include/qmpc_act.h for a BatchedPlant's robots: apply() turns the effort the controller
    wrote into the torque the joints receive -- the reference's motor model (gear, torque constant, winding resistance,
    back-EMF against the battery, a motor-side torque cap, damping and dry friction), a per-robot command latency of up
    to max_delay ticks, and per-robot saturation counters and energies (stats()).  tick -> apply -> plant.step is a
    closed loop without the host (the rollout functions' `actuators` argument).

    Constructed FROM a plant (the stage lives in the same handle), after plant.init().  Every call only enqueues on the
    current stream (or `stream`)."""

    def __init__(self, plant):
        self.plant, self.ctrl = plant, plant.ctrl
        self.torch, self.lib, self.device = plant.torch, plant.lib, plant.device
        self.batch = None
        self._params = {}

    @staticmethod
    def default_config():
        """qmpc_act_config_default as a dict: the Mini Cheetah's motor, friction on, max_delay 0."""
        cfg = ActConfig()
        rc = load_library().qmpc_act_config_default(C.byref(cfg))
        if rc != QMPC_OK:
            raise QmpcError(f"qmpc_act_config_default failed rc={rc}")
        return BatchedActuators._config_dict(cfg)

    @staticmethod
    def _config_dict(cfg):
        return dict(gear=tuple(cfg.gear), **{k: getattr(cfg, k) for k in ACT_CONFIG_FIELDS})

    def init(self, config=None, stream=None, **overrides):
        """The ring, the counters and the accumulators zero, nothing bound.  config: a dict as default_config() returns
        (None: the default); keyword overrides replace single members, e.g. init(max_delay=8, tau_max=1.5)."""
        cfg = dict(self.default_config() if config is None else config)
        unknown = set(overrides) - set(cfg)
        if unknown:
            raise QmpcError(f"BatchedActuators.init: unknown config member(s) {sorted(unknown)}")
        cfg.update(overrides)
        c = ActConfig()
        c.gear = (C.c_double * 3)(*[float(g) for g in cfg["gear"]])
        for k, ty in ACT_CONFIG_FIELDS.items():
            setattr(c, k, int(cfg[k]) if ty is C.c_int else float(cfg[k]))
        self.ctrl._call("qmpc_act_init", self.plant.batch or 0, C.byref(c), self.ctrl._s(stream))
        self.batch = self.plant.batch
        self.config = self._config_dict(c)
        self._params = {}

    def set_params(self, battery_v=None, tau_max=None, strength=None, damping=None, dry_friction=None, delay=None):
        """Per-robot motors: float64 device tensors [B] battery_v (V), tau_max (motor-side cap, N m), strength (a factor on
        the joint torque), damping, dry_friction, and delay, int32 [B] in ticks (clamped to 0 .. max_delay); None: the
        config's value (strength: no factor, delay: 0).  The tensors are read at every later apply() -- write into them
        in place (on the stream) to change a value, also between replays of a captured graph; they are kept referenced
        here.  All None unbinds; init() unbinds."""
        if self.batch is None:
            raise QmpcError("qmpc_act_set_params before init()")
        given = dict(battery_v=battery_v, tau_max=tau_max, strength=strength, damping=damping, dry_friction=dry_friction,
                     delay=delay)
        prm = ActParams()
        for k, dt in ACT_PARAM_FIELDS.items():
            if given[k] is not None:
                setattr(prm, k, self.ctrl._chk(given[k], (self.batch,), getattr(self.torch, dt), k))
        self.ctrl._call("qmpc_act_set_params", self.batch, C.byref(prm))
        self._params = {k: t for k, t in given.items() if t is not None}

    def reset(self, mask_a=None, mask_b=None, stats=False, stream=None):
        """age = 0 -- the next command is applied at once, the ring fills again -- for the robots where either mask is
        set (both None: all); stats=True also zeroes their accumulators."""
        a, pa = self.ctrl._mask(mask_a)
        b, pb = self.ctrl._mask(mask_b)
        self._keep = (a, b)
        self.ctrl._call("qmpc_act_reset", self.batch or 0, pa, pb, 1 if stats else 0, self.ctrl._s(stream))

    def apply(self, effort=None, out=None, stream=None):
        """One control period: effort [B,12] float64 (None: plant.effort) -> out (None: in place) -> the output."""
        if self.batch is None:
            raise QmpcError("qmpc_act before init()")
        effort = self.plant.effort if effort is None else effort
        out = effort if out is None else out
        a = self.ctrl._chk(effort, (self.batch, 12), self.torch.float64, "effort")
        b = self.ctrl._chk(out, (self.batch, 12), self.torch.float64, "out")
        self.ctrl._call("qmpc_act", self.batch, a, b, self.ctrl._s(stream))
        return out

    def view(self):
        """qmpc_act_view_get as zero-copy device tensors that alias the state, like BatchedPlant.view(): ring
        [max_delay + 1, B, 12] float64, head, age, n ([B] int32), n_vsat, n_tsat ([B] int64), tau_peak, e_heat, e_mech,
        e_pos ([B] float64); plus config (a dict), dt, batch.  Read-only by contract."""
        res = self.ctrl._views("qmpc_act_view_get", ActView, {k: (None, ts) for k, ts in ACT_VIEW_FIELDS.items()},
                               ("ring", "config", "dt", "batch"))
        res["config"] = self._config_dict(res["config"])
        shape = (res["config"]["max_delay"] + 1, res["batch"], 12)
        res["ring"] = self.torch.as_tensor(_DeviceArray(res["ring"], shape, "<f8", self.ctrl), device=self.device)
        return res

    def stats(self):
        """The accumulators of view() alone: n, n_vsat, n_tsat, tau_peak, e_heat, e_mech, e_pos ([B] each); plus dt,
        batch.  Read-only by contract."""
        v = self.view()
        return {k: v[k] for k in ACT_STATS + ("dt", "batch")}


class BatchedEpisodes:
    """The episode manager of include/qmpc_episode.h for a BatchedPlant's robots: step() decides on the device which
    robots are done (latched, not finite, tilted, too low, out of range, timed out), logs how each run ended, draws
    where the robot starts again and what it is told next, and resets controller, commands, plant and statistics for
    exactly those robots -- tick_state -> plant.step -> episodes.step is a closed loop in which robots fall and get up
    without the host (see rollout_episodes()).

    Constructed FROM a plant (the manager lives in the same handle), after plant.init().  Every call only enqueues on
    the current stream (or `stream`); log() synchronises.  `vel` / `gait` are the fleet's commands as bound by set():
    the manager hands them to the controller at every step and rewrites a reset robot's rows."""

    def __init__(self, plant):
        self.plant, self.ctrl = plant, plant.ctrl
        self.torch, self.lib, self.device = plant.torch, plant.lib, plant.device
        self.batch = None
        self._bound = {}

    def init(self, seed=0, stream=None):
        """Ages, episode numbers, counters and the log's words zero, start = the plant's x, y, the draws' 64-bit seed;
        no rule, nothing bound."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.ctrl._call("qmpc_episode_init", self.plant.batch or 0, seed, self.ctrl._s(stream))
        self.batch = self.plant.batch
        self._bound = {}
        self.vel = self.gait = None

    def set(self, vel, gait, spawn, commands=None, log_rows=0, causes=0, max_ticks=0, cos_tilt_min=float("nan"),
            z_min=float("nan"), range=float("nan")):
        """The rule and the bindings.  causes: an int of EP_* bits or an iterable of EP_CAUSES' names; a threshold that
        is not finite switches its criterion off.  vel [B,3] float64 and gait [B] int32 are the fleet's commands (the
        tensors ctrl.set_vel / set_gait were given, or copies); spawn float64 [S,3] of (x, y, yaw), or [B,S,3] for a
        table per robot; commands float64 [C,4] of (vx, vy, yaw rate, gait number) or None: a reset robot keeps its
        commands; log_rows > 0 allocates the log [log_rows, 8] (see log()).  The tensors are read and written at every
        later step() -- rewrite them in place (on the stream), also between replays of a captured graph; they are kept
        referenced here.  Host state only."""
        if self.batch is None:
            raise QmpcError("qmpc_episode_set before init()")
        t = self.torch
        if not isinstance(causes, int):
            causes = sum(EP_CAUSES[k] for k in causes)
        B = self.batch
        bind = EpisodeBind()
        bind.vel = self.ctrl._chk(vel, (B, 3), t.float64, "vel")
        bind.gait = self.ctrl._chk(gait, (B,), t.int32, "gait")
        per_robot = spawn is not None and spawn.dim() == 3
        if spawn is None or spawn.dim() not in (2, 3) or spawn.shape[-1] != 3 or (per_robot and spawn.shape[0] != B):
            raise QmpcError(f"spawn: expected a float64 tensor of shape (S, 3) or ({B}, S, 3)")
        bind.spawn = self.ctrl._chk(spawn, tuple(spawn.shape), t.float64, "spawn")
        bind.n_spawn = int(spawn.shape[-2])
        bind.flags = EP_SPAWN_PER_ROBOT if per_robot else 0
        if commands is not None:
            if commands.dim() != 2:
                raise QmpcError("commands: expected a float64 tensor of shape (C, 4)")
            bind.commands = self.ctrl._chk(commands, (commands.shape[0], 4), t.float64, "commands")
            bind.n_commands = int(commands.shape[0])
        log = None
        if int(log_rows) > 0:
            log = self._bound.get("log")
            if log is None or log.shape[0] != int(log_rows):
                log = t.zeros((int(log_rows), 8), dtype=t.float64, device=self.device)
            bind.log = log.data_ptr()
        bind.log_rows = int(log_rows)
        rule = EpisodeRule(int(causes), int(max_ticks), float(cos_tilt_min), float(z_min), float(range))
        self.ctrl._call("qmpc_episode_set", B, C.byref(rule), C.byref(bind))
        self._bound = dict(vel=vel, gait=gait, spawn=spawn, commands=commands, log=log)
        self.vel, self.gait = vel, gait

    def step(self, elapsed=1, stream=None):
        """After plant.step(): `elapsed` control periods have passed since the previous step()."""
        if self.batch is None:
            raise QmpcError("qmpc_episode_step before init()")
        self.ctrl._call("qmpc_episode_step", self.batch, int(elapsed), self.ctrl._s(stream))

    def clear_log(self, stream=None):
        """The log starts again at its row 0, dropped = 0 (on the stream)."""
        self.ctrl._call("qmpc_episode_log_clear", self.ctrl._s(stream))

    def view(self):
        """qmpc_episode_view_get as zero-copy device tensors that alias the manager's state, like BatchedPlant.view():
        age, episode, last_cause, last_ticks ([B] int32), ticks_sum ([B] int64), start ([B,2] float64), count ([B,6]
        int32, one column per cause in bit order), mask ([B] uint8), xyyaw ([B,3] float64), log_count and log_dropped
        ([1] int32); plus batch, seed.  Read-only by contract."""
        res = self.ctrl._views("qmpc_episode_view_get", EpisodeView, EPISODE_VIEW_FIELDS,
                               ("log_count", "log_dropped", "batch", "seed"))
        for k in ("log_count", "log_dropped"):
            res[k] = self.torch.as_tensor(_DeviceArray(res[k], (1,), "<i4", self.ctrl), device=self.device)
        return res

    def log(self):
        """-> dict(rows, dropped): the rows written so far, copied to the host (synchronises) and sorted by (robot,
        episode) -- float64 [n, 8] in EPISODE_LOG_COLUMNS' order --, and how many rows found the log full."""
        v = self.view()
        self.torch.cuda.synchronize(self.device)
        n, dropped = int(v["log_count"].cpu()[0]), int(v["log_dropped"].cpu()[0])
        log = self._bound.get("log")
        rows = np.zeros((0, 8)) if log is None else log[:n].cpu().numpy().copy()
        return dict(rows=rows[np.lexsort((rows[:, 1], rows[:, 0]))], dropped=dropped)


class SensedEpisodes:
    """Episodes on the sensor path (include/qmpc_episode_sense.h) for a BatchedEpisodes manager and the BatchedSensors of
    the same plant: step() is episodes.step() for a fleet that walks on its sensors -- a robot that finishes is reset,
    its sensors start a new noise epoch, and for the next `warm_ticks` control periods it is HELD: the whole tick and
    the plant step run for it as for everybody, and step() undoes all of it except what pre_work would have done, so
    the robot gets sensors.settle() for itself while its neighbours walk (see rollout_sensed_episodes()).  The held
    robots' ticks and solves are computed and thrown away: that, and one launch more per step, is the cost.

    Constructed from the two (all three live in the plant's handle), after episodes.init() and sensors.init().  Every
    call only enqueues on the current stream (or `stream`)."""

    def __init__(self, episodes, sensors):
        if episodes.plant is not sensors.plant:
            raise QmpcError("SensedEpisodes: the episodes and the sensors of one plant")
        self.episodes, self.sensors, self.plant, self.ctrl = episodes, sensors, episodes.plant, episodes.ctrl
        self.torch, self.lib, self.device = self.plant.torch, self.plant.lib, self.plant.device
        self.batch = None
        self.warm_ticks = None

    def init(self, warm_ticks=50, stream=None):
        """Nobody in warm-up; warm_ticks >= 0: the control periods of warm-up a robot gets when step() resets it."""
        self.ctrl._call("qmpc_episode_sense_init", self.plant.batch or 0, int(warm_ticks), self.ctrl._s(stream))
        self.batch, self.warm_ticks = self.plant.batch, int(warm_ticks)

    def hold(self, mask=None, ticks=None, stream=None):
        """`ticks` (None: warm_ticks) control periods of warm-up, from the next step() on, for the robots where mask is
        set (None: all), on the pose the plant holds them in now: the fleet's initial settle, or the warm-up of robots
        the caller has reset (ctrl.reset, plant.reset, sensors.reset, then this, between step() and sensors.sense())."""
        if self.batch is None:
            raise QmpcError("qmpc_episode_sense_hold before init()")
        self._keep, ptr = self.ctrl._mask(mask)
        self.ctrl._call("qmpc_episode_sense_hold", self.batch, ptr, int(self.warm_ticks if ticks is None else ticks),
                        self.ctrl._s(stream))

    def step(self, effort=None, stream=None):
        """After plant.step() and before sensors.sense(), on every tick.  effort: the tick's output [B,12] float64, whose
        rows are zeroed for the robots reset or held; None: left alone."""
        if self.batch is None:
            raise QmpcError("qmpc_episode_sense_step before init()")
        ptr = None if effort is None else self.ctrl._chk(effort, (self.batch, 12), self.torch.float64, "effort")
        self.ctrl._call("qmpc_episode_sense_step", self.batch, ptr, self.ctrl._s(stream))

    def view(self):
        """qmpc_episode_sense_view_get as zero-copy device tensors that alias the state, like BatchedEpisodes.view():
        warm ([B] int32: control periods of warm-up still to come), hold ([B] uint8: held by the last step()); plus
        warm_ticks, batch.  Read-only by contract."""
        return self.ctrl._views("qmpc_episode_sense_view_get", EpisodeSenseView, dict(warm=(None, "<i4"), hold=(None, "|u1")),
                                ("warm_ticks", "batch"))


def _run_ticks(ctrl, who, ticks, graph, tick, block=None):
    """The runner behind rollout() and rollout_sensed() (`who`: the caller's name, which starts its messages): tick()
    `ticks` times on the current stream -- or block() once, where the caller has one call for all of them --, or that
    block captured on a side stream and replayed once -> the graph, or None."""
    torch = ctrl.torch
    ticks = int(ticks)
    if ticks < 1:
        raise QmpcError(f"{who}: ticks must be at least 1")

    if block is None:
        def block():
            for _ in range(ticks):
                tick()

    if not graph:
        block()
        return None
    if ctrl.schedule == "lockstep" and ticks % 13 != 0:
        raise QmpcError(f"{who}: a captured block holds a multiple of 13 ticks in lockstep, not {ticks}")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=ctrl.device)
    s.wait_stream(torch.cuda.current_stream(ctrl.device))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            block()
    torch.cuda.current_stream(ctrl.device).wait_stream(s)
    g.replay()
    return g


def rollout(ctrl, plant, ticks, graph=False, actuators=None, fused=False):
    """`ticks` closed-loop ticks, ctrl.tick_state(plant.state, plant.motor) -> plant.step(effort), on the current
    stream, continuing from wherever the pair stands.  graph=True captures the block of `ticks` ticks into a
    torch.cuda.graph (on a side stream) and replays it once; the graph is returned for further replays, each of which
    runs the block again.  With the lockstep schedule a captured block must hold a multiple of 13 ticks (the host
    decides the MPC ticks from its own count, which replays do not advance: include/qmpc_ctrl.h) -- refused otherwise.
    actuators: a BatchedActuators of the plant, whose apply() then stands between the tick and the step (in place on
    plant.effort); None: nothing is added.
    fused=True: the same ticks through ONE qmpc_fleet_run call (include/qmpc_fleet.h) -- everything between two MPC
    solves in one launch, the same bits in every array; ctrl.fleet_info() tells whether the fused kernel served them or
    the call fell back to the per-tick launches (terrain, ground-decided contact or a height field bound).  Not with
    actuators, which stand between two stages of a tick: refused.
    -> dict(effort, state, motor, graph): the plant's own tensors, as the last tick left them."""
    def tick():
        ctrl.tick_state(plant.state, plant.motor, plant.effort)
        if actuators is not None:
            actuators.apply()
        plant.step(plant.effort)

    block = None
    if fused:
        if actuators is not None:
            raise QmpcError("rollout: fused=True does not take actuators (they stand between the tick and the step)")
        if plant.batch is None:
            raise QmpcError("qmpc_fleet_run before init()")

        def block():
            chk = ctrl._chk
            ctrl._call("qmpc_fleet_run", plant.batch, int(ticks),
                       chk(plant.effort, (plant.batch, 12), ctrl.torch.float64, "effort"),
                       chk(plant.state, (plant.batch, 16), ctrl.torch.float64, "state"),
                       chk(plant.motor, (plant.batch, 24), ctrl.torch.float64, "motor"), ctrl._s(None))

    g = _run_ticks(ctrl, "rollout", ticks, graph, tick, block)
    return dict(effort=plant.effort, state=plant.state, motor=plant.motor, graph=g)


def rollout_sensed(ctrl, plant, sensors, ticks, graph=False, actuators=None):
    """rollout() through the sensor path: `ticks` closed-loop ticks ctrl.tick(sensors.imu, sensors.motor) ->
    plant.step(effort) -> sensors.sense(), continuing from wherever the three stand -- sensors.imu / motor must hold a
    reading (sensors.settle() or one sensors.sense() leaves one).  graph=True as in rollout(): the block is captured and
    replayed once, the graph returned for further replays; in lockstep a captured block holds a multiple of 13 ticks.
    actuators: as in rollout(), between the tick and the step.
    -> dict(effort, state, motor, imu, graph): the plant's own tensors and the sensors' imu, as the last tick left them."""
    def tick():
        ctrl.tick(sensors.imu, sensors.motor, plant.effort)
        if actuators is not None:
            actuators.apply()
        plant.step(plant.effort)
        sensors.sense()

    g = _run_ticks(ctrl, "rollout_sensed", ticks, graph, tick)
    return dict(effort=plant.effort, state=plant.state, motor=plant.motor, imu=sensors.imu, graph=g)


def rollout_episodes(ctrl, plant, episodes, ticks, graph=False, every=1, actuators=None, actuator_stats=False):
    """rollout() with the episode manager in the loop: `ticks` closed-loop ticks ctrl.tick_state(plant.state,
    plant.motor) -> plant.step(effort), and after every `every`-th tick of this call episodes.step(elapsed=every).
    graph=True as in rollout(): the block is captured and replayed once, the graph returned for further replays; in
    lockstep a captured block holds a multiple of 13 ticks.  `ticks` must be a multiple of `every`, so that consecutive
    calls and replays check at the same spacing.  actuators: as in rollout(), between the tick and the step, and after
    every episodes.step() actuators.reset(the manager's mask, stats=actuator_stats): a robot that starts again starts
    with an empty ring (and, with actuator_stats, fresh accumulators).
    -> dict(effort, state, motor, graph): the plant's own tensors, as the last tick left them."""
    every = int(every)
    if every < 1 or int(ticks) % every != 0:
        raise QmpcError(f"rollout_episodes: ticks ({ticks}) must be a multiple of every ({every}) >= 1")
    n = [0]
    mask = episodes.view()["mask"] if actuators is not None else None

    def tick():
        ctrl.tick_state(plant.state, plant.motor, plant.effort)
        if actuators is not None:
            actuators.apply()
        plant.step(plant.effort)
        n[0] += 1
        if n[0] % every == 0:
            episodes.step(every)
            if actuators is not None:
                actuators.reset(mask, stats=actuator_stats)

    g = _run_ticks(ctrl, "rollout_episodes", ticks, graph, tick)
    return dict(effort=plant.effort, state=plant.state, motor=plant.motor, graph=g)


def rollout_sensed_episodes(ctrl, plant, sensors, sensed, ticks, graph=False, actuators=None, actuator_stats=False):
    """rollout_sensed() with the episode manager in the loop: `ticks` closed-loop ticks ctrl.tick(sensors.imu,
    sensors.motor) -> plant.step(effort) -> sensed.step(effort) -> sensors.sense(), continuing from wherever the four
    stand -- sensors.imu / motor must hold a reading (one sensors.sense() leaves one; sensed.hold() beforehand gives the
    whole fleet its warm-up inside the loop).  graph=True as in rollout(): the block is captured and replayed once, the
    graph returned for further replays; in lockstep a captured block holds a multiple of 13 ticks.  actuators: as in
    rollout_episodes(); the reset takes the manager's mask and the robots held by the last step, so a robot leaves its
    warm-up with an empty ring.
    -> dict(effort, state, motor, imu, graph): the plant's own tensors and the sensors' imu, as the last tick left them."""
    if actuators is not None:
        mask, hold = sensed.episodes.view()["mask"], sensed.view()["hold"]

    def tick():
        ctrl.tick(sensors.imu, sensors.motor, plant.effort)
        if actuators is not None:
            actuators.apply()
        plant.step(plant.effort)
        sensed.step(plant.effort)
        if actuators is not None:
            actuators.reset(mask, hold, stats=actuator_stats)
        sensors.sense()

    g = _run_ticks(ctrl, "rollout_sensed_episodes", ticks, graph, tick)
    return dict(effort=plant.effort, state=plant.state, motor=plant.motor, imu=sensors.imu, graph=g)


def rollout_loop(ctrl, plant, ticks, graph=False, actuators=None, episodes=None, every=1, actuator_stats=False):
    """rollout_episodes() through ONE qmpc_loop_run call (include/qmpc_loop.h): `ticks` closed-loop ticks
    ctrl.tick_state -> [actuators.apply] -> plant.step, after every `every`-th tick of the call [episodes.step(every) ->
    actuators.reset(the manager's mask, stats=actuator_stats)], with everything between two MPC solves in one launch and
    the same bits in every array; ctrl.loop_info() tells whether the fused kernel served them or the call fell back to the
    per-tick launches (terrain, ground-decided contact or a height field bound).  actuators: a BatchedActuators of the
    plant or None; episodes: a BatchedEpisodes of the plant, set(), or None (`every` is then ignored); with neither the
    call is rollout(fused=True).  `ticks` must be a multiple of `every`.  graph=True as in rollout(): the call is captured
    and replayed once, the graph returned for further replays; in lockstep a captured block holds a multiple of 13 ticks.
    -> dict(effort, state, motor, graph): the plant's own tensors, as the last tick left them."""
    if plant.batch is None:
        raise QmpcError("qmpc_loop_run before init()")
    every = int(every) if episodes is not None else 0
    if episodes is not None and (every < 1 or int(ticks) % every != 0):
        raise QmpcError(f"rollout_loop: ticks ({ticks}) must be a multiple of every ({every}) >= 1")
    for who, stage in (("actuators", actuators), ("episodes", episodes)):
        if stage is not None and stage.plant is not plant:
            raise QmpcError(f"rollout_loop: the {who} of another plant")
    opts = LoopOpts(1 if actuators is not None else 0, every, 1 if actuator_stats else 0)

    def block():
        chk = ctrl._chk
        ctrl._call("qmpc_loop_run", plant.batch, int(ticks), C.byref(opts),
                   chk(plant.effort, (plant.batch, 12), ctrl.torch.float64, "effort"),
                   chk(plant.state, (plant.batch, 16), ctrl.torch.float64, "state"),
                   chk(plant.motor, (plant.batch, 24), ctrl.torch.float64, "motor"), ctrl._s(None))

    g = _run_ticks(ctrl, "rollout_loop", ticks, graph, None, block)
    return dict(effort=plant.effort, state=plant.state, motor=plant.motor, graph=g)
