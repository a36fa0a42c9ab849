"""The case table of the actuator stage (include/qmpc_act.h) -- TEST SIDE ONLY: per-robot parameters, commands and
joint rates that reach every branch of csrc/qmpc_act_model.h.  tests/test_act_cpu.py feeds it to the stand-alone host
program tests/act_dump.cpp, tests/test_gpu_act.py to the kernel; both are compared with tests/act_model.py bit for bit.
"""
import numpy as np

import act_model as AM

B = 37            # not a multiple of a wave's four robots, more than one wave
NAN_ROBOT = 5     # the robot whose inputs hold NaN and inf
TINY = 5e-324


def params(B=B, seed=3):
    """All six arrays, every robot its own values: voltages and caps low enough that the clamps are reached."""
    rng = np.random.default_rng(seed)
    return dict(battery_v=rng.uniform(2.0, 30.0, B), tau_max=rng.uniform(0.5, 4.0, B), strength=rng.uniform(0.5, 1.2, B),
                damping=rng.uniform(0.0, 0.05, B), dry_friction=rng.uniform(0.0, 0.4, B),
                delay=rng.integers(-3, AM.MAX_DELAY + 6, B).astype(np.int32))


def period(call, B=B, seed=7, hostile=True):
    """(effort [B,12], qd [B,12]) of call number `call`: changing inputs, with the special rows rewritten every call.
    Rows 0..4 hold the clamps (both voltage clamps, both torque clamps, both at once), row NAN_ROBOT the non-finite
    values (hostile=False: finite like its neighbours), rows 6..8 the zeros and tiny rates of both signs."""
    rng = np.random.default_rng(seed * 1000 + call)
    eff = rng.uniform(-25.0, 25.0, (B, 12))
    qd = rng.uniform(-30.0, 30.0, (B, 12))
    if B < 9:
        return eff, qd
    eff[0], qd[0] = 0.5, 40.0          # vdes far above V through the back-EMF alone: upper voltage clamp
    eff[1], qd[1] = -0.5, -40.0        # lower voltage clamp
    eff[2], qd[2] = 40.0, 0.0          # no back-EMF, a large command: upper torque clamp (and the voltage clamp at low V)
    eff[3], qd[3] = -40.0, 0.0         # lower torque clamp
    eff[4], qd[4] = 500.0, -25.0       # the voltage clamped from above and the torque still beyond its cap: both at once
    eff[4, 6:], qd[4, 6:] = -500.0, 25.0
    if hostile:
        eff[NAN_ROBOT] = [np.nan, np.inf, -np.inf, 1.0, 2.0, 3.0, np.nan, np.inf, -np.inf, 1.0, 2.0, 3.0]
        qd[NAN_ROBOT] = [1.0, 2.0, 3.0, np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0]
    qd[6] = [0.0, -0.0, TINY, -TINY, 1e-300, -1e-300, 0.0, -0.0, TINY, -TINY, 1e-300, -1e-300]
    eff[7], qd[7] = 0.0, [0.0, -0.0, TINY, -TINY] * 3
    eff[8], qd[8] = -0.0, 0.0
    return eff, qd


# what each binding of the tests names: nothing, each array alone, all of them
BINDINGS = [()] + [(k,) for k in AM.PARAMS] + [AM.PARAMS]
