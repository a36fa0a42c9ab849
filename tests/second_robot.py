"""The second robot of tests/test_gpu_constants.py and tests/test_constants_cpu.py -- TEST SIDE ONLY, defined once.

Every scalar a caller can set on a handle, at a value that is not the Mini Cheetah's: every link more than 10 % off the
default, the knee offset non-zero; another mass, inertia and gravity; 400 Hz (1 / 400 is no float) and 1000 Hz, on
either side of the Kalman filter's literal dt = 0.002; friction and force limit of the solve and of the plant."""
import numpy as np

GEOM2 = (0.071, 0.243, 0.226, 0.0065)                     # abad, hip, knee, knee_y: qmpc_set_leg_geometry's doubles
GEOM2_F = np.array(GEOM2, np.float32)                     # ... as the handle keeps them
MASS2, IBODY2, GRAVITY2 = 12.5, (0.11, 0.36, 0.41), -9.81  # qmpc_set_robot's
FREQS2 = (400.0, 1000.0)
F_MAX2 = 90.0
SOLVE2 = ((0.013, 0.25), (0.0325, 0.6))                   # (dt_mpc, mu): 13 / 1000, 13 / 400
# the plant's constructor arguments (tests/plant_cases.py's dict, PlantModel's names)
PLANT2 = dict(freq=400.0, mu=0.6, mass=MASS2, ibody=np.array(IBODY2), geom=GEOM2_F.astype(np.float64))
