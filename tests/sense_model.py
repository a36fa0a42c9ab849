"""numpy restatement of the sensor model (include/qmpc_sense.h) -- TEST SIDE ONLY.

Restates, operation by operation, what qmpc_sense.hip's kernels compute: the rearrangement of the plant's read-out into
imu[B][10] / motor[B][24], the counter-based noise (Philox4x32-10 -> the centred sum of its four words, scaled to unit
variance) and the per-robot counters n / epoch.  Everything is integer arithmetic or one fp64 operation at a time, no
transcendental function: the device and this file agree bit for bit (tests/test_gpu_sense.py asserts array_equal).
"""
import numpy as np

u32, u64, f64 = np.uint32, np.uint64, np.float64

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57       # multipliers on counter words 0 and 2
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85       # key increments between rounds
Z_CENTRE = 8589934590.0                             # 4 (2^32 - 1) / 2: the mean of the sum of four words
Z_SCALE = 1.7320508075688772 * 2.0 ** -32           # sqrt(3) / 2^32: the sum's standard deviation is 2^32 / sqrt(3)
Z_MAX = 2.0 * np.sqrt(3.0)
Z_EXCESS_KURTOSIS = -6.0 / (5.0 * 4.0)              # Irwin-Hall, n = 4
N_CHANNELS = 30
CH_ACC, CH_GYRO, CH_Q, CH_QD = 0, 3, 6, 18          # first channel of each group (3, 3, 12, 12)
PARAMS = dict(acc_bias=3, gyro_bias=3, acc_sigma=1, gyro_sigma=1, q_sigma=1, qd_sigma=1)   # qmpc_sense_params' order


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on arrays of 32-bit words (broadcast against each other) -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x).astype(u64) & u64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    mask, sh = u64(0xFFFFFFFF), u64(32)
    for r in range(10):
        p0, p1 = u64(PHILOX_M0) * c0, u64(PHILOX_M1) * c2         # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + u64(PHILOX_W0)) & mask, (k1 + u64(PHILOX_W1)) & mask
    return c0.astype(u32), c1.astype(u32), c2.astype(u32), c3.astype(u32)


def z_of(seed, robot, n, channel, epoch):
    """The unit-variance variate of (seed, robot, n, channel, epoch): arrays broadcast -> float64, |z| <= 2 sqrt(3)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(robot, n, channel, epoch, seed & 0xFFFFFFFF, seed >> 32)
    s = (w[0].astype(u64) + w[1].astype(u64)) + (w[2].astype(u64) + w[3].astype(u64))       # exact: below 2^34
    return (s.astype(f64) - Z_CENTRE) * Z_SCALE


def as_imu(state):
    """state[B][16] -> imu[B][10]: accelerometer, quaternion x y z w, gyro -- copies, bit for bit."""
    state = np.asarray(state, f64)
    return np.concatenate([state[:, 13:16], state[:, 1:4], state[:, 0:1], state[:, 7:10]], 1)


class SenseModel:
    """qmpc_sense_init / set_params / reset / sense for B robots."""

    def __init__(self, B, seed):
        self.B, self.seed = B, int(seed)
        self.n, self.epoch = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.prm = {}

    def set_params(self, **prm):
        """float64 arrays by qmpc_sense_params' names; a name that is missing or None is a NULL member."""
        assert set(prm) <= set(PARAMS), prm.keys()
        self.prm = {k: np.asarray(v, f64) for k, v in prm.items() if v is not None}

    def reset(self, mask=None):
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask) != 0
        self.epoch[m] += 1
        self.n[m] = 0

    def _channel(self, x, first, bias, sigma):
        """x [B,k]: channels first .. first + k - 1 of every robot."""
        bias, sigma = self.prm.get(bias), self.prm.get(sigma)
        if bias is None and sigma is None:
            return x.copy()
        d = np.zeros_like(x)
        if sigma is not None:
            robot = np.arange(self.B, dtype=np.int64)[:, None]
            ch = first + np.arange(x.shape[1], dtype=np.int64)[None, :]
            z = z_of(self.seed, robot, self.n.astype(np.int64)[:, None], ch, self.epoch.astype(np.int64)[:, None])
            with np.errstate(invalid="ignore", over="ignore"):
                d = sigma[:, None] * z
        if bias is not None:
            with np.errstate(invalid="ignore"):
                d = bias + d
        with np.errstate(invalid="ignore"):
            return x + d

    def sense(self, state, motor):
        """-> (imu [B,10], motor_out [B,24]); n += 1."""
        state, motor = np.asarray(state, f64), np.asarray(motor, f64)
        imu = as_imu(state)
        imu[:, 0:3] = self._channel(state[:, 13:16], CH_ACC, "acc_bias", "acc_sigma")
        imu[:, 7:10] = self._channel(state[:, 7:10], CH_GYRO, "gyro_bias", "gyro_sigma")
        out = np.concatenate([self._channel(motor[:, :12], CH_Q, None, "q_sigma"),
                              self._channel(motor[:, 12:], CH_QD, None, "qd_sigma")], 1)
        self.n += 1
        return imu, out
