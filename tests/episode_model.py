"""numpy restatement of the episode manager (include/qmpc_episode.h) -- TEST SIDE ONLY.

Restates, operation by operation, what csrc/qmpc_episode_rule.h decides and draws and what the decision kernel of
csrc/qmpc_episode.hip keeps: ages, episode numbers, starts, counters, the log's rows and its two words.  Comparisons and
one fp64 operation at a time, no transcendental function: the device and this file agree bit for bit.  The draw is
tests/sense_model.py's Philox4x32-10.
"""
import numpy as np

from sense_model import philox4x32_10

UNSAFE, NONFINITE, TILT, HEIGHT, RANGE, TIMEOUT = 1, 2, 4, 8, 16, 32
ALL = 63
N_CAUSES = 6
NAMES = ("unsafe", "nonfinite", "tilt", "height", "range", "timeout")
INT_MAX = 2 ** 31 - 1
f64, u64 = np.float64, np.uint64


def finite(x):
    """x - x == 0: neither NaN nor +-inf."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x, f64)
        return (x - x) == 0.0


def age_after(age, elapsed):
    age = np.asarray(age, np.int64)
    return np.where(age > INT_MAX - elapsed, INT_MAX, age + elapsed).astype(np.int64)


def cause_of(rule, safe, p, q, ground, start, age):
    """rule: dict(causes, max_ticks, cos_tilt_min, z_min, range); safe [B], p [B,3], q [B,4] (w x y z), ground [B],
    start [B,2], age [B] after the increment -> (cause [B] int, facts [B,4] = dx, dy, height, tilt)."""
    p, q, start, ground = (np.asarray(a, f64) for a in (p, q, start, ground))
    with np.errstate(invalid="ignore", over="ignore"):
        xx = q[:, 1] * q[:, 1]
        yy = q[:, 2] * q[:, 2]
        s = xx + yy
        t = 2.0 * s
        tilt = 1.0 - t
        dx = p[:, 0] - start[:, 0]
        dy = p[:, 1] - start[:, 1]
        height = p[:, 2] - ground
        cause = np.zeros(len(p), np.int64)
        cause |= np.where(np.asarray(safe) == 0, UNSAFE, 0)
        cause |= np.where(finite(p).all(1) & finite(q).all(1), 0, NONFINITE)
        if finite(rule["cos_tilt_min"]):
            cause |= np.where(tilt < f64(rule["cos_tilt_min"]), TILT, 0)
        if finite(rule["z_min"]):
            cause |= np.where(height < f64(rule["z_min"]), HEIGHT, 0)
        if finite(rule["range"]):
            cause |= np.where((np.abs(dx) > f64(rule["range"])) | (np.abs(dy) > f64(rule["range"])), RANGE, 0)
        cause |= np.where(np.asarray(age) >= int(rule["max_ticks"]), TIMEOUT, 0)
    return cause & int(rule["causes"]), np.stack([dx, dy, height, tilt], 1)


def gait_of(g):
    """the gait column of a command row: clamped to [0, 31] (a NaN to 0), then truncated."""
    g = np.asarray(g, f64)
    g = np.where(~(g >= 0.0), 0.0, g)
    return np.where(g > 31.0, 31.0, g).astype(np.int32)


def row_of(w, n):
    """the high word of w n: a 32-bit word -> a row of a table of n >= 1 rows."""
    return ((np.asarray(w).astype(u64) * u64(n)) >> u64(32)).astype(np.int64)


def draw(seed, b, episode, n_spawn, n_commands):
    """-> (spawn row, command row) of robot(s) b for episode index(es) `episode` (after the increment); n_commands < 1:
    command row 0."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return draw_keys(seed & 0xFFFFFFFF, seed >> 32, b, episode, n_spawn, n_commands)


def draw_keys(key0, key1, b, episode, n_spawn, n_commands):
    w = philox4x32_10(np.asarray(b, np.int64), np.asarray(episode, np.int64), 0, 0, key0, key1)
    return row_of(w[0], n_spawn), (row_of(w[1], n_commands) if n_commands >= 1 else np.zeros_like(row_of(w[0], 1)))


class EpisodeModel:
    """qmpc_episode_init / set / step / log_clear for B robots.  vel / gait are the model's own copies of the fleet's
    commands, rewritten by step() like the bound tensors."""

    def __init__(self, B, seed, p):
        self.B, self.seed = B, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.age = np.zeros(B, np.int64)
        self.episode = np.zeros(B, np.int64)
        self.start = np.asarray(p, f64)[:, :2].copy()
        self.count = np.zeros((B, N_CAUSES), np.int64)
        self.ticks_sum = np.zeros(B, np.int64)
        self.last_cause = np.zeros(B, np.int64)
        self.last_ticks = np.zeros(B, np.int64)
        self.mask = np.zeros(B, bool)
        self.xyyaw = np.zeros((B, 3))
        self.rows = []              # every row a log without end would hold, in robot order within a step
        self.rows_step = []         # ... and the index of the step() that produced it
        self.steps = 0
        self.log_rows = 0
        self.logging = False
        self.cleared_at = 0         # rows before this one were appended before the last clear_log()

    def set(self, vel, gait, spawn, commands=None, log_rows=0, causes=0, max_ticks=0, cos_tilt_min=np.nan, z_min=np.nan,
            range=np.nan, log=True):
        self.vel, self.gait = np.array(vel, f64), np.array(gait, np.int32)
        self.spawn = np.asarray(spawn, f64)
        self.commands = None if commands is None else np.asarray(commands, f64)
        self.rule = dict(causes=int(causes), max_ticks=int(max_ticks), cos_tilt_min=cos_tilt_min, z_min=z_min, range=range)
        self.log_rows, self.logging = int(log_rows), bool(log)

    def clear_log(self):
        self.cleared_at = len(self.rows)

    @property
    def total(self):
        return len(self.rows) - self.cleared_at

    @property
    def log_count(self):
        return min(self.total, self.log_rows)

    @property
    def dropped(self):
        return self.total - self.log_count

    def all_rows(self):
        """Every row since the last clear, sorted by (robot, episode)."""
        r = np.array(self.rows[self.cleared_at:], f64).reshape(-1, 8)
        return r[np.lexsort((r[:, 1], r[:, 0]))]

    def certain_rows(self):
        """The rows every legal device log holds: those of the steps that ended with the log not yet full (the order in
        which the waves of ONE step append is unspecified, so the step that overflows keeps an unspecified subset)."""
        rows, steps = self.rows[self.cleared_at:], self.rows_step[self.cleared_at:]
        full_at = steps[self.log_rows] if len(rows) > self.log_rows else None
        r = np.array([row for row, st in zip(rows, steps) if full_at is None or st < full_at], f64).reshape(-1, 8)
        return r[np.lexsort((r[:, 1], r[:, 0]))]

    def step(self, p, q, safe, ground=None, elapsed=1):
        """-> (mask [B] bool, xyyaw [B,3]): whom to reset and where; vel / gait updated."""
        self.steps += 1
        B = self.B
        if not self.rule["causes"]:
            return np.zeros(B, bool), self.xyyaw
        ground = np.zeros(B) if ground is None else ground
        self.age = age_after(self.age, elapsed)
        cause, facts = cause_of(self.rule, safe, p, q, ground, self.start, self.age)
        done = cause != 0
        idx = np.flatnonzero(done)
        if self.logging:
            for b in idx:
                self.rows.append([float(b), float(self.episode[b]), float(cause[b]), float(self.age[b])] + list(facts[b]))
                self.rows_step.append(self.steps)
        for k in range(N_CAUSES):
            self.count[idx, k] += (cause[idx] >> k) & 1
        self.ticks_sum[idx] += self.age[idx]
        self.last_cause[idx] = cause[idx]
        self.last_ticks[idx] = self.age[idx]
        nxt = self.episode[idx] + 1
        per_robot = self.spawn.ndim == 3
        S = self.spawn.shape[-2]
        C = 0 if self.commands is None else len(self.commands)
        sr, cr = draw(self.seed, idx, nxt, S, C)
        sp = self.spawn[idx, sr] if per_robot else self.spawn[sr]
        self.xyyaw[idx] = sp
        self.start[idx] = sp[:, :2]
        self.age[idx] = 0
        self.episode[idx] = nxt
        if self.commands is not None:
            self.vel[idx] = self.commands[cr, :3]
            self.gait[idx] = gait_of(self.commands[cr, 3])
        self.mask = done
        return done, self.xyyaw
