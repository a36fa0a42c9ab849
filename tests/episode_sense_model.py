"""numpy restatement of episodes on the sensor path (include/qmpc_episode_sense.h) -- TEST SIDE ONLY.

tests/episode_model.py's EpisodeModel with the two arrays the sensor path adds: warm (control periods of warm-up a robot
still has in front of it) and hold (held by the last step).  A held robot is not judged; every other robot gets
EpisodeModel's own step with elapsed = 1: that step runs on the whole fleet and what it did to the held robots -- state,
commands, log rows -- is taken back, so the bookkeeping is written down once, in that file.

reference_loop_on_epoch() is the CPU check behind the envelope test of tests/test_gpu_episode_sense.py.
"""
import numpy as np

import episode_model as EM

# what EpisodeModel.step may write of a robot
PER_ROBOT = ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "xyyaw", "vel", "gait")


class EpisodeSenseModel(EM.EpisodeModel):
    """qmpc_episode_init / set, qmpc_episode_sense_init / hold / step for B robots."""

    def __init__(self, B, seed, p, warm_ticks):
        super().__init__(B, seed, p)
        self.warm_ticks = int(warm_ticks)
        self.warm = np.zeros(B, np.int64)
        self.hold = np.zeros(B, bool)

    def hold_robots(self, mask=None, ticks=None, xyyaw=None):
        """qmpc_episode_sense_hold: warm = ticks (None: warm_ticks) where mask is set (None: all); xyyaw [B,3]: the pose
        the plant holds the robots in (the kernel recovers it from the plant; the model is told), which becomes the
        robots' xyyaw row and, its x, y, their start."""
        mask = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        self.warm[mask] = self.warm_ticks if ticks is None else int(ticks)
        if xyyaw is not None:
            self.xyyaw[mask] = np.asarray(xyyaw, np.float64)[mask]
            self.start[mask] = self.xyyaw[mask, :2]

    def step(self, p, q, safe, ground=None):
        """-> (mask [B] bool, hold [B] bool, xyyaw [B,3]): whom to reset, whom to hold, and where both stand."""
        held = self.warm > 0
        self.warm[held] -= 1
        self.hold = held.copy()
        kept = {k: getattr(self, k)[held].copy() for k in PER_ROBOT}
        n0 = len(self.rows)
        done, _ = super().step(p, q, safe, ground, 1)
        for k, v in kept.items():                      # a held robot was not judged: nothing of it moved
            getattr(self, k)[held] = v
        new = [(r, s) for r, s in zip(self.rows[n0:], self.rows_step[n0:]) if not held[int(r[0])]]
        self.rows[n0:], self.rows_step[n0:] = [r for r, _ in new], [s for _, s in new]
        done = done & ~held
        self.warm[done] = self.warm_ticks
        self.mask = done
        return done, self.hold, self.xyyaw


def reference_loop_on_epoch(mode, epoch=1, **kw):
    """sense_loop.cpu_loop_sensed(mode, noisy=True, **kw) -- the reference pipeline on the CPU, the reference's own
    qpOASES for every solve -- with the sensor model drawing noise epoch `epoch` instead of 0: what a fleet's second
    episode draws.  -> (stats, info).  About a minute per mode; run by hand:

        python -c "import sys; sys.path[:0] = ['.', 'tests']; import json, numpy as np, plant_loop as L, episode_sense_model as M
        gold = json.load(open('tests/golden/sense_closed_loop_cpu.json'))
        for mode in (0, 1):
            stats, info = M.reference_loop_on_epoch(mode, settle=gold['settle'], seed=gold['seed'])
            rec = gold[f'mode{mode}']['noisy']; env = L.envelope(rec)
            print(mode, (info['safe'] == 1).all(), info['rc_bad'], {k: float(np.abs(stats[k] - np.asarray(rec[k])).max()
                  / max(float((env[k][1] - np.asarray(rec[k])).max()), 1e-300)) for k in L.STATS})"

    which printed, for the committed fixture: every robot safe, rc_bad 0, and as the largest fraction of the allowed
    distance 0.069 (z_min) in mode 0 and 0.039 (z_min) in mode 1; z_max is the start's 0.29 exactly in both."""
    import sense_loop as SL
    import sense_model as SM

    class _Epoch(SM.SenseModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.epoch[:] = epoch

    old = SL.SM.SenseModel
    SL.SM.SenseModel = _Epoch
    try:
        return SL.cpu_loop_sensed(mode, True, **kw)
    finally:
        SL.SM.SenseModel = old
