"""The episode fleets that tests/test_gpu_episode.py, tests/test_gpu_episode_sense.py and tests/test_gpu_act.py share
(-m gpu) -- TEST SIDE ONLY, no test in here.

B = 96: one full wave and one half wave.  Fleet is test_gpu_episode's workload (its module docstring describes the
pushes of Fleet.push), episodes() / model() / host_check() / check_manager() its device manager, its CPU model and the
host-driven counterpart; Managed adds sensors and the sensor-path manager (test_gpu_episode_sense).

This module is not rewritten by pytest's assertion rewriting, so every assert in here carries its own message.
"""
import os
import re

import numpy as np

import episode_model as EM
import fleet_gpu as G
import plant_loop as L
import plant_loop_field as LF
import plant_loop_varied as LV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 96
SEED = 0x5EED0123456789AB            # the draws'
SEED_N = 0x9E3779B97F4A7C15          # the noise's
DT = 1.0 / L.FREQ
# all six causes: time-out at 40 ticks, tilt cosine 0.8, 0.2 m, 0.06 m from the start
RULE_ALL = dict(causes=EM.ALL, max_ticks=40, cos_tilt_min=0.8, z_min=0.2, range=0.06)
COMMANDS = np.array([[0.3, 0.0, 0.05, 0], [0.0, 0.0, 0.0, 4], [0.5, 0.0, -0.1, 5], [0.2, 0.0, 0.0, 10], [0.02, 0.0, 0.0, 0]])
SENSE_COMMANDS = np.array([[0.1, 0.0, 0.05, 0], [0.25, 0.0, 0.0, 5], [0.4, 0.0, -0.1, 0], [0.5, 0.0, 0.0, 10]])
W3 = 5
_dev, _all = G.dev, G.all_robots


def ctrl_arrays():
    """The names of the controller's per-robot arrays (QMPC_CTRL_ARRAYS of csrc/qmpc_glue.h), in its order."""
    src = open(os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_glue.h")).read()
    body = re.search(r"#define QMPC_CTRL_ARRAYS\(X\)((?:.*\\\n)*.*)", src).group(1)
    return [n for _, n, _ in re.findall(r"X\((\w+), (\w+), (\d+)\)", body)]


CTRL = ctrl_arrays()


def to_np(t):
    return t.cpu().numpy().copy()


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rows_equal(a, b):
    """log rows: exact doubles, a NaN equal to a NaN (the device and numpy may sign a fresh NaN differently)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _key(rows):
    return {(int(r[0]), int(r[1])): r for r in rows}


class Fleet:
    """A controller and a plant for B robots on `ground` ("flat", or "field": plant_loop_field's map at the contact
    rung with all three contact flags), per-robot payloads and floors, statistics on, the commands as device tensors."""

    def __init__(self, schedule, ground):
        import torch
        self.torch = torch
        self.c, self.p, (gait, vel, xyyaw) = G.walk_pair(B, schedule)
        self.xyyaw0 = xyyaw
        self.ground = ground
        self.keep = []
        if ground == "field":
            z, place, cell = LF.field_for(B, LF.RUNGS["contact"])
            self.keep += [_dev(self.c, z), _dev(self.c, place)]
            self.p.set_field(self.keep[0], self.keep[1], cell, clamp_swing=True, rebase_z=True)
            self.p.set_contact(**G.ON)
            self.p.reset(_all(self.c, B), _dev(self.c, xyyaw))
        var = LV.variation(B)
        self.ibody = var["ibody"]
        self.prm = dict(mass=_dev(self.c, var["mass"]), ibody=_dev(self.c, var["ibody"]), mu=_dev(self.c, var["mu"]),
                        force=_dev(self.c, np.zeros((B, 3))), torque=_dev(self.c, np.zeros((B, 3))))
        self.p.set_params(**self.prm)
        self.p.enable_stats()
        self.p.reset_stats()
        self.vel, self.gait = _dev(self.c, vel), _dev(self.c, gait)

    def spawn(self):
        """[B, 3, 3] per robot on the field (each robot stays on its own part of the map), [7, 3] shared on flat ground."""
        if self.ground == "field":
            off = np.array([[0.0, 0.0, 0.0], [0.3, 0.1, 0.2], [-0.2, 0.25, -0.3]])
            return self.xyyaw0[:, None, :] + off[None, :, :]
        k = np.arange(7.0)
        return np.stack([0.4 * k - 1.0, 0.3 * (k % 3), 0.1 * (k - 3)], 1)

    def push(self):
        """The pushes of test_gpu_episode's module docstring, written in place into the bound tensors."""
        k = np.arange(B) % 16 % 4
        force, torque = np.zeros((B, 3)), np.zeros((B, 3))
        torque[k == 0, 0] = 0.15 * self.ibody[k == 0, 0] / DT ** 2
        force[k == 1, 2] = -1500.0
        force[k == 2, 0] = 400.0
        slow = np.arange(B) % 32 == 16
        torque[slow, 0] = 0.006 * self.ibody[slow, 0] / DT ** 2
        mass = to_np(self.prm["mass"])
        mass[5] = np.nan
        for name, val in (("force", force), ("torque", torque), ("mass", mass)):
            self.prm[name].copy_(_dev(self.c, val))

    def ground_rows(self):
        return to_np(self.p.terrain()["ground"]) if self.ground == "field" else np.zeros(B)

    def snapshot(self):
        """Plant view, controller view, effort, contact counters, ground, support and statistics as numpy copies
        (synchronises)."""
        from quadruped_ctrl_amd import binding
        ctrl_keys = tuple(binding.CTRL_VIEW_WIDTH)
        self.torch.cuda.synchronize()
        s = {f"plant.{k}": to_np(v) for k, v in self.p.view().items() if k in G.PLANT_KEYS}
        s.update({f"ctrl.{k}": to_np(v) for k, v in self.c.view().items() if k in ctrl_keys})
        s["effort"] = to_np(self.p.effort)
        s.update({f"contact.{k}": to_np(self.p.contact()[k]) for k in G.CONTACT_KEYS})
        t = self.p.terrain()
        s["ground"], s["support"] = to_np(t["ground"]), to_np(t["support"])
        st = self.p.stats()
        s.update({f"stats.{k}": to_np(st[k]) for k in ("n", "z_min", "z_max", "roll_max", "pitch_max", "vx_sum", "vy_sum")})
        return s

    def close(self):
        self.c.close()


def same(fa, fb, what, vel_b=None, gait_b=None):
    """Two fleets' snapshots, and fleet A's commands against vel_b / gait_b when given: every bit."""
    sa, sb = fa.snapshot(), fb.snapshot()
    assert set(sa) == set(sb), f"{what}: the snapshots' keys differ: {sorted(set(sa) ^ set(sb))}"
    for k in ("ctrl.safe", "ctrl.counter", "plant.stance"):
        assert k in sa, f"{what}: the snapshot lacks {k}"
    for k in sa:
        assert bits(sa[k], sb[k]), (what, k, np.flatnonzero((sa[k] != sb[k]).reshape(B, -1).any(1))[:8])
    if vel_b is not None:
        assert bits(to_np(fa.vel), vel_b), f"{what}: the commanded velocities differ from the model's"
        assert bits(to_np(fa.gait), gait_b), f"{what}: the commanded gaits differ from the model's"
    return sa


def episodes(f, rule, log_rows, commands=True):
    from quadruped_ctrl_amd.binding import BatchedEpisodes
    e = BatchedEpisodes(f.p)
    e.init(SEED)
    f.cmd = _dev(f.c, COMMANDS) if commands else None
    f.spawn_t = _dev(f.c, f.spawn())
    e.set(f.vel, f.gait, f.spawn_t, f.cmd, log_rows=log_rows, **rule)
    return e


def model(f, rule, log_rows, commands=True):
    f.torch.cuda.synchronize()
    m = EM.EpisodeModel(B, SEED, to_np(f.p.view()["p"]))
    m.set(to_np(f.vel), to_np(f.gait), f.spawn(), COMMANDS if commands else None, log_rows=log_rows, **rule)
    return m


def host_check(f, m, elapsed=1):
    """What qmpc_episode_step does, by the host: the views to the host, the model decides and draws, and the calls
    that existed before reset -> the mask."""
    f.torch.cuda.synchronize()
    v = f.p.view()
    mask, xyyaw = m.step(to_np(v["p"]), to_np(v["q"]), to_np(f.c.view()["safe"])[:, 0], f.ground_rows(), elapsed)
    mt = _dev(f.c, mask)
    f.gait.copy_(_dev(f.c, m.gait))
    f.vel.copy_(_dev(f.c, m.vel))
    f.c.reset(mt)
    f.c.set_gait(f.gait)
    f.c.set_vel(f.vel)
    f.p.reset(mt, _dev(f.c, xyyaw))
    f.p.reset_stats(mt)
    return mask.copy()


def check_manager(e, m, what):
    """The manager's state is the model's; the log holds every row that must be there, only rows that may, and the two
    words add up."""
    e.torch.cuda.synchronize()
    v = e.view()
    for k in ("age", "episode", "count", "ticks_sum", "last_cause", "last_ticks"):
        G.equal(to_np(v[k]).reshape(getattr(m, k).shape), getattr(m, k), f"{what}: the manager's {k} against the model's")
    assert bits(to_np(v["start"]), m.start), f"{what}: the manager's start differs from the model's"
    assert bits(to_np(v["xyyaw"]), m.xyyaw), f"{what}: the manager's xyyaw differs from the model's"
    G.equal(to_np(v["mask"]) != 0, m.mask, f"{what}: the manager's mask against the model's")
    lg = e.log()
    n = int(to_np(v["log_count"])[0])
    assert n == len(lg["rows"]) == m.log_count and lg["dropped"] == m.dropped == int(to_np(v["log_dropped"])[0]), \
        (what, n, lg["dropped"], m.log_count, m.dropped)
    assert n + lg["dropped"] == m.total, (what, n, lg["dropped"], m.total)
    got, may, must = _key(lg["rows"]), _key(m.all_rows()), _key(m.certain_rows())
    assert len(got) == n, f"{what}: {n} log rows hold {len(got)} different (robot, episode) keys"
    assert set(must) <= set(got) <= set(may), \
        f"{what}: log rows missing {sorted(set(must) - set(got))[:8]}, rows that cannot be {sorted(set(got) - set(may))[:8]}"
    for k, r in got.items():
        assert rows_equal(r, may[k]), (what, k, r, may[k])
    if not m.dropped:
        assert rows_equal(lg["rows"], m.all_rows()), f"{what}: nothing was dropped and the log is not the model's rows"
    return lg


class Managed:
    """Fleet (flat, or the field with all three contact flags; per-robot payloads, statistics on) with sensors and the
    sensor-path manager."""

    def __init__(self, schedule, ground, W, rule, log_rows):
        from quadruped_ctrl_amd.binding import BatchedEpisodes, BatchedSensors, SensedEpisodes
        self.f = Fleet(schedule, ground)
        self.c, self.p, self.torch = self.f.c, self.f.p, self.f.torch
        self.s = BatchedSensors(self.p)
        self.s.init(SEED_N)
        self.keep = G.sense_bind(self.c, self.s, G.sense_values(B, 11))
        self.f.cmd = _dev(self.c, SENSE_COMMANDS)
        self.f.spawn_t = _dev(self.c, self.f.spawn())
        self.e = BatchedEpisodes(self.p)
        self.e.init(SEED)
        self.e.set(self.f.vel, self.f.gait, self.f.spawn_t, self.f.cmd, log_rows=log_rows, **rule)
        self.se = SensedEpisodes(self.e, self.s)
        self.se.init(W)

    def snapshot(self):
        s = self.f.snapshot()
        s.update({f"read.{k}": self.c.read(k) for k in CTRL})
        s.update(imu=to_np(self.s.imu), motor=to_np(self.s.motor))
        v = self.s.view()
        s["sense.n"], s["sense.epoch"] = to_np(v["n"]), to_np(v["epoch"])
        w = self.se.view()
        s["warm"], s["hold"] = to_np(w["warm"]), to_np(w["hold"])
        return s
