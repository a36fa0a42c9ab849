"""CPU suite for episodes on the sensor path (include/qmpc_episode_sense.h): the exported surface, the bookkeeping of the
numpy restatement tests/episode_sense_model.py -- the model the GPU suite (tests/test_gpu_episode_sense.py) holds the
kernels to --, the one list behind the controller's full and partial re-initialisation, and the compiled kernels'
resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import episode_model as EM
import episode_sense_model as ESM
from c_headers import declared, members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
no_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")

# the pre_work set of include/qmpc_episode_sense.h: what a held robot keeps
KEPT = {"q", "qd", "leg_J", "leg_p", "leg_v", "kf_p", "kf_v", "orientation", "rpy", "r_body", "omega_body", "omega_world",
        "a_world", "ori_ini_inv", "xhat", "P", "position", "v_world", "v_body", "first_visit"}


def test_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_episode_sense.h")).read()
    want = {"qmpc_episode_sense_init", "qmpc_episode_sense_hold", "qmpc_episode_sense_step", "qmpc_episode_sense_view_get"}
    assert declared("qmpc_episode_sense.h") == want == set(binding.EPISODE_SENSE_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    assert members(hdr, "qmpc_episode_sense_view") == [n for n, _ in binding.EpisodeSenseView._fields_]
    # the two headers this one stands on still declare exactly what they declared
    assert declared("qmpc_episode.h") == set(binding.EPISODE_EXPORTS) and declared("qmpc_sense.h") == set(binding.SENSE_EXPORTS)
    # without a device every entry point refuses a null handle
    assert lib.qmpc_episode_sense_init(None, 4, 5, None) == 1 and lib.qmpc_episode_sense_hold(None, 4, None, 5, None) == 1
    assert lib.qmpc_episode_sense_step(None, 4, None, None) == 1 and lib.qmpc_episode_sense_view_get(None, None) == 1
    # the Python layer
    assert callable(binding.rollout_sensed_episodes) and {"init", "hold", "step", "view"} <= set(dir(binding.SensedEpisodes))


# ---- the model's bookkeeping --------------------------------------------------------------------------------------------

B = 6
P0 = np.tile([0.0, 0.0, 0.29], (B, 1)) + np.arange(B)[:, None] * [1.0, 0.0, 0.0]
Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
SPAWN = np.arange(21.0).reshape(7, 3)
CMDS = np.array([[0.1, 0, 0, 9], [0.2, 0, 0, 5], [0.3, 0, 0, 4]])
RULE = dict(causes=EM.ALL, max_ticks=50, cos_tilt_min=0.5, z_min=0.1, range=100.0)


def _model(W, log_rows=100, cls=None, **rule):
    m = ESM.EpisodeSenseModel(B, 7, P0, W) if cls is None else cls(B, 7, P0)
    m.set(np.zeros((B, 3)), np.full(B, 9, np.int32), SPAWN, CMDS, log_rows=log_rows, **dict(RULE, **rule))
    return m


def test_model_holds_a_done_robot_exactly_w_steps():
    """Robot 2 latches at step 3 (its safe flag reads 0 once): it is reset there, held for exactly W steps with age 0, no
    log row and no counter moving, and judged again at step 3 + W + 1, where its age is 1."""
    for W in (1, 4):
        m = _model(W)
        safe = np.ones(B, int)
        hist = []
        for t in range(1, 3 + W + 3):
            safe[2] = 0 if t == 3 else 1
            mask, hold, _ = m.step(P0, Q0, safe)
            hist.append((mask[2], hold[2], int(m.age[2]), int(m.warm[2]), m.total, int(m.count.sum())))
            assert not mask[[0, 1, 3, 4, 5]].any() and not hold[[0, 1, 3, 4, 5]].any() and (m.age[[0, 1]] == t).all()
        assert hist[1][:3] == (False, False, 2)
        assert hist[2] == (True, False, 0, W, 1, 1)                                   # reset at step 3, warm-up ahead
        for k in range(W):                                                            # held: nothing moves but warm
            assert hist[3 + k] == (False, True, 0, W - 1 - k, 1, 1), (W, k, hist)
        assert hist[3 + W] == (False, False, 1, 0, 1, 1) and hist[4 + W][2] == 2      # first judged step: age 1
        assert m.episode.tolist() == [0, 0, 1, 0, 0, 0] and m.last_ticks[2] == 3 and m.last_cause[2] == EM.UNSAFE


def test_model_does_not_judge_a_held_robot():
    """A held robot that is latched and whose pose is not finite is not done while it is held."""
    m = _model(3)
    m.hold_robots(np.arange(B) == 1, 5)
    p = P0.copy()
    p[1] = np.nan
    safe = np.ones(B, int)
    safe[1] = 0
    for t in range(1, 6):
        mask, hold, _ = m.step(p, Q0, safe)
        assert hold.tolist() == [False, True, False, False, False, False] and not mask[1] and m.age[1] == 0
        assert not mask.any() and m.count.sum() == 0 and (m.age[[0, 2]] == t).all()
        assert all(r[0] != 1.0 for r in m.rows)
    mask, hold, _ = m.step(p, Q0, safe)                    # the hold is over: judged, and done on the spot
    assert mask[1] and not hold[1] and m.last_ticks[1] == 1 and m.last_cause[1] == EM.UNSAFE | EM.NONFINITE
    assert m.warm[1] == 3


def test_model_w0_is_the_plain_manager():
    """warm_ticks = 0: every array, the log and the masks are EpisodeModel's, step by step."""
    a, b = _model(0, log_rows=5, max_ticks=4), _model(None, log_rows=5, cls=EM.EpisodeModel, max_ticks=4)
    rng = np.random.default_rng(3)
    for t in range(30):
        safe = (rng.uniform(size=B) > 0.2).astype(int)
        p = P0 + rng.uniform(-0.3, 0.3, (B, 3))
        ma, hold, xa = a.step(p, Q0, safe)
        mb, xb = b.step(p, Q0, safe)
        assert np.array_equal(ma, mb) and not hold.any() and not a.warm.any() and np.array_equal(xa, xb)
        for k in ("age", "episode", "start", "count", "ticks_sum", "last_cause", "last_ticks", "vel", "gait"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (t, k)
    assert a.rows == b.rows and a.total > 20 and a.dropped == b.dropped > 0


def test_model_hold_on_a_fresh_fleet_and_with_the_manager_off():
    """hold() on a fresh fleet holds everybody warm_ticks steps; with causes == 0 nobody is judged but holds are processed."""
    for causes in (EM.ALL, 0):
        m = _model(4, causes=causes, max_ticks=3)
        xy = P0 * [1.0, 1.0, 0.0] + [0.0, 0.0, 0.25]
        m.hold_robots(xyyaw=xy)
        assert np.array_equal(m.xyyaw, xy) and np.array_equal(m.start, xy[:, :2])
        for t in range(4):
            mask, hold, _ = m.step(P0, Q0, np.ones(B, int))
            assert hold.all() and not mask.any() and (m.age == 0).all() and (m.warm == 3 - t).all()
        for t in range(3):
            mask, hold, _ = m.step(P0, Q0, np.ones(B, int))
            assert not hold.any() and mask.all() == (causes != 0 and t == 2)
        assert (m.age == 0).all() and (m.warm == (4 if causes else 0)).all() and m.total == (B if causes else 0)
    m.hold_robots(np.arange(B) < 2, 2)                     # explicit ticks, a subset
    assert m.warm.tolist() == [2, 2, 0, 0, 0, 0]


# ---- one list behind the full and the partial re-initialisation ---------------------------------------------------------

def test_kept_and_reinitialised_sets_partition_the_array_list():
    """qmpc_ctrl_init_robot<FULL> (csrc/qmpc_glue.h) writes every array of QMPC_CTRL_ARRAYS exactly once: the pre_work set
    inside its `if constexpr (FULL)` block, everything else behind it -- nothing missing, nothing twice, and the kept set
    is the header's.  Its three users call it and hold no list of their own."""
    src = open(os.path.join(CSRC, "qmpc_glue.h")).read()
    body = re.search(r"#define QMPC_CTRL_ARRAYS\(X\)((?:.*\\\n)*.*)", src).group(1)
    arrays = [n for _, n, _ in re.findall(r"X\((\w+), (\w+), (\d+)\)", body)]
    assert len(arrays) == len(set(arrays)) > 50
    fn = re.search(r"template <bool FULL>\n__device__ __forceinline__ void qmpc_ctrl_init_robot\(.*?\n}\n", src, re.S).group(0)
    head, rest = fn.split("if constexpr (FULL) {", 1)
    kept_text, else_text = rest.split("\n  }\n  // everything else\n", 1)
    assert "S." not in head
    kept, other = re.findall(r"\bS\.(\w+)\[", kept_text), re.findall(r"\bS\.(\w+)\[", else_text)
    assert len(kept) == len(set(kept)) and len(other) == len(set(other))
    assert set(kept) == KEPT and not set(kept) & set(other)
    assert sorted(kept + other) == sorted(arrays)
    # the header names the same set
    hdr = open(os.path.join(ROOT, "include", "qmpc_episode_sense.h")).read()
    listed = re.search(r"which is kept: (.*?)\.\s+Everything else", hdr, re.S).group(1)
    assert set(re.findall(r"\w+", listed.replace("*", " "))) == KEPT
    # the users
    glue = open(os.path.join(CSRC, "qmpc_glue.hip")).read()
    sense = open(os.path.join(CSRC, "qmpc_episode_sense.hip")).read()
    assert glue.count("qmpc_ctrl_init_robot<true>(") == 1 and "S.P[" not in re.search(
        r"void qmpc_ctrl_init_kernel\(.*?\n}\n", glue, re.S).group(0)
    assert sense.count("qmpc_ctrl_init_robot<true>(") == 1 and sense.count("qmpc_ctrl_init_robot<false>(") == 1
    # the hold kernel recovers a yaw for the expression all three of the plant's reset kernels build q with
    for f in ("qmpc_plant.hip", "qmpc_terrain.hip", "qmpc_field.hip"):
        assert open(os.path.join(CSRC, f)).read().count("const double q[4] = {cos(yaw / 2), 0.0, 0.0, sin(yaw / 2)};") == 1, f
    assert "cos(c / 2) == qw && sin(c / 2) == qz" in sense
    # the decision is one text for both managers
    for f in ("qmpc_episode.hip", "qmpc_episode_sense.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert text.count('#include "qmpc_episode_decide_body.h"') == 1 and "qmpc_episode_cause(" not in text, f


# ---- the kernels --------------------------------------------------------------------------------------------------------

@no_hipcc
def test_episode_sense_kernel_resources(tmp_path):
    """The decision, the re-initialisation, the hold and the init kernel compile for gfx950, with the build's own flags,
    without scratch and without LDS."""
    src = os.path.join(CSRC, "qmpc_episode_sense.hip")
    import __graft_entry__ as G                     # the flags the shipped object is compiled with
    assert "qmpc_episode_sense.hip" in G.OTHER_SOURCES
    out = subprocess.run([HIPCC] + G.HIPFLAGS + ["-c", src, "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "es.o")],
                         capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    kernels = ("qmpc_episode_sense_decide_kernel", "qmpc_episode_sense_reinit_kernel", "qmpc_episode_sense_hold_kernel",
               "qmpc_episode_sense_init_kernel")
    assert len(res) == 4 and all(any(k in n for n in res) for k in kernels), sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
