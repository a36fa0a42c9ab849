"""CPU suite for tests/ctrl_cycle_cases.py: the restatement alone (tests/ctrl_model.py fed by estimate_state, as
tests/test_gpu_ctrl_cycle.py feeds it) over the calm and the hard case reaches every branch of qmpc_ctrl_loco_kernel<0>
that the cases promise -- so the GPU comparison on them cannot pass vacuously -- and the suite's 40-tick state-path case
reaches none of them, which is why the cases exist."""
import numpy as np
import pytest

import ctrl_cycle_cases as CC
import ctrl_model as M


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in ("calm", "hard", "existing"):
        case = getattr(CC, name + "_case")()
        trace, m = CC.run_model(case)
        out[name] = (case, trace, CC.coverage(trace))
    return out


def test_cases_are_what_they_say():
    calm, hard = CC.calm_case(), CC.hard_case()
    assert CC.TICKS == 380 == 2 * 14 * 13 + 16 and CC.CYCLE == 182
    assert calm["B"] == 24 and list(calm["gaits_at"]) == [0] and list(calm["vel_at"]) == [0]
    assert np.array_equal(calm["gaits_at"][0], np.r_[0:12, 20:32])              # every gait number and its omni variant
    assert calm["state"].shape == (380, 24, 16) and calm["imu"].shape == (380, 24, 10) and calm["motor"].shape == (380, 24, 24)
    assert hard["B"] == 48 and hard["state"].shape == (380, 48, 16) and "imu" not in hard
    assert sorted(hard["gaits_at"]) == [0, 95, 200] and sorted(hard["vel_at"]) == [0, 250]
    assert np.array_equal(hard["gaits_at"][0], hard["gaits_at"][200])
    g0, g1 = M.split_gait(hard["gaits_at"][0])[0], M.split_gait(hard["gaits_at"][95])[0]
    assert ((g1 == 4) & (g0 != 4)).sum() >= 12 and ((g0 == 4) & (g1 != 4)).sum() >= 2       # into and out of standing
    assert np.array_equal(hard["vel_at"][250][1:], hard["vel_at"][0][:-1])
    # tick 95 is mid-segment (95 % 13 != 0), and the shortest swing of a reachable gait is 4 segments = 52 ticks > 40
    assert 95 % 13 != 0 and min(14 - max(M.GAITS[n][1]) for n in CC.REACHABLE if n != "standing") * 13 == 52
    assert len(CC.REACHABLE) == 9 and "jumping" not in CC.REACHABLE
    for case in (calm, hard):
        assert np.abs(np.linalg.norm(case["state"][..., :4], axis=-1) - 1).max() < 1e-12


def test_calm_case_runs_whole_cycles(runs):
    _, trace, cov = runs["calm"]
    CC.assert_calm_coverage(cov)
    a = trace.arrays()
    names = np.array([M.gait_name(g) for g in a["current_gait"][0]])
    assert (a["swing_state"][:, names == "standing"] == 0).all() and (names == "standing").sum() == 2
    assert (a["counter"][-1] == 380).all()
    assert cov["liftoffs"] > 0 and cov["touchdowns"] > 0
    # the calm case stays inside every clamp: the hard case is the one that reaches them
    for k in CC.COUNTERS[2:]:
        assert cov[k] == 0, (k, cov[k])


def test_hard_case_reaches_every_branch(runs):
    _, trace, cov = runs["hard"]
    CC.assert_hard_coverage(cov)
    a = trace.arrays()
    # the gates of the two integrals are straddled: some robots integrate, some never do
    moved = (a["rpy_int"] != 0).any(0)
    assert moved[:, 0].any() and not moved[:, 0].all() and moved[:, 1].any() and not moved[:, 1].all()
    # the re-anchor robots, once each, after yaw_des_true has climbed from 0 past 1.9
    ydt = np.concatenate([np.zeros((1, 48), np.float32), a["yaw_des_true"][:-1]])
    t, b = np.nonzero(np.abs(a["yaw"] - ydt).astype(np.float64) > 5.0)
    assert sorted(b) == list(range(5, 48, 6)) and t.min() > 100 and (ydt[t, b] > 1.89).all()
    # standing is entered and left mid-run
    gn = a["current_gait"]
    assert ((gn[94] != 4) & (gn[95] == 4)).any() and ((gn[94] == 4) & (gn[95] != 4)).any()
    assert ((gn[199] == 4) & (gn[200] != 4)).any()
    assert (a["swing_state"][gn == 4] == 0).all()
    print({k: cov[k] for k in CC.COUNTERS}, "complete swings", cov["complete_swings"])


def test_the_40_tick_case_reaches_none_of_it(runs):
    """The zero rows of the table in this pull request's reason: 257 robots, 40 ticks, seed 257, switch at 20."""
    _, _, cov = runs["existing"]
    assert (cov["wraps"] == 0).all()
    assert all(v == 0 for v in cov["complete_swings"].values())
    for n in ("bounding", "pronking", "walking", "walking2", "trotRunning"):
        assert cov["natural_liftoffs"][n] == 0, n
    for k in CC.COUNTERS[2:]:                     # the clamps and the re-anchor
        assert cov[k] == 0, (k, cov[k])
    assert (cov["safe"] == 1).all() and cov["finite"]


def test_coverage_counts_a_hand_made_trace():
    """coverage() on six ticks of one robot written by hand: foot 0 lifts off on tick 1 and touches down on tick 3 (one
    complete swing); foot 1 lifts off on tick 2, the gait command changes on tick 4 and the foot touches down there (not
    natural, not complete)."""
    tr = CC.Trace()
    z = lambda *s: np.zeros(s, np.float32)
    fs = [[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    for t in range(6):
        rows = dict(counter=np.array([181 + t + 1]), gait_num=np.array([9 if t < 4 else 4]), current_gait=np.array([9 if t < 4 else 4]),
                    first_swing=np.array([fs[t]]), swing_state=(np.array([fs[t]]) == 0).astype(np.float32), rpy_int=z(1, 2),
                    vel_des=z(1, 3), pf_rel=z(1, 8), yaw_des_true=z(1), safe=np.array([1]), yaw=z(1), finite=True)
        rows["vel_des"][0, 0] = 2.0 if t == 5 else 1.0
        rows["pf_rel"][0, 3] = -0.3
        rows["yaw"][0] = 5.5 if t == 2 else 0.0
        for k, v in rows.items():
            tr.rows[k].append(v)
    cov = CC.coverage(tr)
    assert cov["wraps"].tolist() == [1] and cov["liftoffs"] == 2 and cov["touchdowns"] == 2
    assert cov["natural_liftoffs"]["trotting"] == 2 and cov["natural_touchdowns"]["trotting"] == 1
    assert cov["natural_touchdowns"]["standing"] == 0 and cov["complete_swings"]["trotting"] == 1
    assert cov["vel_x_hi"] == 1 and cov["vel_x_lo"] == 0 and cov["pf_rel_lo"] == 6 and cov["pf_rel_hi"] == 0
    assert cov["reanchors"] == 1 and cov["swinging"]["trotting"] == 4 and cov["finite"]
