"""The inputs of the error-exit suite (tests/error_cases.py), pinned without a device.

Every kind changes only its robot's rows and leaves a well-formed record; the placement poisons at most half of a batch
per call, robot 0 and robot B-1 in some call, every kind, and in the mixed family a robot of each size class; the two
finite kinds are what they claim to be in the fp64 model (H_red = 0; a negative first pivot and a negative eigenvalue for
every robot of every record); f_max = -5 makes the reference's qpOASES report a trot robot's reduced QP infeasible, which
the record's own f_max does not; the family table names every engine family of the iteration-cap suite."""
import functools

import numpy as np
import pytest

import cap_judge as J
import error_cases as E
from oracle import oracle as O

RECORD_KEYS = sorted({J_key for J_key in J.RECORDS} | {v[0] for v in E.MORE_FAMILIES.values()})


@functools.lru_cache(maxsize=None)
def record(key):
    return E.record_of(key)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _only_row_differs(clean, bad, i, fields, where):
    B = int(clean["batch"])
    assert set(bad) == set(clean), where
    for k, v in clean.items():
        w = bad[k]
        if not isinstance(v, np.ndarray):
            assert type(w) is type(v) and w == v, (where, k)
            continue
        assert w.dtype == v.dtype and w.shape == v.shape and w.flags["C_CONTIGUOUS"], (where, k)
        if k not in fields:
            assert _same(v, w), (where, k)
            continue
        assert v.shape[0] == B
        others = np.arange(B) != i
        assert _same(np.ascontiguousarray(v[others]), np.ascontiguousarray(w[others])), (where, k, "another robot's row")
    assert any(not _same(clean[k][i], bad[k][i]) for k in fields), (where, "nothing changed")


@pytest.mark.parametrize("key", RECORD_KEYS)
def test_record_kinds_change_one_robot(key):
    b = record(key)
    before = E.copy(b)
    B = int(b["batch"])
    for kind, (fields, _) in E.RECORD_KINDS.items():
        for i in (0, B // 2, B - 1):
            bad = E.poisoned(b, {i: kind}, E.RECORD_KINDS)
            _only_row_differs(b, bad, i, fields, (key, kind, i))
            finite = all(np.isfinite(bad[f][i]).all() for f in fields)
            assert finite == (kind in E.FINITE_KINDS), (key, kind)
            if kind not in E.FINITE_KINDS:         # one entry, one field
                assert sum(int((~np.isfinite(bad[f])).sum()) for f in fields) == 1, (key, kind)
    assert all(_same(v, before[k]) for k, v in b.items() if isinstance(v, np.ndarray)), "the record itself was written"
    # the traj kind lies in the last horizon step
    bad = E.poisoned(b, {0: "nan_traj_last"}, E.RECORD_KINDS)
    at = np.flatnonzero(np.isnan(bad["traj"][0]))
    assert at.size == 1 and at[0] // 12 == int(b["horizon"]) - 1


@pytest.mark.parametrize("name", list(E.FUSED_FAMILIES))
def test_command_kinds_change_one_robot(name):
    cmd = E.commands_of(name)
    B = int(cmd["batch"])
    assert B == E.FUSED_BATCH and int(cmd["horizon"]) == E.FUSED_FAMILIES[name]
    for kind, (fields, _) in E.COMMAND_KINDS.items():
        for i in (0, 7, B - 1):
            bad = E.poisoned(cmd, {i: kind}, E.COMMAND_KINDS)
            _only_row_differs(cmd, bad, i, fields, (name, kind, i))
            assert sum(int(np.isnan(bad[f]).sum()) for f in fields) == 1
    sw = E.copy(cmd)
    E.all_swing(sw, 3, command=True)
    _only_row_differs(cmd, sw, 3, ("gait_durations", "gait_type"), (name, "all swing"))
    for it in range(E.FUSED_FAMILIES[name]):       # ... and the table the packer builds from it is empty at every phase
        assert not np.any(O.mpc_table(E.FUSED_FAMILIES[name], sw["gait_offsets"][3], sw["gait_durations"][3], it))


def _size_class(b, i):
    """64-row class: n_r = 3 x stance foot-steps <= 64 (include/qmpc.h, qmpc_set_max_stance)."""
    return 64 if 3 * int(np.count_nonzero(b["gait"][i])) <= 64 else 96


def test_placement():
    sizes = {name: int(record(J.FAMILIES[name][0])["batch"]) for name in E.ENGINE_FAMILIES}
    sizes.update({name: int(record(v[0])["batch"]) for name, v in E.MORE_FAMILIES.items()})
    sizes.update({name: E.FUSED_BATCH for name in E.FUSED_FAMILIES})
    assert min(sizes.values()) == 4 and max(sizes.values()) == 48
    for name, B in sizes.items():
        fused = name in E.FUSED_FAMILIES
        kinds = list(E.COMMAND_KINDS) if fused else E.record_kinds(name)
        calls = E.plans(B, kinds, E.command_allowed(E.commands_of(name)) if fused else None)
        assert len(calls) >= 2
        hit = set()
        for plan in calls:
            assert 0 < len(plan) <= B // 2 and all(0 <= i < B for i in plan), name
            hit |= set(plan)
        assert {0, B - 1} <= hit, name
        assert {k for plan in calls for k in plan.values()} == set(kinds), name
    assert "nan_x_drag" not in E.record_kinds("sparse_mixed") and "nan_x_drag" in E.record_kinds("mixed")
    # the mixed families: a robot of each size class is poisoned in some call (and both classes exist)
    for key in ("mixed", "mixed_sparse"):
        b = record(key)
        B = int(b["batch"])
        classes = {_size_class(b, i) for i in range(B)}
        assert classes == {64, 96}
        assert {_size_class(b, i) for plan in E.plans(B, E.record_kinds("mixed")) for i in plan} == classes


@pytest.mark.parametrize("name", list(E.FUSED_FAMILIES))
def test_command_kinds_reach_the_record(name):
    """Every poisoned robot of the fused families' calls gets a non-finite record from the packer (oracle_pack_command, the
    C restatement of ConvexMPCLocomotion.cpp:498-640): the kind sits on a robot whose solve reads the field.  A standing
    robot's record does not depend on vel_des, r_body or world_position_desired at all."""
    cmd = E.commands_of(name)
    B, dt = int(cmd["batch"]), 0.026
    fields = ("p", "v", "q", "w", "r", "yaw", "traj", "x_drag")
    clean = O.pack_commands(cmd, dt)[0]
    stands = np.flatnonzero(cmd["gait_type"] == 4)
    assert 0 < stands.size < B
    for plan in E.plans(B, list(E.COMMAND_KINDS), E.command_allowed(cmd)):
        rec = O.pack_commands(E.poisoned(cmd, plan, E.COMMAND_KINDS), dt)[0]
        for i in range(B):
            finite = all(np.isfinite(rec[f][i]).all() for f in fields)
            assert finite == (i not in plan), (name, i, plan.get(i))
            if i not in plan:
                assert all(_same(rec[f][i], clean[f][i]) for f in fields + ("gait", "weights", "alpha")), (name, i)
    for kind in E.WALKING_ONLY:
        rec = O.pack_commands(E.poisoned(cmd, {int(stands[0]): kind}, E.COMMAND_KINDS), dt)[0]
        assert all(_same(rec[f], clean[f]) for f in fields), (name, kind, "a standing robot's record read the field")


def test_family_table_names_every_engine_family():
    assert set(E.ENGINE_FAMILIES) == set(J.FAMILIES) and len(E.ENGINE_FAMILIES) == len(J.FAMILIES)
    assert all(v[0] in RECORD_KEYS for v in E.MORE_FAMILIES.values())
    assert not (set(E.ENGINE_FAMILIES) & set(E.MORE_FAMILIES)) and not (set(E.MORE_FAMILIES) & set(E.FUSED_FAMILIES))
    assert E.ST_ERROR_MASK == 47 and E.iters_bound("trot", 10) == 1200 and E.iters_bound("jcqp1_trot", 10) == 10000


@pytest.mark.parametrize("key", RECORD_KEYS)
def test_not_pd_kinds_in_the_fp64_model(key):
    b = record(key)
    B = int(b["batch"])
    zero = E.poisoned(b, {i: "zero_hessian" for i in range(B)}, E.RECORD_KINDS)
    neg = E.poisoned(b, {i: "negative_alpha" for i in range(B)}, E.RECORD_KINDS)
    flat = E.copy(b)
    flat["alpha"][:] = 0.0
    s00, pivots, eigs = [], [], []
    for i in range(B):
        H0, _ = J.model_qp(zero, i)
        assert H0.size and not H0.any(), (key, i, "H is not zero")
        s00.append(J.model_qp(flat, i)[0][0, 0] / 2)
        Hn, _ = J.model_qp(neg, i)
        pivots.append(Hn[0, 0])
        eigs.append(np.linalg.eigvalsh(Hn)[0])
        # the clean robot is positive definite: the kind is what makes the difference
        assert np.linalg.eigvalsh(J.model_qp(b, i)[0])[0] > 0, (key, i)
    print(f"{key}: S_00 {min(s00):.2e} .. {max(s00):.2e}, first pivot with alpha = {E.NEG_ALPHA}: at most {max(pivots):.3f}, "
          f"smallest eigenvalue at most {max(eigs):.3f}")
    assert 0 < min(s00) and max(s00) < 0.1 <= -E.NEG_ALPHA / 10           # how NEG_ALPHA was chosen (error_cases.py)
    assert max(pivots) < -1.0 and max(eigs) < -1.0, (key, max(pivots), max(eigs))
    assert float(np.float32(E.NEG_ALPHA)) == E.NEG_ALPHA


def test_not_pd_kinds_in_the_sparse_model():
    """The sparse family's own Hessian (oracle/sparse_model.condensed) under the same two kinds."""
    from oracle import sparse_model as SM
    b = record("mixed_sparse")
    B = int(b["batch"])
    for kind in E.FINITE_KINDS:
        bad = E.poisoned(b, {i: kind for i in range(B)}, E.RECORD_KINDS)
        for i in range(B):
            w, a = bad["weights"][i].astype(np.float64), float(bad["alpha"][i])
            prob = SM.from_batch(bad, i, weights=w, alpha=a, mu=bad["mu"], f_max=bad["f_max"])
            H, _ = SM.condensed(prob, weights=w, alpha=a, traj=bad["traj"][i].reshape(-1, 12))
            if kind == "zero_hessian":
                assert not H.any(), i
            else:
                assert H[0, 0] < 0 and np.linalg.eigvalsh(H)[0] < 0, (i, H[0, 0])


def _reduced_qp(b, i):
    Hf, gf, A, lb, ub, _ = O.assemble(b, i)
    _, Hr, gr, Ar, lr, ur = O.reduce(Hf, gf, A, lb, ub)
    return Hr, gr, Ar, lr, ur


def test_negative_f_max_is_infeasible_for_the_reference():
    b = E.copy(record("trot"))
    for i in (0, int(b["batch"]) - 1):
        x, _, _, rc, irc = O.qpoases(*_reduced_qp(b, i), nwsr=100000)
        assert rc == 0 and irc == 0, (i, rc, irc)
        n = x.size
        assert n == 60                              # 20 stance foot-steps: 20 box rows + two friction rows fit 32 slots
    bad = E.copy(b)
    bad["f_max"] = E.F_MAX_INFEASIBLE
    for i in (0, int(b["batch"]) - 1):
        _, _, _, rc, irc = O.qpoases(*_reduced_qp(bad, i), nwsr=100000)
        assert rc != 0 or irc != 0, (i, "qpOASES solved a QP whose box 0 <= fz <= -5 is empty")
    # the box is empty for every stance foot-step: friction rows give fz >= 0, the f_max row fz <= -5
    _, _, Ar, lr, ur = _reduced_qp(bad, 0)
    assert (ur[4::5] == np.float32(E.F_MAX_INFEASIBLE)).all() and (lr == 0).all()
    sw = E.copy(b)
    E.all_swing(sw, 2)
    assert not sw["gait"][2].any() and sw["gait"][1].any()


@pytest.mark.parametrize("key,robots", [("trot", (0, 5, 23)), ("mixed", (0, 1, 4)), ("standing_h10", (0, 5))])
def test_the_method_needs_a_full_working_set_to_tell(key, robots):
    """Why every engine but the last hands an f_max = -5 robot on, and why a robot beyond the last engine's slots ends
    QMPC_ST_WS_FULL (include/qmpc.h): the fp64 model of the iteration, same selection and same dependence test, does
    find the rows inconsistent -- after its working set has held more rows than the first engine has slots (32 in the
    64-row class, 64 in the 96- and 128-row classes), n_r or nearly n_r of them.  It is the method, not an engine's
    dependence test, that takes that long."""
    b = E.copy(record(key))
    b["f_max"] = E.F_MAX_INFEASIBLE
    for i in robots:
        H, g = J.model_qp(b, i)
        n = g.size
        out = E.gi_until_infeasible(b, i, H, g)
        assert out is not None, (key, i, "the model never found the rows inconsistent")
        iters, most, at_end = out
        print(f"{key} robot {i}: n_r {n}, inconsistent after {iters} iterations, working set up to {most} rows, {at_end} at the end")
        assert most > (32 if n <= 64 else 64) and most >= 0.9 * n and most <= n, (key, i, n, most)
        assert iters < 1000 + 20 * int(b["horizon"])


def test_small_table_is_decided_within_the_smallest_engine():
    b = E.copy(record("trot"))
    E.small_table(b, 3)
    E.all_swing(b, 4)
    assert int(b["gait"][3].sum()) == 6 and b["gait"][3][:4].tolist() == [1, 0, 0, 1]
    b["f_max"] = E.F_MAX_INFEASIBLE
    H, g = J.model_qp(b, 3)
    assert g.size == 18 < E.SMALL_ROWS
    iters, most, _ = E.gi_until_infeasible(b, 3, H, g)
    assert most <= g.size
    for name in E.FUSED_FAMILIES:
        cmd = E.commands_of(name)
        E.small_table(cmd, 3, command=True)
        gait = O.pack_commands(cmd, 0.026)[0]["gait"]
        assert 3 * int(gait[3].sum()) == 12 < E.SMALL_ROWS
