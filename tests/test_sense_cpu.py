"""CPU suite for the sensor model (include/qmpc_sense.h): the exported surface, the generator of the numpy restatement
tests/sense_model.py -- the model the GPU suite (tests/test_gpu_sense.py) holds the kernel to bit for bit -- on its
known answers and its statistics, the CPU closed loop through the estimators that the GPU walk is measured by, and the
compiled kernels' scratch."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import plant_loop as L
import sense_loop as SL
import sense_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_sense_symbols_exported_and_abi_version_kept():
    from quadruped_ctrl_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "qmpc_sense.h")).read()
    decl = set(re.findall(r"^int (qmpc_\w+)\(", hdr, re.M))
    want = {"qmpc_sense_init", "qmpc_sense_set_params", "qmpc_sense_reset", "qmpc_sense", "qmpc_sense_view_get"}
    assert decl == want == set(binding.SENSE_EXPORTS)
    for name in want:
        assert hasattr(lib, name), name
    assert lib.qmpc_abi_version() == binding.ABI_VERSION == 23
    # the structures of the binding follow the header's member order
    for struct, cls in (("qmpc_sense_params", binding.SenseParams), ("qmpc_sense_view", binding.SenseView)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+);", body) == [n for n, _ in cls._fields_], struct
    assert list(SM.PARAMS) == list(binding.SENSE_PARAM_FIELDS) and SM.PARAMS == binding.SENSE_PARAM_FIELDS
    # none of the new symbols went into an older header or list
    older = set(binding.EXPORTS) | set(binding.CTRL_EXPORTS) | set(binding.PLANT_EXPORTS) | set(binding.PLANT_VARY_EXPORTS)
    assert not older & want
    for h in ("qmpc.h", "qmpc_ctrl.h", "qmpc_plant.h", "qmpc_plant_vary.h"):
        assert "qmpc_sense" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S), h


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10.  The second vector's third word is a20bc7c6: the feature
    request quoted it from memory as a20bc7c9; the restatement -- written from the round function alone -- gives c6, as
    Random123's kat_vectors file does, and reproduces the other eleven words of the three vectors as quoted."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        w = SM.philox4x32_10(*ctr, *key)
        assert " ".join("%08x" % int(x) for x in w) == want
    # vectorised over counters: the same words as one call at a time
    c = np.arange(5, dtype=np.int64)
    w = SM.philox4x32_10(c, 7, c * 3, 1, 0xDEADBEEF, 42)
    for i in range(5):
        one = SM.philox4x32_10(int(c[i]), 7, int(c[i]) * 3, 1, 0xDEADBEEF, 42)
        assert [int(x[i]) for x in w] == [int(x) for x in one]


def _grid(N, seed):
    """N variates over robots x readings x all 30 channels x 2 epochs."""
    i = np.arange(N, dtype=np.int64)
    ch, rest = i % SM.N_CHANNELS, i // SM.N_CHANNELS
    return SM.z_of(seed, rest % 64, rest // 128, ch, (rest // 64) % 2)


def test_z_is_centred_with_unit_variance_and_bounded():
    """N = 2^18 variates.  The mean of N unit-variance variates has standard deviation 1 / sqrt(N): the bound is five of
    them.  Their sample variance has standard deviation sqrt((2 + excess) / N) = sqrt(2 / N) sqrt(1 + excess / 2) with the
    Irwin-Hall excess kurtosis -6 / (5 * 4) = -0.3; the bound is 5 sqrt(2 / N) (1 + excess / 2), which is 4.6 of those
    (1 + x / 2 < sqrt(1 + x) for negative x: the tighter of the two readings).  |z| <= 2 sqrt(3) always: the sum of four
    words is at most 4 (2^32 - 1)."""
    N = 1 << 18
    for seed in (0, 0x0123456789ABCDEF):
        z = _grid(N, seed)
        mean, var = float(z.mean()), float(z.var())
        print(f"seed {seed:#x}: mean {mean:.3e} (bound {5 / np.sqrt(N):.3e}), variance - 1 {var - 1:.3e} "
              f"(bound {5 * np.sqrt(2 / N) * (1 + SM.Z_EXCESS_KURTOSIS / 2):.3e}), max |z| {np.abs(z).max():.4f}")
        assert abs(mean) < 5 / np.sqrt(N)
        assert abs(var - 1) < 5 * np.sqrt(2 / N) * (1 + SM.Z_EXCESS_KURTOSIS / 2)
        assert np.abs(z).max() <= SM.Z_MAX
        # the shape is the Irwin-Hall's, not a Gaussian's or a uniform's: excess kurtosis -0.3 (standard error sqrt(24 / N))
        kurt = float(((z - mean) ** 4).mean() / var ** 2 - 3)
        assert abs(kurt - SM.Z_EXCESS_KURTOSIS) < 5 * np.sqrt(24 / N)
    # the extreme sums are reached by the formula: all-zero and all-ones words
    lo = (np.float64(0) - SM.Z_CENTRE) * SM.Z_SCALE
    hi = (np.float64(4 * 0xFFFFFFFF) - SM.Z_CENTRE) * SM.Z_SCALE
    assert lo == -hi and hi <= SM.Z_MAX and hi > SM.Z_MAX * (1 - 1e-9)
    # the seed's two words are both in the key
    a, b, c = SM.z_of(1, 0, 0, 0, 0), SM.z_of(1 + (1 << 32), 0, 0, 0, 0), SM.z_of(2, 0, 0, 0, 0)
    assert a != b and a != c and b != c


def test_channels_robots_readings_and_epochs_are_uncorrelated():
    """Sample correlation of two independent unit-variance streams of N values: standard deviation 1 / sqrt(N); the bound is
    5 / sqrt(N) for every pair -- the 435 pairs of a robot's 30 channels, the 120 pairs of 16 robots on one channel, the
    two epochs of a channel, and a channel against itself one reading later."""
    N = 1 << 14
    n = np.arange(N, dtype=np.int64)[:, None]
    bound = 5 / np.sqrt(N)

    def worst(z):
        c = np.corrcoef(z.T)
        return float(np.abs(c - np.eye(len(c))).max())

    ch = worst(SM.z_of(0, 3, n, np.arange(SM.N_CHANNELS)[None, :], 0))
    rb = worst(SM.z_of(0, np.arange(16)[None, :], n, 5, 0))
    ep = worst(SM.z_of(0, 3, n, 5, np.arange(2)[None, :]))
    z = SM.z_of(0, 3, np.arange(N + 1, dtype=np.int64), 5, 0)
    lag = abs(float(np.corrcoef(z[:-1], z[1:])[0, 1]))
    print(f"largest |correlation|: channels {ch:.4f}, robots {rb:.4f}, epochs {ep:.4f}, lag 1 {lag:.4f}; bound {bound:.4f}")
    assert ch < bound and rb < bound and ep < bound and lag < bound


def test_model_terms_are_absent_when_not_bound():
    B = 5
    rng = np.random.default_rng(3)
    state, motor = rng.uniform(-1, 1, (B, 16)), rng.uniform(-1, 1, (B, 24))
    m = SM.SenseModel(B, 9)
    imu, out = m.sense(state, motor)
    assert np.array_equal(imu, np.concatenate([state[:, 13:16], state[:, 1:4], state[:, 0:1], state[:, 7:10]], 1))
    assert np.array_equal(out, motor) and (m.n == 1).all() and (m.epoch == 0).all()
    # one sigma bound: only its group moves, by sigma z of the robot's own counter
    sg = rng.uniform(0.01, 0.1, B)
    m.set_params(gyro_sigma=sg)
    m.reset(np.array([0, 1, 0, 0, 1]))
    assert list(m.n) == [1, 0, 1, 1, 0] and list(m.epoch) == [0, 1, 0, 0, 1]
    imu2, out2 = m.sense(state, motor)
    assert np.array_equal(out2, motor) and np.array_equal(imu2[:, :7], imu[:, :7])
    z = SM.z_of(9, np.arange(B)[:, None], np.array([1, 0, 1, 1, 0])[:, None], 3 + np.arange(3)[None, :],
                np.array([0, 1, 0, 0, 1])[:, None])
    assert np.array_equal(imu2[:, 7:10], state[:, 7:10] + sg[:, None] * z) and (imu2[:, 7:10] != imu[:, 7:10]).all()
    # a bias alone is a constant offset; a reset robot does not repeat its first epoch's noise
    m.set_params(acc_bias=np.full((B, 3), 0.5))
    assert np.array_equal(m.sense(state, motor)[0][:, 0:3], state[:, 13:16] + 0.5)
    a, b = SM.SenseModel(B, 9), SM.SenseModel(B, 9)
    a.set_params(q_sigma=sg)
    b.set_params(q_sigma=sg)
    b.reset()
    assert (a.sense(state, motor)[1][:, :12] != b.sense(state, motor)[1][:, :12]).all()


def test_cpu_closed_loop_through_the_estimators_is_safe_and_is_what_the_fixture_records():
    """The yardstick of the GPU walk through the sensor path: plant_model + sense_model + CtrlModel.estimate (VectorNav
    orientation estimator, Kalman filter) + the reference's qpOASES, 16 robots, 50 settle calls, 650 ticks.  Mode 0 with
    the noisy sensors is run again here (the fixture holds both modes, ideal and noisy): every robot stays safe, every
    solve returns 0, and the statistics are the fixture's (1e-6: tests/test_plant_cpu.py's reasoning -- the realisation
    of the noise is the same, bit for bit, wherever numpy runs)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "sense_closed_loop_cpu.json")))
    assert gold["ticks"] == L.TICKS == 650 and tuple(gold["pid"]) == L.PID
    assert gold["settle"] == SL.SETTLE == 50 and gold["seed"] == SL.SEED
    nz = SL.noise(L.N_CMD)
    for k, v in nz.items():
        assert np.array_equal(gold["noise"][k], v), k
    # the stated levels: biases inside their ranges and not all alike, sigmas as listed
    assert np.abs(nz["acc_bias"]).max() <= 0.2 and np.abs(nz["gyro_bias"]).max() <= 0.02 and np.ptp(nz["acc_bias"]) > 0.2
    assert (nz["acc_sigma"] == 0.3).all() and (nz["gyro_sigma"] == 0.02).all()
    assert (nz["q_sigma"] == 0.002).all() and (nz["qd_sigma"] == 0.05).all()
    mode = 0
    stats, info = SL.cpu_loop_sensed(mode, True)
    rec = gold[f"mode{mode}"]
    gait, vel, xyyaw = L.commands(mode)
    assert np.array_equal(rec["gait"], gait) and np.array_equal(rec["vel"], vel) and np.array_equal(rec["xyyaw"], xyyaw)
    assert (info["safe"] == 1).all() and info["rc_bad"] == 0 and info["nwsr_max"] < 100, info
    assert info["n_solves"] >= 16 * 45 and (info["sense_n"] == SL.SETTLE + L.TICKS).all()
    for k in L.STATS:
        print(k, np.abs(stats[k] - np.asarray(rec["noisy"][k])).max())
        assert np.abs(stats[k] - np.asarray(rec["noisy"][k])).max() < 1e-6, k
    # the robots walk, and the filter has found the body: its height is right to 3 mm under this noise
    assert (stats["z_min"] > 0.2).all() and (stats["roll_max"] < 0.1).all() and (stats["pitch_max"] < 0.1).all()
    assert np.abs(stats["vx_mean"] - vel[:, 0]).max() < 0.05 and info["z_err"] < 3e-3
    # every recorded run kept its fleet and differs from its ideal twin: the noise is felt
    for md in (0, 1):
        for name in ("ideal", "noisy"):
            r = gold[f"mode{md}"][name]
            assert r["nwsr_max"] < 100 and min(r["z_min"]) > 0.2 and r["z_max"] == [0.29] * 16, (md, name)
        assert np.abs(np.asarray(gold[f"mode{md}"]["noisy"]["roll_max"]) - gold[f"mode{md}"]["ideal"]["roll_max"]).max() > 1e-4


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_sense_kernel_resources(tmp_path):
    """The two instantiations of the sensor kernel and the reset kernel compile for gfx950 without scratch, spills or
    LDS (profiles/sense_kernel_resources.txt)."""
    src = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_sense.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-c", src,
                          "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "sense.o")],
                         capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    sense = {k: v for k, v in res.items() if "qmpc_sense_kernel" in k}
    assert len(res) == 3 and len(sense) == 2, sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
