"""numpy float32 copy of oracle/glue_oracle.c's oracle_kf_step, vectorised over robots -- TEST SIDE ONLY.

Not a second reference: tests/test_est_cases_cpu.py first holds it to the C restatement bit for bit, and then uses its
switches -- one per decision of the filter that the GPU suites pin -- to show that each decision moves bits on the
committed cases (no second C build).  Every element is formed by the C code's operations in the C code's order."""
import numpy as np

f32 = np.float32
N, M, W = 18, 28, 28 + 1 + 18
HIP = np.array([0.19, 0.049, 0.0], f32)
CA = np.array([r % 3 if r < 12 else (3 + r % 3 if r < 24 else 8 + 3 * (r - 24)) for r in range(M)])
CB = np.array([6 + r if r < 12 else -1 for r in range(M)])


def _c_rows(X):
    """C X for X [B, N, ...]: row r is X[CA[r]] - X[CB[r]], or X[CA[r]] alone."""
    two = CB >= 0
    out = X[:, CA].copy()
    out[:, two] = X[:, CA[two]] - X[:, CB[two]]
    return out


def kf_step(xhat, P, r_body, a_world, omega_body, contact, leg_p, leg_v, swap=True, window=0.2, clip=True,
            reset_at=0.000001):
    """One run() for every robot -> (xhat', P', position, v_world, v_body); the arguments are left alone.
    swap=False: the pivot row is found but not exchanged.  window: trust_window.  clip=False: no fminf(phase, 1).
    reset_at: the determinant above which the covariance is reset."""
    B = xhat.shape[0]
    x = np.array(xhat, f32)
    P = np.array(P, f32).reshape(B, N, N)
    rB, om = np.asarray(r_body, f32), np.asarray(omega_body, f32)
    lp, lv = np.asarray(leg_p, f32).reshape(B, 4, 3), np.asarray(leg_v, f32).reshape(B, 4, 3)
    dt, one = f32(0.002), f32(1)
    Q = np.zeros((B, N), f32)
    Q[:, 0:3] = (dt / f32(20)) * f32(0.02)
    Q[:, 3:6] = (dt * f32(9.8) / f32(20)) * f32(0.02)
    Q[:, 6:] = dt * f32(0.002)
    R = np.zeros((B, M), f32)
    R[:, :12], R[:, 12:24], R[:, 24:] = one * f32(0.001), one * f32(0.1), one * f32(0.001)
    a = np.asarray(a_world, f32) + np.array([0, 0, -9.81], f32)
    y = np.zeros((B, M), f32)
    p0, v0 = x[:, 0:3].copy(), x[:, 3:6].copy()
    tw = f32(window)
    for i in range(4):
        ph = np.array([HIP[0] if i < 2 else -HIP[0], HIP[1] if i in (1, 3) else -HIP[1], HIP[2]], f32)
        p_rel = ph + lp[:, i]
        w = np.stack([(om[:, 1] * p_rel[:, 2] - om[:, 2] * p_rel[:, 1]) + lv[:, i, 0],
                      (om[:, 2] * p_rel[:, 0] - om[:, 0] * p_rel[:, 2]) + lv[:, i, 1],
                      (om[:, 0] * p_rel[:, 1] - om[:, 1] * p_rel[:, 0]) + lv[:, i, 2]], 1)
        p_f = np.stack([(rB[:, k] * p_rel[:, 0] + rB[:, 3 + k] * p_rel[:, 1]) + rB[:, 6 + k] * p_rel[:, 2] for k in range(3)], 1)
        dp_f = np.stack([(rB[:, k] * w[:, 0] + rB[:, 3 + k] * w[:, 1]) + rB[:, 6 + k] * w[:, 2] for k in range(3)], 1)
        phase = np.asarray(contact, f32)[:, i]
        if clip:
            phase = np.fmin(phase, one)
        trust = np.where(phase < tw, phase / tw, np.where(phase > (one - tw), (one - phase) / tw, one)).astype(f32)
        factor = one + (one - trust) * f32(100)
        sl = slice(3 * i, 3 * i + 3)
        Q[:, 6 + 3 * i:9 + 3 * i] = factor[:, None] * Q[:, 6 + 3 * i:9 + 3 * i]
        R[:, 12 + 3 * i:15 + 3 * i] = factor[:, None] * R[:, 12 + 3 * i:15 + 3 * i]
        y[:, sl] = -p_f
        y[:, 12 + 3 * i:15 + 3 * i] = (one - trust)[:, None] * v0 + trust[:, None] * (-dp_f)
        R[:, 24 + i] = factor * R[:, 24 + i]
        y[:, 24 + i] = (one - trust) * (p0[:, 2] + p_f[:, 2])
    xp = x[:, 0:3] + dt * x[:, 3:6]
    x[:, 3:6] = x[:, 3:6] + dt * a
    x[:, 0:3] = xp
    AP = P.copy()
    AP[:, 0:3] = P[:, 0:3] + dt * P[:, 3:6]
    Pm = AP.copy()
    Pm[:, :, 0:3] = AP[:, :, 0:3] + dt * AP[:, :, 3:6]
    d = np.arange(N)
    Pm[:, d, d] = Pm[:, d, d] + Q
    ey = y - _c_rows(x)
    CP = _c_rows(Pm)                                             # [B, M, N]
    K1 = _c_rows(Pm.transpose(0, 2, 1)).transpose(0, 2, 1).copy()  # Pm C^T [B, N, M]
    S = _c_rows(CP.transpose(0, 2, 1)).transpose(0, 2, 1).copy()   # C Pm C^T [B, M, M]
    r = np.arange(M)
    S[:, r, r] = S[:, r, r] + R
    Sa = np.zeros((B, M, W), f32)
    Sa[:, :, :M] = S
    Sa[:, :, M] = ey
    Sa[:, r, M + 1 + CA] = 1
    two = CB >= 0
    Sa[:, r[two], M + 1 + CB[two]] = -1
    rows = np.arange(B)
    for k in range(M):
        piv = k + np.argmax(np.abs(Sa[:, k:, k]), 1)             # (argmax: the first largest wins)
        if swap:
            t = Sa[rows, k].copy()
            Sa[rows, k] = Sa[rows, piv]
            Sa[rows, piv] = t
        l = Sa[:, k + 1:, k] / Sa[:, k, k][:, None]
        Sa[:, k + 1:, k + 1:] = Sa[:, k + 1:, k + 1:] - l[:, :, None] * Sa[:, k, None, k + 1:]
    for rr in range(M - 1, -1, -1):
        acc = Sa[:, rr, M:].copy()
        for j in range(rr + 1, M):
            acc = acc - Sa[:, rr, j][:, None] * Sa[:, j, M:]
        Sa[:, rr, M:] = acc / Sa[:, rr, rr][:, None]
    acc = np.zeros((B, N), f32)
    T1 = np.zeros((B, N, N), f32)
    for c in range(M):
        acc = acc + K1[:, :, c] * Sa[:, c, M][:, None]
        T1 = T1 + K1[:, :, c][:, :, None] * Sa[:, c, None, M + 1:]
    x = x + acc
    T1 = np.eye(N, dtype=f32)[None] - T1
    Pn = np.zeros((B, N, N), f32)
    for k in range(N):
        Pn = Pn + T1[:, :, k][:, :, None] * Pm[:, k, None, :]
    Pn = (Pn + Pn.transpose(0, 2, 1)) / f32(2)
    reset = Pn[:, 0, 0] * Pn[:, 1, 1] - Pn[:, 0, 1] * Pn[:, 1, 0] > f32(reset_at)
    Z = Pn[reset]
    Z[:, 0:2, 2:] = 0
    Z[:, 2:, 0:2] = 0
    Z[:, 0:2, 0:2] = Z[:, 0:2, 0:2] / f32(10)
    Pn[reset] = Z
    v_body = np.stack([(rB[:, 3 * k] * x[:, 3] + rB[:, 3 * k + 1] * x[:, 4]) + rB[:, 3 * k + 2] * x[:, 5] for k in range(3)], 1)
    return x, Pn.reshape(B, N * N), x[:, 0:3].copy(), x[:, 3:6].copy(), v_body
