"""Dense fp64 NumPy restatement of the rules of include/ext/slamhip_linear.h: the update from a caller's linear measurement
(src/ekf.jl:67-75 with an explicit dense H), its gate, the predict from a caller's vehicle Jacobian and the predict from an odometry
increment.  State indices are 0-based: 0, 1, 2 the vehicle, landmark j (1-based) at f(j) and f(j) + 1.

tests/test_linear_ref_cpu.py pins this file against the oracle's update and predict, tests/merge_ref.py and hand-derived answers;
tests/test_gpu_ekf_linear.py compares the kernels with it."""
import math

import numpy as np

MAXROWS = 16
MAXNNZ = 8
MEASURED, INNOVATION = 0, 1
PI = math.pi


def f(j):
    """First 0-based state index of landmark j (1-based)."""
    return 3 + 2 * (int(j) - 1)


def mpi_to_pi(a):
    """ONE conditional wrap (src/common.jl:102-110)."""
    if a > PI:
        return a - 2 * PI
    if a < -PI:
        return a + 2 * PI
    return a


def dense_H(n, rows):
    """k x n from a list of {state index: value} rows."""
    H = np.zeros((len(rows), n))
    for i, r in enumerate(rows):
        for c, v in r.items():
            H[i, int(c)] = float(v)
    return H


def csr(rows):
    """(ptr, idx, val) of a list of {state index: value} rows, in the dicts' order."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([c for r in rows for c in r.keys()], dtype=np.int32)
    val = np.array([v for r in rows for v in r.values()], dtype=np.float64)
    return ptr, idx, val


def chol_lower(S):
    """(L, j, d): the lower factor, row by row pivots; j = -1, or the first failing column and its pivot d (<= 0 or not finite)."""
    k = S.shape[0]
    L = np.zeros((k, k))
    A = np.array(S, dtype=np.float64)
    for j in range(k):
        d = A[j, j]
        if not (d > 0.0) or not (d < np.inf):
            return L, j, float(d)
        L[j, j] = math.sqrt(d)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L, -1, 0.0


def innovation(x, H, z, mode=MEASURED, wrap_mask=0):
    z = np.asarray(z, dtype=np.float64)
    if mode == INNOVATION:
        assert wrap_mask == 0
        return z.copy()
    v = z - H @ x
    for i in range(len(v)):
        if (wrap_mask >> i) & 1:
            v[i] = mpi_to_pi(v[i])
    return v


def gate(x, P, H, z, R, mode=MEASURED, wrap_mask=0):
    """(out[4], S-pieces): out = [v' inv(S) v, log det S, min l_jj, -1], or [0, 0, d_j, j] when pivot j fails."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    v = innovation(x, H, z, mode, wrap_mask)
    PHt = P @ H.T
    S = H @ PHt + np.asarray(R, dtype=np.float64)
    S = (S + S.T) * 0.5
    L, j, d = chol_lower(S)
    if j >= 0:
        return np.array([0.0, 0.0, d, float(j)]), None
    C = np.linalg.inv(L).T                                  # the reference's inv(chol(S)), upper
    y = C.T @ v
    out = np.array([float(y @ y), 2.0 * float(np.sum(np.log(np.diag(L)))), float(np.min(np.diag(L))), -1.0])
    return out, (PHt, C, v)


def update(x, P, H, z, R, mode=MEASURED, wrap_mask=0):
    """(x, P, out) after the update; x and P come back unchanged (copies) when S is not positive definite (out[3] >= 0).
    The heading is not wrapped afterwards (src/ekf.jl:74)."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    out, pieces = gate(x, P, H, z, R, mode, wrap_mask)
    if pieces is None:
        return x.copy(), P.copy(), out
    PHt, C, v = pieces
    W1 = PHt @ C
    return x + W1 @ (C.T @ v), P - W1 @ W1.T, out


def predict_linear(x, P, xv, Gv, Qv):
    """x[0:3] = xv, P_vv = Gv P_vv Gv' + Qv (Qv read from its lower triangle), P_vm = Gv P_vm and its mirror."""
    x = np.array(x, dtype=np.float64)
    P = np.array(P, dtype=np.float64)
    Gv = np.asarray(Gv, dtype=np.float64)
    Ql = np.tril(np.asarray(Qv, dtype=np.float64))
    Qs = Ql + np.tril(Ql, -1).T
    x[0:3] = np.asarray(xv, dtype=np.float64)
    vv = np.tril(Gv @ P[0:3, 0:3] @ Gv.T + Qs)              # the lower triangle formed once and mirrored
    P[0:3, 0:3] = vv + np.tril(vv, -1).T
    P[0:3, 3:] = Gv @ P[0:3, 3:]
    P[3:, 0:3] = P[0:3, 3:].T
    return x, P


def odometry_model(phi, d, Q3):
    """(xv increment in the map frame, Gv, Qv) of an increment d = (dx, dy, dtheta) at heading phi."""
    s, c = math.sin(phi), math.cos(phi)
    dx, dy = float(d[0]), float(d[1])
    Gv = np.array([[1.0, 0.0, -(s * dx + c * dy)], [0.0, 1.0, c * dx - s * dy], [0.0, 0.0, 1.0]])
    Gu = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    Ql = np.tril(np.asarray(Q3, dtype=np.float64))
    Qs = Ql + np.tril(Ql, -1).T
    return np.array([c * dx - s * dy, s * dx + c * dy]), Gv, Gu @ Qs @ Gu.T


def strip_pairs(col, xv, Gv, Qv, xv_mag, Gv_mag=None, Qv_mag=None):
    """The entries a predict owns as (ref, mag) pairs in the extended precision of tests/strip_ref.py, for its bound
    u_T |ref| + c 2^-53 mag: 'strip' (n - 3, 3), 'vv' (3, 3), 'x' (3,).  col = P[:, 0:3]; xv, Gv, Qv already extended.  Gv_mag,
    Qv_mag: the magnitudes of Gv and Qv where they are sums themselves (default: their absolute values)."""
    from tests import strip_ref as S
    col = S._ld(col)
    Gv, Qv = S._ld(Gv), S._ld(Qv)
    Ql = np.tril(Qv)
    Qs = Ql + np.tril(Ql, -1).T
    strip = col[3:] @ Gv.T
    Gm = np.abs(Gv) if Gv_mag is None else S._ld(Gv_mag)
    Qm = np.abs(Qs) if Qv_mag is None else S._ld(Qv_mag)
    strip_mag = np.abs(col[3:]) @ Gm.T
    vv = np.tril(Gv @ col[0:3] @ Gv.T + Qs)
    vv = vv + np.tril(vv, -1).T
    vv_mag = Gm @ np.abs(col[0:3]) @ Gm.T + Qm
    return {"strip": (strip, strip_mag), "vv": (vv, vv_mag), "x": (S._ld(xv), S._ld(xv_mag))}


def odometry_pairs(x3, col, d, Q3):
    """strip_pairs of predict_odometry from pose x3 (float64 values of the state's dtype): sin and cos of the float64 heading in
    extended precision, as tests/strip_ref.py takes them for predict."""
    from tests import strip_ref as S
    LD = S.LD
    x3 = np.asarray(x3, dtype=np.float64)
    s, c = S._sincos(x3[2])
    dx, dy, dth = (LD(np.float64(t)) for t in d)
    gx, gy = c * dx - s * dy, s * dx + c * dy
    one, zero = LD(1), LD(0)
    Gv = np.array([[one, zero, -gy], [zero, one, gx], [zero, zero, one]], dtype=LD)
    Gu = np.array([[c, -s, zero], [s, c, zero], [zero, zero, one]], dtype=LD)
    Ql = np.tril(S._ld(Q3))
    Qs = Ql + np.tril(Ql, -1).T
    t = LD(x3[2]) + dth
    wrapped = 0
    if t > LD(PI):
        t, wrapped = t - 2 * LD(PI), 1
    elif t < -LD(PI):
        t, wrapped = t + 2 * LD(PI), -1
    xv = np.array([LD(x3[0]) + gx, LD(x3[1]) + gy, t], dtype=LD)
    step = abs(dx) + abs(dy)
    xm = np.array([abs(LD(x3[0])) + step, abs(LD(x3[1])) + step, abs(LD(x3[2])) + abs(dth) + (2 * LD(PI) if wrapped else 0)], dtype=LD)
    Gm = np.array([[one, zero, step], [zero, one, step], [zero, zero, one]], dtype=LD)      # |sin|, |cos| <= 1 dropped
    Um = np.array([[one, one, zero], [one, one, zero], [zero, zero, one]], dtype=LD)
    out = strip_pairs(col, xv, Gv, Gu @ Qs @ Gu.T, xm, Gm, Um @ np.abs(Qs) @ Um.T)
    out["wrapped"] = wrapped
    return out


def predict_odometry(x, P, d, Q3):
    x = np.asarray(x, dtype=np.float64)
    step, Gv, Qv = odometry_model(x[2], d, Q3)
    xv = np.array([x[0] + step[0], x[1] + step[1], mpi_to_pi(x[2] + float(d[2]))])
    return predict_linear(x, P, xv, Gv, Qv)
