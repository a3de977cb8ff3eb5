"""Dense fp64 NumPy restatement of the two map-repair definitions (include/slamhip_diag.h):

find   every pair a < b (1-based) with D = P_aa + P_bb - P_ab - P_ab' (symmetrised) positive definite as computed and
       delta' inv(D) delta < gate, by exhaustive search over all pairs, in ascending lexicographic order;
merge  the pairs (a_p, b_p) of one call as ONE update in the reference's Cholesky form (src/ekf.jl:67-75) with an explicit
       dense H (+I2 at a_p, -I2 at b_p), measurement 0 and noise blockdiag(Rc); then the b_p are deleted.

tests/test_merge_ref_cpu.py pins this file against known answers and the generic Kalman update; the GPU tests compare the
kernels with it."""
import numpy as np


def f(j):
    """First 0-based state index of landmark j (1-based)."""
    return 3 + 2 * (int(j) - 1)


def difference(x, P, a, b):
    """(delta, D) of landmarks a, b (1-based): the difference of the means and its covariance, symmetrised."""
    fa, fb = f(a), f(b)
    delta = x[fb:fb + 2] - x[fa:fa + 2]
    Pab = P[fa:fa + 2, fb:fb + 2]
    D = ((P[fa:fa + 2, fa:fa + 2] + P[fb:fb + 2, fb:fb + 2]) - Pab) - Pab.T
    return delta, (D + D.T) * 0.5


def d2_of(delta, D):
    """delta' inv(D) delta, or inf when D is not positive definite as computed (D00 > 0 and det > 0)."""
    det = D[0, 0] * D[1, 1] - D[0, 1] * D[0, 1]
    if not (D[0, 0] > 0.0 and det > 0.0):
        return np.inf
    return (D[1, 1] * delta[0] * delta[0] - 2.0 * D[0, 1] * delta[0] * delta[1] + D[0, 0] * delta[1] * delta[1]) / det


def d2_table(x, P):
    """[N, N] float64: d2 of every pair a < b at [a - 1, b - 1], inf elsewhere (vectorised over b)."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    N = (len(x) - 3) // 2
    out = np.full((N, N), np.inf)
    m = x[3:].reshape(N, 2)
    fs = 3 + 2 * np.arange(N)
    for a in range(N - 1):
        fa = fs[a]
        bs = np.arange(a + 1, N)
        fb = fs[bs]
        dx, dy = m[bs, 0] - m[a, 0], m[bs, 1] - m[a, 1]
        c00, c01, c10, c11 = P[fa, fb], P[fa, fb + 1], P[fa + 1, fb], P[fa + 1, fb + 1]      # P_ab
        D00 = ((P[fa, fa] + P[fb, fb]) - c00) - c00
        D11 = ((P[fa + 1, fa + 1] + P[fb + 1, fb + 1]) - c11) - c11
        D01 = ((P[fa, fa + 1] + P[fb, fb + 1]) - c01) - c10
        D10 = ((P[fa + 1, fa] + P[fb + 1, fb]) - c10) - c01
        Ds = (D01 + D10) * 0.5
        det = D00 * D11 - Ds * Ds
        ok = (D00 > 0.0) & (det > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            d2 = (D11 * dx * dx - 2.0 * Ds * dx * dy + D00 * dy * dy) / det
        out[a, bs] = np.where(ok, d2, np.inf)
    return out


def find(x, P, gate):
    """(pairs int32 [count, 2], count): every duplicate pair, ascending."""
    t = d2_table(x, P)
    a, b = np.nonzero(t < gate)                     # row-major order of nonzero = ascending (a, b)
    pairs = np.stack([a + 1, b + 1], axis=1).astype(np.int32)
    return pairs, int(pairs.shape[0])


def prefilter_keeps(delta, Paa, Pbb, gate):
    """The cheap test of the kernel: False = the pair is rejected without reading P_ab."""
    return float(delta @ delta) < 2.0 * gate * (np.trace(Paa) + np.trace(Pbb))


def dense_H(n, pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    H = np.zeros((2 * len(pairs), n))
    for p, (a, b) in enumerate(pairs):
        H[2 * p:2 * p + 2, f(a):f(a) + 2] = np.eye(2)
        H[2 * p:2 * p + 2, f(b):f(b) + 2] = -np.eye(2)
    return H


def new_index_of(N, pairs):
    """new_index of a merge: survivors renumbered in order; a removed b_p carries the new id of its a_p."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    gone = np.zeros(N, dtype=bool)
    gone[pairs[:, 1] - 1] = True
    ni = np.zeros(N, dtype=np.int32)
    ni[~gone] = np.arange(1, int((~gone).sum()) + 1)
    for a, b in pairs:
        ni[b - 1] = ni[a - 1]
    return ni


def fuse(x, P, pairs, Rc=None):
    """The update alone (before the removal): (x, P) after the constraint rows of `pairs`, src/ekf.jl:67-75.
    Raises np.linalg.LinAlgError when S is not positive definite."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return x.copy(), P.copy()
    H = dense_H(len(x), pairs)
    RR = np.kron(np.eye(len(pairs)), np.zeros((2, 2)) if Rc is None else np.asarray(Rc, dtype=np.float64))
    v = -(H @ x)                                    # z = 0
    PHt = P @ H.T
    S = H @ PHt + RR
    S = (S + S.T) * 0.5
    C = np.linalg.inv(np.linalg.cholesky(S).T)      # chol(S) of the reference is the upper factor
    W1 = PHt @ C
    return x + W1 @ (C.T @ v), P - W1 @ W1.T


def merge(x, P, pairs, Rc=None):
    """(x, P, new_index) after merging `pairs` ((a_p, b_p) 1-based; b_p leaves) in one update."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    N = (len(x) - 3) // 2
    xm, Pm = fuse(x, P, pairs, Rc)
    rm = pairs[:, 1]
    keep = np.delete(np.arange(len(xm)), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]).astype(np.int64))
    return xm[keep], Pm[np.ix_(keep, keep)], new_index_of(N, pairs)
