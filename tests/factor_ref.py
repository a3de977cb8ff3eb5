"""The rule of include/ext/slamhip_factor.h, run literally on the CPU: the column Cholesky with its failing-pivot rule, forward
substitution, the product, and the bounds the GPU tests hold the device to.  Loops over columns with NumPy dot products; no
library factorisation is called here (tests/test_factor_ref_cpu.py holds this file against numpy and LAPACK).

    d_i  = a_ii - sum_{j < i} l_ij^2          fails when <= 0 or not finite: i is reported, the factorisation stops
    l_ii = sqrt(d_i),  l_ri = (a_ri - sum_{j < i} l_rj l_ij) / l_ii

Bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.), all entrywise and valid for ANY order of summation:
    Thm 10.3   |L L' - A| <= gamma_(n+1) |L| |L|'             the computed Cholesky factor
    Thm 8.5    |L Y - B|  <= gamma_n |L| |Y|                   forward substitution
    (3.11)     |fl(L Z) - L Z| <= gamma_n |L| |Z|              a matrix product
with gamma_k = k u / (1 - k u) and u the unit roundoff of the arithmetic (2^-24, 2^-53)."""
import math

import numpy as np

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP = {"f32": np.float32, "f64": np.float64}
EDGE = {"f32": 128, "f64": 64}


def gamma(k, u):
    return k * u / (1.0 - k * u)


def lower_view(P):
    """The matrix the factorisation reads: the stored LOWER entries, mirrored."""
    P = np.asarray(P)
    return np.tril(P) + np.tril(P, -1).T


def cholesky(A, dtype="f64"):
    """(L, index, pivot): the column Cholesky of the lower triangle of A in `dtype` arithmetic.  index = -1 and pivot = 0.0 on
    success; otherwise the first failing column, its pivot, and L holds the columns before it (zero elsewhere)."""
    t = NP[dtype]
    A = np.asarray(A, dtype=t)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=t)
    for i in range(n):
        row = L[i, :i]
        d = t(A[i, i] - t(np.dot(row, row))) if i else t(A[i, i])
        if not (d > 0) or not np.isfinite(d):
            return L, i, float(d)
        lii = t(np.sqrt(d))
        L[i, i] = lii
        if i + 1 < n:
            s = (L[i + 1:, :i] @ row).astype(t) if i else t(0)
            L[i + 1:, i] = ((A[i + 1:, i] - s) / lii).astype(t)
    return L, -1, 0.0


def forward_solve(L, B):
    """Y = L^-1 B by forward substitution, float64."""
    L = np.asarray(L, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def product(L, Z):
    """L Z with the lower triangle of L only, float64, row by row."""
    L = np.asarray(L, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    out = np.zeros_like(Z)
    for i in range(L.shape[0]):
        out[i] = L[i, :i + 1] @ Z[:i + 1]
    return out


def logdet(L):
    """2 sum log l_ii in float64, in column order."""
    s = 0.0
    for v in np.diag(np.asarray(L, dtype=np.float64)):
        s += math.log(v)
    return 2.0 * s


def mpi_to_pi(phi):
    if phi > math.pi:
        return phi - 2 * math.pi
    if phi < -math.pi:
        return phi + 2 * math.pi
    return phi


def nees(mean, x_true, L):
    """e' (L L')^-1 e with e = mean - x_true, the heading difference wrapped once."""
    e = np.asarray(mean, dtype=np.float64) - np.asarray(x_true, dtype=np.float64)
    e[2] = mpi_to_pi(e[2])
    y = forward_solve(L, e[:, None])[:, 0]
    return float(np.dot(y, y))


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def factor_bound(L, dtype):
    """gamma_(n+1) |L| |L|' (Thm 10.3), float64."""
    Lm = np.abs(np.asarray(L, dtype=np.float64))
    return gamma(Lm.shape[0] + 1, U[dtype]) * (Lm @ Lm.T)


def factor_ratio(L, A, dtype):
    """(the largest |L L' - A|_ij / bound_ij over the entries with a positive bound, the largest |L L' - A|_ij where the bound is 0)."""
    Ld = np.asarray(L, dtype=np.float64)
    err = np.abs(Ld @ Ld.T - np.asarray(A, dtype=np.float64))
    bound = factor_bound(L, dtype)
    pos = bound > 0
    return (float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0), (float(np.max(err[~pos])) if (~pos).any() else 0.0)


def _exact_product(L, X):
    """tril(L) X in extended precision (np.longdouble, 64-bit significand on x86): its own rounding error is 2^-11 of the float64
    bounds below, so a residual formed with it measures the device and not this file."""
    return np.tril(np.asarray(L, dtype=np.longdouble)) @ np.asarray(X, dtype=np.longdouble)


def _worst(err, bound):
    pos = bound > 0
    return (float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0), (float(np.max(err[~pos])) if (~pos).any() else 0.0)


def solve_ratio(L, Y, B):
    """The largest |L Y - B| / (gamma_n |L| |Y|) (Thm 8.5, u = 2^-53) and the largest residual where that bound is 0."""
    Ld = np.tril(np.asarray(L, dtype=np.float64))
    err = np.abs(_exact_product(L, Y) - np.asarray(B, dtype=np.longdouble)).astype(np.float64)
    return _worst(err, gamma(Ld.shape[0], U["f64"]) * (np.abs(Ld) @ np.abs(Y)))


def product_ratio(L, Z, out):
    """The largest |out - L Z| / (gamma_n |L| |Z|) (u = 2^-53) and the largest error where that bound is 0; L Z in extended
    precision."""
    Ld = np.tril(np.asarray(L, dtype=np.float64))
    err = np.abs(np.asarray(out, dtype=np.longdouble) - _exact_product(L, Z)).astype(np.float64)
    return _worst(err, gamma(Ld.shape[0], U["f64"]) * (np.abs(Ld) @ np.abs(Z)))


def logdet_bound(P, L, dtype):
    """First-order bound of |log det(L L') - log det P|: 1.1 sum_ij |P^-1|_ij B_ij with B the bound of Thm 10.3 (d log det P =
    trace(P^-1 dP); 1.1 covers the second order while the bound is small).  Only meaningful below 0.1."""
    Pinv = np.linalg.inv(np.asarray(P, dtype=np.float64))
    return 1.1 * float(np.sum(np.abs(Pinv) * factor_bound(L, dtype)))


# ---- designed failures -----------------------------------------------------------------------------------------------------------
def plant_failure(P, i, dtype):
    """P with P[i, i] = fl((1 - 2^-8) sum_{j < i} l_ij^2), l from the float64 factor of P (i = 0: P[0, 0] = -P[0, 0]): the pivot
    of column i is then negative by 2^-8 of a sum whose rounding error is at most gamma_n of it, so column i is the first to
    fail in either arithmetic."""
    P = np.array(P, dtype=np.float64)
    if i == 0:
        P[0, 0] = -P[0, 0]
        return P
    L, idx, _ = cholesky(P, "f64")
    assert idx == -1
    P[i, i] = float(NP[dtype]((1.0 - 2.0 ** -8) * float(np.dot(L[i, :i], L[i, :i]))))
    return P


# ---- a model of the device's blocked order, with defects to show what the bound catches --------------------------------------------
def _bf16(v):
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def blocked_model(A, dtype, E=None, defect=None):
    """The right-looking blocked Cholesky over E x E tiles in `dtype` arithmetic (one-tile panels).  defect: None,
    "dropped_tile_product" (one L_Ip L_Jp' of the trailing update is left out) or "bf16_operands" (the trailing update's operands
    are rounded to bfloat16 first).  Returns (L, index): index = -1, or the state index at which a pivot failed (a defect can
    make a positive definite matrix fail)."""
    t = NP[dtype]
    E = EDGE[dtype] if E is None else E
    A = np.array(lower_view(A), dtype=t)
    n = A.shape[0]
    T = (n + E - 1) // E
    L = np.zeros_like(A)
    for k in range(T):
        a, b = k * E, min(n, (k + 1) * E)
        Lkk, idx, _ = cholesky(A[a:b, a:b], dtype)
        if idx != -1:
            return L, a + idx
        L[a:b, a:b] = Lkk
        if b == n:
            break
        X = np.zeros((n - b, b - a), dtype=t)
        for c in range(b - a):                                           # x L_kk' = a, row-wise substitution
            X[:, c] = ((A[b:, a + c] - (X[:, :c] @ Lkk[c, :c]).astype(t)) / Lkk[c, c]).astype(t)
        L[b:, a:b] = X
        W = _bf16(X).astype(t) if defect == "bf16_operands" else X
        upd = (W @ W.T).astype(t)
        if defect == "dropped_tile_product" and k == 0 and T > 2:
            upd[E:2 * E, :E] = 0                                         # tile (2, 1) misses its product with column 0
            upd[:E, E:2 * E] = 0
        A[b:, b:] = (A[b:, b:] - upd).astype(t)
    return L, -1
