"""The EKF update (csrc/ekf_update.hip, csrc/ekf_syrk.hip) entry by entry: designed states, a one-call restatement in extended
precision with a DERIVED per-entry bound, a correctly rounded model of each dtype, and planted defects.  Host-only NumPy;
nothing here needs a GPU.  Companion of tests/strip_ref.py (predict, add_features) and tests/lm_records.py (FastSLAM).

Why
    tests/test_gpu_ekf.py and tests/test_gpu_ekf_dispatch.py hold the update to TOL (fp32 5e-6, fp64 1e-9) of max|x| and of
    sqrt(P_ii P_jj), from `random_state` = A A' + 0.01 I with A of rank 6.  x is then allowed 5e-4 .. 2e-3 m (and rad) where the
    corrections are 0.02 .. 0.2, and after the first few observations the panel W1 has almost no mass left in its later columns:
    a gain off by 1e-3 or a panel column scaled by 0.99 passes (tests/test_update_records_cpu.py prints the list).

The states (`make_inputs`), each already rounded to the dtype and positive definite after that rounding
    independent  a small pose block, NO pose-landmark correlation, landmark blocks with own scales 1e-3 .. 10 m^2 and anisotropy
                 up to 100 at a random orientation.  Every observation's two W1 columns carry that landmark's down-date, and an
                 unobserved landmark has an exactly zero row of P H': its rows of P and entries of x come back BIT FOR BIT.
    slam         what the filter produces: every landmark initialised by add_features' formula from one pose uncertainty
                 (P = Gv Pvv Gv' + Gz R Gz'), then five predicts with large control noise.  Strong common mode: the scaled
                 condition number of S is 1e4 .. 1e7 from m = 8 on.
    mixed        variances 1e-6, 1e-4, 1e-2, 1, 1e2 in one map, correlated (rho = 0.3 of a common +-1 factor), every scale
                 with observed and unobserved landmarks: entries from 1e-6 to 1e2, each judged on its own magnitude.
    geometry     ranges 0.5 m and 2000 m in one batch; landmarks exactly on an axis and on a diagonal from the pose (dx = 0,
                 dy = 0, dx = dy); landmarks behind the vehicle whose bearing innovation needs the wrap; heading within 5e-4
                 of +-pi.
    rank6        `random_state` of tests/test_gpu_ekf.py, kept for continuity with the existing figures.

The restatement (`restate`)
    ONE update from the given (on the GPU side: downloaded, bit-identical) state in np.longdouble (`strip_ref.EXTENDED`; the
    float64 fall-back doubles the fp64 slack, `strip_ref.C_FACTOR`): the oracle's formulas (oracle/ekf_ref.py: obs_blocks,
    _update_front, update_sparse, update_joseph_sparse) with a hand-written Cholesky factorisation and triangular solves
    (LAPACK has no longdouble; k <= 130).  Per entry it returns `ref` and a magnitude `mag`,
        x                  |x_i| + sum_a |W1_ia| |y_a|,          y = C' v  (x+ = x + W1 y, update_sparse)
        P, reference form  |P_ij| + sum_a |W1_ia| |W1_ja|
        P, Joseph form     |P_ij| + (|K| |T|' + |T| |K|')_ij
    kappa = cond(D^-1/2 S D^-1/2), D = diag(S), and per entry a `floor` (below).

The bound, from what the kernels do
    Front half (ekf_update.hip:11-15): P H' (pht_entry, :45-48), S (s_build_kernel, :149-225, or factor_body :776-790), the
    LDL' elimination, y, g = inv(S) v (:838-863), C (:871-909) or inv(S) (:911-924), W1 = P H' C (w1_mfma_body / panel_gemm_kernel)
    are `double` in BOTH dtypes.  Whatever passes through the factorisation carries a relative error of up to a modest
    multiple of 2^-53 kappa (the scaling by D is free: the elimination is invariant under it up to rounding), measured against
    the magnitude of the sum it ends in: the term 2^-53 kappa mag.
    The floor.  `mag` is built from W1 (K, T) and y as they come OUT; three roundings on the way IN do not shrink with them, and
    the fp64 model needs up to 2000 times 2^-53 kappa mag where they dominate (tests/test_update_records_cpu.py keeps that case):
      * an entry of P H' is a sum of five products (pht_entry) and is off by 2^-53 (|P| |H'|)_ia however far it cancels -- on
        `slam` an observation sees only the common mode and the rows of the OTHER landmarks cancel to rounding level;
      * C is formed explicitly (ekf_update.hip:871-909): |dC| <= 2^-53 |C| |U| |C| (Higham, Accuracy and Stability, 14.1), which
        matters where P_ij = 0 gives the entry no magnitude of its own (`independent`, `geometry`);
      * the innovation is a difference, off by 2^-53 (|z| + |zp|) (factor_body :746-747), and x += P H' g sums |P H'| |g|.
    Propagated to first order: W1 is uncertain by Wf = |P||H'| |C| + |P H'| |C||U||C| (in units of 2^-53), so
        floor(P) = Wf |W1|' + |W1| Wf'                                                    (reference form)
                   Kf |T|' + |K| Tf' + transposed,  Kf = Wf |C|' + |W1| (|C||U||C|)',  Tf = |P||H'| + Kf |S| / 2     (Joseph form)
        floor(x) = Wf |y| + |W1| ((|C||U||C|)' |v| + |C|' (|z| + |zp|)) + |P H'| |g|
    and the fp64 term of every bound is  c 2^-53 (kappa mag + floor).
      x   x_update_kernel (:1472), w1_mfma_body (:1168) and w1_stream_body (:1401) store (T)(xo + s), s = sum_a PHt[r][a] g[a] in double:
              |got - ref| <= u_T |ref| + c_x 2^-53 (kappa mag + floor)          u_T = 2^-24 (fp32: that ONE rounding) or 0 (fp64)
      P, fp64 (ekf_syrk.hip:1103: v_mfma_f64_16x16x4_f64, exact fp64 FMAs; W1 is not rounded again):
              |got - ref| <= c_P 2^-53 (kappa mag + floor)
      P, fp32 has three parts on top of the fp64 term:
          * W1 (K, T) is rounded to float once (ekf_update.hip:14-15): each factor of a product moves by 2^-24 relative, 2 u per
            product, 2 u (mag - |P|) on the sum;
          * the products are exact -- fp32 MFMA (ekf_syrk.hip:20) or the three-way bf16 split (ekf_syrk.hip:394-405; the three
            split products left out are below 2^-25 of the product: another u / 2 per product);
          * the sum is accumulated FROM ZERO in fp32 and subtracted from P once (ekf_syrk.hip:23-25).  The order inside a
            matrix-core instruction is not ours to know, so the derived limit takes the worst case in the number of terms K
            (the panel's columns, up to 128 on the streaming bodies, 2 kp in the Joseph form; 6 K fp32 additions on the
            split path): every addition rounds by at most u times a partial sum, which is at most mag.  The subtraction and
            the store are one rounding, u |ref| <= u mag.
              |got - ref| <= c_32 2^-24 mag + c_P 2^-53 (kappa mag + floor),     c_32 <= 3.5 + 6 K by derivation
    The derived limit is a worst case nobody reaches (errors of K additions add like sqrt(K)); what is ASSERTED is the margin
    rule of DESIGN 5.2a: MARGINS[form][class] = (c_x, c_P, c_32) = max(4, 4 x what the correctly rounded MODEL below needs on
    the class's own records), committed here, re-derived by tests/test_update_records_cpu.py, and never above the derived limit
    of the cell.  Nothing in the table comes from a device.  Every entry of every cell is compared: there are no exclusions,
    and the classes keep c 2^-53 kappa below 1e-6 (checked on the CPU), so the bound never goes slack.  An entry whose mag and
    floor are both zero must be exact.

The model (`model_update`)
    float64 front half exactly as the device forms it (explicit C = inv(chol(S)), W1 = P H' C, g = C (C' v), x = (T)(x + P H' g);
    Joseph: inv(S) = C C', K = P H' inv(S), T = P H' - K S / 2), W1 / K / T rounded to the dtype, products exact (fp32) or
    rounded once (fp64), the sum accumulated from zero in the dtype column after column, one subtraction, lower triangle
    mirrored.  `defect=` plants one of DEFECTS in it.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import ekf_ref as O
from tests.strip_ref import C_FACTOR, EPS53, EXTENDED, LD, NP_DTYPE, TILE, U_T   # noqa: F401  (EXTENDED: re-exported)
from tests.test_gpu_ekf import R, TOL, noisy_obs, random_state, relerr, relerr_cov
from tests.test_gpu_ekf_dispatch import FALLBACKS, LABELS, expected_path   # noqa: F401  (re-exported for the tests)

PI = math.pi
U32 = 2.0 ** -24
CLASSES = ("independent", "slam", "mixed", "geometry", "rank6")
FORMS = ("cholesky", "joseph")
KAPPA_SLACK = 1e-6                     # c 2^-53 kappa stays below this on every cell

# MARGINS[form][class] = (c_x, c_P, c_32): max(4, 4 x the model's need) over the class's cells of CELLS.  c_x and c_P (units
# 2^-53 (kappa mag + floor)) belong to the fp64 front half and hold for both dtypes; c_32 (units 2^-24 mag) is fp32's own.
# Re-derived by tests/test_update_records_cpu.py::test_committed_margins_follow_the_rule, which prints the table to commit.
MARGINS = {
    "cholesky": {"independent": (4.0, 22.3, 30.8),
                 "slam": (4.0, 4.0, 18.6),
                 "mixed": (4.0, 4.0, 44.5),
                 "geometry": (4.0, 23.8, 37.1),
                 "rank6": (4.0, 4.0, 38.3)},
    "joseph": {"independent": (4.0, 4.0, 13.5),
               "slam": (4.0, 4.0, 15.1),
               "mixed": (4.0, 4.0, 39.9),
               "geometry": (4.0, 4.0, 16.4),
               "rank6": (4.0, 4.0, 27.4)},
}

Cell = namedtuple("Cell", "cls N m dtype form xflags", defaults=(0,))


# ---- the designed states ----------------------------------------------------------------------------------------------------
def _spread(N):
    return 90.0 if N < 127 else 300.0


def _seed(cls, N, m, dtype):
    return 1_000_000 * CLASSES.index(cls) + 1000 * N + 10 * m + (dtype == "f64")


def _mm(A, B):
    """A B with the inner index walked in order and nothing but element-wise products and sums, in the operands' own float type:
    the same bits on every CPU (a BLAS product differs in the last place from one machine to the next, and the margins below
    are to be re-derived exactly)."""
    A, B = np.asarray(A), np.asarray(B)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.result_type(A, B))
    for a in range(A.shape[1]):
        acc += A[:, a:a + 1] * B[a:a + 1, :]
    return acc


def _block2(s1, s2, t):
    """Q diag(s1, s2) Q' for the rotation Q by t, written out."""
    c, s = math.cos(t), math.sin(t)
    off = c * s * (s1 - s2)
    return np.array([[c * c * s1 + s * s * s2, off], [off, s * s * s1 + c * c * s2]])


def _positions(rng, N, spread, pose, dmin=3.0):
    """2 N coordinates in the square of edge `spread` around (50, 50), none closer than dmin to the pose."""
    out = np.empty((N, 2))
    for j in range(N):
        while True:
            p = rng.uniform(50 - spread / 2, 50 + spread / 2, 2)
            if math.hypot(p[0] - pose[0], p[1] - pose[1]) >= dmin:
                break
        out[j] = p
    return out.reshape(-1)


def _pose_block(rng, sxy=0.2, sphi=0.03):
    d = np.array([sxy, sxy, sphi])
    c = np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.25], [-0.2, 0.25, 1.0]])
    return d[:, None] * c * d[None, :]


def _block_diag_state(rng, N, spread, lo, hi, aniso, phi=None):
    n = 3 + 2 * N
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3) if phi is None else phi])
    x = np.concatenate([pose, _positions(rng, N, spread, pose)])
    P = np.zeros((n, n))
    P[0:3, 0:3] = _pose_block(rng)
    for j in range(N):
        s = 10.0 ** rng.uniform(math.log10(lo), math.log10(hi))
        a = 10.0 ** rng.uniform(0, math.log10(aniso))
        f = 3 + 2 * j
        P[f:f + 2, f:f + 2] = _block2(s, s / a, rng.uniform(0, PI))
    return x, (P + P.T) / 2


def _state_independent(rng, N):
    return _block_diag_state(rng, N, _spread(N), 1e-3, 10.0, 100.0)


def _state_slam(rng, N):
    """add_features of all N landmarks from ONE pose uncertainty (src/ekf.jl:84-122 by formula: P = J Pvv J' + the landmarks' own
    Gz R Gz', J = [I; Gv_1; ..; Gv_N]), then five predicts with large control noise (src/ekf.jl:8-43 on the column strip)."""
    n = 3 + 2 * N
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3)])
    r, b = rng.uniform(5.0, _spread(N) / 2, N), rng.uniform(-PI, PI, N)
    sn, cs = np.sin(pose[2] + b), np.cos(pose[2] + b)
    x = np.concatenate([pose, np.stack([pose[0] + r * cs, pose[1] + r * sn], axis=1).reshape(-1)])
    J = np.zeros((n, 3))
    J[0, 0] = J[1, 1] = J[2, 2] = 1.0
    J[3::2, 0], J[3::2, 2] = 1.0, -r * sn
    J[4::2, 1], J[4::2, 2] = 1.0, r * cs
    P = _mm(_mm(J, _pose_block(rng, 0.3, 0.02)), J.T)
    for i in range(N):
        Gz = np.array([[cs[i], -r[i] * sn[i]], [sn[i], r[i] * cs[i]]])
        P[3 + 2 * i:5 + 2 * i, 3 + 2 * i:5 + 2 * i] += _mm(_mm(Gz, R), Gz.T)
    Qc = np.array([[3.0 ** 2, 0.0], [0.0, (10 * PI / 180) ** 2]])
    v, w, dt = 0.4, 4.0, 1.0
    for _ in range(5):
        g = rng.uniform(-0.2, 0.2)
        s_, c_ = math.sin(g + x[2]), math.cos(g + x[2])
        Gv = np.array([[1.0, 0.0, -v * dt * s_], [0.0, 1.0, v * dt * c_], [0.0, 0.0, 1.0]])
        Gu = np.array([[dt * c_, -v * dt * s_], [dt * s_, v * dt * c_], [dt * math.sin(g) / w, v * dt * math.cos(g) / w]])
        col = _mm(P[:, 0:3], Gv.T)                             # P Gv' on the pose columns, then Gv (..) on the pose rows
        col[0:3] = _mm(Gv, col[0:3]) + _mm(_mm(Gu, Qc), Gu.T)
        P[:, 0:3] = col
        P[0:3, :] = col.T
        x[0:3] = [x[0] + v * dt * c_, x[1] + v * dt * s_, O.mpi_to_pi(x[2] + v * dt * math.sin(g) / w)]
    d = np.hypot(x[3::2] - x[0], x[4::2] - x[1])
    assert d.min() > 1.0
    return x, (P + P.T) / 2


MIXED_SCALES = (1e-6, 1e-4, 1e-2, 1.0, 1e2)


def _state_mixed(rng, N):
    """P = D^1/2 ((1 - rho) I + rho u u') D^1/2, u = +-1: landmark j has the variance MIXED_SCALES[j % 5] (times 1 .. 4 per axis)."""
    n = 3 + 2 * N
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3)])
    x = np.concatenate([pose, _positions(rng, N, _spread(N), pose)])
    d = np.empty(n)
    d[0:3] = [1e-2, 1e-2, 1e-4]
    for j in range(N):
        d[3 + 2 * j:5 + 2 * j] = MIXED_SCALES[j % 5] * rng.uniform(1, 4, 2)
    u = rng.choice([-1.0, 1.0], n)
    rho = 0.3
    Cm = (1 - rho) * np.eye(n) + rho * np.outer(u, u)
    h = np.sqrt(d)
    return x, h[:, None] * Cm * h[None, :]


GEOMETRY_SPECIALS = ((25.0, 0.001953125), (0.0, 0.5), (2000.0, 0.0), (30.0, 30.0), (-0.5, 0.0), (0.0, -2000.0), (-40.0, -40.0),
                     (25.0, -0.001953125))      # (dx, dy) of landmarks 1 .. 8; the first and the last are BEHIND a vehicle heading +-pi


def _state_geometry(rng, N):
    sign = 1.0 if rng.integers(2) else -1.0
    phi = sign * (PI - 5e-4 * rng.uniform(0.2, 0.9))
    x, P = _block_diag_state(rng, N, _spread(N), 1e-2, 1.0, 10.0, phi=phi)
    for j, (dx, dy) in enumerate(GEOMETRY_SPECIALS):
        x[3 + 2 * j], x[4 + 2 * j] = 50.0 + dx, 50.0 + dy      # exact in fp32 too
    return x, P


def _state_rank6(rng, N):
    """`random_state`, its covariance rounded to float32 values in BOTH dtypes: its BLAS product A A' differs in the last place
    between CPUs, and the cells are to be the same bits everywhere (0.01 I keeps it positive definite by a wide margin)."""
    x, P = random_state(rng, N, spread=_spread(N))
    return x, P.astype(np.float32).astype(np.float64)


_STATES = {"independent": _state_independent, "slam": _state_slam, "mixed": _state_mixed, "geometry": _state_geometry,
           "rank6": _state_rank6}


def _wrap_mod(a):
    """Into [-pi, pi): what a sensor reports (a true modulo -- the filter's own wrap is ONE conditional step)."""
    return (np.asarray(a) + PI) % (2 * PI) - PI


def designed_state(cls, N, dtype, seed):
    """(x, P) of class `cls`, float64 arrays that hold values of the dtype exactly, positive definite after the rounding."""
    rng = np.random.default_rng(seed)
    x, P = _STATES[cls](rng, N)
    P = (P + P.T) / 2
    t = NP_DTYPE[dtype]
    x = x.astype(t).astype(np.float64)
    P = P.astype(t).astype(np.float64)
    assert np.array_equal(P, P.T)
    assert_positive_definite(P, f"{cls} N={N} {dtype}")
    return x, P


def assert_positive_definite(P, what):
    """Cholesky of the Jacobi-scaled matrix in float64 (the scaling is exact enough not to matter and keeps `mixed` honest)."""
    d = np.sqrt(np.diag(P))
    assert np.all(d > 0), what
    try:
        np.linalg.cholesky(P / d[:, None] / d[None, :])
    except np.linalg.LinAlgError:
        raise AssertionError(f"{what}: not positive definite after rounding to the dtype")


def choose_ids(cls, rng, N, m):
    """The observed landmarks (1-based): `mixed` starts with one of each scale and leaves one of each unobserved where N - m
    allows it; `geometry` observes the special landmarks first."""
    if cls == "mixed":
        first = rng.permutation(5)
        keep = 5 + rng.permutation(5)                       # landmarks 6 .. 10: unobserved while N - m >= 5
        rest = np.setdiff1d(np.arange(N), np.concatenate([first, keep]))
        order = np.concatenate([first, rng.permutation(rest), keep])
        return order[:m] + 1
    if cls == "geometry":
        ns = len(GEOMETRY_SPECIALS)
        order = np.concatenate([np.arange(ns), ns + rng.permutation(N - ns)])[:m]
        return order[rng.permutation(m)] + 1
    return rng.permutation(N)[:m] + 1


def observations(cls, rng, x, ids):
    """z (2 x m): the predicted observation plus R-sized noise, the bearing as a sensor reports it, in [-pi, pi)."""
    if cls == "rank6":
        return noisy_obs(rng, x, ids)
    zp, _, _ = O.obs_blocks(x, ids)
    z = zp.T + rng.normal(0, [0.1, PI / 180], (len(ids), 2)).T
    if cls == "geometry":                                    # the landmarks behind the vehicle: pushed across the cut
        for i, j in enumerate(ids):
            if j in (1, len(GEOMETRY_SPECIALS)):
                z[1, i] = zp[i, 1] + (-0.01 if x[2] > 0 else 0.01)
    z[1] = _wrap_mod(z[1])
    return z


@functools.lru_cache(maxsize=16)
def make_inputs(cls, N, m, dtype):
    """(x, P, z, ids) of one cell; the form and SLAMHIP_X do not enter."""
    seed = _seed(cls, N, m, dtype)
    x, P = designed_state(cls, N, dtype, seed)
    rng = np.random.default_rng(seed + 7)
    ids = choose_ids(cls, rng, N, m)
    z = observations(cls, rng, x, ids)
    for a in (x, P, z, ids):
        a.setflags(write=False)
    return x, P, z, ids


# ---- linear algebra in any float type -------------------------------------------------------------------------------------------
def _chol(S):
    """Lower Cholesky factor in S's own float type, right-looking: element-wise operations only (see _mm)."""
    M = np.array(S)
    k = M.shape[0]
    L = np.zeros_like(M)
    for j in range(k):
        assert M[j, j] > 0, "S is not positive definite"
        L[j:, j] = M[j:, j] / np.sqrt(M[j, j])
        if j + 1 < k:
            M[j + 1:, j + 1:] -= L[j + 1:, j:j + 1] * L[j + 1:, j:j + 1].T
    return L


def _solve_lower(L, B):
    """inv(L) B by forward substitution, column after column of L."""
    X = np.array(B, dtype=L.dtype)
    X = X.reshape(X.shape[0], -1)
    for j in range(L.shape[0]):
        X[j] = X[j] / L[j, j]
        X[j + 1:] -= L[j + 1:, j:j + 1] * X[j:j + 1]
    return X.reshape(np.shape(B))


def _solve_upper(U, B):
    """inv(U) B by back substitution, column after column of U."""
    X = np.array(B, dtype=U.dtype)
    X = X.reshape(X.shape[0], -1)
    for j in range(U.shape[0] - 1, -1, -1):
        X[j] = X[j] / U[j, j]
        X[:j] -= U[:j, j:j + 1] * X[j:j + 1]
    return X.reshape(np.shape(B))


def front(x, P, z, Rm, ids, ft, wrap=True, hf_bearing_power=2, magnitude=False):
    """Innovation v, A = P H', S = H A + RR symmetrised (oracle/ekf_ref.py: obs_blocks, _update_front; device_math.h:28-42),
    evaluated in the float type `ft`.  `wrap` / `hf_bearing_power` exist for the planted defects; `magnitude` returns |P| |H'| in
    A's place (every product of P H' by its absolute value) and |z| + |zp| in v's."""
    x = np.asarray(x, dtype=ft)
    P = np.asarray(P, dtype=ft)
    z = np.asarray(z, dtype=ft).reshape(2, -1)
    Rm = np.asarray(Rm, dtype=ft)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    m, n = len(ids), len(x)
    pi = ft(PI)
    f = 3 + 2 * (ids - 1)
    dx, dy = x[f] - x[0], x[f + 1] - x[1]
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2)
    db = d2 if hf_bearing_power == 2 else d
    v = np.empty(2 * m, dtype=ft)
    v[0::2] = z[0] - d
    b = z[1] - (np.arctan2(dy, dx) - x[2])
    v[1::2] = np.where(b > pi, b - 2 * pi, np.where(b < -pi, b + 2 * pi, b)) if wrap else b
    Hv = np.zeros((m, 2, 3), dtype=ft)
    Hv[:, 0, 0], Hv[:, 0, 1] = -dx / d, -dy / d
    Hv[:, 1, 0], Hv[:, 1, 1], Hv[:, 1, 2] = dy / d2, -dx / d2, -1
    Hf = np.zeros((m, 2, 2), dtype=ft)
    Hf[:, 0, 0], Hf[:, 0, 1] = dx / d, dy / d
    Hf[:, 1, 0], Hf[:, 1, 1] = -dy / db, dx / db
    if magnitude:
        P, Hv, Hf = np.abs(P), np.abs(Hv), np.abs(Hf)
        v[0::2] = np.abs(z[0]) + d                              # the innovation is a difference of these
        v[1::2] = np.abs(z[1]) + np.abs(np.arctan2(dy, dx)) + np.abs(x[2]) + 2 * pi
    A = np.empty((n, 2 * m), dtype=ft)
    S = np.empty((2 * m, 2 * m), dtype=ft)
    for i in range(m):                                        # the five non-zero columns, in pht_entry's order (ekf_update.hip:45-48)
        for r in range(2):
            A[:, 2 * i + r] = (P[:, 0] * Hv[i, r, 0] + P[:, 1] * Hv[i, r, 1] + P[:, 2] * Hv[i, r, 2] + P[:, f[i]] * Hf[i, r, 0] +
                               P[:, f[i] + 1] * Hf[i, r, 1])
    for i in range(m):
        for r in range(2):
            S[2 * i + r] = (Hv[i, r, 0] * A[0] + Hv[i, r, 1] * A[1] + Hv[i, r, 2] * A[2] + Hf[i, r, 0] * A[f[i]] +
                            Hf[i, r, 1] * A[f[i] + 1])
        S[2 * i:2 * i + 2, 2 * i:2 * i + 2] += Rm
    return v, A, (S + S.T) / 2


def scaled_condition(S):
    S = np.asarray(S, dtype=np.float64)
    h = 1.0 / np.sqrt(np.diag(S))
    return float(np.linalg.cond(h[:, None] * S * h[None, :]))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate(x, P, z, ids, form, Rm=R):
    """One update in extended precision.  Returns a dict: 'x', 'P' = (ref, mag, floor) triples, 'kappa', 'W1' (or 'K', 'T'), 'y'.
    `ref` is formed in longdouble throughout (NumPy's own loops: no BLAS); the magnitudes and floors are sums of non-negative
    terms and are formed in float64."""
    v, A, S = front(x, P, z, Rm, ids, LD)
    f64 = lambda t: np.asarray(t, dtype=np.float64)          # noqa: E731
    vbar, Abar, _ = (f64(t) for t in front(x, P, z, Rm, ids, LD, magnitude=True))      # |z| + |zp|, |P| |H'|
    k = len(v)
    L = _chol(S)
    W1 = _solve_lower(L, A.T).T                              # A inv(L)' = A C
    y = _solve_lower(L, v)                                   # C' v
    g = _solve_upper(L.T, y)                                 # inv(S) v
    Ca = f64(np.abs(_solve_lower(L, np.eye(k, dtype=LD)))).T      # |C|, C = inv(chol(S)) upper
    CUC = Ca @ f64(np.abs(L)).T @ Ca                         # |C| |U| |C|: what an explicitly formed inverse is uncertain by
    aA, aW, ay, av = f64(np.abs(A)), f64(np.abs(W1)), f64(np.abs(y)), f64(np.abs(v))
    Wf = Abar @ Ca + aA @ CUC                                # floor of W1 = (P H') C
    xl, Pl = np.asarray(x, dtype=LD), np.asarray(P, dtype=LD)
    out = {"kappa": scaled_condition(S), "y": y,
           "x": (xl + W1 @ y, f64(np.abs(xl)) + aW @ ay, Wf @ ay + aW @ (CUC.T @ av + Ca.T @ vbar) + aA @ f64(np.abs(g)))}
    if form == "joseph":
        K = _solve_upper(L.T, W1.T).T                        # A inv(S)
        T = A - K @ S / 2
        aK, aT = f64(np.abs(K)), f64(np.abs(T))
        Kf = Wf @ Ca.T + aW @ CUC.T
        Tf = Abar + Kf @ f64(np.abs(S)) / 2
        KT, aKT, fl = K @ T.T, aK @ aT.T, Kf @ aT.T + aK @ Tf.T
        out.update(K=K, T=T, P=(Pl - KT - KT.T, f64(np.abs(Pl)) + aKT + aKT.T, fl + fl.T))
    else:
        fl = Wf @ aW.T
        out.update(W1=W1, P=(Pl - W1 @ W1.T, f64(np.abs(Pl)) + aW @ aW.T, fl + fl.T))
    return out


@functools.lru_cache(maxsize=4)
def restate_cell(cls, N, m, dtype, form):
    x, P, z, ids = make_inputs(cls, N, m, dtype)
    return restate(x, P, z, ids, form)


# ---- the model and the planted defects --------------------------------------------------------------------------------------------
DEFECTS = ("gain_1e-3", "g_last_dropped", "w1_last_column_0.99", "stale_columns", "bf16_two_terms", "front_half_float",
           "bearing_not_wrapped", "hf_over_d", "tile_not_mirrored", "side_stale")
DEFECT_CLASS = {"gain_1e-3": "independent", "g_last_dropped": "independent", "w1_last_column_0.99": "independent",
                "stale_columns": "independent", "bf16_two_terms": "independent", "front_half_float": "slam",
                "bearing_not_wrapped": "geometry", "hf_over_d": "geometry", "tile_not_mirrored": "independent",
                "side_stale": "mixed"}          # the class each defect was designed for
F32_ONLY = ("bf16_two_terms",)


def _bf16(v):
    """float32 -> nearest-even bf16, as float32."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = ((b >> 16) & 1) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _two_term(v):
    """h + m of the three-way bf16 split (ekf_update.hip:1064-1078): the float with its last 8 bits' worth dropped."""
    v = np.asarray(v, dtype=np.float32)
    h = _bf16(v)
    return (h + _bf16(v - h)).astype(np.float64)


def _accumulate(X, Y, t):
    """sum_a X[:, a] Y[:, a]' from zero in the dtype t, column after column: exact products in fp32 (a float64 product of two
    floats is exact, and so -- up to a double rounding nobody sees -- is its sum with the float accumulator)."""
    acc = np.zeros((X.shape[0], Y.shape[0]), dtype=np.float64)
    for a in range(X.shape[1]):
        acc = (acc + np.outer(X[:, a], Y[:, a])).astype(t).astype(np.float64)
    return acc


def model_update(x, P, z, ids, dtype, form, Rm=R, defect=None, previous=None):
    """The correctly rounded model of one update.  Returns (x+, P+, side) as float64 arrays that hold values of the dtype;
    side = [P[f, f], P[f + 1, f], P[f + 1, f + 1]] as the packed side array would hold them.
    `previous` = (z, ids) of an earlier, larger update on the same handle, for the stale-column defect."""
    t = NP_DTYPE[dtype]
    ft = np.float32 if defect == "front_half_float" else np.float64
    n = len(x)

    def panel(z_, ids_):
        v, A, S = front(x, P, z_, Rm, ids_, ft, wrap=defect != "bearing_not_wrapped",
                        hf_bearing_power=1 if defect == "hf_over_d" else 2)
        L = _chol(S)
        C = _solve_lower(L, np.eye(len(v), dtype=ft)).T       # inv(chol(S)), upper: explicit, as the device forms it
        return v, A, S, C

    v, A, S, C = panel(z, ids)
    g = _mm(C, _mm(C.T, v[:, None]))[:, 0]
    if defect == "g_last_dropped":
        g[-1] = 0
    dxv = _mm(A, g[:, None])[:, 0]
    if defect == "gain_1e-3":
        dxv = dxv * (1 + 1e-3)
    xn = (np.asarray(x, dtype=np.float64) + dxv.astype(np.float64)).astype(t).astype(np.float64)
    if form == "joseph":
        K = _mm(A, _mm(C, C.T))
        T = A - 0.5 * _mm(K, S)
        X, Y = np.hstack([K, T]), np.hstack([T, K])
    else:
        X = _mm(A, C)
        Y = X
    X, Y = (np.asarray(M, dtype=np.float64).astype(t).astype(np.float64) for M in (X, Y))
    k = X.shape[1]
    if defect == "w1_last_column_0.99":
        X = X.copy()
        X[:, k - 1] *= 0.99
        X = X.astype(t).astype(np.float64)
        Y = X if form != "joseph" else Y
    if defect == "stale_columns":
        # the panel of the earlier update stays behind this one's columns: from column 96 on where this update is that wide
        # (a chunk not rewritten), else in the padding up to the next multiple of 16 (the padding not zeroed)
        assert previous is not None and form != "joseph"
        _, Ap, _, Cp = panel(*previous)
        Wp = _mm(Ap, Cp).astype(t).astype(np.float64)
        c0 = 96 if k > 96 else k
        c1 = k if k > 96 else min(Wp.shape[1], -(-k // 16) * 16)
        assert Wp.shape[1] >= c1 > c0
        X = np.hstack([X[:, :c0], Wp[:, c0:c1]])
        Y = X
    if defect == "bf16_two_terms":
        X = _two_term(X)
        Y = X if form != "joseph" else _two_term(Y)
    acc = _accumulate(X, Y, t)
    Pn = (np.asarray(P, dtype=np.float64) - acc).astype(t).astype(np.float64)
    Pn = np.tril(Pn) + np.tril(Pn, -1).T                     # one triangle is computed, the other mirrored
    if defect == "tile_not_mirrored":
        E = TILE[dtype]
        assert n > E, "needs a second tile row"
        Pn[0:E, E:min(n, 2 * E)] = np.asarray(P, dtype=np.float64)[0:E, E:min(n, 2 * E)]
    f = 3 + 2 * np.arange((n - 3) // 2)
    src = np.asarray(P, dtype=np.float64) if defect == "side_stale" else Pn
    side = np.stack([src[f, f], src[f + 1, f], src[f + 1, f + 1]])
    return xn, Pn, side


# ---- judging a result -------------------------------------------------------------------------------------------------------
def derived_limit_p32(form, m):
    """The derivation's worst case for c_32: 3.5 + 6 K, K the number of panel columns that hold a term."""
    return 3.5 + 6 * (4 * m if form == "joseph" else 2 * m)


def _over(err, den):
    """err / den per entry; where the denominator is zero the entry must be exact (0, else inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0.0, np.inf))


def ratios(xg, Pg, ref, dtype):
    """What the constants would have to be for this result: dict x, P (units 2^-53 (kappa mag + floor)), P32 (units 2^-24 mag,
    fp32 only, where P is not separated: the fp64 constant comes from the fp64 cells)."""
    kap = ref["kappa"]
    xr, xm, xf = ref["x"]
    Pr, Pm, Pf = ref["P"]
    xg, Pg = np.asarray(xg, dtype=LD), np.asarray(Pg, dtype=LD)
    assert xg.shape == xr.shape and Pg.shape == Pr.shape
    ex = np.maximum(np.abs(xg - xr) - LD(U_T[dtype]) * np.abs(xr), 0)
    eP = np.abs(Pg - Pr)
    out = {"x": float(np.max(_over(ex, LD(EPS53) * (kap * xm + xf))))}
    if dtype == "f32":
        out["P32"] = float(np.max(_over(eP, LD(U32) * Pm)))
    else:
        out["P"] = float(np.max(_over(eP, LD(EPS53) * (kap * Pm + Pf))))
    return out


def bound_constants(cls, dtype, form, m, margins=None):
    """(c_x, c_P, c_32) of a cell: the committed margins, c_32 never above the derived worst case (and absent in fp64)."""
    cx, cP, c32 = (MARGINS if margins is None else margins)[form][cls]
    return cx * C_FACTOR, cP * C_FACTOR, (min(c32, derived_limit_p32(form, m)) if dtype == "f32" else 0.0)


def judge(xg, Pg, ref, cls, dtype, form, m, what="", log=None, margins=None, enforce=True):
    """Every entry of x and P against its bound.  Returns the worst error / bound per quantity ({'x': .., 'P': ..}; for x: what
    is left of the error after the storage rounding u_T |ref|, over the fp64 term); raises AssertionError outside the bound
    unless enforce=False.  `log` keeps the running maximum per quantity when a dict is passed."""
    kap = ref["kappa"]
    cx, cP, c32 = bound_constants(cls, dtype, form, m, margins)
    assert max(cx, cP) * EPS53 * kap < KAPPA_SLACK * C_FACTOR, f"{what}: kappa = {kap:.3g} makes the bound slack"
    xr, xm, xf = ref["x"]
    Pr, Pm, Pf = ref["P"]
    xg, Pg = np.asarray(xg, dtype=LD), np.asarray(Pg, dtype=LD)
    assert xg.shape == xr.shape and Pg.shape == Pr.shape, what
    # x: the one storage rounding u_T |ref| is taken off first, what is left is held to the fp64 term (the same condition as
    # |got - ref| <= u_T |ref| + c_x 2^-53 kappa mag, but the reported ratio then says how much of the fp64 term was used)
    bx = LD(cx * EPS53) * (kap * xm + xf)
    bP = LD(c32 * U32) * Pm + LD(cP * EPS53) * (kap * Pm + Pf)
    ex, eP = np.maximum(np.abs(xg - xr) - LD(U_T[dtype]) * np.abs(xr), 0), np.abs(Pg - Pr)
    qx, qP = _over(ex, bx), _over(eP, bP)
    worst = {"x": float(np.max(qx)), "P": float(np.max(qP))}
    if log is not None:
        for q, w in worst.items():
            log[q] = max(log.get(q, 0.0), w)
    if enforce:
        for q, arr, got, refv in (("x", qx, xg, xr), ("P", qP, Pg, Pr)):
            if not worst[q] <= 1.0:
                i = np.unravel_index(int(np.argmax(arr)), arr.shape)
                raise AssertionError(f"{what}: {int(np.sum(arr > 1))} of {arr.size} entries of {q} outside the bound, worst at {i}: "
                                     f"got {float(got[i])!r}, ref {float(refv[i])!r}, error / bound = {worst[q]:.3g} (kappa {kap:.3g})")
    return worst


def structure_ok(Pg, side):
    """P exactly symmetric and the packed side array equal to the matrix's own entries (check_side's condition)."""
    n = Pg.shape[0]
    f = 3 + 2 * np.arange((n - 3) // 2)
    return bool(np.array_equal(Pg, Pg.T) and np.array_equal(side[0], Pg[f, f]) and np.array_equal(side[1], Pg[f + 1, f]) and
                np.array_equal(side[2], Pg[f + 1, f + 1]))


def accepted(xg, Pg, side, ref, cls, dtype, form, m, margins=None):
    """Would the per-entry checks (bounds, symmetry, side array) let this result through?"""
    w = judge(xg, Pg, ref, cls, dtype, form, m, enforce=False, margins=margins)
    return structure_ok(Pg, side) and w["x"] <= 1.0 and w["P"] <= 1.0


def tol_accepts(xg, Pg, side, ref, P0, dtype, form):
    """Would `_check` of tests/test_gpu_ekf_dispatch.py (TOL, symmetry, check_side) let this result through?"""
    xo, Po = np.asarray(ref["x"][0], dtype=np.float64), np.asarray(ref["P"][0], dtype=np.float64)
    return bool(structure_ok(Pg, side) and relerr(xg, xo) <= TOL[dtype]["x"] and
                relerr_cov(Pg, Po, np.diag(P0)) <= TOL[dtype]["P"] * (2.0 if form == "joseph" else 1.0))


def untouched_rows(N, ids):
    """State indices of the landmarks NOT in ids (1-based)."""
    un = np.setdiff1d(np.arange(1, N + 1), np.asarray(ids))
    f = 3 + 2 * (un - 1)
    return np.sort(np.concatenate([f, f + 1]))


# ---- the cells -----------------------------------------------------------------------------------------------------------
NS = (66, 127, 200)
MS = (1, 8, 16, 17, 32, 33, 48, 49, 64, 65)


def _n_for(ci, mi, m):
    N = NS[(ci + mi) % 3]
    return 127 if (m > N - 5) else N                          # m = 65 at N = 66: `mixed` keeps one landmark of each scale unobserved


def _cells():
    out = []
    for ci, cls in enumerate(CLASSES):
        for mi, m in enumerate(MS):
            N = _n_for(ci, mi, m)
            out.append(Cell(cls, N, m, "f32", "cholesky"))                         # every class, every m: fp32 reference form
            if (mi + ci) % 2 == 0 or m in (17, 65):
                out.append(Cell(cls, NS[(ci + mi + 1) % 3] if m < 60 else 200, m, "f32", "joseph"))
            if (mi + ci) % 3 == 0 or m == 65:
                out.append(Cell(cls, NS[(ci + mi + 2) % 3] if m < 60 else 127, m, "f64", "cholesky"))
            if (mi + ci) % 3 == 1:
                out.append(Cell(cls, _n_for(ci, mi + 1, m), m, "f64", "joseph"))
    return out


CELLS = _cells()
# SLAMHIP_X (read when the handle is created): each value on two cells
X_CELLS = [Cell(CLASSES[(i + j) % 4], (127, 200)[j], (33, 64)[j], "f32", "cholesky", xf)
           for i, xf in enumerate((4, 8, 16, 128)) for j in range(2)]
# observe(): host bound nz, device count j -> the three fallbacks, on `independent`
OBSERVE_CELLS = [(127, 64, 40), (127, 64, 17), (127, 64, 0)]
SCHEDULE_MS = (64, 17, 64)                                    # one handle, `independent`, N = 127


@functools.lru_cache(maxsize=4)
def observe_case(N, nz, j):
    """(x, P, z, assoc) for observe() on `independent` in fp32: nz observations of which the oracle matches exactly j (the others
    fall between the gates 4 and 25: neither matched nor new), built as tests/test_gpu_ekf_dispatch.py builds them."""
    from tests.test_gpu_ekf_dispatch import _observe_oracle, observe_inputs
    seed = 5_000_000 + 1000 * N + 10 * nz + j
    x, P = designed_state("independent", N, "f32", seed)
    rng = np.random.default_rng(seed + 7)
    z = observe_inputs(rng, x, P, N, nz, j)
    return x, P, z, _observe_oracle(x, P, z, j, 0)


def cell_paths():
    out = [expected_path(c.dtype, c.form, c.m, c.xflags) for c in CELLS + X_CELLS]
    out += [expected_path("f32", "cholesky", nz, 0, device_m=j) for _N, nz, j in OBSERVE_CELLS]
    return out


def cell_id(c):
    return f"{c.cls}-N{c.N}-m{c.m}-{c.dtype}-{c.form}" + (f"-X{c.xflags}" if c.xflags else "")


# ---- the margins, from the model -------------------------------------------------------------------------------------------
def model_needs(cells=None):
    """{(form, class): {quantity: the largest ratio the model needs over the class's cells}} and the per-cell rows."""
    need, rows = {}, []
    for c in (CELLS if cells is None else cells):
        x, P, z, ids = make_inputs(c.cls, c.N, c.m, c.dtype)
        ref = restate_cell(c.cls, c.N, c.m, c.dtype, c.form)
        xm, Pm, _ = model_update(x, P, z, ids, c.dtype, c.form)
        r = ratios(xm, Pm, ref, c.dtype)
        rows.append((c, ref["kappa"], r))
        slot = need.setdefault((c.form, c.cls), {})
        for q, v in r.items():
            slot[q] = max(slot.get(q, 0.0), v)
    return need, rows


def margins_from(need):
    """The rule: max(4, 4 x need) per form and class, in MARGINS' layout."""
    return {f: {c: tuple(max(4.0, 4 * need[(f, c)].get(q, 0.0)) for q in ("x", "P", "P32")) for c in CLASSES} for f in FORMS}
