"""The landmark merge (slam_ekf_merge_landmarks, csrc/ekf_merge.hip) entry by entry: designed states, a one-call restatement in
extended precision with a DERIVED per-entry bound, a correctly rounded model of each dtype, and planted defects.  Host-only
NumPy; nothing here needs a GPU.  Companion of tests/update_records.py, whose helpers, `judge` and margin rule it uses as they are.

Why
    tests/test_gpu_ekf_merge.py holds the merge to max(TOL, 4 x an 8-observation update's error) of max|x| and sqrt(P_ii P_jj)
    on `grid_state` = `random_state` (A A' + 0.01 I, A of rank 6): the class tests/update_records.py:5-9 shows to hide errors.  A
    mean correction scaled by 1.001 passes it in fp32 (tests/test_merge_records_cpu.py prints the list).

The states (`make_inputs`), each already rounded to the dtype and positive definite after that rounding
    independent, slam, mixed, rank6   update_records.designed_state, unchanged (`geometry` is not used: H is linear here).
    duplicates   the `slam` state, then every b_p entered AGAIN as a second sighting of a_p from the current, drifted pose by
                 add_features' formula: P_b,: = Gv P_v,:, P_bb = Gv P_vv Gv' + Gz R Gz', Gv and Gz at a_p's range and bearing from
                 the pose -- what gated association produces after a loop.  D is a difference of large, correlated entries.
    echo         b_p is a_p plus independent noise, on `independent` or `slam`: the rows and columns of b_p are bit copies of
                 a_p's, P_bb = P_aa + D0 with D0 a well-conditioned 2 x 2 of P_aa's scale (P_aa is first put on a grid of
                 2^-12 of that scale, so that the sum is exact in both dtypes).  P H' is then exactly zero in every row but
                 b_p's: every survivor's entry of x and row of P must come back BIT FOR BIT.
    Means: x_b = x_a + L u sqrt(t), L L' = D (merge_ref.difference), |u| = 1, t from {0.25, 2, 4}: the correction has the size a
    real merge has.  Rc is NULL or [[0.02, 0.005], [0.005, 0.03]]; on `mixed` times the geometric mean of the call's tr D / 2
    (the ABI takes ONE Rc per call; with one pair that is the pair's own tr D / 2).
    Pairs (`pairs_for`): survivor first and removed last, b < a, an adjacent pair, tile-edge straddlers (f(j) + 1 a multiple of
    128 in fp32, of 64 in fp64) as a and as b; `mixed` at cnt = 8 has a pair inside every scale and one or more across.

The restatement (`restate`)
    ONE merge before the removal in np.longdouble: merge_ref.fuse's formulas with update_records' hand-written Cholesky and
    triangular solves, and the `keep` index of the removal (bit-exact, DESIGN 5.4: the reference after it is ref[keep],
    `after_removal`).  Per entry `ref`, `mag` and `floor`, and kappa = cond(D^-1/2 S D^-1/2), laid out as
    update_records.restate returns them for the Cholesky form, so that update_records.judge is used as it is.

The bound, from what ekf_merge.hip does (line numbers of that file)
    merge_pht (:108-111)          an entry of P H' is ONE difference P[r, fa + c] - P[r, fb + c] in double: off by
                                  2^-53 (|P[r, fa + c]| + |P[r, fb + c]|) however far it cancels -- this is |P| |H'| here.
    merge_factor_kernel :139-148  S from 4 k^2 gathered entries, (A[fa + r, j] - A[fb + r, j]) + Rc, in double.
                    :153          v = -(x_a - x_b): off by 2^-53 (|x_a| + |x_b|), the |z| + |zp| of the update.
                    :158-166      S symmetrised (exact: a mean of two doubles).
                    :168-182      right-looking Cholesky in double; :186-192 inv(L) formed EXPLICITLY by columns
                                  (|dC| <= 2^-53 |C| |U| |C|, Higham 14.1); :194-204 g = C (C' v).
    merge_panel_kernel :230-244   W1 = P H' C summed over i <= j in double, rounded ONCE to the dtype (:238);
                                  x = (T)(x + sum_j PHt[r][j] g[j]) (:244): one rounding u_T |ref|.
    launch_merge_update :331      launch_downdate with 16 columns, no pre-split image: the f32_tile body (exact fp32 products,
                                  fp32 accumulation from zero, one subtraction) or the fp64 body, both held by the update records.
    With Wf = |P||H'| |C| + |P H'| |C||U||C| (units of 2^-53) exactly as in update_records (its docstring, "The floor"):
        floor(P) = Wf |W1|' + |W1| Wf'
        floor(x) = Wf |y| + |W1| ((|C||U||C|)' |v| + |C|' (|x_a| + |x_b|)) + |P H'| |g|
        x        |got - ref| <= u_T |ref| + c_x 2^-53 (kappa mag + floor)
        P, fp64  |got - ref| <= c_P 2^-53 (kappa mag + floor)
        P, fp32  |got - ref| <= c_32 2^-24 mag + c_P 2^-53 (kappa mag + floor),    c_32 <= 3.5 + 6 (2 cnt) by derivation
    (update_records.derived_limit_p32; the padding columns 2 cnt .. 15 add exact zeros).  What is ASSERTED is the margin rule of
    DESIGN 5.2a: MARGINS[class] = (c_x, c_P, c_32) = max(4, 4 x what `model_merge` needs on the class's own cells), committed
    here, re-derived by tests/test_merge_records_cpu.py, never above the derived limit.  Nothing in the table comes from a
    device.  No entry is excluded; an entry whose mag and floor are both zero must be exact; every cell keeps
    c 2^-53 kappa < KAPPA_SLACK (checked on the CPU).

The model (`model_merge`)
    float64 front half as the device forms it (explicit C = inv(chol S), g = C (C' v), W1 = P H' C, x = (T)(x + P H' g)), W1
    rounded to the dtype, products exact (fp32) or rounded once (fp64), the sum accumulated from zero in the dtype column after
    column, one subtraction, lower triangle mirrored, then the removal.  `defect=` plants one of DEFECTS in it.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import merge_ref as MR
from tests import update_records as U
from tests.strip_ref import C_FACTOR, EPS53, LD, NP_DTYPE, TILE, U_T   # noqa: F401  (re-exported for the tests)
from tests.test_gpu_ekf import R, TOL, relerr, relerr_cov
from tests.update_records import (KAPPA_SLACK, _accumulate, _chol, _mm, _over, _solve_lower, _solve_upper,   # noqa: F401
                                  assert_positive_definite, designed_state, scaled_condition)

PI = math.pi
CLASSES = ("independent", "slam", "mixed", "rank6", "duplicates", "echo")
RC = np.array([[0.02, 0.005], [0.005, 0.03]])
T_SET = (0.25, 2.0, 4.0)                # d2 of the planted pairs

# MARGINS[class] = (c_x, c_P, c_32): max(4, 4 x the model's need) over the class's cells of CELLS.  c_x and c_P (units
# 2^-53 (kappa mag + floor)) belong to the fp64 front half and hold for both dtypes; c_32 (units 2^-24 mag) is fp32's own.
# Re-derived by tests/test_merge_records_cpu.py::test_committed_margins_follow_the_rule, which prints the table to commit.
MARGINS = {"independent": (4.0, 4.0, 10.8),
           "slam": (4.0, 4.0, 20.6),
           "mixed": (4.0, 4.0, 11.8),
           "rank6": (4.0, 4.0, 13.3),
           "duplicates": (4.0, 4.0, 4.2),
           "echo": (4.0, 4.0, 4.0)}

Cell = namedtuple("Cell", "cls N cnt dtype noisy")


# ---- pairs ----------------------------------------------------------------------------------------------------------------
def straddlers(dtype, N):
    """Landmarks whose two state indices lie in two tiles: f(j) + 1 a multiple of the tile edge."""
    E = TILE[dtype]
    return [k * E // 2 - 1 for k in range(1, 2 * N // E + 2) if 2 <= k * E // 2 - 1 <= N]


def pairs_for(cls, dtype, N, cnt):
    """cnt disjoint pairs (a_p, b_p), N = 2 or N >= 66: the first landmark survives and the last one leaves, a straddler as
    a and (where the map has a second one that is not N, else the first landmark of the next tile) as b, pairs with b < a, an
    adjacent pair.  `mixed` (scale of landmark j: (j - 1) % 5): pairs 4 .. 8 lie inside one scale each, pair 3 crosses two
    (pairs 1 and 2 do where their ids fall so)."""
    if N == 2:
        assert cnt == 1
        return ((1, 2),)
    assert N >= 66 and 1 <= cnt <= 8
    S = straddlers(dtype, N)
    Sa = S[0]
    Sb = next((s for s in S[1:] if s != N), Sa + 1)
    if cls == "mixed":
        base = [(1, N), (Sa, 16), (50, Sb), (11, 6), (12, 7), (8, 13), (9, 14), (10, 15)]
    else:
        base = [(1, N), (Sa, 12), (50, Sb), (45, 40), (20, 21), (7, 26), (55, 9), (33, 58)]
    flat = [j for p in base for j in p]
    assert len(set(flat)) == 16 and max(flat) <= N
    return tuple(base[:cnt])


def keep_index(n, pairs):
    """State indices that stay when every b_p leaves."""
    rm = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:, 1]
    return np.delete(np.arange(n), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))


def untouched_rows(N, pairs):
    """State indices of the landmarks in no pair."""
    un = np.setdiff1d(np.arange(1, N + 1), np.asarray(pairs).reshape(-1))
    f = 3 + 2 * (un - 1)
    return np.sort(np.concatenate([f, f + 1]))


# ---- the designed states ----------------------------------------------------------------------------------------------------
def _seed(cls, N, cnt, dtype):
    return 7_000_000 + 1_000_000 * CLASSES.index(cls) + 1000 * N + 10 * cnt + (dtype == "f64")


def _reenter(x, P, pairs):
    """`duplicates`: every b_p becomes a second sighting of a_p from the current pose (add_features' formula, src/ekf.jl:84-122)."""
    for a, b in pairs:
        fa, fb = MR.f(a), MR.f(b)
        dx, dy = x[fa] - x[0], x[fa + 1] - x[1]
        r = math.hypot(dx, dy)
        Gv = np.array([[1.0, 0.0, -dy], [0.0, 1.0, dx]])
        Gz = np.array([[dx / r, -dy], [dy / r, dx]])
        rows = _mm(Gv, P[0:3, :])
        P[fb:fb + 2, :] = rows
        P[:, fb:fb + 2] = rows.T
        P[fb:fb + 2, fb:fb + 2] = _mm(_mm(Gv, P[0:3, 0:3]), Gv.T) + _mm(_mm(Gz, R), Gz.T)
    return (P + P.T) / 2


def _echo(P, pairs):
    """`echo`: P_aa on a grid of 2^-12 of its scale, the rows and columns of b_p copies of a_p's, P_bb = P_aa + D0."""
    n = P.shape[0]
    src = np.arange(n)
    scales = []
    for a, b in pairs:
        fa, fb = MR.f(a), MR.f(b)
        s = 2.0 ** math.floor(math.log2((P[fa, fa] + P[fa + 1, fa + 1]) / 2))
        q = s / 4096
        P[fa:fa + 2, fa:fa + 2] = np.round(P[fa:fa + 2, fa:fa + 2] / q) * q
        src[fb:fb + 2] = [fa, fa + 1]
        scales.append(s)
    P = P[np.ix_(src, src)]
    for (a, b), s in zip(pairs, scales):
        fb = MR.f(b)
        P[fb:fb + 2, fb:fb + 2] += s * np.array([[1.0, 0.25], [0.25, 0.75]])
    return P


def _chol2(D):
    l00 = math.sqrt(D[0, 0])
    l10 = D[0, 1] / l00
    return np.array([[l00, 0.0], [l10, math.sqrt(D[1, 1] - l10 * l10)]])


def place_means(x, P, pairs, dtype, rng):
    """x with every b_p at x_a + L u sqrt(t), L L' = D of the pair, |u| = 1, t from T_SET in turn; rounded to the dtype."""
    x = np.array(x, dtype=np.float64)
    for i, (a, b) in enumerate(pairs):
        _d, D = MR.difference(x, P, a, b)
        assert D[0, 0] > 0 and D[0, 0] * D[1, 1] - D[0, 1] ** 2 > 0, ("D is not positive definite", a, b)
        phi = rng.uniform(0, 2 * PI)
        step = _mm(_chol2(D), np.array([[math.cos(phi)], [math.sin(phi)]]))[:, 0] * math.sqrt(T_SET[i % 3])
        x[MR.f(b):MR.f(b) + 2] = x[MR.f(a):MR.f(a) + 2] + step
    return x.astype(NP_DTYPE[dtype]).astype(np.float64)


def echo_base(N, cnt):
    return "slam" if (N + cnt) % 2 == 0 else "independent"


def rc_for(cls, x, P, pairs, noisy):
    if not noisy:
        return None
    if cls != "mixed":
        return RC.copy()
    half_traces = [np.trace(MR.difference(x, P, a, b)[1]) / 2 for a, b in pairs]
    return RC * math.exp(sum(math.log(h) for h in half_traces) / len(half_traces))


@functools.lru_cache(maxsize=8)
def _state(cls, N, cnt, dtype):
    seed = _seed(cls, N, cnt, dtype)
    pairs = pairs_for(cls, dtype, N, cnt)
    if cls in ("duplicates", "echo"):
        rng = np.random.default_rng(seed)
        x, P = U._STATES["slam" if cls == "duplicates" else echo_base(N, cnt)](rng, N)
        P = (P + P.T) / 2
        P = _reenter(x, P, pairs) if cls == "duplicates" else _echo(P, pairs)
        t = NP_DTYPE[dtype]
        x, P = x.astype(t).astype(np.float64), P.astype(t).astype(np.float64)
        assert np.array_equal(P, P.T)
        assert_positive_definite(P, f"{cls} N={N} cnt={cnt} {dtype}")
    else:
        x, P = designed_state(cls, N, dtype, seed)
    x = place_means(x, P, pairs, dtype, np.random.default_rng(seed + 7))
    x.setflags(write=False)
    P.setflags(write=False)
    return x, P, pairs


def make_inputs(cls, N, cnt, dtype, noisy):
    """(x, P, pairs, Rc) of one cell: float64 arrays that hold values of the dtype exactly; read-only, cached."""
    x, P, pairs = _state(cls, N, cnt, dtype)
    return x, P, pairs, rc_for(cls, x, P, pairs, noisy)


# ---- the front half in any float type -----------------------------------------------------------------------------------------
def front(x, P, pairs, Rc, ft, magnitude=False, transposed=False):
    """v, A = P H', S = H A + blockdiag(Rc) symmetrised, as ekf_merge.hip forms them (merge_pht, merge_factor_kernel), in the
    float type `ft`.  `magnitude`: every difference replaced by the sum of the absolute values (|x_a| + |x_b|, |P||H'|).
    `transposed` plants the defect: P_ab read as its transpose in the column differences."""
    x = np.asarray(x, dtype=ft)
    P = np.asarray(P, dtype=ft)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    fa, fb = 3 + 2 * (pairs[:, 0] - 1), 3 + 2 * (pairs[:, 1] - 1)
    n, k = len(x), 2 * len(pairs)
    RR = np.zeros((2, 2), dtype=ft) if Rc is None else np.asarray(Rc, dtype=ft)
    if transposed:
        P = P.copy()
        for p in range(len(pairs)):
            blk = P[fa[p]:fa[p] + 2, fb[p]:fb[p] + 2].copy()
            P[fa[p]:fa[p] + 2, fb[p]:fb[p] + 2] = blk.T
            P[fb[p]:fb[p] + 2, fa[p]:fa[p] + 2] = blk
    if magnitude:
        x, P, RR = np.abs(x), np.abs(P), np.abs(RR)
    sg = ft(1) if magnitude else ft(-1)
    A = np.empty((n, k), dtype=ft)
    v = np.empty(k, dtype=ft)
    for q in range(len(pairs)):
        for c in range(2):
            A[:, 2 * q + c] = P[:, fa[q] + c] + sg * P[:, fb[q] + c]
            v[2 * q + c] = x[fa[q] + c] + sg * x[fb[q] + c]
    if not magnitude:
        v = -v
    S = np.empty((k, k), dtype=ft)
    for p in range(len(pairs)):
        for r in range(2):
            S[2 * p + r] = A[fa[p] + r] + sg * A[fb[p] + r]
        S[2 * p:2 * p + 2, 2 * p:2 * p + 2] += RR
    return v, A, (S + S.T) / 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate(x, P, pairs, Rc=None):
    """One merge in extended precision BEFORE the removal.  Returns a dict: 'x', 'P' = (ref, mag, floor) triples, 'kappa',
    'W1', 'y', 'A' and 'keep'."""
    v, A, S = front(x, P, pairs, Rc, LD)
    f64 = lambda t: np.asarray(t, dtype=np.float64)          # noqa: E731
    vbar, Abar, _ = (f64(t) for t in front(x, P, pairs, Rc, LD, magnitude=True))      # |x_a| + |x_b|, |P| |H'|
    k = len(v)
    L = _chol(S)
    W1 = _solve_lower(L, A.T).T                              # A inv(L)' = A C
    y = _solve_lower(L, v)                                   # C' v
    g = _solve_upper(L.T, y)                                 # inv(S) v
    Ca = f64(np.abs(_solve_lower(L, np.eye(k, dtype=LD)))).T      # |C|, C = inv(chol(S)) upper
    CUC = Ca @ f64(np.abs(L)).T @ Ca                         # |C| |U| |C|
    aA, aW, ay, av, ag = (f64(np.abs(t)) for t in (A, W1, y, v, g))
    Wf = Abar @ Ca + aA @ CUC                                # floor of W1 = (P H') C
    xl, Pl = np.asarray(x, dtype=LD), np.asarray(P, dtype=LD)
    fl = Wf @ aW.T
    return {"kappa": scaled_condition(S), "y": y, "W1": W1, "A": A, "keep": keep_index(len(xl), pairs),
            "x": (xl + W1 @ y, f64(np.abs(xl)) + aW @ ay, Wf @ ay + aW @ (CUC.T @ av + Ca.T @ vbar) + aA @ ag),
            "P": (Pl - W1 @ W1.T, f64(np.abs(Pl)) + aW @ aW.T, fl + fl.T)}


def after_removal(ref):
    """The restatement after every b_p has left: every triple indexed by `keep` (the compaction moves bits)."""
    keep = ref["keep"]
    return {"kappa": ref["kappa"], "x": tuple(t[keep] for t in ref["x"]), "P": tuple(t[np.ix_(keep, keep)] for t in ref["P"])}


@functools.lru_cache(maxsize=4)
def restate_cell(cell):
    x, P, pairs, Rc = make_inputs(*cell)
    return after_removal(restate(x, P, pairs, Rc))


# ---- the model and the planted defects --------------------------------------------------------------------------------------------
DEFECTS = ("gain_1e-3", "g_last_dropped", "w1_last_column_0.99", "stale_columns", "stale_image", "cross_block_transposed",
           "rc_diagonal_swapped", "rc_dropped", "v_sign", "front_half_float", "side_stale")
DEFECT_CLASS = {"gain_1e-3": "independent", "g_last_dropped": "independent", "w1_last_column_0.99": "independent",
                "stale_columns": "independent", "stale_image": "independent", "cross_block_transposed": "slam",
                "rc_diagonal_swapped": "independent", "rc_dropped": "independent", "v_sign": "independent",
                "front_half_float": "duplicates", "side_stale": "mixed"}          # the class each defect was designed for


def update_panel(x, P, z, ids, dtype):
    """W1 of an ordinary update of the same state, rounded to the dtype: what stays behind in the handle's panel."""
    _v, A, S = U.front(x, P, z, R, ids, np.float64)
    C = _solve_lower(_chol(S), np.eye(S.shape[0])).T
    return _mm(A, C).astype(NP_DTYPE[dtype]).astype(np.float64)


def model_merge(x, P, pairs, Rc, dtype, defect=None, previous=None):
    """The correctly rounded model of one merge call.  Returns (x+, P+, side) AFTER the removal, float64 arrays that hold values
    of the dtype; side as the packed side array would hold it.  `previous` = (z, ids) of an earlier update on the same handle
    (8 observations for `stale_columns`, 64 for `stale_image`)."""
    t = NP_DTYPE[dtype]
    ft = np.float32 if defect == "front_half_float" else np.float64
    if defect == "rc_dropped":
        assert Rc is not None
        Rc = None
    if defect == "rc_diagonal_swapped":
        assert Rc is not None
        Rc = np.array([[Rc[1][1], Rc[0][1]], [Rc[1][0], Rc[0][0]]])
    v, A, S = front(x, P, pairs, Rc, ft, transposed=defect == "cross_block_transposed")
    if defect == "v_sign":
        v = -v
    k = len(v)
    C = _solve_lower(_chol(S), np.eye(k, dtype=ft)).T         # inv(chol(S)), upper: explicit, as the device forms it
    g = _mm(C, _mm(C.T, v[:, None]))[:, 0]
    if defect == "g_last_dropped":
        g[-1] = 0
    dxv = _mm(A, g[:, None])[:, 0]
    if defect == "gain_1e-3":
        dxv = dxv * (1 + 1e-3)
    xn = (np.asarray(x, dtype=np.float64) + dxv.astype(np.float64)).astype(t).astype(np.float64)
    X = np.asarray(_mm(A, C), dtype=np.float64).astype(t).astype(np.float64)
    if defect == "w1_last_column_0.99":
        X[:, k - 1] *= 0.99
        X = X.astype(t).astype(np.float64)
    if defect == "stale_columns":
        assert previous is not None and k < 16 and len(previous[1]) == 8
        X = np.hstack([X, update_panel(x, P, *previous, dtype)[:, k:16]])
    if defect == "stale_image":
        assert previous is not None and len(previous[1]) >= 8
        X = update_panel(x, P, *previous, dtype)[:, :16]
    P0 = np.asarray(P, dtype=np.float64)
    Pn = (P0 - _accumulate(X, X, t)).astype(t).astype(np.float64)
    Pn = np.tril(Pn) + np.tril(Pn, -1).T                     # one triangle is computed, the other mirrored
    keep = keep_index(len(xn), pairs)
    xn, Pn = xn[keep], Pn[np.ix_(keep, keep)]
    src = P0[np.ix_(keep, keep)] if defect == "side_stale" else Pn
    f = 3 + 2 * np.arange((len(xn) - 3) // 2)
    return xn, Pn, np.stack([src[f, f], src[f + 1, f], src[f + 1, f + 1]])


# ---- judging a result -------------------------------------------------------------------------------------------------------
def _as_form(margins):
    return {"cholesky": MARGINS if margins is None else margins}


def judge(xg, Pg, ref, cls, dtype, cnt, what="", log=None, margins=None, enforce=True):
    """update_records.judge as it is, with this file's margins: every entry of x and P (after the removal) against its bound."""
    return U.judge(xg, Pg, ref, cls, dtype, "cholesky", cnt, what=what, log=log, margins=_as_form(margins), enforce=enforce)


def accepted(xg, Pg, side, ref, cls, dtype, cnt, margins=None):
    """Would the per-entry checks (bounds, symmetry, side array) let this result through?"""
    w = judge(xg, Pg, ref, cls, dtype, cnt, enforce=False, margins=margins)
    return U.structure_ok(Pg, side) and w["x"] <= 1.0 and w["P"] <= 1.0


def tol_accepts(xg, Pg, side, ref, P0, keep, dtype):
    """Would the acceptance of tests/test_gpu_ekf_merge.py (TOL, symmetry, check_side) let this result through?  (The test
    there allows max(TOL, 4 x an update's error): whatever passes TOL passes it.)"""
    xo, Po = np.asarray(ref["x"][0], dtype=np.float64), np.asarray(ref["P"][0], dtype=np.float64)
    return bool(U.structure_ok(Pg, side) and relerr(xg, xo) <= TOL[dtype]["x"] and
                relerr_cov(Pg, Po, np.diag(P0)[keep]) <= TOL[dtype]["P"])


# ---- the cells -----------------------------------------------------------------------------------------------------------
SHAPES = ((2, 1),) + tuple((N, cnt) for N in (66, 127, 200) for cnt in (1, 3, 8))
COMBOS = (("f32", False), ("f64", True), ("f32", True), ("f64", False))


def _cells():
    """Every class at every shape; dtype x noisy in rotation, so that every class meets each of the four at two shapes or more
    and cnt = 8 in both dtypes."""
    return [Cell(cls, N, cnt, *COMBOS[(ci + si) % 4]) for ci, cls in enumerate(CLASSES) for si, (N, cnt) in enumerate(SHAPES)]


CELLS = _cells()


def cell_id(c):
    return f"{c.cls}-N{c.N}-c{c.cnt}-{c.dtype}-{'Rc' if c.noisy else 'Rc0'}"


# ---- one handle: merges behind wide updates ------------------------------------------------------------------------------------
# `independent`, N = 127.  The merges of this schedule are cells of `independent` too (their need enters its margins): after
# the updates the observed landmarks are correlated through the pose, and every panel column is dense in their rows.
SCHEDULE = (("update", 64), ("merge", 1), ("update", 17), ("merge", 8), ("merge", 3))
SCHEDULE_CLASS, SCHEDULE_N = "independent", 127


def schedule_start(dtype):
    """(x, P, rng) the schedule begins with."""
    x, P = designed_state(SCHEDULE_CLASS, SCHEDULE_N, dtype, 4_000_000 + (dtype == "f64"))
    return x, P, np.random.default_rng(99 + (dtype == "f64"))


def schedule_update(rng, xo, N, m):
    """(z, ids) of an update step from the state the handle holds."""
    ids = U.choose_ids(SCHEDULE_CLASS, rng, N, m)
    return U.observations(SCHEDULE_CLASS, rng, xo, ids), ids


def schedule_merge(rng, xo, Po, dtype, N, cnt, step):
    """(x with the pairs' means placed, pairs, Rc) of a merge step from the state the handle holds."""
    pairs = pairs_for(SCHEDULE_CLASS, dtype, N, cnt)
    return place_means(xo, Po, pairs, dtype, rng), pairs, (RC.copy() if step % 2 else None)


@functools.lru_cache(maxsize=2)
def model_schedule(dtype):
    """The schedule with the models in the device's place.  Returns one row per step: (kind, m, what U.ratios says the
    constants would have to be (merges) or the error / bound under update_records' own margins (updates), kappa)."""
    x, P, rng = schedule_start(dtype)
    rows = []
    for step, (kind, m) in enumerate(SCHEDULE):
        N = (len(x) - 3) // 2
        if kind == "update":
            z, ids = schedule_update(rng, x, N, m)
            ref = U.restate(x, P, z, ids, "cholesky")
            x, P, _side = U.model_update(x, P, z, ids, dtype, "cholesky")
            rows.append((kind, m, U.judge(x, P, ref, SCHEDULE_CLASS, dtype, "cholesky", m, enforce=False), ref["kappa"]))
        else:
            x, pairs, Rc = schedule_merge(rng, x, P, dtype, N, m, step)
            ref = after_removal(restate(x, P, pairs, Rc))
            x, P, _side = model_merge(x, P, pairs, Rc, dtype)
            rows.append((kind, m, U.ratios(x, P, ref, dtype), ref["kappa"]))
    return rows


# ---- the margins, from the model -------------------------------------------------------------------------------------------
def model_needs(cells=None):
    """{class: {quantity: the largest ratio the model needs over the class's cells and, for `independent`, over the merges of
    the schedule}} and the per-cell rows."""
    need, rows = {}, []
    for c in (CELLS if cells is None else cells):
        x, P, pairs, Rc = make_inputs(*c)
        ref = restate_cell(c)
        xm, Pm, _side = model_merge(x, P, pairs, Rc, c.dtype)
        r = U.ratios(xm, Pm, ref, c.dtype)
        rows.append((c, ref["kappa"], r))
        slot = need.setdefault(c.cls, {})
        for q, val in r.items():
            slot[q] = max(slot.get(q, 0.0), val)
    if cells is None:
        for dtype in ("f32", "f64"):
            for kind, _m, r, _kap in model_schedule(dtype):
                if kind == "merge":
                    for q, val in r.items():
                        need[SCHEDULE_CLASS][q] = max(need[SCHEDULE_CLASS].get(q, 0.0), val)
    return need, rows


def margins_from(need):
    """The rule: max(4, 4 x need) per class, in MARGINS' layout."""
    return {c: tuple(max(4.0, 4 * need[c].get(q, 0.0)) for q in ("x", "P", "P32")) for c in CLASSES}
