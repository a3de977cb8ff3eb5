"""The covariance factor on the device (slam_ekf_factor_*, include/ext/slamhip_factor.h) against the bounds of tests/factor_ref.py.

States: update_records.designed_state, classes independent / slam / mixed / rank6.  Sizes: the smallest at which each kernel path
can go wrong -- fp32 (E = 128) N = 1, 62, 63, 64, 190, 200, 330 (n = 5, 127, 129, 131, 383, 403, 663: one partial tile, a full tile but
one, two tile rows with a one-row last tile, 2, 3, 4, 6 tile rows), fp64 (E = 64) N = 1, 30, 31, 100, 170 -- with panel_tiles 1, 2
and 4 at every size (three tile rows: a ragged last panel for 2; six: the panel-wide trailing update for 4).  The source handle's
capacity and the factor's are N or larger, independently by class, so the allocation's tile rows differ from the used ones and
from each other.

Every bound is entrywise, from Higham (factor_ref.py), with no margin: gamma_(n+1) |L| |L|' for the factor (u of the factor's
dtype), gamma_n |L| |Y| and gamma_n |L| |Z| in fp64 for solve and multiply.  Where a bound is exactly 0 the error must be 0."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import factor_ref as FR
from tests import update_records as UR

pytestmark = pytest.mark.gpu

CLASSES = ("independent", "slam", "mixed", "rank6")
SIZES = {"f32": (1, 62, 63, 64, 190, 200, 330), "f64": (1, 30, 31, 100, 170)}
CASES = [(d, N) for d in ("f32", "f64") for N in SIZES[d]]
EXTRA = 200                                                   # landmarks of spare capacity: at least three more tile rows
# (source capacity beyond N, factor capacity beyond N) per class: each equal and larger, independently
SPARE = {"independent": (0, 0), "slam": (EXTRA, 0), "mixed": (0, EXTRA), "rank6": (EXTRA, EXTRA + 70)}
FAIL_AT = {"f32": (200, (0, 4, 127, 128, 257, 402)), "f64": (100, (0, 63, 64, 130, 202))}


@functools.lru_cache(maxsize=None)
def _state(cls, N, dtype):
    x, P = UR.designed_state(cls, N, dtype, 1000 + N)
    x.setflags(write=False)
    P.setflags(write=False)
    return x, P


@functools.lru_cache(maxsize=None)
def _ref_factor(cls, N, dtype):
    L, idx, _ = FR.cholesky(_state(cls, N, dtype)[1], "f64")
    assert idx == -1
    L.setflags(write=False)
    return L


def _upload(pkg, cls, N, dtype, spare=0, P=None):
    x, P0 = _state(cls, N, dtype)
    return pkg.EKFSlamState(x, P0 if P is None else P, dtype=dtype, max_landmarks=max(N + spare, 1))


def _check_factor(f, P, fdtype, what):
    """The backward error, the structure and info's pivots and log det on a computed factor; returns (worst ratio to the bound, L)."""
    n = P.shape[0]
    assert f.n == n
    L = f.L()
    assert L.dtype == FR.NP[fdtype] and L.shape == (n, n)
    assert not np.any(np.triu(L, 1)) and not np.any(np.signbit(np.triu(L, 1)))       # +0.0 above the diagonal
    ratio, at_zero = FR.factor_ratio(L, P, fdtype)
    print(f"FACTOR_RATIO {what} ratio {ratio:.4f} at_zero {at_zero:.3g}")
    assert ratio <= 1.0 and at_zero == 0.0, (what, ratio, at_zero)
    # log det and pivots: info against the downloaded diagonal
    d = np.diag(L).astype(np.float64)
    assert f.min_pivot == d.min() and f.max_pivot == d.max(), what
    mine = FR.logdet(L)
    assert abs(f.logdet - mine) <= n * 2.0 ** -52 * abs(mine), (what, f.logdet, mine)
    return ratio, L


@pytest.mark.parametrize("pt", [1, 2, 4])
@pytest.mark.parametrize("dtype,N", CASES)
def test_backward_error_structure_logdet(pkg, dtype, N, pt):
    for cls in CLASSES:
        x, P = _state(cls, N, dtype)
        s_src, s_fac = SPARE[cls]
        st = _upload(pkg, cls, N, dtype, s_src)
        f = pkg.CovarianceFactor(dtype, max(N + s_fac, 1), panel_tiles=pt)
        try:
            x0, P0 = st.download()
            info = f.compute(st)
            what = f"{dtype} pt={pt} {cls} N={N}"
            assert info[0] == 3 + 2 * N and info[1] == 0 and info[2] == -1 and info[3] == 0 and info[7] == pt, (what, info)
            assert f.panel_tiles == pt and np.array_equal(info, f.info)
            _ratio, L = _check_factor(f, P, dtype, what)
            assert np.array_equal(f.mean(), x)
            # log det against the fp64 reference where the first-order bound says something
            bound = FR.logdet_bound(P, L, dtype)
            ref = FR.logdet(_ref_factor(cls, N, dtype))
            print(f"FACTOR_LOGDET {what} err {abs(f.logdet - ref):.3g} bound {bound:.3g}")
            if bound < 0.1:
                assert abs(f.logdet - ref) <= bound, (what, f.logdet, ref, bound)
            # a block read-out is the same entries
            n = 3 + 2 * N
            r0, c0 = n // 3, n // 5
            assert np.array_equal(f.L(r0, c0, n - r0, n - c0 - 1), L[r0:, c0:n - 1])
            # a second run: the same bits; the source: untouched
            info2 = f.compute(st)
            assert np.array_equal(info2, info) and np.array_equal(f.L(), L), what
            x1, P1 = st.download()
            assert np.array_equal(x1, x0) and np.array_equal(P1, P0), what
        finally:
            f.close()
            st.close()


@pytest.mark.parametrize("pt", [1, 2, 4])
@pytest.mark.parametrize("N", [63, 200])
def test_fp64_factor_of_an_fp32_state(pkg, N, pt):
    """The copy-in converts and re-tiles 128 -> 64; the bound is the fp64 one against the stored fp32 values."""
    for cls in CLASSES:
        x, P = _state(cls, N, "f32")
        s_src, s_fac = SPARE[cls]
        st = _upload(pkg, cls, N, "f32", s_src)
        try:
            f = st.factor(dtype="f64", panel_tiles=pt) if s_fac == 0 else st.factor(
                out=pkg.CovarianceFactor("f64", N + s_fac, panel_tiles=pt))
            try:
                _check_factor(f, P, "f64", f"f64<-f32 pt={pt} {cls} N={N}")
                assert np.array_equal(f.mean(), x)
            finally:
                f.close()
        finally:
            st.close()


@pytest.mark.parametrize("dtype,big,small", [("f32", 200, 62), ("f64", 100, 30)])
def test_a_second_compute_does_not_see_what_a_larger_state_left(pkg, dtype, big, small):
    for cls in ("slam", "mixed"):
        a, b = _upload(pkg, cls, big, dtype), _upload(pkg, cls, small, dtype)
        used, fresh = pkg.CovarianceFactor(dtype, big, panel_tiles=2), pkg.CovarianceFactor(dtype, big, panel_tiles=2)
        try:
            used.compute(a)
            i1, i2 = used.compute(b), fresh.compute(b)
            assert np.array_equal(i1, i2) and np.array_equal(used.L(), fresh.L()) and np.array_equal(used.mean(), fresh.mean())
        finally:
            for o in (a, b, used, fresh):
                o.close()


@pytest.mark.parametrize("cls", ["mixed", "slam"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_not_positive_definite_at_designed_indices(pkg, dtype, cls):
    N, indices = FAIL_AT[dtype]
    x, P = _state(cls, N, dtype)
    n = 3 + 2 * N
    good = _upload(pkg, cls, N, dtype)
    f = pkg.CovarianceFactor(dtype, N)
    z = np.zeros((n, 1))
    try:
        planted = [(i, FR.plant_failure(P, i, dtype)) for i in indices]
        Pn = np.array(P)
        Pn[indices[2], indices[2]] = np.nan
        planted.append((indices[2], Pn))
        for i, Pb in planted:
            st = _upload(pkg, cls, N, dtype, P=Pb)
            try:
                with pytest.raises(pkg.NotPositiveDefinite):
                    f.compute(st)
                info = f.info
                assert info[0] == n and info[1] == pkg._lib.SLAM_E_NOTPD and info[2] == i, (dtype, cls, i, info)
                assert not (info[3] > 0) and info[4] == info[5] == info[6] == 0
                with pytest.raises(pkg.NotPositiveDefinite):
                    st.factor()
                assert st.is_positive_definite(dtype) == (False, i, 0 if i < 3 else (i - 3) // 2 + 1)
                for call in (f.L, f.mean, lambda: f.whiten(z), lambda: f.colour(z)):      # every read-out is refused
                    with pytest.raises(pkg.SlamHipError) as e:
                        call()
                    assert e.value.code == pkg._lib.SLAM_E_BADARG
            finally:
                st.close()
        info = f.compute(good)                                # ... and a good state is factored again
        assert info[1] == 0 and FR.factor_ratio(f.L(), P, dtype)[0] <= 1.0
        assert good.is_positive_definite(dtype) == (True, -1, -1)
    finally:
        f.close()
        good.close()


@pytest.mark.parametrize("r", [1, 3, 64])
@pytest.mark.parametrize("dtype,N", [("f32", 63), ("f32", 200), ("f64", 31), ("f64", 100)])
def test_solve_and_multiply(pkg, dtype, N, r):
    rng = np.random.default_rng(100 * N + r)
    n = 3 + 2 * N
    for cls in ("slam", "mixed"):
        st = _upload(pkg, cls, N, dtype, SPARE[cls][0])
        f = pkg.CovarianceFactor(dtype, N + SPARE[cls][1])
        try:
            f.compute(st)
            L = f.L().astype(np.float64)
            B = rng.standard_normal((n, r))
            Y, d2 = f.whiten(B, return_d2=True)
            ratio, at_zero = FR.solve_ratio(L, Y, B)
            print(f"FACTOR_SOLVE {dtype} {cls} N={N} r={r} ratio {ratio:.4f}")
            assert ratio <= 1.0 and at_zero == 0.0, (dtype, cls, N, r, ratio)
            s = (Y * Y).sum(axis=0)
            assert np.all(np.abs(d2 - s) <= n * 2.0 ** -52 * s)
            out = f.colour(B)
            ratio, at_zero = FR.product_ratio(L, B, out)
            print(f"FACTOR_MULTIPLY {dtype} {cls} N={N} r={r} ratio {ratio:.4f}")
            assert ratio <= 1.0 and at_zero == 0.0, (dtype, cls, N, r, ratio)
        finally:
            f.close()
            st.close()


def test_nees_wraps_the_heading_and_follows_select(pkg):
    rng = np.random.default_rng(5)
    N = 62
    x, P = _state("slam", N, "f64")
    x = np.array(x)
    x[2] = 3.1
    st = pkg.EKFSlamState(x, P, dtype="f64", max_landmarks=N)
    try:
        L = FR.cholesky(P, "f64")[0]
        x_true = x + rng.standard_normal(x.size) * 0.01
        x_true[2] = -3.1                                       # the heading error 6.2 wraps to 6.2 - 2 pi
        want = FR.nees(x, x_true, L)
        e = x - x_true
        assert abs(e[2]) > math.pi
        got = st.nees(x_true)
        assert abs(got - want) <= 1e-9 * want, (got, want)
        f = st.factor()
        try:
            assert f.nees(x_true) == got
        finally:
            f.close()
        ids = np.array([7, 3, 50, 21])
        s = pkg.select_map(N, ids)
        sub = st.select(ids)
        try:
            f = sub.factor(dtype="f64")
            try:
                assert st.nees(x_true[s], ids) == f.nees(x_true[s])
            finally:
                f.close()
        finally:
            sub.close()
        Ls = FR.cholesky(P[np.ix_(s, s)], "f64")[0]
        want = FR.nees(x[s], x_true[s], Ls)
        assert abs(st.nees(x_true[s], ids) - want) <= 1e-9 * want
    finally:
        st.close()


def test_samples_whiten_to_a_chi_square(pkg):
    """The whitened deviations of 4096 samples have a sum of squares that is chi-square with n 4096 degrees of freedom: mean n 4096,
    variance 2 n 4096; six standard deviations are a condition, not a measurement."""
    N, count = 62, 4096
    n = 3 + 2 * N
    st = _upload(pkg, "slam", N, "f32")
    try:
        f = st.factor()
        try:
            S = f.sample(count, np.random.default_rng(11))
            assert S.shape == (n, count)
            again = f.sample(count, np.random.default_rng(11))
            assert np.array_equal(S, again)                   # the caller's generator decides the draw
            _Y, d2 = f.whiten(S - f.mean()[:, None], return_d2=True)
            total = float(d2.sum())
            assert abs(total - n * count) <= 6.0 * math.sqrt(2.0 * n * count), (total, n * count)
        finally:
            f.close()
    finally:
        st.close()


def test_refusals_leave_the_source_and_the_factor_unchanged(pkg):
    L = pkg._lib
    lib = L.factor_lib()
    N = 64
    st32, st64 = _upload(pkg, "slam", N, "f32"), _upload(pkg, "slam", N, "f64")
    f32, small = pkg.CovarianceFactor("f32", N), pkg.CovarianceFactor("f64", N - 1)
    info = np.full(8, 7.0)
    try:
        f32.compute(st32)
        L0, i0, m0 = f32.L(), f32.info, f32.mean()
        x0, P0 = st64.download()
        ip = info.ctypes.data_as(L._dp)
        assert lib.slam_ekf_factor_compute(f32._h, st64._h, ip) == L.SLAM_E_BADARG                 # fp32 over fp64
        assert lib.slam_ekf_factor_compute(small._h, st64._h, ip) == L.SLAM_E_CAPACITY
        assert lib.slam_ekf_factor_compute(f32._h, None, ip) == L.SLAM_E_BADARG
        assert lib.slam_ekf_factor_compute(f32._h, st32._h, None) == L.SLAM_E_BADARG
        assert np.array_equal(info, np.full(8, 7.0))
        n = 3 + 2 * N
        buf = np.zeros((n, 65), order="F")
        bp = buf.ctypes.data_as(L._dp)
        for bad in ((-1, 0, 1, 1, 1), (0, -1, 1, 1, 1), (0, 0, n + 1, 1, n + 1), (1, 0, n, 1, n), (0, 1, 1, n, 1), (0, 0, 4, 1, 3)):
            r0, c0, nr, nc, ld = bad
            assert lib.slam_ekf_factor_get(f32._h, r0, c0, nr, nc, buf.ctypes.data, ld) == L.SLAM_E_BADARG, bad
        assert lib.slam_ekf_factor_get(f32._h, 0, 0, 1, 1, None, 1) == L.SLAM_E_BADARG
        for r, ld in ((0, n), (65, n), (1, n - 1)):
            assert lib.slam_ekf_factor_solve(f32._h, bp, r, ld, bp, None) == L.SLAM_E_BADARG
            assert lib.slam_ekf_factor_multiply(f32._h, bp, r, ld, bp) == L.SLAM_E_BADARG
        assert lib.slam_ekf_factor_solve(f32._h, None, 1, n, bp, None) == L.SLAM_E_BADARG
        assert lib.slam_ekf_factor_mean(f32._h, None) == L.SLAM_E_BADARG
        never = pkg.CovarianceFactor("f64", N)
        try:
            assert lib.slam_ekf_factor_mean(never._h, bp) == L.SLAM_E_BADARG and never.info[2] == -1
            h = ctypes.c_void_p()
            assert lib.slam_ekf_factor_create(ctypes.byref(h), L.SLAM_F64, N, 10 ** 6, 0) == L.SLAM_E_BADARG   # no such device
        finally:
            never.close()
        assert not buf.any()
        assert np.array_equal(f32.L(), L0) and np.array_equal(f32.info, i0) and np.array_equal(f32.mean(), m0)
        x1, P1 = st64.download()
        assert np.array_equal(x1, x0) and np.array_equal(P1, P0)
        assert small.info[0] == 0 and small.info[2] == -1
    finally:
        for o in (st32, st64, f32, small):
            o.close()


@pytest.mark.parametrize("dtype,fdtype,N", [("f32", "f32", 200), ("f64", "f64", 100), ("f32", "f64", 200)])
def test_the_lower_entries_of_a_diagonal_tile_are_the_ones_read(pkg, dtype, fdtype, N):
    """A diagonal tile is stored complete.  With other values above the diagonal -- the upload stores them as given -- the factor
    is, bit for bit, that of the matrix whose upper entries mirror the lower ones."""
    x, P = _state("slam", N, dtype)
    Pu = (np.tril(P) + 1.5 * np.triu(P, 1)).astype(FR.NP[dtype]).astype(np.float64)      # (values of the dtype: stored as given)
    a, b = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N), pkg.EKFSlamState(x, Pu, dtype=dtype, max_landmarks=N + EXTRA)
    try:
        E = FR.EDGE[dtype]
        stored = b.download("cov")
        assert np.array_equal(stored[:E, :E], Pu[:E, :E]) and not np.array_equal(stored[:E, :E], stored[:E, :E].T)
        fa, fb = a.factor(dtype=fdtype), b.factor(dtype=fdtype)
        try:
            assert np.array_equal(fa.info, fb.info) and np.array_equal(fa.L(), fb.L())
        finally:
            fa.close()
            fb.close()
    finally:
        a.close()
        b.close()


def test_sim_logs_the_nees(pkg, golden_dir):
    """The last sample is taken from the final state: it is held against the reference's NEES of the downloaded x and P.  Both
    sides solve with a factor that is exact for a matrix within gamma_(n+1) |L| |L|' of P (norm-wise at most n gamma_(n+1) |P|), so
    the values differ by at most 2 n gamma_(n+1) kappa_2(P) |e|^2 / lambda_min(P) to first order."""
    sim = pkg.sim
    wp = sim.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    lm = sim.make_landmarks(30, (wp[0].min(), wp[0].max(), wp[1].min(), wp[1].max()), 0.1, np.random.default_rng(2))
    filt = pkg.EKFSlamState(sim.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=64)
    try:
        log = sim.sim(filt, wp, lm, seed=4, nlaps=1, max_steps=90, nees_every=30)
        assert [s for s, _v, _d in log.nees] == [30, 60, 90] and len(log.nees_truth) == 3
        for (_s, v, dof), xt in zip(log.nees, log.nees_truth):
            assert 3 <= dof <= filt.n and (dof - 3) % 2 == 0 and xt.size == dof
            assert math.isnan(v) or v >= 0                  # (NaN: a matrix without a factor, e.g. before P_vv has full rank)
        x, P = filt.download()
        n = x.size
        x_true, tags = log.nees_truth[-1], log.landmark_tags
        assert n > 3 and tags.size == filt.N
        # the truth: the simulator's pose and the landmark whose observation created each map landmark
        assert np.array_equal(x_true[:3], log.true_track[-1]) and np.array_equal(x_true[3:], lm[:, tags - 1].T.reshape(-1))
        assert np.all(np.hypot(*(x[3:] - x_true[3:]).reshape(-1, 2).T) < 2.0)       # 2.25 s of driving: no estimate is metres off
        L, idx, _ = FR.cholesky(P, "f64")
        assert idx == -1
        want = FR.nees(x, x_true, L)
        e = x - x_true
        e[2] = FR.mpi_to_pi(e[2])
        w = np.linalg.eigvalsh(P)
        tol = 2 * n * FR.gamma(n + 1, FR.U["f64"]) * (w[-1] / w[0]) * float(e @ e) / w[0]
        got = log.nees[-1][1]
        print(f"FACTOR_SIM nees {got:.9g} reference {want:.9g} tolerance {tol:.3g} kappa {w[-1] / w[0]:.3g}")
        assert math.isfinite(got) and abs(got - want) <= tol, (got, want, tol)
    finally:
        filt.close()
    filt = pkg.EKFSlamState(sim.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=64)
    try:
        assert sim.sim(filt, wp, lm, seed=4, nlaps=1, max_steps=20).nees == []
    finally:
        filt.close()
