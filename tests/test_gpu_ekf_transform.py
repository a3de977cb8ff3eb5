"""The EKF state expressed in another frame on the device (slam_ekf_transform, csrc/ekf_transform.hip) against the dense fp64
restatement of tests/transform_ref.py, entry by entry within its DERIVED bound (one rounding to the dtype, four double
multiply-adds, an ulp in c and s), from the state as the device held it before the call; the storage invariants after every
call; what must not change at all; the filter going on in the new frame (range-bearing observations do not know the frame);
the round trip; `align`; bad arguments; and the ordering behind a failed asynchronous update."""
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import merge_ref as MR
from tests import strip_ref as SR
from tests import transform_ref as X
from tests.strip_ref import check_storage
from tests.test_gpu_ekf import DTYPES, R, TOL, check_state, noisy_obs, random_state, rounded

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 2, 35, 200]
ANGLES = [(3.0, -7.0, 0.0), (0.0, 0.0, 0.7), (1000.0, -2000.0, -2.9), (5.0, 5.0, math.pi), (0.0, 1.0, 7.0)]
GATE1, GATE2 = 4.0, 25.0


def _eq_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(np.ascontiguousarray(a)), SR._bits(np.ascontiguousarray(b)))


def _within(st, x0, P0, tx, ty, theta, dtype, what, factor=1.0, bounds=None, ref=None):
    """The device state against the restatement of (x0, P0) (float64 copies of what the device held); returns the worst
    error-to-bound ratios (x, P)."""
    xo, Po = ref if ref is not None else X.transform(x0, P0, tx, ty, theta)
    bx, bP = bounds if bounds is not None else (X.bound_x(x0, tx, ty, theta, dtype), X.bound_P(P0, theta, dtype))
    xg, Pg = st.download()
    rx, rP = X.worst_ratio(xg, xo, factor * bx), X.worst_ratio(Pg, Po, factor * bP)
    print(f"{what}: worst error / bound  x {rx:.3f}  P {rP:.3f}")
    assert rx <= 1.0 and rP <= 1.0, f"{what}: x {rx:.3f} P {rP:.3f} of the bound"
    return xg, Pg


@pytest.fixture(scope="module")
def states():
    """One seeded state per shape, shared (and never written) by the tests below."""
    return {N: random_state(np.random.default_rng(9100 + N), N) for N in SHAPES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", SHAPES)
def test_transform_against_the_restatement_entry_by_entry(pkg, states, dtype, N):
    x, P = states[N]
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    E = SR.TILE[dtype]
    if N == 200:                                       # the shape holds what it is chosen for: straddling pairs, several tile rows
        assert (3 + 2 * N - 1) // E + 1 == (4 if dtype == "f32" else 7)
        assert [j for j in range(1, N + 1) if (MR.f(j) + 1) % E == 0][:2] == ([63, 127] if dtype == "f32" else [31, 63])
    for tx, ty, theta in ANGLES:
        what = f"{dtype} N={N} ({tx}, {ty}, {theta:.3f})"
        x0, P0 = rounded(st)
        xb, Pb = st.download()
        st.transform(tx, ty, theta)
        xg, Pg = _within(st, x0, P0, tx, ty, theta, dtype, what)
        check_storage(st, pkg, Pg, what=what)
        assert _eq_bits(Pg[2:3, 2:3], Pb[2:3, 2:3]), f"{what}: P[2, 2] changed"
        if theta == 0.0:                               # a pure translation: P and the heading keep their bits
            assert _eq_bits(Pg, Pb) and _eq_bits(xg[2:3], xb[2:3]), what
        assert np.array_equal(Pg, Pg.T), what
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_heading_takes_the_single_wrap(pkg, dtype):
    for phi, theta, want in ((3.0, 0.7, 3.7 - 2 * math.pi), (-3.0, -0.7, -3.7 + 2 * math.pi), (0.5, 7.0, 0.5 + X.reduce_angle(7.0))):
        x = np.array([1.0, 2.0, phi, 10.0, -4.0])
        st = pkg.EKFSlamState(x, np.eye(5) * 0.1, dtype=dtype, max_landmarks=4)
        st.transform(0.0, 0.0, theta)
        got = float(st.download("x")[2])
        assert abs(got) <= math.pi and abs(got - want) <= (X.U[dtype] + X.SLACK) * (abs(phi) + abs(theta) + 2 * math.pi), (phi, theta, got)
        assert _eq_bits(st.download("cov")[2:3, 2:3], np.full((1, 1), 0.1, dtype=st.np_dtype))
        st.close()


def _margins(nis, what):
    """A condition on the INPUT: every decision is at least 1 % clear of both gates -- every (observation, landmark) statistic
    of gate1 (which landmarks are candidates), every observation's smallest statistic of gate2 (new feature or dropped)."""
    with np.errstate(invalid="ignore"):
        rel = min(float(np.nanmin(np.abs(nis - GATE1) / GATE1)), float(np.nanmin(np.abs(np.nanmin(nis, axis=1) - GATE2) / GATE2)))
    assert rel >= 0.01, f"{what}: a decision lies within 1 % of a gate ({rel:.4f})"


def _frame_invariance(pkg, dtype, x, P, z, g, what, expect=None):
    N = (len(x) - 3) // 2
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    st.set_gate_mode("grid")                           # a grid of the OLD means and a variance bound of the OLD matrix exist
    before = st.associate_vector(z, R, GATE1, GATE2)
    st.set_gate_mode("sweep")
    assert np.array_equal(st.associate_vector(z, R, GATE1, GATE2), before)
    x0, P0 = rounded(st)
    st.transform(*g)
    xt, Pt = X.transform(x0, P0, *g)                   # the transformed reference state
    nis, nd = O.association_table_sparse(xt, Pt, z, R)
    _margins(nis, what)
    want = O.assoc_vector(nis, nd, GATE1, GATE2)
    if expect is not None:
        assert want.tolist() == expect, (want.tolist(), expect)
    got = {}
    for mode in ("sweep", "grid"):
        st.set_gate_mode(mode)
        got[mode] = st.associate_vector(z, R, GATE1, GATE2)
        assert st.gate_info()["form"] == mode
    assert np.array_equal(got["sweep"], want) and np.array_equal(got["grid"], want), (what, got, want.tolist())
    assert np.array_equal(before, want), what           # ... and the decisions are those of the old frame
    xs, Ps = rounded(st)                               # the update: the oracle from the transformed state as the device holds it
    zf, idf, _zn = O.split_assoc(z, want)
    st.update(zf, R, idf)
    xo, Po = O.update_sparse(xs, Ps, zf, R, idf)
    check_state(st, xo, Po, dtype, what, prior=Ps)
    check_storage(st, pkg, what=what)
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_filter_goes_on_in_the_new_frame_far_translation(pkg, states, dtype):
    """(1000, -2000): with a stale grid every landmark would sit in the wrong cell."""
    x, P = states[200]
    rng = np.random.default_rng(13)
    ids = rng.choice(np.arange(1, 201), size=14, replace=False)
    z = np.hstack([noisy_obs(rng, x, ids), np.array([[400.0, 650.0], [0.4, -1.0]])])
    _frame_invariance(pkg, dtype, x, P, z, (1000.0, -2000.0, -2.9), f"{dtype} far translation")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_filter_goes_on_in_the_new_frame_variance_turned_onto_an_axis(pkg, dtype):
    """Every landmark block is [[a, 0.95 a], [0.95 a, a]]; theta = -pi/4 turns its long axis onto x: the largest landmark
    variance grows from a to 1.95 a.  Two observations are displaced ALONG that axis: one inside gate1, one between the
    gates whose distance a variance bound of the old matrix (a) would put outside gate2 (a new feature)."""
    N, a = 40, 0.5
    rng = np.random.default_rng(21)
    n = 3 + 2 * N
    ang = rng.uniform(0, 2 * math.pi, N)
    rad = rng.uniform(15.0, 60.0, N)
    x = np.concatenate([[50.0, 50.0, 0.4], np.stack([50 + rad * np.cos(ang), 50 + rad * np.sin(ang)], axis=1).reshape(-1)])
    P = np.zeros((n, n))
    P[:3, :3] = np.diag([1e-4, 1e-4, 1e-8])
    for j in range(1, N + 1):
        f = MR.f(j)
        P[f:f + 2, f:f + 2] = [[a, 0.95 * a], [0.95 * a, a]]
    axis = np.array([1.0, 1.0]) / math.sqrt(2.0)
    ids = [3, 11, 27]
    cols = []
    for j, d in zip(ids, (0.0, math.sqrt(3.0 * 1.95 * a), math.sqrt(36.0 * a))):
        xm = x.copy()
        f = MR.f(j)
        xm[f:f + 2] += d * axis
        zp, _ = O.predict_observation(xm, j)
        cols.append(zp)
    z = np.stack(cols, axis=1)
    # the other landmarks must be far from these three observations (else their nis decides): assert on the oracle
    nis, _nd = O.association_table_sparse(x, P, z, R)
    others = np.delete(nis, [j - 1 for j in ids], axis=1)
    assert others.min() > 4 * GATE1                     # (no other landmark is a candidate)
    assert GATE2 * a < 36.0 * a < GATE2 * 1.95 * a          # outside gate2 for the old bound, inside for the matrix as it is
    _frame_invariance(pkg, dtype, x, P, z, (0.0, 0.0, -math.pi / 4), f"{dtype} turned variance", expect=[3, 11, 0])
    # the block itself: 1.95 a on x, 0.05 a on y
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    st.transform(0.0, 0.0, -math.pi / 4)
    blk = st.landmark_blocks().astype(np.float64)
    assert np.allclose(blk[0], 1.95 * a, rtol=1e-6) and np.allclose(blk[2], 0.05 * a, rtol=1e-5) and np.all(np.abs(blk[1]) <= 1e-6 * a)
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [35, 200])
def test_round_trip_returns_the_state_within_twice_the_bound(pkg, states, dtype, N):
    x, P = states[N]
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    for tx, ty, theta in ANGLES:
        x0, P0 = rounded(st)
        st.transform(tx, ty, theta)
        st.transform(*X.inverse(tx, ty, X.reduce_angle(theta)))
        ref = x0.copy()
        t = X.reduce_angle(theta)
        ref[2] = X.mpi_to_pi(X.mpi_to_pi(x0[2] + t) - t)
        _within(st, x0, P0, tx, ty, theta, dtype, f"round trip {dtype} N={N} theta={theta:.3f}", ref=(ref, P0),
                bounds=X.roundtrip_bounds(x0, P0, tx, ty, theta, dtype))
        check_storage(st, pkg, what="round trip")
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_align_brings_the_map_back_onto_surveyed_positions(pkg, states, dtype):
    """Five landmarks of a transformed N = 35 state are fitted back onto their original means.  The fit h is the inverse
    transform to 1e-9 (fp64) / 1e-4 (fp32: the means carry 2^-24 relative rounding at a scale of about 100 m).  The state after
    `align` is held to the restatement of g FOLLOWED BY THE RETURNED h from the original state, within the derived bound of two
    calls (tests/transform_ref.compose_bounds: twice one call's) and nothing else: what is applied is what is returned, at
    rounding level.  How far that is from the original state is printed against twice the bound as well (the fit's own error
    is in that figure, so it is not asserted)."""
    x, P = states[35]
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=39)
    x0, P0 = rounded(st)
    ids = np.array([2, 9, 17, 26, 35])
    f = 3 + 2 * (ids - 1)
    surveyed = np.stack([x0[f], x0[f + 1]])            # the means in the original frame
    g = (40.0, -25.0, 2.2)
    st.transform(*g)
    snap = SR.snapshot(st)
    tol = 1e-9 if dtype == "f64" else 1e-4
    want = X.inverse(*g)
    got = st.align(ids, surveyed, apply=False)
    assert SR.changed_offsets(st, snap).size == 0      # apply=False only fits
    assert all(abs(p - q) <= tol for p, q in zip(got[:2], want[:2])) and abs(math.remainder(got[2] - want[2], 2 * math.pi)) <= tol, (got, want)
    print(f"{dtype} align: fit minus inverse  tx {got[0] - want[0]:.3e}  ty {got[1] - want[1]:.3e}  theta {math.remainder(got[2] - want[2], 2 * math.pi):.3e}")
    got2 = st.align(ids, surveyed.T)                    # [k, 2] as well; applies
    assert got2 == got
    x1, P1 = X.transform(x0, P0, *g)
    ref = X.transform(x1, P1, *got)
    xg, Pg = _within(st, x0, P0, *g, dtype, f"{dtype} g then the fitted transform", ref=ref, bounds=X.compose_bounds(x0, P0, g, got, dtype))
    check_storage(st, pkg, Pg, what="align")
    bx, bP = X.roundtrip_bounds(x0, P0, *g, dtype)
    orig = x0.copy()
    orig[2] = X.mpi_to_pi(X.mpi_to_pi(x0[2] + g[2]) + got[2])
    print(f"{dtype} align: distance from the ORIGINAL state / twice the bound  x {X.worst_ratio(xg, orig, bx):.3f}  P {X.worst_ratio(Pg, P0, bP):.3f}")
    with pytest.raises(ValueError):
        st.align([3], surveyed[:, :1])
    with pytest.raises(ValueError):
        st.align([3, 4], np.array([[1.0, 1.0], [2.0, 2.0]]))      # 2 x 2 is read as [2, k]: the points (1, 2) and (1, 2), coincident
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_leave_the_state_bit_identical(pkg, states, dtype):
    x, P = states[35]
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=39)
    snap, x0, blk0 = SR.snapshot(st), st.download("x"), st.landmark_blocks()
    lib = pkg._lib.frame_lib()
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf), (0.0, 0.0, math.nan)):
        assert lib.slam_ekf_transform(st._h, *bad) == pkg._lib.SLAM_E_BADARG, bad
        assert SR.changed_offsets(st, snap).size == 0 and _eq_bits(st.download("x"), x0) and _eq_bits(st.landmark_blocks(), blk0), bad
    assert lib.slam_ekf_transform(None, 0.0, 0.0, 0.0) == pkg._lib.SLAM_E_BADARG
    with pytest.raises(pkg.SlamHipError) as ei:
        st.transform(0.0, math.nan, 0.0)
    assert ei.value.code == pkg._lib.SLAM_E_BADARG
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_transform_is_ordered_behind_a_failed_async_update(pkg, dtype):
    """R = -eps I with a landmark observed twice: S is not positive definite, the asynchronous update leaves the state alone
    and defers its status.  The transform enqueued behind it still applies; slam_ekf_sync still reports the update."""
    rng = np.random.default_rng(4)
    x, P = random_state(rng, 6)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=8)
    x0, P0 = rounded(st)
    Rbad = -1e-5 * np.eye(2)
    zp, _ = O.predict_observation(x0, 3)
    z = np.stack([zp + [0.01, 0.0005], zp - [0.01, 0.0005]], axis=1)
    st.set_async(True)
    st.update(z, Rbad, [3, 3])
    g = (4.0, -9.0, 1.1)
    st.transform(*g)
    with pytest.raises(pkg.NotPositiveDefinite):
        st.sync()
    st.sync()
    st.set_async(False)
    _within(st, x0, P0, *g, dtype, f"{dtype} behind a failed async update")
    check_storage(st, pkg, what="async")
    st.close()
