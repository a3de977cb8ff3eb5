"""The rigid frame change (slam_ekf_transform / slam_pf_transform), the parts that need no GPU: both entry points are declared
where they belong (include/slamhip_frame.h, the companion library), exported and bound; the host-side argument check; the blockwise formulas against T P T'; a literal NumPy
run of the EKF kernels' ownership rule (tests/transform_ref.run_in_place) on a small tile-major buffer; composition with the
inverse; the closed-form rigid fit behind `align`; and the smallest-normal rule of the FastSLAM records."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import strip_ref as SR
from tests import transform_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slam_ekf_transform", "slam_pf_transform")
ANGLES = [(3.0, -7.0, 0.0), (0.0, 0.0, 0.7), (1000.0, -2000.0, -2.9), (5.0, 5.0, math.pi), (0.0, 1.0, 7.0)]


def test_both_entry_points_are_declared_in_the_frame_header_exported_and_bound(pkg):
    """libslamhip.so exports exactly what slamhip.h and slamhip_diag.h declare (tests/test_abi_cpu.py, and 22 hooks in the latter:
    tests/test_merge_ref_cpu.py), so the frame change is declared in include/slamhip_frame.h and exported by the companion
    library libslamhip_frame.so, which links against libslamhip.so: tests/test_companions_cpu.py holds the header, the library,
    this table and the Julia binding to the same names.  Here: which names, and their argument types."""
    assert set(pkg._lib.FRAME_SIGNATURES) == set(NAMES)
    for name in NAMES:
        res, args = pkg._lib.FRAME_SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    assert "transform!" in src.split("const libslamhip")[0]
    for obj in (pkg.EKFSlamState.transform, pkg.EKFSlamState.align, pkg.transform_features, pkg.transform_features_,
                pkg.PFShard.transform, pkg.FastSLAM.transform, pkg.FastSLAM.align, pkg.PFSlamState.transform):
        assert callable(obj)


def test_null_handle_is_a_status_code(pkg):
    lib = pkg._lib.frame_lib()
    assert lib.slam_ekf_transform(None, 0.0, 0.0, 0.0) == pkg._lib.SLAM_E_BADARG
    assert "null handle" in pkg._lib.last_error()          # (the message is libslamhip.so's: one error slot for both libraries)
    assert lib.slam_pf_transform(None, 0.0, 0.0, 0.0) == pkg._lib.SLAM_E_BADARG


def _state(rng, N):
    n = 3 + 2 * N
    x = np.concatenate([[rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3)], rng.uniform(-90, 90, 2 * N)])
    A = rng.normal(0, 0.3, (n, n))
    return x, A @ A.T + 0.01 * np.eye(n)


@pytest.mark.parametrize("N", [0, 1, 2, 9])
def test_blockwise_formulas_against_the_dense_product(N):
    rng = np.random.default_rng(N)
    x, P = _state(rng, N)
    NG = N + 2
    for tx, ty, theta in ANGLES:
        xo, Po = X.transform(x, P, tx, ty, theta)
        c, s = X.cs_of(theta)
        got = np.empty_like(P)
        for gr in range(NG):
            for gc in range(NG):
                r, q, nr, nc = X.grp_first(gr), X.grp_first(gc), X.grp_size(gr), X.grp_size(gc)
                got[r:r + nr, q:q + nc] = X.block_image(P[r:r + nr, q:q + nc], nr, nc, c, s)
        assert X.worst_ratio(got, Po, X.bound_P(P, theta, "f64")) <= 1.0
        assert got[2, 2] == P[2, 2]
        T = X.T_of(3 + 2 * N, theta)
        assert np.allclose(T @ T.T, np.eye(3 + 2 * N), atol=1e-15)
        assert abs(xo[2]) <= math.pi and math.isclose(math.sin(xo[2]), math.sin(x[2] + theta), abs_tol=1e-12)
        if theta == 0.0:
            assert np.array_equal(Po, P)


@pytest.mark.parametrize("E,N", [(4, 0), (4, 1), (4, 2), (4, 3), (4, 5), (4, 8), (8, 1), (8, 2), (8, 3), (8, 6), (8, 7), (8, 13), (8, 18)])
def test_ownership_rule_writes_every_stored_entry_once_and_matches_the_dense_result(E, N):
    """T = 1 .. 5 tile rows of state inside an allocation one tile row larger (so there is padding beside and below);
    n = 3 + 2N puts the last pair inside a tile (E = 8, N = 3), across an edge (E = 4, N = 1: the pair (3, 4); E = 8, N = 3 ...)
    and leaves padding inside the last tile."""
    rng = np.random.default_rng(100 * E + N)
    n = 3 + 2 * N
    L = E.bit_length() - 1
    ld = (((n - 1) >> L) + 2) * E
    assert ld // E <= 6
    x, P = _state(rng, N)
    theta = 0.7
    _xo, Po = X.transform(x, P, 0.0, 0.0, theta)
    want = SR.expected_storage(Po, ld, E)
    below = SR.expected_storage(np.ones((n, n)), ld, E) != 0          # the stored entries with r < n and c < n
    perms = [None, lambda k: range(k - 1, -1, -1), lambda k: np.random.default_rng(k).permutation(k)]
    for order in perms:
        buf = SR.expected_storage(P, ld, E)
        writes = X.run_in_place(buf, ld, E, n, theta, order)
        unwritten = SR.stored_offsets(ld, L, [2], [2])                 # P[2, 2] keeps its bits: no store at all
        expect = below.astype(np.int64)
        expect[unwritten] = 0
        assert np.array_equal(writes, expect), (np.flatnonzero(writes != expect)[:8], writes[writes != expect][:8])
        assert not buf[~below].any() and not np.signbit(buf[~below]).any()          # padding untouched: +0.0
        assert np.allclose(buf, want, rtol=0, atol=1e-12 * np.abs(P).max())
        T = ld // E
        for J in range(T):                                             # mirrored entries of diagonal tiles are equal
            b = int(SR.tile_base(J, J, T, L))
            tile = buf[b:b + E * E].reshape(E, E)
            assert np.array_equal(tile, tile.T)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_transform_then_inverse_stays_within_twice_the_bound(dtype):
    rng = np.random.default_rng(5)
    x, P = _state(rng, 12)
    npdt = X.NP[dtype]
    x, P = x.astype(npdt).astype(np.float64), P.astype(npdt).astype(np.float64)
    for tx, ty, theta in ANGLES:
        x1, P1 = X.transform(x, P, tx, ty, theta)
        x1, P1 = x1.astype(npdt).astype(np.float64), P1.astype(npdt).astype(np.float64)      # one rounding, as the device
        ix, iy, it = X.inverse(tx, ty, X.reduce_angle(theta))
        x2, P2 = X.transform(x1, P1, ix, iy, it)
        x2, P2 = x2.astype(npdt).astype(np.float64), P2.astype(npdt).astype(np.float64)
        bx, bP = X.roundtrip_bounds(x, P, tx, ty, theta, dtype)
        ref = x.copy()
        ref[2] = X.mpi_to_pi(X.mpi_to_pi(x[2] + X.reduce_angle(theta)) - X.reduce_angle(theta))
        assert X.worst_ratio(P2, P, bP) <= 1.0 and X.worst_ratio(x2, ref, bx) <= 1.0


def test_rigid_fit_recovers_a_planted_transform(pkg):
    rng = np.random.default_rng(3)
    src = rng.uniform(-80, 80, (2, 5))
    for tx, ty, theta in ANGLES + [(1.0, 2.0, math.pi - 1e-9), (1.0, 2.0, -math.pi + 1e-9), (0.0, 0.0, -math.pi)]:
        t = X.reduce_angle(theta)
        c, s = math.cos(t), math.sin(t)
        dst = np.array([[c, -s], [s, c]]) @ src + np.array([[tx], [ty]])
        for a, b in ((src, dst), (src.T, dst.T), (src[:, :2], dst[:, :2])):
            gx, gy, gt = pkg.rigid_fit(a, b)
            # absolute: 1e-12 m, plus 8 ulp of the larger of the translation and the destination centroid (t = cb - R ca is a
            # difference of numbers of that size: at 2000 m one ulp is 2.3e-13)
            lim = 1e-12 + 8 * np.spacing(max(abs(tx), abs(ty), float(np.abs(b).max())))
            assert abs(gx - tx) <= lim and abs(gy - ty) <= lim, (gx - tx, gy - ty, lim)
            assert abs(math.remainder(gt - t, 2 * math.pi)) <= 1e-12
    for bad in (src[:, :1], np.repeat(src[:, :1], 3, axis=1)):
        with pytest.raises(ValueError):
            pkg.rigid_fit(bad, bad + 1.0)
    with pytest.raises(ValueError):
        pkg.rigid_fit(src, src[:, :4])


@pytest.mark.parametrize("dtype,tiny_var", [("f32", 1e-30), ("f64", 1e-300)])
def test_records_in_use_rule_and_smallest_normal_rule(dtype, tiny_var):
    npdt = X.NP[dtype]
    lm = np.zeros((4, 5, 3), dtype=npdt)
    lm[0, :, :] = np.array([10.0, -4.0, tiny_var, 0.0, 0.0], dtype=npdt)[:, None]       # rank one, along x
    lm[1, 2, :] = -1.0                                                                  # empty slots
    lm[2, :, 0] = [1.0, 2.0, 0.5, 0.1, 0.25]                                            # row 3: all zero
    seen = [False, False, False, True]                                                  # ... but seen: a var = 0 record
    out, bound, use = X.records(lm, seen, 1.0, 2.0, math.pi / 2, dtype)
    assert use[0].all() and not use[1].any() and use[2].tolist() == [True, False, False] and use[3].all()
    assert np.all(out[0, 2] == npdt(X.TINY[dtype])) and np.all(out[0, 4] == npdt(tiny_var))      # turned onto the y axis, still in use
    assert np.array_equal(out[1], lm[1]) and np.array_equal(out[2, :, 1:], lm[2, :, 1:])
    assert np.array_equal(out[3, :2, 0], np.array([1.0, 2.0], dtype=npdt)) and not out[3, 2:].any()    # moved, covariance still zero
    assert X.in_use(out[:, 2, :], seen).tolist() == use.tolist()                        # no record changes sides
    c, s = X.cs_of(math.pi / 2)
    Pf = np.array([[0.5, 0.1], [0.1, 0.25]])
    Rm = np.array([[c, -s], [s, c]])
    want = Rm @ Pf @ Rm.T
    assert np.allclose([out[2, 2, 0], out[2, 3, 0], out[2, 4, 0]], [want[0, 0], want[0, 1], want[1, 1]], rtol=2e-7, atol=0)
    assert np.all(bound[~np.broadcast_to(use[:, None, :], bound.shape)] == 0)
