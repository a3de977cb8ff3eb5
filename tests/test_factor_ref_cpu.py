"""The covariance factor (slam_ekf_factor_*, include/ext/slamhip_factor.h), the parts that need no GPU: tests/factor_ref.py against
numpy.linalg.cholesky and LAPACK's potrf (factor, first failing index), what the entrywise bound catches on a model with a defect
injected, what is particular to this library's surface (the checks every side library shares are made from its row of the table
by tests/test_companions_cpu.py) and the null-handle status codes."""
import ctypes
import os

import numpy as np
import pytest
from scipy.linalg import lapack

from tests import abi_surface as ABI
from tests import factor_ref as FR
from tests import update_records as UR

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_factor.h")
NAMES = {"slam_ekf_factor_create", "slam_ekf_factor_destroy", "slam_ekf_factor_compute", "slam_ekf_factor_info",
         "slam_ekf_factor_get", "slam_ekf_factor_mean", "slam_ekf_factor_solve", "slam_ekf_factor_multiply"}
POTRF = {"f32": lapack.spotrf, "f64": lapack.dpotrf}
FAIL_AT = {"f32": (200, (0, 4, 127, 128, 257, 402)), "f64": (100, (0, 63, 64, 130, 202))}


def _state(cls, N, dtype):
    return UR.designed_state(cls, N, dtype, 1000 + N)


# ---- the reference against numpy and LAPACK -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["independent", "slam", "mixed", "rank6"])
def test_reference_factor_agrees_with_numpy_and_lapack(cls):
    for dtype, N in (("f64", 31), ("f64", 100), ("f32", 63), ("f32", 200)):
        _x, P = _state(cls, N, dtype)
        L, idx, piv = FR.cholesky(P, dtype)
        assert idx == -1 and piv == 0.0 and np.array_equal(L, np.tril(L))
        ratio, at_zero = FR.factor_ratio(L, P, dtype)
        assert ratio <= 1.0 and at_zero == 0.0, (cls, dtype, N, ratio, at_zero)
        Lk, info = POTRF[dtype](np.asarray(P, dtype=FR.NP[dtype]), lower=1, clean=1)
        assert info == 0
        rk, zk = FR.factor_ratio(Lk, P, dtype)
        assert rk <= 1.0 and zk == 0.0, (cls, dtype, N, rk, zk)
        if dtype == "f64":
            Ln = np.linalg.cholesky(P)
            # two factors inside the bound of one matrix: their difference is bounded through the first-order perturbation of the
            # factor, here simply by a loose multiple of the bound's scale
            assert np.max(np.abs(L - Ln)) <= 1e-6 * np.max(np.abs(Ln))
            assert abs(FR.logdet(L) - np.linalg.slogdet(P)[1]) <= 1e-8 * max(1.0, abs(FR.logdet(L)))


def test_reference_solve_and_product():
    rng = np.random.default_rng(3)
    _x, P = _state("slam", 62, "f64")
    L, idx, _ = FR.cholesky(P, "f64")
    assert idx == -1
    B = rng.standard_normal((P.shape[0], 5))
    Y = FR.forward_solve(L, B)
    assert FR.solve_ratio(L, Y, B)[0] <= 1.0
    assert FR.product_ratio(L, B, FR.product(L, B))[0] <= 1.0
    assert np.finfo(np.longdouble).nmant >= 63            # the residuals above are formed in extended precision
    e = rng.standard_normal(P.shape[0])
    x_true = np.zeros(P.shape[0])
    x_true[2] = 3.0
    mean = x_true + e
    mean[2] = -3.1                                           # the heading error crosses -pi: -6.1 wraps to 2 pi - 6.1
    ew = mean - x_true
    ew[2] += 2 * np.pi
    want = float(ew @ np.linalg.solve(P, ew))
    assert abs(FR.nees(mean, x_true, L) - want) <= 1e-9 * want


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("cls", ["mixed", "slam"])
def test_planted_failures_are_reported_at_their_index_by_the_reference_and_by_lapack(cls, dtype):
    N, indices = FAIL_AT[dtype]
    _x, P = _state(cls, N, dtype)
    for i in indices:
        Pb = FR.plant_failure(P, i, dtype)
        assert np.array_equal(Pb.astype(FR.NP[dtype]).astype(np.float64), Pb)
        _L, idx, piv = FR.cholesky(Pb, dtype)
        assert idx == i and piv <= 0, (cls, dtype, i, idx, piv)
        _Lk, info = POTRF[dtype](np.asarray(Pb, dtype=FR.NP[dtype]), lower=1)
        assert info - 1 == i, (cls, dtype, i, info)
    Pn = np.array(P)
    Pn[7, 7] = np.nan
    assert FR.cholesky(Pn, dtype)[1] == 7


def test_the_entrywise_bound_catches_a_dropped_tile_product_and_bf16_operands():
    """n = 403: four tile rows of 128.  A defect shows either as an error far outside the bound or, where it is large enough to
    turn a pivot negative, as a failure reported for a positive definite matrix -- which the GPU test counts as a failure too."""
    for cls in ("slam", "mixed"):
        _x, P = _state(cls, 200, "f32")
        good, idx = FR.blocked_model(P, "f32")
        assert idx == -1 and FR.factor_ratio(good, P, "f32")[0] <= 1.0
        for defect in ("dropped_tile_product", "bf16_operands"):
            bad, idx = FR.blocked_model(P, "f32", defect=defect)
            assert idx != -1 or FR.factor_ratio(bad, P, "f32")[0] > 10.0, (cls, defect)
    _x, P = _state("mixed", 200, "f32")
    bad, idx = FR.blocked_model(P, "f32", defect="bf16_operands")
    assert idx == -1 and FR.factor_ratio(bad, P, "f32")[0] > 100.0


# ---- the surface: the checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table --------
def test_what_is_particular_to_this_library(pkg):
    L = pkg._lib
    assert NAMES == set(L.factor_lib.signatures)
    with open(HEADER) as f:
        assert '#include "slamhip.h"' in f.read()


def test_null_handles_and_bad_arguments_are_status_codes(pkg):
    L = pkg._lib
    lib = L.factor_lib()
    BAD = L.SLAM_E_BADARG
    info = (ctypes.c_double * 8)(*([7.0] * 8))
    buf = (ctypes.c_double * 8)()
    assert lib.slam_ekf_factor_create(None, L.SLAM_F64, 8, 0, 0) == BAD
    h = ctypes.c_void_p(0x1000)
    assert lib.slam_ekf_factor_create(ctypes.byref(h), 7, 8, 0, 0) == BAD and not h.value
    for pt in (-1, 3, 5, 8):
        assert lib.slam_ekf_factor_create(ctypes.byref(h), L.SLAM_F64, 8, 0, pt) == BAD and "panel_tiles" in L.last_error()
    assert lib.slam_ekf_factor_create(ctypes.byref(h), L.SLAM_F32, -1, 0, 0) == BAD
    assert lib.slam_ekf_factor_destroy(None) == L.SLAM_OK
    assert lib.slam_ekf_factor_compute(None, None, info) == BAD and "null handle" in L.last_error()
    assert lib.slam_ekf_factor_compute(ctypes.c_void_p(0x1000), None, info) == BAD
    assert lib.slam_ekf_factor_compute(None, ctypes.c_void_p(0x1000), info) == BAD
    assert list(info) == [7.0] * 8
    assert lib.slam_ekf_factor_info(None, info) == BAD
    assert lib.slam_ekf_factor_get(None, 0, 0, 1, 1, buf, 1) == BAD
    assert lib.slam_ekf_factor_mean(None, buf) == BAD
    assert lib.slam_ekf_factor_solve(None, buf, 1, 8, buf, buf) == BAD
    assert lib.slam_ekf_factor_multiply(None, buf, 1, 8, buf) == BAD
