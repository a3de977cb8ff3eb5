"""Caller-supplied models for the EKF (slam_ekf_update_linear / linear_nis / predict_linear / predict_odometry,
include/ext/slamhip_linear.h), the parts that need no GPU: tests/linear_ref.py against the oracle's update and predict,
tests/merge_ref.py and hand-derived answers; what is particular to this library's surface (the checks every side library shares are
made from its row of the table by tests/test_companions_cpu.py); and the status codes that are decided before a device is touched."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import abi_surface as ABI
from tests import linear_ref as LR
from tests import merge_ref as MR
from tests import update_records as UR

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_linear.h")
NAMES = {"slam_ekf_update_linear", "slam_ekf_linear_nis", "slam_ekf_predict_linear", "slam_ekf_predict_odometry"}
R2 = np.array([[0.01, 0.0], [0.0, (math.pi / 180) ** 2]])


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    return np.max(np.abs(got - want)) <= tol * max(1.0, float(np.max(np.abs(want))))


# ---- the reference against the existing oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 8])
def test_innovation_mode_reproduces_the_oracle_update(m):
    x, P, z, ids = UR.make_inputs("slam", 66, m, "f64")
    H = np.vstack([O.predict_observation(x, j)[1] for j in ids])
    v = np.concatenate([[z[0, i] - O.predict_observation(x, j)[0][0], O.mpi_to_pi(z[1, i] - O.predict_observation(x, j)[0][1])]
                        for i, j in enumerate(ids)])
    assert H.shape == (2 * m, len(x)) and int(np.max(np.count_nonzero(H, axis=1))) <= LR.MAXNNZ
    xr, Pr, out = LR.update(x, P, H, v, np.kron(np.eye(m), R2), mode=LR.INNOVATION)
    xo, Po = O.update(np.array(x), np.array(P), z, R2, ids)
    assert out[3] == -1 and _close(xr, xo) and _close(Pr, Po)
    # the gate's numbers: v' inv(S) v and log det S of the same S
    S = H @ P @ H.T + np.kron(np.eye(m), R2)
    assert abs(out[0] - v @ np.linalg.solve(S, v)) <= 1e-9 * out[0]
    assert abs(out[1] - np.linalg.slogdet(S)[1]) <= 1e-9 * max(1.0, abs(out[1]))


@pytest.mark.parametrize("noisy", [False, True])
def test_difference_rows_reproduce_the_merge_before_compaction(noisy):
    x, P = UR.designed_state("slam", 66, "f64", 31)
    pairs = [(3, 40), (32, 7), (66, 1)]
    x = np.array(x)
    for a, b in pairs:                                                    # near duplicates, so that the constraint is a sane one
        x[MR.f(b):MR.f(b) + 2] = x[MR.f(a):MR.f(a) + 2] + 0.01
    Rc = np.array([[0.02, 0.005], [0.005, 0.03]]) if noisy else None
    rows = []
    for a, b in pairs:
        rows += [{MR.f(a): 1.0, MR.f(b): -1.0}, {MR.f(a) + 1: 1.0, MR.f(b) + 1: -1.0}]
    H = LR.dense_H(len(x), rows)
    assert np.array_equal(H, MR.dense_H(len(x), pairs))
    RR = np.kron(np.eye(len(pairs)), np.zeros((2, 2)) if Rc is None else Rc)
    xr, Pr, out = LR.update(x, P, H, np.zeros(len(rows)), RR)
    xm, Pm = MR.fuse(x, P, pairs, Rc)
    assert out[3] == -1 and _close(xr, xm) and _close(Pr, Pm)


def _bicycle(x, v, g, w, Q, dt):
    phi = x[2]
    s, c = math.sin(g + phi), math.cos(g + phi)
    vts, vtc = v * dt * s, v * dt * c
    Gv = np.array([[1.0, 0.0, -vts], [0.0, 1.0, vtc], [0.0, 0.0, 1.0]])
    Gu = np.array([[dt * c, -vts], [dt * s, vtc], [dt * math.sin(g) / w, v * dt * math.cos(g) / w]])
    xv = np.array([x[0] + vtc, x[1] + vts, O.mpi_to_pi(phi + v * dt * math.sin(g) / w)])
    return xv, Gv, Gu @ Q @ Gu.T


def test_predict_linear_with_the_bicycle_jacobians_reproduces_the_oracle_predict():
    Q = np.array([[0.25, 0.01], [0.01, (3 * math.pi / 180) ** 2]])
    for N, phi in ((0, 0.3), (5, -2.0), (66, 3.13)):                      # the last heading crosses +pi
        x, P = UR.designed_state("slam", 66, "f64", 5)
        n = 3 + 2 * N
        x, P = np.array(x[:n]), np.array(P[:n, :n])
        x[2] = phi
        xv, Gv, Qv = _bicycle(x, 7.5, 0.4, 4.0, Q, 0.25)
        xr, Pr = LR.predict_linear(x, P, xv, Gv, Qv)
        xo, Po = O.predict(np.array(x), np.array(P), 7.5, 0.4, 4.0, Q, 0.25)
        assert _close(xr, xo) and _close(Pr, Po) and np.array_equal(Pr, Pr.T)
    assert xo[2] < 0 < phi


def test_predict_odometry_on_a_hand_written_three_landmark_case():
    """Heading 0: the rotation is the identity, so Gv = [1 0 -dy; 0 1 dx; 0 0 1] and Qv = Q3, written out entry by entry."""
    rng = np.random.default_rng(2)
    A = rng.normal(0, 0.3, (9, 9))
    P = A @ A.T + 0.1 * np.eye(9)
    x = np.array([4.0, -1.0, 0.0, 10.0, 2.0, -3.0, 8.0, 0.5, 0.25])
    d = np.array([2.0, 0.5, 0.3])
    Q3 = np.array([[0.04, 0.01, 0.002], [0.01, 0.09, 0.003], [0.002, 0.003, 0.0025]])
    xr, Pr = LR.predict_odometry(x, P, d, Q3)
    want = np.array(P)
    for f in range(3, 9):                                                 # the strip: row f against the vehicle's columns
        want[f, 0] = want[0, f] = P[f, 0] - 0.5 * P[f, 2]
        want[f, 1] = want[1, f] = P[f, 1] + 2.0 * P[f, 2]
    G = [[1.0, 0.0, -0.5], [0.0, 1.0, 2.0], [0.0, 0.0, 1.0]]
    for r in range(3):
        for c in range(3):
            want[r, c] = sum(G[r][a] * P[a, b] * G[c][b] for a in range(3) for b in range(3)) + Q3[r, c]
    assert _close(Pr, want) and np.array_equal(Pr[3:, 3:], P[3:, 3:])
    assert _close(xr, [6.0, -0.5, 0.3, 10.0, 2.0, -3.0, 8.0, 0.5, 0.25])
    # heading pi / 2: the increment points along +y, (dx, dy) -> (-dy, dx); the heading crosses +pi on the way
    x[2] = math.pi / 2
    xr, Pr = LR.predict_odometry(x, P, [2.0, 0.5, 2.0], Q3)
    assert _close(xr[:3], [4.0 - 0.5, -1.0 + 2.0, math.pi / 2 + 2.0 - 2 * math.pi])
    assert _close(Pr[0:3, 0:3] - (np.array([[1, 0, -2.0], [0, 1, -0.5], [0, 0, 1]]) @ P[0:3, 0:3] @ np.array([[1, 0, -2.0], [0, 1, -0.5], [0, 0, 1]]).T),
                  np.array([[0.09, -0.01, -0.003], [-0.01, 0.04, 0.002], [-0.003, 0.002, 0.0025]]), 1e-12)


# ---- hand-derived known answers -------------------------------------------------------------------------------------------------
def test_position_fix_on_a_bare_vehicle_gives_the_scalar_kalman_gains():
    x = np.array([1.0, 2.0, 0.5])
    P = np.diag([4.0, 9.0, 0.01])
    R = np.diag([1.0, 3.0])
    z = np.array([2.0, 0.5])
    xr, Pr, out = LR.update(x, P, LR.dense_H(3, [{0: 1.0}, {1: 1.0}]), z, R)
    kx, ky = 4.0 / 5.0, 9.0 / 12.0
    assert _close(xr, [1.0 + kx * 1.0, 2.0 + ky * -1.5, 0.5])
    assert _close(Pr, np.diag([4.0 * 1.0 / 5.0, 9.0 * 3.0 / 12.0, 0.01]))
    assert _close(out, [1.0 / 5.0 + 2.25 / 12.0, math.log(5.0 * 12.0), math.sqrt(5.0), -1.0])


def test_heading_fix_across_the_cut_differs_by_two_pi_times_the_gain():
    x = np.array([0.0, 0.0, 3.1])
    P = np.diag([1.0, 1.0, 0.04])
    H = LR.dense_H(3, [{2: 1.0}])
    gain = 0.04 / 0.05
    xw, Pw, ow = LR.update(x, P, H, [-3.1], [[0.01]], wrap_mask=1)
    xn, Pn, on = LR.update(x, P, H, [-3.1], [[0.01]], wrap_mask=0)
    assert _close(xw[2], 3.1 + gain * (2 * math.pi - 6.2)) and _close(xn[2], 3.1 - gain * 6.2)
    assert _close(xw[2] - xn[2], 2 * math.pi * gain) and np.array_equal(Pw, Pn) and _close(Pw[2, 2], 0.04 * 0.01 / 0.05)
    assert xw[2] > math.pi                                                # the heading is not wrapped after the update
    assert _close(ow[0], (2 * math.pi - 6.2) ** 2 / 0.05) and _close(on[0], 6.2 ** 2 / 0.05)


def test_a_singular_s_is_reported_with_its_pivot_and_leaves_the_state():
    x, P = UR.designed_state("slam", 66, "f64", 9)
    H = LR.dense_H(len(x), [{0: 1.0, 7: 2.0}, {0: 1.0, 7: 2.0}])
    xr, Pr, out = LR.update(x, P, H, [0.1, 0.1], np.zeros((2, 2)))
    assert out[3] == 1 and out[0] == 0 and out[1] == 0 and not out[2] > 1e-12 * P[0, 0]
    assert np.array_equal(xr, x) and np.array_equal(Pr, P)
    ptr, idx, val = LR.csr([{0: 1.0, 7: 2.0}, {5: -1.0}])
    assert ptr.tolist() == [0, 2, 3] and idx.tolist() == [0, 7, 5] and val.tolist() == [1.0, 2.0, -1.0]


# ---- the surface: the checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table --------
def test_what_is_particular_to_this_library(pkg):
    L = pkg._lib
    assert NAMES == set(L.linear_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("update_linear!", "linear_nis", "predict_linear!", "predict_odometry!", "fix_position!", "fix_heading!", "fix_landmark!"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text
    assert (L.SLAM_LINEAR_MAXROWS, L.SLAM_LINEAR_MAXNNZ) == (16, 8) == (LR.MAXROWS, LR.MAXNNZ)
    assert "#define SLAM_LINEAR_MAXROWS 16" in text and "#define SLAM_LINEAR_MAXNNZ 8" in text
    assert (L.SLAM_LINEAR_MEASURED, L.SLAM_LINEAR_INNOVATION) == (0, 1) == (LR.MEASURED, LR.INNOVATION)
    for word in ("update_linear", "linear_nis", "predict_linear", "predict_odometry", "fix_position", "fix_heading", "fix_landmark",
                 "constrain_landmarks"):
        assert callable(getattr(pkg.EKFSlamState, word)), word


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before the handle is read: the handle here is not one."""
    L = pkg._lib
    lib = L.linear_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    ptr = (ctypes.c_int32 * 18)(*range(18))
    idx = (ctypes.c_int32 * 17)(*([0] * 17))
    dbl = (ctypes.c_double * 289)(*([1.0] * 289))
    out = (ctypes.c_double * 4)(*([7.0] * 4))
    for fn in (lib.slam_ekf_update_linear, lib.slam_ekf_linear_nis):
        assert fn(None, 1, ptr, idx, dbl, dbl, dbl, 0, 0, out) == BAD and "null handle" in L.last_error()
        for hole in range(2, 7):
            args = [fake, 1, ptr, idx, dbl, dbl, dbl, 0, 0, out]
            args[hole] = None
            assert fn(*args) == BAD, hole
        assert fn(fake, 1, ptr, idx, dbl, dbl, dbl, 0, 0, None) == BAD
        assert fn(fake, 0, ptr, idx, dbl, dbl, dbl, 0, 0, out) == BAD and "SLAM_LINEAR_MAXROWS" in L.last_error()
        assert fn(fake, 17, ptr, idx, dbl, dbl, dbl, 0, 0, out) == BAD
        assert fn(fake, -1, ptr, idx, dbl, dbl, dbl, 0, 0, out) == BAD
        assert fn(fake, 2, ptr, idx, dbl, dbl, dbl, 2, 0, out) == BAD and "mode" in L.last_error()
        assert fn(fake, 2, ptr, idx, dbl, dbl, dbl, 1, 1, out) == BAD and "wrap_mask" in L.last_error()
        assert fn(fake, 2, ptr, idx, dbl, dbl, dbl, 0, 4, out) == BAD and "wrap_mask" in L.last_error()
        assert list(out) == [7.0] * 4
    assert lib.slam_ekf_predict_linear(None, dbl, dbl, dbl) == BAD
    assert lib.slam_ekf_predict_linear(fake, None, dbl, dbl) == BAD
    assert lib.slam_ekf_predict_linear(fake, dbl, None, dbl) == BAD
    assert lib.slam_ekf_predict_linear(fake, dbl, dbl, None) == BAD
    assert lib.slam_ekf_predict_odometry(None, dbl, dbl) == BAD
    assert lib.slam_ekf_predict_odometry(fake, None, dbl) == BAD
    assert lib.slam_ekf_predict_odometry(fake, dbl, None) == BAD
    nan = (ctypes.c_double * 9)(*([float("nan")] * 9))
    assert lib.slam_ekf_predict_linear(fake, dbl, nan, dbl) == BAD and "finite" in L.last_error()
    assert lib.slam_ekf_predict_odometry(fake, nan, dbl) == BAD


def test_linear_rows_takes_a_dense_matrix_or_a_list_of_rows(pkg):
    rows = [{0: 1.0, 7: 2.0}, {5: -1.0}]
    ptr, idx, val = pkg.ekf.linear_rows(rows, 9)
    want = LR.csr(rows)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip((ptr, idx, val), want))
    ptr, idx, val = pkg.ekf.linear_rows(LR.dense_H(9, rows), 9)
    assert all(np.array_equal(a, b) for a, b in zip((ptr, idx, val), want))
    with pytest.raises(ValueError):
        pkg.ekf.linear_rows(np.zeros((2, 8)), 9)
