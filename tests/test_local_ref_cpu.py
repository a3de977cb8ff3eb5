"""Compressed local-area updates (slam_ekf_local_*, include/ext/slamhip_local.h), the parts that need no GPU: tests/local_ref.py
against the oracle's full filter, what is particular to this library's surface (the checks every side library shares are made from
its row of the table by tests/test_companions_cpu.py), and the status codes decided before a device is touched."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import abi_surface as ABI
from tests import local_ref as LF

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_local.h")
NAMES = {"slam_ekf_local_" + w for w in ("create", "destroy", "open", "state", "predict", "update", "augment", "close", "abort",
                                         "info", "get")}
R2 = np.array([[0.01, 0.0], [0.0, (math.pi / 180) ** 2]])
Q2 = np.array([[0.25, 0.0], [0.0, (3 * math.pi / 180) ** 2]])


def spd_state(N, seed):
    """A fully correlated SPD state, as smoke() builds it."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[50.0, 50.0, 0.3], rng.uniform(10, 90, 2 * N)])
    A = rng.normal(0, 0.2, (n, 8))
    return x, A @ A.T + 0.01 * np.eye(n), rng


def observe(x, ids, rng):
    z = np.zeros((2, len(ids)))
    for i, j in enumerate(ids):
        z[:, i] = O.predict_observation(x, j)[0] + rng.normal(0, [0.05, 0.005])
    return z


def run_both(N, ids, seed, steps):
    """The step list on the reference area and on the oracle's full filter; local ids are translated through ids.  A step is
    ("p", v, g), ("u", local ids) or ("a", new observations)."""
    x, P, rng = spd_state(N, seed)
    area = LF.LocalRef(x, P, ids)
    xo, Po = np.array(x), np.array(P)
    gids = list(ids)
    for st in steps:
        if st[0] == "p":
            area.predict(st[1], st[2], 4.0, Q2, 0.025)
            xo, Po = O.predict_sparse(xo, Po, st[1], st[2], 4.0, Q2, 0.025)
        elif st[0] == "u":
            z = observe(area.x, st[1], rng)
            area.update(z, st[1], R2)
            xo, Po = O.update_sparse(xo, Po, z, R2, [gids[j - 1] for j in st[1]])
        else:
            zn = np.asarray(st[1], dtype=float).reshape(2, -1)
            area.augment(zn, R2)
            xo, Po = O.add_features_sparse(xo, Po, zn, R2)
            gids += [(len(xo) - 3) // 2 - zn.shape[1] + 1 + i for i in range(zn.shape[1])]
    xc, Pc = area.close()
    return xc, Pc, xo, Po, area


SEQ = [("p", 7.5, 0.1), ("u", [2, 5, 7]), ("p", 7.0, -0.05), ("a", [[30.0, 22.0], [0.4, -0.7]]), ("u", [1, 9]), ("p", 7.5, 0.0)]


# ---- the reference against the oracle's full filter -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,ids,seed", [(24, [19, 3, 11, 24, 1, 8, 15], 1), (9, [4], 2), (12, list(range(12, 0, -1)), 3)])
def test_close_reproduces_the_full_filter(N, ids, seed):
    """Both sides are fp64 evaluations of the same rational function of the inputs; they differ by the rounding of two different
    orders of summation over at most n terms per entry and six steps, each amplified by the conditioning of S (R keeps it
    modest on these states).  1e3 u max|P| covers n (51) x steps (6) x a factor 3 for that amplification: u = 2^-53."""
    steps = SEQ if len(ids) >= 7 else [("p", 7.5, 0.1), ("u", [1]), ("a", [[30.0], [0.4]]), ("u", [2, 1]), ("p", 7.0, 0.0)]
    xc, Pc, xo, Po, area = run_both(N, ids, seed, steps)
    assert xc.shape == xo.shape and Pc.shape == Po.shape == (len(xo), len(xo))
    tol = 1e3 * 2.0 ** -53
    assert np.max(np.abs(Pc - Po)) <= tol * np.max(np.abs(Po))
    assert np.max(np.abs(xc - xo)) <= tol * np.max(np.abs(xo))
    assert np.max(np.abs(Pc - Pc.T)) <= tol * np.max(np.abs(Po))
    # the invariant P_ab(now) = phi P_ab(at open), on the oracle's own final state
    sel = LF.select_indices(ids)
    l2g = LF.local_to_global(ids, 3 + 2 * N, len(area.x))
    B = np.setdiff1d(np.arange(3 + 2 * N), sel)
    x0, P0, _ = spd_state(N, seed)
    if B.size:                                                            # (the last case: A is every landmark, B is empty)
        assert np.max(np.abs(Po[np.ix_(l2g, B)] - area.phi @ P0[np.ix_(sel, B)])) <= tol * np.max(np.abs(Po))


def test_no_steps_and_predict_only_areas():
    x, P, _ = spd_state(10, 5)
    xc, Pc = LF.LocalRef(x, P, [7, 2]).close()
    assert np.array_equal(xc, x) and np.array_equal(Pc, P)                # phi = I, psi = 0, theta = 0: every product is exact
    area = LF.LocalRef(x, P, [])                                           # the vehicle alone: P_vb follows the chain of Gv
    xo, Po = np.array(x), np.array(P)
    G = np.eye(3)
    for v, g in ((7.5, 0.1), (7.0, -0.2), (6.0, 0.3)):
        p = area.x[2]
        G = np.array([[1, 0, -v * 0.025 * math.sin(g + p)], [0, 1, v * 0.025 * math.cos(g + p)], [0, 0, 1]]) @ G
        area.predict(v, g, 4.0, Q2, 0.025)
        xo, Po = O.predict_sparse(xo, Po, v, g, 4.0, Q2, 0.025)
    xc, Pc = area.close()
    assert np.allclose(area.phi, G, rtol=0, atol=1e-15) and not area.psi.any() and not area.theta.any()
    assert np.max(np.abs(Pc[0:3, 3:] - G @ P[0:3, 3:])) <= 1e-15 and np.max(np.abs(Pc - Po)) <= 1e-14
    assert np.array_equal(xc[3:], x[3:]) and np.array_equal(Pc[3:, 3:], P[3:, 3:])


def test_the_bound_of_close_holds_for_a_rounded_model_of_it():
    """close with T and the stored results rounded to fp32 as the device rounds them (products and sums in double: fewer
    roundings than the matrix cores make) lies inside close_bound; a planted defect (psi transposed into psi + 0.01 psi') does not."""
    x, P, rng = spd_state(24, 8)
    x, P = x.astype(np.float32).astype(float), P.astype(np.float32).astype(float)
    ids = [19, 3, 11, 24, 1, 8, 15]
    area = LF.LocalRef(x, P, ids, np.float32)
    area.predict(7.5, 0.1, 4.0, Q2, 0.025)
    area.update(observe(area.x, [2, 5, 7], rng), [2, 5, 7], R2)
    xe, Pe = area.close()
    sel = LF.select_indices(ids)
    B = np.setdiff1d(np.arange(len(x)), sel)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(float)

    def model(psi):
        A0 = P[np.ix_(B, sel)]
        xm, Pm = np.array(xe), np.array(Pe)
        xm[B] = f32(x[B] + A0 @ area.theta)
        Pm[np.ix_(B, B)] = f32(P[np.ix_(B, B)] - f32(A0 @ psi) @ A0.T)
        Pab = f32(area.phi @ A0.T)
        Pm[np.ix_(sel, B)], Pm[np.ix_(B, sel)] = Pab, Pab.T
        return xm, Pm

    Bx, BP = LF.close_bound(x, P, ids, len(area.x), area.phi, area.psi, area.theta, xe, Pe, np.float32)
    xm, Pm = model(area.psi)
    assert np.all(np.abs(xm - xe) <= Bx) and np.all(np.abs(Pm - Pe) <= BP)
    assert not BP[np.ix_(sel, sel)].any() and BP[np.ix_(B, B)].min() > 0
    xm, Pm = model(area.psi * 1.01)
    assert np.any(np.abs(Pm - Pe) > BP)


# ---- the surface: the checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table --------
def test_what_is_particular_to_this_library(pkg):
    L = pkg._lib
    assert NAMES == set(L.local_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("LocalArea", "open_area!", "close!", "abort!", "landmarks_within"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text
    assert L.SLAM_LOCAL_MAXLM == 1024 == LF.MAXLM and "#define SLAM_LOCAL_MAXLM 1024" in text
    for word in ("local", "landmarks_within"):
        assert callable(getattr(pkg.EKFSlamState, word)), word
    for word in ("predict", "update", "add_features", "associate", "observe", "close", "abort", "accumulators"):
        assert callable(getattr(pkg.LocalArea, word)), word
    assert inspect.signature(pkg.sim.sim).parameters["local_radius"].default is None


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before a handle is read: the handles here are none."""
    L = pkg._lib
    lib = L.local_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    out = ctypes.c_void_p(0x7)
    assert lib.slam_ekf_local_create(None, fake, 4) == BAD
    assert lib.slam_ekf_local_create(ctypes.byref(out), None, 4) == BAD and "null handle" in L.last_error() and not out.value
    for bad in (0, -1, 1025):
        out = ctypes.c_void_p(0x7)
        assert lib.slam_ekf_local_create(ctypes.byref(out), fake, bad) == BAD and "SLAM_LOCAL_MAXLM" in L.last_error()
        assert not out.value
    dbl = (ctypes.c_double * 8)(*([1.0] * 8))
    i32 = (ctypes.c_int32 * 4)(1, 2, 3, 4)
    first = ctypes.c_int(-5)
    i64 = (ctypes.c_int64 * 8)()
    assert lib.slam_ekf_local_open(None, i32, 2) == BAD
    assert lib.slam_ekf_local_state(None, ctypes.byref(out)) == BAD
    assert lib.slam_ekf_local_predict(None, 1.0, 0.0, 4.0, dbl, 0.1) == BAD
    assert lib.slam_ekf_local_update(None, dbl, i32, 2, dbl, 0) == BAD
    assert lib.slam_ekf_local_augment(None, dbl, 2, dbl) == BAD
    assert lib.slam_ekf_local_close(None, ctypes.byref(first)) == BAD and first.value == -5
    assert lib.slam_ekf_local_abort(None) == BAD
    assert lib.slam_ekf_local_info(None, i64) == BAD
    assert lib.slam_ekf_local_get(None, dbl, dbl, dbl) == BAD
    assert lib.slam_ekf_local_destroy(None) == L.SLAM_OK
