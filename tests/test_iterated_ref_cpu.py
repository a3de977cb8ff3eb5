"""The iterated EKF update (slam_ekf_update_iterated, include/ext/slamhip_iterated.h), the parts that need no GPU:
tests/iterated_ref.py against the oracle's update, against the full n-dimensional iteration and against the cost it minimises; the
conditions the designed hard scenes of tests/test_gpu_ekf_iterated.py must meet; what is particular to this library's surface (the
checks every side library shares are made from its row of the table by tests/test_companions_cpu.py); and the status codes decided
before a device is touched."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import abi_surface as ABI
from tests import iterated_ref as IR

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_iterated.h")
NAMES = {"slam_ekf_update_iterated", "slam_ekf_iterated_nis", "slam_ekf_iterated_limits"}
DTYPES = ["f64", "f32"]
HARD = [name for name in IR.SCENES if name != "N200-m11"]


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


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ids", [(24, [19, 3, 11]), (9, [4]), (12, [12, 1, 5, 7, 2, 9, 10, 3])])
def test_one_iteration_is_the_oracles_update(N, ids):
    x, P, rng = spd_state(N, len(ids))
    R = np.array([[0.01, 0.001], [0.001, (math.pi / 180) ** 2]])
    z = observe(x, ids, rng)
    xr, Pr, out = IR.update(x, P, z, R, ids, max_iter=1, tol=0.0)
    xo, Po = O.update_sparse(x, P, z, R, ids)
    assert out[0] == 1 and out[1] == 0 and out[6] == -1 and out[7] == -1
    assert np.max(np.abs(xr - xo)) <= 1e-12 * np.max(np.abs(xo)) and np.max(np.abs(Pr - Po)) <= 1e-12 * np.max(np.abs(Po))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", HARD)
def test_the_reduced_iteration_is_the_full_one(name, dtype):
    """The iterates of the states H touches depend on P only through P[a, a]: both forms run the same number of iterations and end
    in the same state, to 1e-12 of the largest entry."""
    x, P, z, ids = IR.scene(name, dtype)
    xr, Pr, out = IR.update(x, P, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
    xf, Pf, it = IR.update_full(x, P, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
    assert it == out[0]
    assert np.max(np.abs(xr - xf)) <= 1e-12 * np.max(np.abs(xf)) and np.max(np.abs(Pr - Pf)) <= 1e-12 * np.max(np.abs(Pf))
    assert np.max(np.abs(Pr - Pr.T)) <= 1e-12 * np.max(np.abs(Pf))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(IR.SCENES))
def test_the_hard_scenes_meet_their_conditions(name, dtype):
    """What tests/test_gpu_ekf_iterated.py relies on: the reference converges within ITER_HARD iterations at TOL_HARD, and no step
    lies within a factor 4 of TOL_HARD, so that an ulp of difference in the device's trigonometry cannot change the iteration
    count.  The scene is what its description says: landmarks 3 .. 10 m away, the inflated vehicle block."""
    x, P, z, ids = IR.scene(name, dtype)
    d = np.hypot(x[IR.f(1) + 2 * (ids - 1)] - x[0], x[IR.f(1) + 2 * (ids - 1) + 1] - x[1])
    assert np.all(d > 2.99) and np.all(d < 10.01)
    assert np.allclose(np.diag(P)[:3], [0.25, 0.25, 0.04], rtol=1e-6) and not P[0:3, 3:].any()
    for s in range(0, len(ids), IR.MAXOBS):
        zz, ii = z[:, s:s + IR.MAXOBS], ids[s:s + IR.MAXOBS]
        x, P, out, steps = IR.update(x, P, zz, IR.R_HARD, ii, IR.ITER_HARD, IR.TOL_HARD, with_steps=True)
        assert out[6] == -1 and out[1] == 1 and out[0] == len(steps) <= IR.ITER_HARD, (name, out)
        assert IR.steps_clear_of(steps, IR.TOL_HARD), (name, steps)
        assert len(steps) >= 3                                            # one linearisation is not enough here
    if name == "N70-m3-cut":                                              # the bearing IS 2 pi off at the prior mean
        x0, _, z0, ids0 = IR.scene(name, dtype)
        assert abs(z0[1, 0] - O.predict_observation(x0, ids0[0])[0][1]) > math.pi
    if name == "N200-m3-duplicate":
        assert len(set(ids.tolist())) < len(ids)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n in HARD if n != "N200-m3-duplicate"])
def test_the_fixed_point_minimises_the_cost_the_one_shot_update_does_not(name, dtype):
    """At the fixed point the central-difference gradient of J is below 1e-6 of the gradient at the one-shot result, J_last is less
    than half of J_first, and out[8], out[9] are J at x_1 and at x_last (the closed form of the prior's term against the explicit
    quadratic form: 1e-9 relative)."""
    x, P, z, ids = IR.scene(name, dtype)
    a = IR.state_indices(ids)
    x0a, Pa = x[a], P[np.ix_(a, a)]
    x1, _, out1 = IR.update(x, P, z, IR.R_HARD, ids, 1, 0.0)
    xl, _, out = IR.update(x, P, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
    g1 = np.max(np.abs(IR.cost_gradient(x1[a], x0a, Pa, z, IR.R_HARD)))
    gl = np.max(np.abs(IR.cost_gradient(xl[a], x0a, Pa, z, IR.R_HARD)))
    print(f"iterated ref {name} {dtype}: |grad J| {g1:.3e} -> {gl:.3e}, J {out[8]:.4f} -> {out[9]:.4f} in {int(out[0])} iterations")
    assert gl < 1e-6 * g1
    assert out[9] < 0.5 * out[8] and out[8] == out1[8] == out1[9]
    assert abs(IR.map_cost(x1[a], x0a, Pa, z, IR.R_HARD) - out[8]) <= 1e-9 * out[8]
    assert abs(IR.map_cost(xl[a], x0a, Pa, z, IR.R_HARD) - out[9]) <= 1e-9 * out[9]


def test_duplicated_ids_work():
    """The same landmark observed twice in one call: the reduced block repeats its rows and columns, H has its Hf blocks in separate
    columns, and the result is the full iteration's, where the two blocks share the landmark's columns."""
    x, P, z, ids = IR.scene("N200-m3-duplicate", "f64")
    assert ids[0] == ids[2]
    xr, Pr, out = IR.update(x, P, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
    xf, Pf, it = IR.update_full(x, P, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
    assert it == out[0] and out[1] == 1 and out[9] < 0.5 * out[8]
    assert np.max(np.abs(xr - xf)) <= 1e-12 * np.max(np.abs(xf)) and np.max(np.abs(Pr - Pf)) <= 1e-12 * np.max(np.abs(Pf))
    x1, P1, _ = IR.update(x, P, z, IR.R_HARD, ids, 1, 0.0)
    xo, Po = O.update_sparse(x, P, z, IR.R_HARD, ids)
    assert np.max(np.abs(x1 - xo)) <= 1e-12 * np.max(np.abs(xo)) and np.max(np.abs(P1 - Po)) <= 1e-12 * np.max(np.abs(Po))


def test_a_failing_pivot_is_reported_and_changes_nothing():
    x, P, z, ids = IR.scene("N70-m3-straddler", "f64")
    P = P.copy()
    P[0, 0] = P[1, 1] = -10.0
    xr, Pr, out = IR.update(x, P, z, IR.R_HARD, ids, 5, 1e-9)
    assert out[6] == 0 and out[7] == 0 and out[0] == 0 and out[5] < 0 and out[3] == 0 and out[4] == 0
    assert np.array_equal(xr, x) and np.array_equal(Pr, P)


# ---- the surface: the checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table --------
def test_what_is_particular_to_this_library(pkg):
    L = pkg._lib
    assert NAMES == set(L.iterated_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("update_iterated!", "iterated_nis", "observe_iterated!"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text
    assert L.SLAM_ITERATED_MAXOBS == 8 == IR.MAXOBS and "#define SLAM_ITERATED_MAXOBS 8" in text
    assert L.SLAM_ITERATED_MAXITER == 64 == IR.MAXITER and "#define SLAM_ITERATED_MAXITER 64" in text
    lim = (ctypes.c_int32 * 2)()
    assert L.iterated_lib().slam_ekf_iterated_limits(lim) == L.SLAM_OK and list(lim) == [8, 64]      # (touches no device)
    for word in ("update_iterated", "iterated_nis", "observe_iterated"):
        assert callable(getattr(pkg.EKFSlamState, word)), word
    assert inspect.signature(pkg.EKFSlamState.update_iterated).parameters["max_iter"].default == 10
    assert inspect.signature(pkg.EKFSlamState.update_iterated).parameters["tol"].default == 1e-9
    assert inspect.signature(pkg.sim.sim).parameters["iterated"].default is None
    assert "not the joint update" in pkg.EKFSlamState.update_iterated.__doc__


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before a handle is read: the handle here is none."""
    L = pkg._lib
    lib = L.iterated_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    z = (ctypes.c_double * 16)(*([5.0, 0.1] * 8))
    ids = (ctypes.c_int32 * 8)(*range(1, 9))
    R = (ctypes.c_double * 4)(0.01, 0.0, 0.0, 0.0003)
    out = (ctypes.c_double * 10)(*([7.0] * 10))
    nan, inf = float("nan"), float("inf")
    for fn in (lib.slam_ekf_update_iterated, lib.slam_ekf_iterated_nis):
        assert fn(None, z, ids, 2, R, 5, 1e-9, out) == BAD and "null handle" in L.last_error()
        for args in ((None, ids, 2, R, 5, 1e-9, out), (z, None, 2, R, 5, 1e-9, out), (z, ids, 2, None, 5, 1e-9, out),
                     (z, ids, 2, R, 5, 1e-9, None)):
            assert fn(fake, *args) == BAD and "null argument" in L.last_error()
        for m in (0, -1, 9):
            assert fn(fake, z, ids, m, R, 5, 1e-9, out) == BAD and "SLAM_ITERATED_MAXOBS" in L.last_error()
        for it in (0, -3, 65):
            assert fn(fake, z, ids, 2, R, it, 1e-9, out) == BAD and "max_iter" in L.last_error()
        for tol in (-1e-12, nan, inf):
            assert fn(fake, z, ids, 2, R, 5, tol, out) == BAD and "tol" in L.last_error()
        for bad in (nan, inf):
            zb = (ctypes.c_double * 16)(*([5.0, 0.1, 6.0, bad] + [0.0] * 12))
            assert fn(fake, zb, ids, 2, R, 5, 1e-9, out) == BAD and "zf" in L.last_error()
        for Rb in ((0.01, 0.0, 0.0, nan), (0.01, 1e-4, 2e-4, 0.0003), (0.01, 0.0, 0.0, -0.0003), (0.0, 0.0, 0.0, 0.0003),
                   (0.01, 0.02, 0.02, 0.0003)):
            assert fn(fake, z, ids, 2, (ctypes.c_double * 4)(*Rb), 5, 1e-9, out) == BAD and "R is" in L.last_error(), Rb
    assert list(out) == [7.0] * 10
    assert lib.slam_ekf_iterated_limits(None) == BAD
