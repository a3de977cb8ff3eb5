"""The iterated EKF update (slam_ekf_update_iterated, include/ext/slamhip_iterated.h), the parts that need no GPU:
tests/iterated_ref.py against the oracle's update, against the full n-dimensional iteration and against the cost it minimises; the
conditions the designed hard scenes of tests/test_gpu_ekf_iterated.py must meet; and the surface checks tests/test_local_ref_cpu.py
makes for its library, here for this one (header == ctypes table == exports == Julia ccalls, how it finds its neighbour, disjoint
export sets, the two loader tables unchanged, the loader's two refusals, the status codes decided before a device is touched)."""
import ctypes
import glob
import inspect
import math
import os
import shutil
import subprocess
import sys

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


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_ctypes_library_and_julia_name_the_same_surface(pkg):
    L = pkg._lib
    loader = L.iterated_lib
    sigs = L.ITERATED_SIGNATURES
    assert loader.signatures is sigs and loader.name == "iterated"
    assert loader.path == L.ITERATED_LIB_PATH == os.path.join(os.path.dirname(L.LIB_PATH), "libslamhip_iterated.so")
    names = ABI.declared(HEADER)
    assert names == NAMES == set(sigs) == ABI.exported(loader.path), (names, set(sigs), ABI.exported(loader.path))
    protos = ABI.prototypes(HEADER)
    assert set(protos) == names
    for sym, (res, args) in sigs.items():
        assert protos[sym] == len(args), (sym, protos[sym], len(args))
        assert res is ctypes.c_int, sym
    needed = ABI.dynamic_section(loader.path)
    assert "libslamhip.so" in needed and "$ORIGIN" in needed
    ldd = subprocess.run(["ldd", loader.path], capture_output=True, text=True).stdout
    assert "libslamhip.so" in ldd and "torch" not in ldd and "python" not in ldd
    lib = loader()
    assert lib is loader() and all(getattr(lib, sym).argtypes == args for sym, (_res, args) in sigs.items())
    calls = ABI.julia_ccalls("libslamhip_iterated")
    assert {c[0] for c in calls} == names
    for sym, ret, nargs in calls:
        assert ret == "Cint" and nargs == len(sigs[sym][1]), (sym, ret, nargs, len(sigs[sym][1]))
    with open(ABI.JULIA) as f:
        src = f.read()
    for sym in names:
        assert f"(:{sym}, libslamhip_iterated)" in src
    assert "SLAMHIP_ITERATED_LIB" in src
    for word in ("update_iterated!", "iterated_nis", "observe_iterated!"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text
    assert L.SLAM_ITERATED_MAXOBS == 8 == IR.MAXOBS and "#define SLAM_ITERATED_MAXOBS 8" in text
    assert L.SLAM_ITERATED_MAXITER == 64 == IR.MAXITER and "#define SLAM_ITERATED_MAXITER 64" in text
    lim = (ctypes.c_int32 * 2)()
    assert lib.slam_ekf_iterated_limits(lim) == L.SLAM_OK and list(lim) == [8, 64]      # (touches no device)


def test_the_tables_are_unchanged_and_the_export_sets_disjoint(pkg):
    L = pkg._lib
    assert list(L.COMPANIONS) == ["frame", "join", "evidence", "jc", "path", "copy", "handover", "pfcopy"]
    assert list(L.EXTENSIONS) == ["factor"]
    assert L.iterated_lib not in list(L.COMPANIONS.values()) + list(L.EXTENSIONS.values())
    mine = ABI.exported(L.ITERATED_LIB_PATH)
    assert mine == NAMES
    assert not mine & ABI.exported(L.LIB_PATH)
    assert not NAMES & set(L.SIGNATURES)
    # libslamhip.so exports what its two headers declare, no more: this library added nothing to it
    product = ABI.declared(os.path.join(ABI.INCLUDE, "slamhip.h")) | ABI.declared(os.path.join(ABI.INCLUDE, "slamhip_diag.h"))
    assert ABI.exported(L.LIB_PATH) == product == set(L.SIGNATURES)
    others = [("linear", L.linear_lib), ("proposal", L.proposal_lib), ("local", L.local_lib)]
    for name, c in list(L.COMPANIONS.items()) + list(L.EXTENSIONS.items()) + others:
        assert not mine & ABI.exported(c.path), name
        assert not NAMES & set(c.signatures), name
    assert HEADER not in glob.glob(os.path.join(ABI.INCLUDE, "slamhip*.h"))
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


REFUSAL = """
import os, sys
sys.path.insert(0, {root!r})
from __graft_entry__ import load_package
L = load_package()._lib
assert L.LIB_PATH == os.environ["SLAMHIP_LIBRARY"]
own = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "libslamhip.so")
try:
    L.iterated_lib()
except ImportError as e:
    for word in ("libslamhip_iterated.so", own, L.LIB_PATH, "SLAMHIP_LIBRARY"):
        assert word in str(e), (word, str(e))
else:
    raise SystemExit("opened although the handles belong to another library")
print("refused")
"""

MISSING = """
import importlib.util, os, sys
d = {copy!r}
spec = importlib.util.spec_from_file_location("slam_copy_without_iterated", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
mod = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = mod
spec.loader.exec_module(mod)
loader = mod._lib.iterated_lib
assert loader.path == os.path.join(d, "libslamhip_iterated.so") and not os.path.exists(loader.path)
try:
    loader()
except ImportError as e:
    for word in (loader.path, "is missing", "make -C slam.jl_amd/csrc"):
        assert word in str(e), (word, str(e))
else:
    raise SystemExit("opened although it is not there")
print("missing")
"""


def _child(script, env):
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout.split()


def test_the_loader_refuses_a_foreign_product_library(pkg, tmp_path):
    foreign = str(tmp_path / "libslamhip.so")
    shutil.copy(pkg._lib.LIB_PATH, foreign)
    assert _child(REFUSAL.format(root=ABI.ROOT), dict(os.environ, SLAMHIP_LIBRARY=foreign)) == ["refused"]


def test_the_loader_names_the_build_command_when_the_library_was_not_built(pkg, tmp_path):
    copy = tmp_path / "pkg"
    copy.mkdir()
    pkgdir = os.path.dirname(os.path.abspath(pkg._lib.__file__))
    for path in glob.glob(os.path.join(pkgdir, "*.py")) + [os.path.join(pkgdir, "libslamhip.so")]:
        shutil.copy(path, str(copy))
    env = {k: v for k, v in os.environ.items() if k != "SLAMHIP_LIBRARY"}
    assert _child(MISSING.format(copy=str(copy)), env) == ["missing"]
