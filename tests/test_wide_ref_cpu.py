"""The joint update of up to 64 observations (libslamhip_wide.so, include/ext/slamhip_wide.h), the parts that need no GPU:
tests/wide_ref.py against tests/fej_ref.py (m <= 8: the same rule) and against the oracle (the points re-set to x); H N = 0 for the
wide H; that the joint update and the chain of 8-observation batches are DIFFERENT filters; the condition of the scenes the GPU
tests use; failing pivots at m > 8; and what is particular to this library's surface (the checks every side library shares are
made from its row of the table by tests/test_companions_cpu.py).

The bars: 1e-12 where fp64 rounding alone separates two quantities (two NumPy evaluations of the same rule on matrices of
condition <= 1e5).  The scenes: positive definite in the reference for both dtypes' rounded states and both seeds, cond(S) <= 2e6
(the double front half then carries cond(S) u64 = 2e-10, below the fp64 bar 1e-9 of the GPU tests), the smallest l_ii >= 0.010."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import abi_surface as ABI
from tests import fej_ref as F
from tests import iterated_ref as IR
from tests import wide_ref as W

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_wide.h")
NAMES = {"slam_ekf_wide_" + w for w in ("update", "nis", "limits")}
FEJ_NAMES = {"slam_ekf_fej_" + w for w in ("create", "destroy", "predict", "update", "augment", "reset", "remap", "transform", "get",
                                           "set", "limits")}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. the rule against its siblings -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["N1-m1", "N70-m3-straddler", "N70-m8", "N200-m8-last", "N200-m3-duplicate"])
def test_up_to_eight_observations_it_is_the_fej_rule(name):
    x, P, z, ids = IR.scene(name, "f64")
    lin, first = W.displaced(x, 11)
    xa, Pa, oa, Ha = W.update(x, P, lin, first, z, IR.R_HARD, ids)
    xb, Pb, ob, Hb = F.update(x, P, lin, first, z, IR.R_HARD, ids)
    assert oa[3] == -1 == ob[3] and np.array_equal(Ha, Hb)
    assert _rel(xa, xb) <= 1e-12 and _rel(Pa, Pb) <= 1e-12 and _rel(oa[:3], ob[:3]) <= 1e-12


@pytest.mark.parametrize("N,m,repeat", [(70, 9, False), (70, 33, True), (200, 64, False)])
def test_with_the_points_reset_to_the_state_it_is_the_oracles_update(N, m, repeat):
    x, P, z, ids = W.scene(N, m, "f64", 3, repeat)
    xa, Pa, out, _ = W.update_at_estimates(x, P, z, IR.R_HARD, ids)
    xo, Po = O.update(x, P, z, IR.R_HARD, ids)
    ex, eP = _rel(xa, xo), _rel(Pa, Po)
    print(f"wide rule at the estimates against the oracle, N {N} m {m}: x {ex:.3e} P {eP:.3e}")
    assert out[3] == -1 and ex <= 1e-12 and eP <= 1e-12


@pytest.mark.parametrize("N,m,repeat", [(70, 17, False), (200, 64, True)])
def test_the_wide_jacobian_is_blind_to_the_three_directions(N, m, repeat):
    x, P, z, ids = W.scene(N, m, "f64", 5, repeat)
    lin, first = W.displaced(x, 11)
    H = W.update(x, P, lin, first, z, IR.R_HARD, ids)[3]
    assert H.shape == (2 * m, len(x))
    ratio = np.max(np.abs(H @ F.N_matrix(lin, first))) / np.max(np.abs(H))
    std = np.max(np.abs(H @ F.N_matrix(*F.create(x)))) / np.max(np.abs(H))
    print(f"wide max|H N| / max|H|, N {N} m {m}: at the points {ratio:.3e}, against the estimates' directions {std:.3e}")
    assert ratio <= 1e-12


def test_the_joint_update_and_the_chain_of_batches_are_different_filters():
    """Eleven observations: the chain takes the residuals of the second batch at the mean the first one left, with Jacobians that did
    not follow it; the joint update takes all eleven at the mean before the call.  With displaced points the two differ far above
    rounding -- they are different estimators, not two evaluations of one."""
    x, P, z, ids = IR.scene("N200-m11", "f64")
    lin, first = W.displaced(x, 11)
    xj, Pj, out, _ = W.update(x, P, lin, first, z, IR.R_HARD, ids)
    xb, Pb, outs = F.update_batches(x, P, lin, first, z, IR.R_HARD, ids)
    assert out[3] == -1 and len(outs) == 2
    dx, dP = _rel(xj, xb), _rel(Pj, Pb)
    print(f"wide joint against 8 + 3: x differs by {dx:.3e}, P by {dP:.3e}")
    assert dx > 1e-6
    # (P agrees to rounding: the Jacobians do not move between the batches, so both add the same information)
    assert dP <= 1e-12
    x2, P2, _ = W.update_batches(x, P, lin, first, z, IR.R_HARD, ids)
    assert np.array_equal(x2, xj) and np.array_equal(P2, Pj)             # (11 <= 64: one batch of this rule)


# ---- 2. the scenes of the GPU tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_gpu_scene_is_positive_definite_and_well_conditioned_in_the_reference(dtype):
    worst = dict(cond=0.0, lmin=math.inf, nis=(math.inf, 0.0))
    for seed in W.SEEDS:
        for N, m, repeat in W.SCENES:
            x, P, z, ids = W.scene(N, m, dtype, seed, repeat)
            assert len(ids) == m and ids[0] == IR.STRADDLER[dtype] and (m < 2 or ids[1] == N or (repeat and m == 2))
            assert (len(set(ids.tolist())) == m - 1) if repeat else (len(set(ids.tolist())) == m)
            for l, f in (W.displaced(x, 11), F.create(x)):
                _, _, out, H = W.update(x, P, l, f, z, IR.R_HARD, ids)
                S = H @ P @ H.T + np.kron(np.eye(m), IR.R_HARD)
                assert out[3] == -1, (dtype, seed, N, m, repeat)
                worst["cond"] = max(worst["cond"], np.linalg.cond(S))
                worst["lmin"] = min(worst["lmin"], out[2])
                worst["nis"] = (min(worst["nis"][0], out[0]), max(worst["nis"][1], out[0]))
    print(f"wide scenes {dtype}: {worst}")
    assert worst["cond"] <= 2e6 and worst["lmin"] >= 0.010 and worst["nis"][1] <= 25.0


# ---- 3. failing pivots at m > 8 -----------------------------------------------------------------------------------------------------
def test_a_failing_pivot_and_coinciding_points_change_nothing_at_twenty_observations():
    x, P, z, ids = W.scene(70, 20, "f64", 3)
    lin, first = W.displaced(x, 11)
    j = int(ids[12])
    Pn = P.copy()
    Pn[F.f(j), F.f(j)] = Pn[F.f(j) + 1, F.f(j) + 1] = -10.0
    Pn[F.f(j), F.f(j) + 1] = Pn[F.f(j) + 1, F.f(j)] = 0.0
    xr, Pr, out, _ = W.update(x, Pn, lin, first, z, IR.R_HARD, ids)
    assert out[3] == 24 and out[2] < 0 and out[0] == 0 and out[1] == 0
    assert np.array_equal(xr, x) and np.array_equal(Pr, Pn)
    same = first.copy()
    same[2 * (j - 1):2 * j] = lin[0:2]                                     # that landmark's first estimate IS the linearisation pose
    xr, Pr, out, _ = W.update(x, P, lin, same, z, IR.R_HARD, ids)
    assert out[3] == 24 and not math.isfinite(out[2])
    assert np.array_equal(xr, x) and np.array_equal(Pr, P)


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------
def test_what_is_particular_to_this_library(pkg):
    """The checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table (that it is linked
    against the product library only, not against libslamhip_fej.so, among them)."""
    L = pkg._lib
    assert len(NAMES) == 3
    assert NAMES == set(L.wide_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("update_joint!", "joint_nis", "wide_limits"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip_fej.h"' in text
    assert L.SLAM_WIDE_MAXOBS == 64 == W.MAXOBS and "#define SLAM_WIDE_MAXOBS 64" in text
    lim = (ctypes.c_int32 * 1)()
    assert L.wide_lib().slam_ekf_wide_limits(lim) == L.SLAM_OK and list(lim) == [64]      # (touches no device)
    assert ABI.exported(L.FEJ_LIB_PATH) == FEJ_NAMES and len(FEJ_NAMES) == 11      # moving the object's layout added no export there
    for word in ("update_joint", "joint_nis"):
        assert callable(getattr(pkg.FirstEstimates, word)), word
    assert callable(pkg.EKFSlamState.update_joint_at_estimates)
    assert inspect.signature(pkg.FirstEstimates.observe).parameters["joint"].default is False
    params = inspect.signature(pkg.sim.sim).parameters
    assert params["fej"].default is False and params["fej_joint"].default is False
    # the library reads the object's layout from one internal header that both sources include
    csrc = os.path.join(os.path.dirname(L.LIB_PATH), "csrc")
    for src in ("ekf_fej.hip", "ekf_wide.hip"):
        with open(os.path.join(csrc, src)) as f:
            text = f.read()
        assert '#include "fej_object.h"' in text and "struct slam_ekf_fej {" not in text, src


def test_sim_refuses_fej_joint_without_fej(pkg):
    """Decided before the filter is touched: the filter here is none."""
    wp = np.array([[0.0, 10.0], [0.0, 0.0]])
    with pytest.raises(ValueError, match="fej_joint needs fej"):
        pkg.sim.sim(None, wp, np.zeros((2, 0)), seed=0, fej_joint=True)


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before a handle or an object is read: both here are none."""
    L = pkg._lib
    lib = L.wide_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    z = (ctypes.c_double * 130)(*([5.0, 0.1] * 65))
    ids = (ctypes.c_int32 * 65)(*range(1, 66))
    R = (ctypes.c_double * 4)(0.01, 0.0, 0.0, 0.0003)
    out = (ctypes.c_double * 4)(*([7.0] * 4))
    nan, inf = float("nan"), float("inf")
    for fn in (lib.slam_ekf_wide_update, lib.slam_ekf_wide_nis):
        assert fn(None, None, z, ids, 2, R, out) == BAD and "null handle" in L.last_error()
        for args in ((None, ids, 2, R, out), (z, None, 2, R, out), (z, ids, 2, None, out), (z, ids, 2, R, None)):
            assert fn(fake, None, *args) == BAD and "null argument" in L.last_error()
        for m in (0, -1, 65):
            assert fn(fake, None, z, ids, m, R, out) == BAD and "SLAM_WIDE_MAXOBS" in L.last_error()
        for bad in (nan, inf):
            zb = (ctypes.c_double * 130)(*([5.0, 0.1] * 40 + [6.0, bad] + [0.0] * 48))
            assert fn(fake, None, zb, ids, 64, R, out) == BAD and "zf" in L.last_error()
        for Rb in ((0.01, 0.0, 0.0, nan), (0.01, 1e-4, 2e-4, 0.0003), (0.01, 0.0, 0.0, -0.0003), (0.0, 0.0, 0.0, 0.0003),
                   (0.01, 0.02, 0.02, 0.0003)):
            assert fn(fake, None, z, ids, 2, (ctypes.c_double * 4)(*Rb), out) == BAD and "R is" in L.last_error(), Rb
    assert list(out) == [7.0] * 4
    assert lib.slam_ekf_wide_limits(None) == BAD
