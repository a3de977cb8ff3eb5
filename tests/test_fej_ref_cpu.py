"""First-estimates Jacobian predict, update and augment (libslamhip_fej.so, include/ext/slamhip_fej.h), the parts that need no GPU:
tests/fej_ref.py against the oracle (its twin, with the linearisation points re-set before every call, IS the oracle's filter);
the observability argument the rule rests on -- H N = 0 at every update, N' inv(P) N constant without process noise, neither of
which the standard filter keeps --; remap / reset / transform on the reference; and what is particular to this library's surface
(the checks every side library shares are made from its row of the table by tests/test_companions_cpu.py).

The bars of the first three tests are the ones the rule was prototyped against: 1e-12 where fp64 rounding alone separates two
quantities (measured 2e-13, 7e-15), 1e-9 for the drift of N' inv(P) N, which passes through inv(P) with cond(P) ~ 3e7 (measured
4e-14), and 0.1 / 1 for the standard filter's violations, which are of order one (measured 0.72 .. 1.5 and 2.6 .. 12)."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import abi_surface as ABI
from tests import fej_ref as F

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_fej.h")
NAMES = {"slam_ekf_fej_" + w for w in ("create", "destroy", "predict", "update", "augment", "reset", "remap", "transform", "get", "set",
                                       "limits")}
SEEDS = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def noisy():
    """drive(seed, 240, Q_DRIVE) through the rule and through the twin, once for the tests that share it."""
    runs = {}
    for seed in SEEDS:
        ops = F.drive(seed, 240, F.Q_DRIVE)
        runs[seed] = (ops, F.run(ops, "rule"), F.run(ops, "twin"))
    return runs


# ---- 1. the twin is the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_with_the_points_reset_before_every_call_the_rule_is_the_oracles_filter(noisy, seed):
    ops, _rule, twin = noisy[seed]
    assert sum(op[0] == "update" for op in ops) >= 20 and any(op[0] == "augment" for op in ops)
    x, P = F.X0_DRIVE.copy(), F.P0_DRIVE.copy()
    worst = 0.0
    for op, rec in zip(ops, twin[1:]):
        if op[0] == "predict":
            x, P = O.predict(x.copy(), P.copy(), *op[1:])
        elif op[0] == "update":
            x, P = O.update(x, P, op[1], F.R_DRIVE, op[2])
        else:
            x, P = O.add_features(x, P, op[1], F.R_DRIVE)
        worst = max(worst, np.max(np.abs(x - rec[1])) / np.max(np.abs(x)), np.max(np.abs(P - rec[2])) / np.max(np.abs(P)))
    print(f"fej twin against the oracle, seed {seed}: {worst:.3e} over {len(ops)} calls")
    assert worst <= 1e-12


# ---- 2. H N = 0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_every_update_is_blind_to_the_three_directions_the_standard_filter_is_not(noisy, seed):
    """N is carried forward by the Jacobians the filter itself used.  Under the rule it stays N(lin, first) -- Gv of predict maps the
    old vehicle rows to the new ones, Gv of augment produces the new landmark's rows -- and H N vanishes at every update."""
    _ops, rule, twin = noisy[seed]
    for rec in rule:
        assert np.max(np.abs(rec[5] - F.N_matrix(rec[3], rec[4]))) <= 1e-12 * np.max(np.abs(rec[5]))
    ratio = {name: max(np.max(np.abs(rec[6] @ rec[5])) / np.max(np.abs(rec[6])) for rec in hist if rec[6] is not None)
             for name, hist in (("rule", rule), ("twin", twin))}
    print(f"fej max|H N| / max|H|, seed {seed}: rule {ratio['rule']:.3e}, standard {ratio['twin']:.3e}")
    assert ratio["rule"] <= 1e-12
    assert ratio["twin"] >= 0.1


# ---- 3. no information along them ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_without_process_noise_the_information_along_the_directions_is_constant(seed):
    ops = F.drive(seed, 96, np.zeros((2, 2)))
    got = {}
    for mode in ("rule", "twin"):
        hist = F.run(ops, mode)
        M0 = F.information(hist[0][5], hist[0][2])
        got[mode] = F.drift(F.information(hist[-1][5], hist[-1][2]), M0)
    print(f"fej drift of N' inv(P) N over 96 steps, seed {seed}: rule {got['rule']:.3e}, standard {got['twin']:.3e}")
    assert got["rule"] <= 1e-9
    assert got["twin"] >= 1.0


# ---- 4. remap, reset, transform -----------------------------------------------------------------------------------------------------
def _mid_run(seed=0):
    hist = F.run(F.drive(seed, 96, F.Q_DRIVE))
    _, x, P, lin, first, _, _ = hist[-1]
    return x, P, lin, first


def test_a_permutation_and_its_inverse_restore_the_first_estimates_and_zero_takes_the_mean():
    x, _P, _lin, first = _mid_run()
    N = len(first) // 2
    assert N == 10
    perm = np.random.default_rng(5).permutation(N) + 1
    xp = x[np.concatenate([np.arange(3)] + [[F.f(j), F.f(j) + 1] for j in perm]).astype(int)]
    moved = F.remap(xp, first, perm)
    assert np.array_equal(moved.reshape(-1, 2), first.reshape(-1, 2)[perm - 1])
    inv = np.argsort(perm) + 1
    assert np.array_equal(F.remap(x, moved, inv), first)
    # a removal: the survivors keep theirs; 0 takes the current stored mean
    keep = np.array([1, 2, 4, 5, 6, 8, 9, 10])
    xs = x[np.concatenate([np.arange(3)] + [[F.f(j), F.f(j) + 1] for j in keep]).astype(int)]
    ids = keep.copy()
    ids[3] = 0
    got = F.remap(xs, first, ids).reshape(-1, 2)
    assert np.array_equal(got[[0, 1, 2, 4, 5, 6, 7]], first.reshape(-1, 2)[keep[[0, 1, 2, 4, 5, 6, 7]] - 1])
    assert np.array_equal(got[3], xs[3 + 2 * 3:5 + 2 * 3]) and not np.array_equal(got[3], first.reshape(-1, 2)[keep[3] - 1])


def test_reset_takes_the_listed_means_and_the_pose_on_request():
    x, _P, lin, first = _mid_run()
    l2, f2 = F.reset(x, lin, first, ids=[3, 7])
    assert np.array_equal(l2, lin)
    want = first.copy()
    want[4:6] = x[F.f(3):F.f(3) + 2]
    want[12:14] = x[F.f(7):F.f(7) + 2]
    assert np.array_equal(f2, want) and not np.array_equal(f2, first)
    l3, f3 = F.reset(x, lin, first, pose=True)
    assert np.array_equal(l3, x[0:3]) and np.array_equal(f3, x[3:])
    lc, fc = F.create(x)
    assert np.array_equal(lc, l3) and np.array_equal(fc, f3)


@pytest.mark.parametrize("frame", [(3.0, -7.5, 0.9), (0.0, 0.0, -2.5), (120.0, 40.0, 3.0)])
def test_an_update_commutes_with_a_rigid_frame_change(frame):
    x, P, lin, first = _mid_run(1)
    ids = np.array([2, 9, 4])
    rng = np.random.default_rng(3)
    z = O.obs_blocks(x, ids)[0].T + rng.normal(0, [0.1, math.pi / 180], (3, 2)).T
    xa, Pa, outa, _ = F.update(x, P, lin, first, z, F.R_DRIVE, ids)
    xa, Pa = F.transform_state(xa, Pa, *frame)
    xt, Pt = F.transform_state(x, P, *frame)
    lt, ft = F.transform(lin, first, *frame)
    # the sensor's reading does not depend on the frame, but the branch of the predicted bearing does (atan2 and the wrapped heading
    # each move by a multiple of 2 pi): the reading is reported on the new frame's branch, the ONE wrap of the rule then suffices
    zt = z.copy()
    zt[1] += np.round((O.obs_blocks(xt, ids)[0][:, 1] - O.obs_blocks(x, ids)[0][:, 1]) / (2 * math.pi)) * 2 * math.pi
    xb, Pb, outb, _ = F.update(xt, Pt, lt, ft, zt, F.R_DRIVE, ids)
    ex = np.max(np.abs(xa - xb)) / np.max(np.abs(xa))
    eP = np.max(np.abs(Pa - Pb)) / np.max(np.abs(Pa))
    print(f"fej update / frame change {frame}: x {ex:.3e} P {eP:.3e} nis {outa[0]:.6f} / {outb[0]:.6f}")
    assert ex <= 1e-10 and eP <= 1e-10
    assert abs(outa[0] - outb[0]) <= 1e-10 * outa[0] and abs(outa[1] - outb[1]) <= 1e-10 * abs(outa[1])


def test_a_failing_pivot_and_coinciding_points_change_nothing():
    x, P, lin, first = _mid_run()
    ids = np.array([1, 5])
    z = O.obs_blocks(x, ids)[0].T
    Pn = P.copy()
    Pn[F.f(1), F.f(1)] = Pn[F.f(1) + 1, F.f(1) + 1] = -10.0
    xr, Pr, out, _ = F.update(x, Pn, lin, first, z, F.R_DRIVE, ids)
    assert out[3] == 0 and out[2] < 0 and out[0] == 0 and out[1] == 0
    assert np.array_equal(xr, x) and np.array_equal(Pr, Pn)
    same = first.copy()
    same[8:10] = lin[0:2]                                                 # landmark 5's first estimate IS the linearisation pose
    xr, Pr, out, _ = F.update(x, P, lin, same, z, F.R_DRIVE, ids)
    assert out[3] == 2 and not math.isfinite(out[2])
    assert np.array_equal(xr, x) and np.array_equal(Pr, P)


def test_batches_keep_the_jacobians_and_move_the_residuals():
    x, P, lin, first = _mid_run(2)
    ids = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 3])
    z = O.obs_blocks(x, ids)[0].T + np.random.default_rng(8).normal(0, [0.1, math.pi / 180], (11, 2)).T
    xb, Pb, outs = F.update_batches(x, P, lin, first, z, F.R_DRIVE, ids)
    x1, P1, o1, _ = F.update(x, P, lin, first, z[:, :8], F.R_DRIVE, ids[:8])
    x2, P2, o2, _ = F.update(x1, P1, lin, first, z[:, 8:], F.R_DRIVE, ids[8:])
    assert len(outs) == 2 and np.array_equal(outs[0], o1) and np.array_equal(outs[1], o2)
    assert np.array_equal(xb, x2) and np.array_equal(Pb, P2)


# ---- 5. the surface -----------------------------------------------------------------------------------------------------------------
def test_what_is_particular_to_this_library(pkg):
    """The checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table."""
    L = pkg._lib
    assert len(NAMES) == 11
    assert NAMES == set(L.fej_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("FirstEstimates", "fej", "remap!", "reset!"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text
    assert L.SLAM_FEJ_MAXOBS == 8 == F.MAXOBS == L.SLAM_ITERATED_MAXOBS and "#define SLAM_FEJ_MAXOBS 8" in text
    lim = (ctypes.c_int32 * 1)()
    assert L.fej_lib().slam_ekf_fej_limits(lim) == L.SLAM_OK and list(lim) == [8]      # (touches no device)
    assert callable(pkg.EKFSlamState.fej) and pkg.FirstEstimates is pkg.ekf.FirstEstimates
    for word in ("predict", "update", "add_features", "observe", "reset", "remap", "transform", "get", "set", "close"):
        assert callable(getattr(pkg.FirstEstimates, word)), word
    assert inspect.signature(pkg.sim.sim).parameters["fej"].default is False


def test_sim_refuses_fej_with_the_modes_it_does_not_cover(pkg):
    """Decided before the filter is touched: the filter here is none."""
    wp = np.array([[0.0, 10.0], [0.0, 0.0]])
    for kw in (dict(submap_steps=3), dict(local_radius=40.0), dict(iterated=3), dict(prune_after=2), dict(merge_gate=4.0)):
        with pytest.raises(ValueError, match="fej is not available"):
            pkg.sim.sim(None, wp, np.zeros((2, 0)), seed=0, fej=True, **kw)


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before an object is read: the object here is none."""
    L = pkg._lib
    lib = L.fej_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    z = (ctypes.c_double * 16)(*([5.0, 0.1] * 8))
    ids = (ctypes.c_int32 * 8)(*range(1, 9))
    R = (ctypes.c_double * 4)(0.01, 0.0, 0.0, 0.0003)
    out = (ctypes.c_double * 4)(*([7.0] * 4))
    nan, inf = float("nan"), float("inf")
    # update
    assert lib.slam_ekf_fej_update(None, z, ids, 2, R, out) == BAD and "null handle" in L.last_error()
    for args in ((None, ids, 2, R, out), (z, None, 2, R, out), (z, ids, 2, None, out), (z, ids, 2, R, None)):
        assert lib.slam_ekf_fej_update(fake, *args) == BAD and "null argument" in L.last_error()
    for m in (0, -1, 9):
        assert lib.slam_ekf_fej_update(fake, z, ids, m, R, out) == BAD and "SLAM_FEJ_MAXOBS" in L.last_error()
    for bad in (nan, inf):
        zb = (ctypes.c_double * 16)(*([5.0, 0.1, 6.0, bad] + [0.0] * 12))
        assert lib.slam_ekf_fej_update(fake, zb, ids, 2, R, out) == BAD and "zf" in L.last_error()
    bad_R = ((0.01, 0.0, 0.0, nan), (0.01, 1e-4, 2e-4, 0.0003), (0.01, 0.0, 0.0, -0.0003), (0.0, 0.0, 0.0, 0.0003), (0.01, 0.02, 0.02, 0.0003))
    for Rb in bad_R:
        assert lib.slam_ekf_fej_update(fake, z, ids, 2, (ctypes.c_double * 4)(*Rb), out) == BAD and "R is" in L.last_error(), Rb
        assert lib.slam_ekf_fej_augment(fake, z, 2, (ctypes.c_double * 4)(*Rb)) == BAD and "R is" in L.last_error(), Rb
    assert list(out) == [7.0] * 4
    # predict
    Q = (ctypes.c_double * 4)(0.25, 0.0, 0.0, 0.003)
    assert lib.slam_ekf_fej_predict(None, 1.0, 0.1, 4.0, Q, 0.025) == BAD
    assert lib.slam_ekf_fej_predict(fake, 1.0, 0.1, 4.0, None, 0.025) == BAD
    for args in ((nan, 0.1, 4.0, Q, 0.025), (1.0, inf, 4.0, Q, 0.025), (1.0, 0.1, nan, Q, 0.025), (1.0, 0.1, 4.0, Q, -inf),
                 (1.0, 0.1, 4.0, (ctypes.c_double * 4)(0.25, 0.0, nan, 0.003), 0.025)):
        assert lib.slam_ekf_fej_predict(fake, *args) == BAD and "not finite" in L.last_error()
    # augment, reset, remap, transform, get, set, create, limits
    assert lib.slam_ekf_fej_augment(None, z, 2, R) == BAD
    assert lib.slam_ekf_fej_augment(fake, z, -1, R) == BAD and "cnt" in L.last_error()
    assert lib.slam_ekf_fej_augment(fake, None, 2, R) == BAD and lib.slam_ekf_fej_augment(fake, z, 2, None) == BAD
    assert lib.slam_ekf_fej_augment(fake, (ctypes.c_double * 4)(5.0, nan, 1.0, 0.0), 2, R) == BAD and "zn" in L.last_error()
    assert lib.slam_ekf_fej_reset(None, ids, 2, 0) == BAD
    assert lib.slam_ekf_fej_reset(fake, ids, -2, 0) == BAD and lib.slam_ekf_fej_reset(fake, None, 2, 0) == BAD
    assert lib.slam_ekf_fej_remap(None, ids, 2) == BAD
    assert lib.slam_ekf_fej_transform(None, 1.0, 2.0, 0.3) == BAD
    for args in ((nan, 2.0, 0.3), (1.0, inf, 0.3), (1.0, 2.0, nan)):
        assert lib.slam_ekf_fej_transform(fake, *args) == BAD and "finite" in L.last_error()
    assert lib.slam_ekf_fej_get(None, None, None, None) == BAD and lib.slam_ekf_fej_set(None, None, None) == BAD
    made = ctypes.c_void_p(0x7)
    assert lib.slam_ekf_fej_create(None, fake) == BAD
    assert lib.slam_ekf_fej_create(ctypes.byref(made), None) == BAD and not made.value      # nothing is handed out
    assert lib.slam_ekf_fej_destroy(None) == L.SLAM_OK
    assert lib.slam_ekf_fej_limits(None) == BAD
