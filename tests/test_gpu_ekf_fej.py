"""libslamhip_fej.so on the device, both dtypes: the slam_ekf_fej_* calls (include/ext/slamhip_fej.h) against tests/fej_ref.py,
against slam_ekf_update_iterated(max_iter = 1) and against the oracle.

Every cell is re-anchored: the reference repeats the call from the device's own state and linearisation points, downloaded right
before it.  x and P are held to the project's per-call bars (tests/test_gpu_ekf.py: TOL, relerr, relerr_cov), lin and first to the
bar of x, the packed diagonal blocks bit for bit (check_side), the outputs to OUT_BAR = 1e-9 relative (the bar of the linear and
iterated tests).  A FRESH object's update and slam_ekf_update_iterated(max_iter = 1) run the same shared front half
(csrc/small_front.h, csrc/obs_panel.h) on the same numbers: x, P and the three outputs are compared bit for bit (test 2).
Shapes: the scenes of tests/iterated_ref.py -- N = 1, 70, 200 landmarks in handles of 256, i.e. n = 5, 143, 403 over tile edges 128
(fp32) / 64 (fp64): one and several tile rows, n no multiple of the edge, several workgroups of the strip, panel and augment
kernels; m = 1, 3, 8 observations; the landmark that straddles a tile edge (63 / 31), the last landmark, a repeated id; new
landmarks that land on and behind a tile edge.  lin and first are DISPLACED from the estimates (set through slam_ekf_fej_set), so
that a Jacobian evaluated at the estimates instead would miss the bars by orders of magnitude.

The chained run (test 3) measures what the library is for: the drift of N' inv(P) N, the information along the three unobservable
directions, over drive(seed = 0, steps = 96, Q = 0).  It is rounding only, about cond(P) u calls = 5e7 * 1e-16 * 100 = 5e-7, while
the standard filter's is of order one to ten: the bar 1e-3 lies three orders from either.  fp32 is not asserted there:
cond(P) u > 1.  The measured values are recorded in profiles/fej_bounds.txt."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import fej_ref as F
from tests import iterated_ref as IR
from tests.test_gpu_ekf import DTYPES, TOL, check_side, relerr, relerr_cov, rounded

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-9
SCENES = ["N1-m1", "N70-m3-straddler", "N70-m8", "N200-m8-last", "N200-m3-duplicate"]
Q2 = np.array([[0.25, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
RND = {"f64": F.ident, "f32": lambda a: float(np.float32(a))}


def _bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def snapshot(st, fe):
    lin, first, count = fe.get()
    return st.download("x"), st.download("cov"), st.landmark_blocks(), lin, first, count


def unchanged(st, fe, snap):
    now = snapshot(st, fe)
    return all(_bits_eq(a, b) for a, b in zip(now[:5], snap[:5])) and now[5] == snap[5]


def displaced(x, seed):
    """The linearisation points of the tests: the estimates moved by (0.3, -0.2, 0.05) and N(0, 0.2^2) per landmark coordinate."""
    rng = np.random.default_rng(seed)
    return x[0:3] + [0.3, -0.2, 0.05], x[3:] + rng.normal(0.0, 0.2, len(x) - 3)


def upload(pkg, name, dtype, displace=True):
    """The scene on the device with an object whose points are displaced (or fresh); returns (st, fe, xb, Pb, z, ids)."""
    x, P, z, ids = IR.scene(name, dtype)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
    fe = st.fej()
    xb, Pb = rounded(st)
    assert np.array_equal(xb, x) and np.array_equal(Pb, P)
    if displace:
        fe.set(*displaced(xb, 11))
    return st, fe, xb, Pb, z, ids


def held(st, fe, xo, Po, lo, fo, prior, dtype, what, calls=1, side=True):
    xg, Pg = st.download()
    lg, fg, count = fe.get()
    assert count == st.N == len(fo) // 2, what
    if side:
        check_side(st, Pg, what)
    assert _bits_eq(Pg, Pg.T), f"{what}: P is not symmetric"
    ex, eP = relerr(xg, xo), relerr_cov(Pg, Po, np.diag(prior))
    el, ef = relerr(lg, lo), (relerr(fg, fo) if len(fo) else 0.0)
    print(f"fej {what} {dtype}: x {ex:.3e} P {eP:.3e} lin {el:.3e} first {ef:.3e}")
    assert ex <= calls * TOL[dtype]["x"], f"{what}: x rel err {ex:.3e}"
    assert eP <= calls * TOL[dtype]["P"], f"{what}: P rel err {eP:.3e}"
    assert el <= calls * TOL[dtype]["x"] and ef <= calls * TOL[dtype]["x"], f"{what}: lin {el:.3e} first {ef:.3e}"
    return xg.astype(np.float64), np.array(Pg, dtype=np.float64), lg, fg


def new_observations(rng, k):
    return np.stack([rng.uniform(5.0, 30.0, k), rng.uniform(-math.pi, math.pi, k)])


# ---- 1. predict, update and augment against the reference, the points displaced ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SCENES)
def test_predict_update_and_augment_against_the_reference(pkg, dtype, name):
    st, fe, x, P, z, ids = upload(pkg, name, dtype)
    rnd = RND[dtype]
    try:
        lin, first, _ = fe.get()
        assert np.array_equal(lin, displaced(x, 11)[0]) and np.array_equal(first, displaced(x, 11)[1])      # set / get are exact
        fe.predict(7.5, 0.1, 4.0, Q2, 0.025)
        xo, Po, lo, fo, _ = F.predict(x, P, lin, first, 7.5, 0.1, 4.0, Q2, 0.025, rnd=rnd)
        x, P, lin, first = held(st, fe, xo, Po, lo, fo, P, dtype, f"{name} predict")
        assert np.array_equal(lin, x[0:3])                                # lin IS the stored pose
        out = fe.update(z, IR.R_HARD, ids)
        xo, Po, ref, _ = F.update(x, P, lin, first, z, IR.R_HARD, ids)
        assert out.shape == (1, 4) and out[0, 3] == -1 == ref[3]
        err = np.abs(out[0, :3] - ref[:3]) / np.abs(ref[:3])
        print(f"fej out {name} {dtype}: rel {err}")
        assert np.all(err <= OUT_BAR), (out, ref)
        x, P, lin, first = held(st, fe, xo, Po, lin, first, P, dtype, f"{name} update")
        rng = np.random.default_rng(21)
        for k in (1, 3, 5):
            zn = new_observations(rng, k)
            fe.add_features(zn, IR.R_HARD)
            xo, Po, lo, fo, _ = F.add_features(x, P, lin, first, zn, IR.R_HARD, rnd=rnd)
            x, P, lin, first = held(st, fe, xo, Po, lo, fo, P, dtype, f"{name} augment {k}")
            assert np.array_equal(first[-2 * k:], x[-2 * k:])             # a new landmark's first estimate IS its stored mean
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("back,k", [(0, 1), (2, 3)])
def test_augment_across_a_tile_edge(pkg, dtype, back, k):
    """N = 63 -> 64 (fp32) and 31 -> 32 (fp64): the new landmark is the first one wholly behind the tile edge; from two landmarks
    earlier, three new ones: before, on (its pair straddles) and behind the edge."""
    N0 = IR.STRADDLER[dtype] - back
    x, P = IR.base_state(N0, dtype)
    t = IR.NP_DTYPE[dtype]
    st = pkg.EKFSlamState(x.astype(t), P.astype(t), dtype=dtype, max_landmarks=IR.CAP)
    try:
        fe = st.fej()
        x, P = rounded(st)
        fe.set(*displaced(x, 12))
        lin, first, _ = fe.get()
        zn = new_observations(np.random.default_rng(22), k)
        fe.add_features(zn, IR.R_HARD)
        assert st.N == N0 + k
        xo, Po, lo, fo, _ = F.add_features(x, P, lin, first, zn, IR.R_HARD, rnd=RND[dtype])
        x, P, lin, first = held(st, fe, xo, Po, lo, fo, P, dtype, f"augment {N0} -> {N0 + k}")
        ids = np.arange(N0 - 1, N0 + k + 1)                               # an update over the old and the new ones, across the edge
        z = O.obs_blocks(x, ids)[0].T + np.random.default_rng(23).normal(0, [0.05, 0.005], (len(ids), 2)).T
        fe.update(z, IR.R_HARD, ids)
        xo, Po, _, _ = F.update(x, P, lin, first, z, IR.R_HARD, ids)
        held(st, fe, xo, Po, lin, first, P, dtype, f"update after augment {N0} -> {N0 + k}")
    finally:
        st.close()


# ---- 2. a fresh object is the standard filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SCENES)
def test_a_fresh_object_gives_the_oracles_update_and_the_iterated_updates_first_iteration(pkg, dtype, name):
    st, fe, xb, Pb, z, ids = upload(pkg, name, dtype, displace=False)
    b = st.copy()
    try:
        lin, first, count = fe.get()
        assert count == st.N and np.array_equal(lin, xb[0:3]) and np.array_equal(first, xb[3:])
        out = fe.update(z, IR.R_HARD, ids)[0]
        res = b.update_iterated(z, IR.R_HARD, ids, max_iter=1, tol=0.0)
        xo, Po = O.update_sparse(xb, Pb, z, IR.R_HARD, ids)
        held(st, fe, xo, Po, lin, first, Pb, dtype, f"{name} fresh against the oracle")
        # with lin = x and first = x the two front halves run the same shared statements on the same numbers (the iterated kernel's
        # v = r - H 0 is exact), and the panel kernel and the down-date are the same: bit for bit
        (xg, Pg), (xi, Pi) = st.download(), b.download()
        print(f"fej fresh {name} {dtype}: x differs at {np.flatnonzero(xg != xi)}, P in {np.count_nonzero(Pg != Pi)} entries; "
              f"out {out[:3]} against {res.out[3:6]}")
        assert _bits_eq(xg, xi), f"{name}: x differs from the iterated update's first iteration"
        assert _bits_eq(Pg, Pi), f"{name}: P differs from the iterated update's first iteration"
        assert _bits_eq(out[:3], res.out[3:6]) and out[3] == -1 == res.out[6], (out, res.out)
    finally:
        st.close()
        b.close()


# ---- 3. the chained run: no information along the unobservable directions ------------------------------------------------------------
def test_the_chained_run_gains_no_information_along_the_three_directions_the_standard_filter_does(pkg):
    ops = F.drive(0, 96, np.zeros((2, 2)))
    hist = F.run(ops)
    st = pkg.EKFSlamState(F.X0_DRIVE, F.P0_DRIVE, dtype="f64", max_landmarks=64)
    std = st.copy()
    try:
        fe = st.fej()
        lin, first, _ = fe.get()
        M0 = F.information(F.N_matrix(lin, first), F.P0_DRIVE)
        Ns = F.N_matrix(lin, first)                                       # the standard filter's directions, carried on the host
        for op in ops:
            if op[0] == "predict":
                fe.predict(*op[1:])
                before = std.pose()
                std.predict(*op[1:])
                Gv = np.eye(3)
                Gv[0:2, 2] = F.J2 @ (std.pose()[0:2] - before[0:2])
                Ns = F.carry_predict(Ns, Gv)
            elif op[0] == "update":
                fe.update(op[1], F.R_DRIVE, op[2])
                std.update(op[1], F.R_DRIVE, op[2])
            else:
                fe.add_features(op[1], F.R_DRIVE)
                std.add_features(op[1], F.R_DRIVE)
                xs = std.download("x").astype(np.float64)
                k = op[1].shape[1]
                Ns = F.carry_augment(Ns, [np.hstack([np.eye(2), (F.J2 @ (xs[len(xs) - 2 * (k - a):][:2] - xs[0:2])).reshape(2, 1)])
                                          for a in range(k)])
        _, xo, Po, lo, fo, _, _ = hist[-1]
        xg, Pg, lg, fg = held(st, fe, xo, Po, lo, fo, Po, "f64", f"chained run of {len(ops)} calls", calls=len(ops))
        d_fej = F.drift(F.information(F.N_matrix(lg, fg), Pg), M0)
        xs, Ps = rounded(std)
        d_std = F.drift(F.information(Ns, Ps), M0)
        print(f"fej chained run: drift of N' inv(P) N over {len(ops)} calls: {d_fej:.3e} (FEJ), {d_std:.3e} (standard); cond(P) "
              f"{np.linalg.cond(Pg):.2e}")
        assert d_fej <= 1e-3
        assert d_std >= 1.0
        assert st.is_positive_definite()[0]
    finally:
        st.close()
        std.close()


# ---- 4. S not positive definite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_indefinite_s_is_refused_and_leaves_everything_bit_identical(pkg, dtype):
    """Landmark 12 carries a NEGATIVE diagonal block: the second observation's first pivot is -10 + (what the vehicle and R add, below
    1), minus two squares -- negative in any evaluation order.  Then a first estimate that coincides with lin: the Jacobian, and with
    it the pivot, is not finite."""
    x, P, z, ids = IR.scene("N70-m3-straddler", dtype)
    assert ids[1] == 70 and ids[2] == 12
    ids = np.array([ids[0], 12, 70])
    z = z[:, [0, 2, 1]]
    f = IR.f(12)
    P[f, f] = P[f + 1, f + 1] = -10.0
    P[f, f + 1] = P[f + 1, f] = 0.0
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
    try:
        fe = st.fej()
        fe.set(*displaced(x, 13))
        good = np.array([ids[0], 70])
        fe.update(z[:, [0, 2]], IR.R_HARD, good)                          # a valid call first: its panel is what a stale W1 would be
        xb, Pb = rounded(st)
        lin, first, _ = fe.get()
        snap = snapshot(st, fe)
        L = pkg._lib
        zp = np.ascontiguousarray(z.T)
        ii = np.ascontiguousarray(ids, dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        ref = F.update(xb, Pb, lin, first, z, IR.R_HARD, ids)[2]
        assert ref[3] == 2 and ref[2] < 0
        out = np.full(4, 7.0)
        rc = L.fej_lib().slam_ekf_fej_update(fe._f, p(zp), p(ii, C.c_int32), 3, p(rr), p(out))
        assert rc == L.SLAM_E_NOTPD and "not positive definite" in L.last_error()
        assert out[3] == 2 and out[0] == 0 and out[1] == 0 and abs(out[2] - ref[2]) <= 1e-9 * abs(ref[2]), out
        assert unchanged(st, fe, snap)
        with pytest.raises(pkg.NotPositiveDefinite):
            fe.update(z, IR.R_HARD, ids)
        assert unchanged(st, fe, snap)
        # lin coincides with the first estimate of landmark 70
        same = first.copy()
        same[2 * 69:2 * 70] = lin[0:2]
        fe.set(None, same)
        snap2 = snapshot(st, fe)
        out = np.full(4, 7.0)
        rc = L.fej_lib().slam_ekf_fej_update(fe._f, p(np.ascontiguousarray(zp[[0, 2]])), p(np.ascontiguousarray(good, dtype=np.int32), C.c_int32), 2,
                                             p(rr), p(out))
        assert rc == L.SLAM_E_NOTPD and out[3] == 2 and not math.isfinite(out[2]), out
        assert unchanged(st, fe, snap2)
        # the next valid call on the object works
        fe.set(None, first)
        assert unchanged(st, fe, snap)
        fe.update(z[:, [0, 2]], IR.R_HARD, good)
        xo, Po, _, _ = F.update(xb, Pb, lin, first, z[:, [0, 2]], IR.R_HARD, good)
        held(st, fe, xo, Po, lin, first, Pb, dtype, "after the refusals")
    finally:
        st.close()


# ---- 5. bad arguments, and a map that changed outside the object --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_and_a_renumbered_map_are_refused_until_remap(pkg, dtype):
    st, fe, xb, Pb, z, ids = upload(pkg, "N70-m3-straddler", dtype)
    try:
        snap = snapshot(st, fe)
        L = pkg._lib
        lib = L.fej_lib()
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        zp = np.ascontiguousarray(np.tile(z.T, (3, 1)))                    # 9 pairs
        ii = np.ascontiguousarray(np.tile(ids, 3), dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        qq = np.ascontiguousarray(Q2.T).reshape(4)
        out = np.full(4, 7.0)
        nan, inf = float("nan"), float("inf")
        keep = []

        def z_with(v):
            keep.append(zp.copy())
            keep[-1][1, 1] = v
            return p(keep[-1])

        def ids_with(v):
            keep.append(ii.copy())
            keep[-1][2] = v
            return p(keep[-1], C.c_int32)

        def arr(vals, t=np.float64):
            keep.append(np.array(vals, dtype=t))
            return p(keep[-1], C.c_double if t is np.float64 else C.c_int32)

        f = fe._f
        up, ag, pr, rs, rm, tr = (lib.slam_ekf_fej_update, lib.slam_ekf_fej_augment, lib.slam_ekf_fej_predict, lib.slam_ekf_fej_reset,
                                  lib.slam_ekf_fej_remap, lib.slam_ekf_fej_transform)
        cases = [("update null z", up, (f, None, p(ii, C.c_int32), 3, p(rr), p(out))),
                 ("update null ids", up, (f, p(zp), None, 3, p(rr), p(out))),
                 ("update null R", up, (f, p(zp), p(ii, C.c_int32), 3, None, p(out))),
                 ("update null out", up, (f, p(zp), p(ii, C.c_int32), 3, p(rr), None))]
        cases += [(f"update m = {m}", up, (f, p(zp), p(ii, C.c_int32), m, p(rr), p(out))) for m in (0, -1, 9)]
        cases += [(f"update id {j}", up, (f, p(zp), ids_with(j), 3, p(rr), p(out))) for j in (0, 71, -4)]
        cases += [(f"update z {v}", up, (f, z_with(v), p(ii, C.c_int32), 3, p(rr), p(out))) for v in (nan, inf, -inf)]
        for Rb in ((0.0025, 0.0, 0.0, nan), (inf, 0.0, 0.0, 1e-4), (0.0025, 1e-5, 2e-5, 1e-4), (0.0025, 0.0, 0.0, -1e-4),
                   (0.0, 0.0, 0.0, 1e-4), (0.0025, 0.001, 0.001, 1e-4)):
            cases.append((f"update R {Rb}", up, (f, p(zp), p(ii, C.c_int32), 3, arr(Rb), p(out))))
            cases.append((f"augment R {Rb}", ag, (f, p(zp), 2, arr(Rb))))
        cases += [("augment cnt", ag, (f, p(zp), -1, p(rr))), ("augment null z", ag, (f, None, 2, p(rr))),
                  ("augment z nan", ag, (f, z_with(nan), 2, p(rr)))]
        cases += [("predict null Q", pr, (f, 7.5, 0.1, 4.0, None, 0.025)), ("predict nan", pr, (f, nan, 0.1, 4.0, p(qq), 0.025)),
                  ("predict inf dt", pr, (f, 7.5, 0.1, 4.0, p(qq), inf)), ("predict Q nan", pr, (f, 7.5, 0.1, 4.0, arr((0.25, 0.0, 0.0, nan)), 0.025))]
        cases += [("reset cnt", rs, (f, p(ii, C.c_int32), -2, 0)), ("reset null", rs, (f, None, 2, 0)),
                  ("reset id 0", rs, (f, arr((1, 0), np.int32), 2, 0)), ("reset id 71", rs, (f, arr((71,), np.int32), 1, 1)),
                  ("reset too many", rs, (f, arr(np.ones(71), np.int32), 71, 0))]
        cases += [("remap cnt", rm, (f, p(ii, C.c_int32), 9)), ("remap null", rm, (f, None, 70)),
                  ("remap id 71", rm, (f, arr(np.full(70, 71), np.int32), 70)), ("remap id -1", rm, (f, arr(np.full(70, -1), np.int32), 70))]
        cases += [(f"transform {v}", tr, (f, 1.0, v, 0.3)) for v in (nan, inf)] + [("transform theta", tr, (f, 1.0, 2.0, nan))]
        for what, fn, args in cases:
            assert fn(*args) == L.SLAM_E_BADARG, what
            assert "bad argument" in L.last_error(), what
            assert unchanged(st, fe, snap), what
        assert np.all(out == 7.0)
        # capacity: decided before anything is enqueued
        many = np.ascontiguousarray(np.tile([10.0, 0.1], IR.CAP))
        assert ag(f, p(many), IR.CAP - 69, p(rr)) == L.SLAM_E_CAPACITY and unchanged(st, fe, snap)
        # the map renumbered outside the object
        new_index = st.remove_landmarks([5, 40])
        assert st.N == 68
        snap = snapshot(st, fe)
        assert snap[5] == 70
        for what, fn, args in (("predict", pr, (f, 7.5, 0.1, 4.0, p(qq), 0.025)), ("update", up, (f, p(zp), p(ii, C.c_int32), 3, p(rr), p(out))),
                               ("augment", ag, (f, p(zp), 2, p(rr))), ("transform", tr, (f, 1.0, 2.0, 0.3)),
                               ("reset", rs, (f, None, -1, 1))):
            assert fn(*args) == L.SLAM_E_BADARG and "the map changed outside the object" in L.last_error(), what
            assert unchanged(st, fe, snap), what
        lin, first_old, _ = fe.get()
        old_of_new = np.flatnonzero(new_index) + 1                       # the survivors keep their order
        assert np.array_equal(new_index[old_of_new - 1], np.arange(1, 69))
        old_of_new[9] = 0                                                 # and one of them starts over from its current mean
        fe.remap(old_of_new)
        xb, Pb = rounded(st)
        lin2, first, count = fe.get()
        assert count == 68 and np.array_equal(lin2, lin)
        assert np.array_equal(first, F.remap(xb, first_old, old_of_new)) and np.array_equal(first[18:20], xb[21:23])
        ids2 = new_index[ids - 1]
        assert np.all(ids2 > 0)
        fe.update(z, IR.R_HARD, ids2)
        xo, Po, _, _ = F.update(xb, Pb, lin, first, z, IR.R_HARD, ids2)
        held(st, fe, xo, Po, lin, first, Pb, dtype, "after remap")
        # reset: the listed first estimates and the pose are taken from the state
        x2, _ = rounded(st)
        fe.reset([3, 68], pose=True)
        lo, fo = F.reset(x2, lin, first, [3, 68], pose=True)
        lg, fg, _ = fe.get()
        assert np.array_equal(lg, lo) and np.array_equal(fg, fo)
        fe.reset()
        lg, fg, _ = fe.get()
        assert np.array_equal(lg, lo) and np.array_equal(fg, x2[3:])
    finally:
        st.close()


# ---- 6. the frame change -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", [(3.0, -7.5, 0.9), (-40.0, 12.0, -2.5)])
def test_transform_then_update_is_update_then_transform(pkg, dtype, frame):
    """Two chains of two calls each, compared on the device.  The scene is N70-m8: all eight observation slots, several tiles.  What
    the bar has to absorb beside the calls' own rounding is that one chain STORES the transformed state before the update and the
    other after it; with exact arithmetic between the roundings (tests/fej_ref.py, the stored values rounded to fp32) that alone is
    2e-7 for the N = 70 scenes and 1e-6 .. 2e-6 for the N = 200 ones, whose landmark variances are 60 times the vehicle's, so that
    their rounding leaks into the vehicle block at a third of the fp32 bar before any kernel has rounded anything.  Hence N = 70."""
    a, fa, xb, Pb, z, ids = upload(pkg, "N70-m8", dtype)
    b = a.copy()
    try:
        fb = b.fej()
        lin, first, _ = fa.get()
        fb.set(lin, first)
        a.transform(*frame)
        fa.transform(*frame)
        lt, ft = F.transform(lin, first, *frame)
        lg, fg, _ = fa.get()
        assert relerr(lg, lt) <= 1e-14 and relerr(fg, ft) <= 1e-14         # doubles, whatever the dtype
        xt, _ = rounded(a)
        zt = z.copy()                                                      # the reading on the new frame's branch (tests/test_fej_ref_cpu.py)
        zt[1] += np.round((O.obs_blocks(xt, ids)[0][:, 1] - O.obs_blocks(xb, ids)[0][:, 1]) / (2 * math.pi)) * 2 * math.pi
        oa = fa.update(zt, IR.R_HARD, ids)[0]
        ob = fb.update(z, IR.R_HARD, ids)[0]
        b.transform(*frame)
        xa, Pa = rounded(a)
        xg, Pg = rounded(b)
        _, Pt = F.transform_state(xb, Pb, *frame)
        ex, eP = relerr(xa, xg), relerr_cov(Pa, Pg, np.diag(Pt))
        print(f"fej frame {frame} {dtype}: x {ex:.3e} P {eP:.3e} nis {oa[0]:.6f} / {ob[0]:.6f}")
        assert ex <= TOL[dtype]["x"] and eP <= TOL[dtype]["P"]
    finally:
        a.close()
        b.close()


# ---- 7. more than eight observations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_eleven_observations_are_batches_of_eight_and_three(pkg, dtype):
    st, fe, xb, Pb, z, ids = upload(pkg, "N200-m11", dtype)
    try:
        assert len(ids) == 11
        lin, first, _ = fe.get()
        outs = fe.update(z, IR.R_HARD, ids)
        xo, Po, refs = F.update_batches(xb, Pb, lin, first, z, IR.R_HARD, ids)
        assert outs.shape == (2, 4) and len(refs) == 2 and np.all(outs[:, 3] == -1)
        err = np.abs(outs[0, :3] - refs[0][:3]) / np.abs(refs[0][:3])
        assert np.all(err <= OUT_BAR), (outs, refs)
        # the second batch starts from the DEVICE's state after the first (rounded to the dtype), the reference from its own
        held(st, fe, xo, Po, lin, first, Pb, dtype, "8 + 3")
    finally:
        st.close()


# ---- 8. the simulator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grow", [False, True])
def test_sim_with_first_estimates_completes(pkg, golden_dir, grow):
    """30 steps of the golden course through filt.fej(): it completes, the state is finite and its covariance positive definite; from
    a capacity of 4 with grow=True the object follows the state into the larger handles.  nees_every works with it."""
    Sm = pkg.sim
    wp = Sm.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    got = {}
    for fej in (False, True):
        st = pkg.EKFSlamState(Sm.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=4 if grow else 40, grow=grow)
        try:
            log = Sm.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=2, max_steps=30, fej=fej, nees_every=10)
            assert len(log.true_track) == 30 and len(log.obs_steps) >= 2 and len(log.nees) == 3
            xg, Pg = st.download()
            assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg)) and st.N >= 1
            assert st.is_positive_definite()[0]
            assert not getattr(st, "_fej", None)                          # the object was closed
            if grow:
                assert st.N > 4 and st.capacity > 4
            got[fej] = (np.array(log.true_track), sum(len(a[0]) for a in log.assoc), xg, [v for _, v, _ in log.nees])
        finally:
            st.close()
    print(f"fej sim (grow={grow}): NEES {got[False][3]} (standard) / {got[True][3]} (FEJ); {got[True][1]} matched observations")
    assert np.array_equal(got[False][0], got[True][0]) and got[True][1] >= 1     # the same seeded run, and the update was used
    assert not np.array_equal(got[False][2], got[True][2])                     # ... and it is another filter
