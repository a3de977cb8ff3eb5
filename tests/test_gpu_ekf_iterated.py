"""libslamhip_iterated.so on the device, both dtypes: slam_ekf_update_iterated / slam_ekf_iterated_nis (include/ext/slamhip_iterated.h)
against tests/iterated_ref.py, against slam_ekf_update and against the oracle.

Every cell is re-anchored: the reference repeats the call from the device's own state, downloaded right before it.  x and P are held
to the project's per-call bars (tests/test_gpu_ekf.py: TOL, relerr, relerr_cov), the iteration count and the converged flag are
compared exactly (tests/test_iterated_ref_cpu.py checks that no step of the reference lies within a factor 4 of the tolerance), and
out[3..5], out[8..9] to OUT_BAR relative.
Shapes: the hard scenes of tests/iterated_ref.py -- N = 1, 70, 200 landmarks in handles of 256, i.e. n = 5, 143, 403 over tile edges
128 (fp32) / 64 (fp64): one and several tile rows, n no multiple of the edge, several workgroups of the panel kernel; m = 1, 3, 8
observations; the landmark that straddles a tile edge (63 / 31), the last landmark, a duplicated id, a bearing from across the cut.

OUT_BAR: the bar tests/test_gpu_ekf_linear.py holds its outputs to, 1e-9 relative.  The measured worst case over the cases of this
file is recorded in profiles/iterated_bounds.txt."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import iterated_ref as IR
from tests.test_gpu_ekf import DTYPES, TOL, check_side, relerr, relerr_cov, rounded

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-9
R2 = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
HARD = [name for name in IR.SCENES if name != "N200-m11"]


def _bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def snapshot(st):
    return st.download("x"), st.download("cov"), st.landmark_blocks()


def unchanged(st, snap):
    return _bits_eq(st.download("x"), snap[0]) and _bits_eq(st.download("cov"), snap[1]) and _bits_eq(st.landmark_blocks(), snap[2])


def upload(pkg, name, dtype):
    """The scene on the device; its x and P hold values of the dtype exactly, so the device's state IS the scene."""
    x, P, z, ids = IR.scene(name, dtype)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
    xb, Pb = rounded(st)
    assert np.array_equal(xb, x) and np.array_equal(Pb, P)
    return st, xb, Pb, z, ids


def held_to_the_bars(st, xo, Po, prior, dtype, what):
    xg, Pg = st.download()
    check_side(st, Pg, what)
    assert _bits_eq(Pg, Pg.T), f"{what}: P is not symmetric"
    ex, eP = relerr(xg, xo), relerr_cov(Pg, Po, np.diag(prior))
    print(f"iterated {what} {dtype}: x {ex:.3e} P {eP:.3e}")
    assert ex <= TOL[dtype]["x"], f"{what}: x rel err {ex:.3e}"
    assert eP <= TOL[dtype]["P"], f"{what}: P rel err {eP:.3e}"
    return xg, Pg


def out_close(got, ref, what, scale):
    """Counts and flags exactly, out[3..5] and out[8..9] to OUT_BAR relative; the last step -- a difference of two iterates -- to the
    bar of x (1e-9 of the largest state entry, in double whatever the dtype)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got[0] == ref[0] and got[1] == ref[1] and got[6] == ref[6] and got[7] == ref[7], (what, got, ref)
    idx = [3, 4, 5, 8, 9]
    err = np.abs(got[idx] - ref[idx]) / np.maximum(np.abs(ref[idx]), 1e-300)
    print(f"iterated out {what}: iterations {int(got[0])} rel {err} step {got[2]:.3e} / {ref[2]:.3e}")
    assert np.all(err <= OUT_BAR), (what, got, ref, err)
    assert abs(got[2] - ref[2]) <= 1e-9 * scale, (what, got[2], ref[2])


# ---- 1. one iteration is the update ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", HARD)
def test_one_iteration_is_the_cholesky_form_update(pkg, dtype, name):
    a, xb, Pb, z, ids = upload(pkg, name, dtype)
    b = a.copy()
    try:
        res = b.update_iterated(z, IR.R_HARD, ids, max_iter=1, tol=0.0)
        assert res.iterations == 1 and res.out[0] == 1 and not res.converged and res.out[6] == -1
        a.update(z, IR.R_HARD, ids)
        xa, Pa = rounded(a)
        xg, Pg = held_to_the_bars(b, xa, Pa, Pb, dtype, f"{name} max_iter=1 against slam_ekf_update")
        xo, Po = O.update_sparse(xb, Pb, z, IR.R_HARD, ids)
        assert relerr(xg, xo) <= TOL[dtype]["x"] and relerr_cov(Pg, Po, np.diag(Pb)) <= TOL[dtype]["P"]
        assert relerr(xa, xo) <= TOL[dtype]["x"] and relerr_cov(Pa, Po, np.diag(Pb)) <= TOL[dtype]["P"]
    finally:
        a.close()
        b.close()


# ---- 2. the hard scenes against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", HARD)
def test_hard_scenes_against_the_reference(pkg, dtype, name):
    st, xb, Pb, z, ids = upload(pkg, name, dtype)
    try:
        res = st.update_iterated(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
        xo, Po, ref, steps = IR.update(xb, Pb, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD, with_steps=True)
        assert IR.steps_clear_of(steps, IR.TOL_HARD) and ref[1] == 1 and ref[0] >= 3
        assert res.iterations == ref[0] and res.converged
        out_close(res.out, ref, name, np.max(np.abs(xb)))
        held_to_the_bars(st, xo, Po, Pb, dtype, name)
        assert res.cost_last < 0.5 * res.cost_first                        # what the iteration is for
        if name == "N70-m3-cut":                                           # the wrap was honoured: without it r is 2 pi off
            assert abs(z[1, 0] - O.predict_observation(xb, ids[0])[0][1]) > math.pi and xb[2] == np.asarray(3.1, IR.NP_DTYPE[dtype])
        if name == "N200-m3-duplicate":
            assert ids[0] == ids[2]
    finally:
        st.close()


# ---- 3. a fixed number of iterations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["N70-m8", "N200-m3-duplicate"])
def test_tol_zero_runs_exactly_max_iter_iterations(pkg, dtype, name):
    st, xb, Pb, z, ids = upload(pkg, name, dtype)
    try:
        res = st.update_iterated(z, IR.R_HARD, ids, max_iter=3, tol=0.0)
        assert res.iterations == 3 and res.out[0] == 3 and not res.converged and res.out[1] == 0
        xo, Po, ref = IR.update(xb, Pb, z, IR.R_HARD, ids, 3, 0.0)
        assert ref[0] == 3 and ref[1] == 0
        out_close(res.out, ref, name + " stopped at 3", np.max(np.abs(xb)))
        held_to_the_bars(st, xo, Po, Pb, dtype, name + " stopped at 3")
    finally:
        st.close()


# ---- 4. the dry run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["N1-m1", "N200-m8-last"])
def test_the_dry_run_reads_only_and_reports_what_the_update_reports(pkg, dtype, name):
    st, xb, Pb, z, ids = upload(pkg, name, dtype)
    try:
        snap = snapshot(st)
        dry = st.iterated_nis(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
        assert unchanged(st, snap)
        res = st.update_iterated(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
        assert _bits_eq(dry.out, res.out) and res.iterations >= 3
        assert not unchanged(st, snap)
    finally:
        st.close()


# ---- 5. S not positive definite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_indefinite_s_is_refused_and_leaves_the_state_bit_identical(pkg, dtype):
    """Landmark 12 carries a NEGATIVE diagonal block: the second observation's first pivot is -10 + (what the vehicle and R add, below
    1), minus two squares -- negative in any evaluation order, at the first iteration."""
    x, P, z, ids = IR.scene("N70-m3-straddler", dtype)
    assert ids[1] == 70 and ids[2] == 12
    ids = np.array([ids[0], 12, 70])
    z = z[:, [0, 2, 1]]
    f = IR.f(12)
    P[f, f] = P[f + 1, f + 1] = -10.0
    P[f, f + 1] = P[f + 1, f] = 0.0
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
    try:
        good = np.array([ids[0], 70])
        st.update_iterated(z[:, [0, 2]], IR.R_HARD, good, max_iter=2, tol=0.0)      # a valid call first: its panel is what a stale W1 would be
        xb, Pb = rounded(st)
        snap = snapshot(st)
        L = pkg._lib
        zp = np.ascontiguousarray(z.T)
        ii = np.ascontiguousarray(ids, dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        ref = IR.update(xb, Pb, z, IR.R_HARD, ids, 5, 1e-9)[2]
        assert ref[6] == 2 and ref[7] == 0
        for fn in (L.iterated_lib().slam_ekf_iterated_nis, L.iterated_lib().slam_ekf_update_iterated):
            out = np.full(10, 7.0)
            rc = fn(st._h, p(zp), p(ii, C.c_int32), 3, p(rr), 5, 1e-9, p(out))
            assert rc == L.SLAM_E_NOTPD and "not positive definite" in L.last_error()
            assert out[6] == 2 and out[7] == 0 and out[0] == 0 and out[1] == 0 and out[3] == 0 and out[4] == 0 and out[5] < 0, out
            assert abs(out[5] - ref[5]) <= 1e-9 * abs(ref[5])
            assert unchanged(st, snap)
        with pytest.raises(pkg.NotPositiveDefinite):
            st.update_iterated(z, IR.R_HARD, ids)
        assert unchanged(st, snap)
        # the next ordinary update on the handle works
        st.update(z[:, [0, 2]], IR.R_HARD, good)
        xo, Po = O.update_sparse(xb, Pb, z[:, [0, 2]], IR.R_HARD, good)
        held_to_the_bars(st, xo, Po, Pb, dtype, "after the refusal")
    finally:
        st.close()


# ---- 6. bad arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_are_refused_with_the_state_bit_identical(pkg, dtype):
    st, xb, Pb, z, ids = upload(pkg, "N70-m3-straddler", dtype)
    try:
        snap = snapshot(st)
        L = pkg._lib
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        zp = np.ascontiguousarray(np.tile(z.T, (3, 1)))                    # 9 pairs
        ii = np.ascontiguousarray(np.tile(ids, 3), dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        out = np.full(10, 7.0)
        nan, inf = float("nan"), float("inf")

        def z_with(v):
            zz = zp.copy()
            zz[1, 1] = v
            return zz

        def ids_with(v):
            jj = ii.copy()
            jj[2] = v
            return jj

        cases = [("null z", (None, p(ii, C.c_int32), 3, p(rr), 5, 1e-9, p(out))),
                 ("null ids", (p(zp), None, 3, p(rr), 5, 1e-9, p(out))),
                 ("null R", (p(zp), p(ii, C.c_int32), 3, None, 5, 1e-9, p(out))),
                 ("null out", (p(zp), p(ii, C.c_int32), 3, p(rr), 5, 1e-9, None))]
        cases += [(f"m = {m}", (p(zp), p(ii, C.c_int32), m, p(rr), 5, 1e-9, p(out))) for m in (0, -1, 9)]
        cases += [(f"max_iter = {k}", (p(zp), p(ii, C.c_int32), 3, p(rr), k, 1e-9, p(out))) for k in (0, -1, 65)]
        cases += [(f"tol = {t}", (p(zp), p(ii, C.c_int32), 3, p(rr), 5, t, p(out))) for t in (-1e-300, nan, inf)]
        keep = []
        for j in (0, 71, -4):
            keep.append(ids_with(j))
            cases.append((f"id {j}", (p(zp), p(keep[-1], C.c_int32), 3, p(rr), 5, 1e-9, p(out))))
        for v in (nan, inf, -inf):
            keep.append(z_with(v))
            cases.append((f"z {v}", (p(keep[-1]), p(ii, C.c_int32), 3, p(rr), 5, 1e-9, p(out))))
        for Rb in ((0.0025, 0.0, 0.0, nan), (inf, 0.0, 0.0, 1e-4), (0.0025, 1e-5, 2e-5, 1e-4), (0.0025, 0.0, 0.0, -1e-4),
                   (0.0, 0.0, 0.0, 1e-4), (0.0025, 0.001, 0.001, 1e-4)):
            keep.append(np.array(Rb))
            cases.append((f"R {Rb}", (p(zp), p(ii, C.c_int32), 3, p(keep[-1]), 5, 1e-9, p(out))))
        for fn in (L.iterated_lib().slam_ekf_update_iterated, L.iterated_lib().slam_ekf_iterated_nis):
            for what, args in cases:
                assert fn(st._h, *args) == L.SLAM_E_BADARG, what
                assert "bad argument" in L.last_error(), what
                assert unchanged(st, snap), what
            assert fn(None, p(zp), p(ii, C.c_int32), 3, p(rr), 5, 1e-9, p(out)) == L.SLAM_E_BADARG
        assert np.all(out == 7.0)
        with pytest.raises(ValueError):
            st.iterated_nis(zp.T, IR.R_HARD, ii)                          # nine observations: the dry run takes one batch
        # and the handle is as good as before: the same call with good arguments is the reference's
        res = st.update_iterated(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
        xo, Po, ref = IR.update(xb, Pb, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
        out_close(res.out, ref, "after the refusals", np.max(np.abs(xb)))
        held_to_the_bars(st, xo, Po, Pb, dtype, "after the refusals")
    finally:
        st.close()


# ---- 7. the gating after an iterated update ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gating_follows_an_iterated_update_in_grid_and_sweep_mode(pkg, dtype):
    """A grid built BEFORE the call must not be used after it: the means moved.  Landmark 120 enters with a wide prior, 3 m from where
    the sensor then sees it; the iterated update moves it there, and the next association -- grid form and sweep form -- equals the
    oracle's on the downloaded state."""
    results = {}
    j = 120
    for mode in ("grid", "sweep"):
        x, P, z, ids = IR.scene("N200-m8-last", dtype)
        assert ids[2] == j
        fj = IR.f(j)
        P[fj, fj] = P[fj + 1, fj + 1] = 9.0
        truth = x.copy()
        truth[fj:fj + 2] += [3.0, -1.0]
        zj = O.predict_observation(truth, j)[0]
        z[:, 2] = [zj[0], O.mpi_to_pi(zj[1])]
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
        try:
            st.set_gate_mode(mode)
            xb, _ = rounded(st)
            st.associate_vector(O.obs_blocks(xb, ids)[0].T, R2, 4.0, 25.0)      # the grid exists now
            res = st.update_iterated(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
            assert res.out[6] == -1 and res.iterations >= 2
            xg, Pg = rounded(st)
            moved = float(np.hypot(*(xg[fj:fj + 2] - xb[fj:fj + 2])))
            print(f"iterated gating {mode} {dtype}: landmark {j} moved {moved:.3f} m in {res.iterations} iterations")
            assert moved > 1.0
            check_side(st, st.download("cov"), mode)
            rng = np.random.default_rng(9)
            zq = O.obs_blocks(xg, ids)[0].T + rng.normal(0, [0.05, 0.005], (len(ids), 2)).T
            zq = np.hstack([zq, [[500.0], [0.3]]])                        # and one that is nobody's
            zf, idf, zn = st.associate(zq, R2, 4.0, 25.0)
            zfo, idfo, zno = O.associate_sparse(xg, Pg, zq, R2, 4.0, 25.0)
            assert np.array_equal(idf, idfo) and np.array_equal(zf, zfo) and np.array_equal(zn, zno), (mode, idf, idfo)
            assert j in np.asarray(idf).reshape(-1).tolist() and zn.shape[1] >= 1      # the moved landmark is found where it is now
            assert st.gate_info()["form"] == mode
            results[mode] = (np.asarray(idf).copy(), st.download(), res.out)
        finally:
            st.close()
    assert np.array_equal(results["grid"][0], results["sweep"][0]) and _bits_eq(results["grid"][2], results["sweep"][2])
    assert _bits_eq(results["grid"][1][0], results["sweep"][1][0]) and _bits_eq(results["grid"][1][1], results["sweep"][1][1])


# ---- 8. more than eight observations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_eleven_observations_are_batches_of_eight_and_three(pkg, dtype):
    st, xb, Pb, z, ids = upload(pkg, "N200-m11", dtype)
    try:
        assert len(ids) == 11
        res = st.update_iterated(z, IR.R_HARD, ids, max_iter=IR.ITER_HARD, tol=IR.TOL_HARD)
        xo, Po, outs = IR.update_batches(xb, Pb, z, IR.R_HARD, ids, IR.ITER_HARD, IR.TOL_HARD)
        assert len(res.batches) == 2 == len(outs) and res.batches[-1] is res
        for b, ref in zip(res.batches, outs):
            assert b.out[0] == ref[0] and b.out[1] == ref[1] == 1 and b.out[6] == -1, (b.out, ref)
        # the second batch starts from the DEVICE's state after the first (rounded to the dtype), the reference from its own: the
        # states are compared at the bars of x and P, the first batch's numbers at the bar of the outputs
        out_close(res.batches[0].out, outs[0], "first batch of 8", np.max(np.abs(xb)))
        held_to_the_bars(st, xo, Po, Pb, dtype, "8 + 3")
    finally:
        st.close()


# ---- 9. the simulator -------------------------------------------------------------------------------------------------------------
def test_sim_with_the_iterated_update_completes(pkg, golden_dir):
    """30 steps of the golden course with update_iterated(max_iter=5) in place of update: it completes, the state is finite and its
    covariance positive definite.  The final pose error is printed beside the plain run's: reported, not asserted."""
    Sm = pkg.sim
    wp = Sm.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    got = {}
    for it in (None, 5):
        st = pkg.EKFSlamState(Sm.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=40)
        try:
            log = Sm.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=2, max_steps=30, iterated=it)
            assert len(log.true_track) == 30 and len(log.obs_steps) >= 2
            xg, Pg = st.download()
            assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg)) and st.N >= 1
            assert st.is_positive_definite()
            got[it] = (float(np.linalg.norm(log.true_track[-1][:2] - log.slam_track[-1][:2])), np.array(log.true_track),
                       sum(len(a[0]) for a in log.assoc))
        finally:
            st.close()
    print(f"iterated sim: final pose error {got[None][0]:.4f} m (update) / {got[5][0]:.4f} m (update_iterated, max_iter = 5); "
          f"{got[5][2]} matched observations")
    assert np.array_equal(got[None][1], got[5][1]) and got[5][2] >= 1     # the same seeded run, and the iterated update was used
