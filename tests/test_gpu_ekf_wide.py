"""libslamhip_wide.so on the device, both dtypes: slam_ekf_wide_update / _nis (include/ext/slamhip_wide.h) against tests/wide_ref.py,
against the oracle and against slam_ekf_update.

The scenes (tests/wide_ref.py: SCENES, seed 3) are the smallest at which each piece can go wrong: m = 1, 9, 17, 33, 48, 64 give
k_p = 32 / 64 / 96 / 128 rows of S in the factor kernel and panels of 16, 32, 48, 80, 96 and 128 columns, i.e. every branch the
down-date takes without a pre-split image (the default kernel, the 2-chunk stream, the split-bf16 one-workgroup-per-tile path at 3
and 4 chunks, the fp64 kernel); N = 70 and 200 in handles of 256 give n = 143 and 403 over tile edges 128 / 64 -- several tile rows,
n no multiple of the edge, several workgroups of the panel kernel, one of them half beyond n; the ids start with the landmark whose
pair straddles a tile edge and the last landmark; m = 64 of N = 70 is m close to N; two scenes observe a landmark twice.

Every cell is re-anchored: the reference repeats the call from the state and the points downloaded right before it, and is held by
relerr / relerr_cov of tests/test_gpu_ekf.py.  The bar is the project's per-call TOL (fp64 1e-9, fp32 5e-6) -- but nobody had
measured a 64-observation update on these hardened scenes against it, so each cell also runs slam_ekf_update on a copy of the same
uploaded state with the same observations and takes its error e_prod against the oracle: the bar of both modes of the wide call on
that cell is max(TOL, 2 e_prod) (both calls round the same double-precision front half in another summation order, and the
down-date is the same kernel).  The errors of both calls are printed per cell and recorded in profiles/wide_bounds.txt."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import fej_ref as F
from tests import iterated_ref as IR
from tests import wide_ref as W
from tests.test_gpu_ekf import DTYPES, TOL, check_side, relerr, relerr_cov, rounded
from tests.test_gpu_ekf_fej import _bits_eq, snapshot, unchanged

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-9
SEED = 3


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def upload(pkg, dtype, x, P, points=11):
    """The state on the device with an object whose points are displaced; returns (st, fe, xb, Pb, lin, first)."""
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=IR.CAP)
    fe = st.fej()
    xb, Pb = rounded(st)
    assert np.array_equal(xb, x) and np.array_equal(Pb, P)
    fe.set(*W.displaced(xb, points))
    lin, first, _ = fe.get()
    return st, fe, xb, Pb, lin, first


def errors(st, xo, Po, prior, what):
    xg, Pg = st.download()
    check_side(st, Pg, what)
    assert _bits_eq(Pg, Pg.T), f"{what}: P is not symmetric"
    return relerr(xg, xo), relerr_cov(Pg, Po, np.diag(prior)), xg.astype(np.float64), np.array(Pg, dtype=np.float64)


# ---- 1. both modes against the reference, the oracle and the product's update -------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,m,repeat", W.SCENES)
def test_both_modes_against_the_reference_and_the_products_update(pkg, dtype, N, m, repeat):
    x, P, z, ids = W.scene(N, m, dtype, SEED, repeat)
    st, fe, xb, Pb, lin, first = upload(pkg, dtype, x, P)
    prod, est = st.copy(), st.copy()
    what = f"N{N}-m{m}{'-repeat' if repeat else ''} {dtype}"
    try:
        # the product's update on a copy: its error against the oracle sets the cell's bar
        prod.update(z, IR.R_HARD, ids)
        xo, Po = O.update_sparse(xb, Pb, z, IR.R_HARD, ids)
        exp, ePp, xp, Pp = errors(prod, xo, Po, Pb, what + " product")
        bar = dict(x=max(TOL[dtype]["x"], 2 * exp), P=max(TOL[dtype]["P"], 2 * ePp))
        # the joint gate first: the state, the blocks and the points are only read
        xr, Pr, ref, _ = W.update(xb, Pb, lin, first, z, IR.R_HARD, ids)
        assert ref[3] == -1, what
        snap = snapshot(st, fe)
        gate = fe.joint_nis(z, IR.R_HARD, ids)
        assert unchanged(st, fe, snap), what
        out = fe.update_joint(z, IR.R_HARD, ids)
        assert out.shape == (1, 4) and out[0, 3] == -1
        assert _bits_eq(gate, out), (gate, out)                            # the same front half
        eo = np.abs(out[0, :3] - ref[:3]) / np.abs(ref[:3])
        assert np.all(eo <= OUT_BAR), (out, ref)
        ex, eP, xf, Pf = errors(st, xr, Pr, Pb, what + " at the points")
        now = snapshot(st, fe)
        assert _bits_eq(now[3], snap[3]) and _bits_eq(now[4], snap[4]) and now[5] == snap[5], what      # lin / first did not move
        # f == NULL: the Jacobians at the stored state, the oracle's update
        oute = est.update_joint_at_estimates(z, IR.R_HARD, ids)
        refe = W.update_at_estimates(xb, Pb, z, IR.R_HARD, ids)[2]
        assert refe[3] == -1 == oute[0, 3] and np.all(np.abs(oute[0, :3] - refe[:3]) / np.abs(refe[:3]) <= OUT_BAR), (oute, refe)
        exe, ePe, xe, Pe = errors(est, xo, Po, Pb, what + " at the estimates")
        dxp, dPp = relerr(xe, xp), relerr_cov(Pe, Pp, np.diag(Pb))
        apart, apartP = relerr(xf, xe), relerr_cov(Pf, Pe, np.diag(Pb))
        print(f"wide {what}: product x {exp:.3e} P {ePp:.3e} | points x {ex:.3e} P {eP:.3e} | estimates x {exe:.3e} P {ePe:.3e} | "
              f"estimates - product x {dxp:.3e} P {dPp:.3e} | bar x {bar['x']:.3e} P {bar['P']:.3e} | out {eo.max():.1e} | "
              f"points - estimates x {apart:.3e} P {apartP:.3e}")
        assert ex <= bar["x"] and eP <= bar["P"], f"{what} at the points: x {ex:.3e} P {eP:.3e}, bar {bar}"
        assert exe <= bar["x"] and ePe <= bar["P"], f"{what} at the estimates: x {exe:.3e} P {ePe:.3e}, bar {bar}"
        # against the product on its copy: within the sum of both calls' bars
        assert dxp <= bar["x"] + max(TOL[dtype]["x"], exp) and dPp <= bar["P"] + max(TOL[dtype]["P"], ePp), what
        # the points are honoured: with displaced points the two modes are far apart.  Held in P: the gain, and with it the
        # down-date, changes with the Jacobians whatever the residual is, while the change of x is the gain times a residual that a
        # scene may leave small (N70-m1: v' inv(S) v = 0.06) and relerr divides it by the extent of the map
        assert apartP > 100 * bar["P"], f"{what}: the two modes differ by {apartP:.3e} in P only"
    finally:
        st.close()
        prod.close()
        est.close()


# ---- 2. S not positive definite -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_coinciding_points_are_refused_and_leave_everything_bit_identical(pkg, dtype):
    """m = 20: the first estimate of the 13th observed landmark IS lin[0:2]; its Jacobian, and with it pivot 24, is not finite."""
    x, P, z, ids = W.scene(70, 20, dtype, SEED)
    st, fe, xb, Pb, lin, first = upload(pkg, dtype, x, P)
    try:
        fe.update_joint(z[:, :5], IR.R_HARD, ids[:5])                       # a valid call first: its panel is what a stale W1 would be
        xb, Pb = rounded(st)
        j = int(ids[12])
        same = first.copy()
        same[2 * (j - 1):2 * j] = lin[0:2]
        fe.set(None, same)
        snap = snapshot(st, fe)
        ref = W.update(xb, Pb, lin, same, z, IR.R_HARD, ids)[2]
        assert ref[3] == 24
        L = pkg._lib
        zp, ii = np.ascontiguousarray(z.T), np.ascontiguousarray(ids, dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        for fn in (L.wide_lib().slam_ekf_wide_nis, L.wide_lib().slam_ekf_wide_update):
            out = np.full(4, 7.0)
            rc = fn(st._h, fe._f, _p(zp), _p(ii, C.c_int32), 20, _p(rr), _p(out))
            assert rc == L.SLAM_E_NOTPD and "not positive definite" in L.last_error()
            assert out[3] == ref[3] and out[0] == 0 and out[1] == 0 and not np.isfinite(out[2]), out
            assert unchanged(st, fe, snap)
        with pytest.raises(pkg.NotPositiveDefinite):
            fe.update_joint(z, IR.R_HARD, ids)
        assert unchanged(st, fe, snap)
        # the next valid call works
        fe.set(None, first)
        out = fe.update_joint(z, IR.R_HARD, ids)
        xr, Pr, ref, _ = W.update(xb, Pb, lin, first, z, IR.R_HARD, ids)
        assert ref[3] == -1 == out[0, 3] and np.all(np.abs(out[0, :3] - ref[:3]) / np.abs(ref[:3]) <= OUT_BAR)
    finally:
        st.close()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_another_states_object_and_a_renumbered_map_are_refused(pkg, dtype):
    x, P, z, ids = IR.scene("N70-m3-straddler", dtype)
    st, fe, xb, Pb, lin, first = upload(pkg, dtype, x, P)
    other = st.copy()
    try:
        fo = other.fej()
        L = pkg._lib
        lib = L.wide_lib()
        zp, ii = np.ascontiguousarray(z.T), np.ascontiguousarray(ids, dtype=np.int32)
        rr = np.ascontiguousarray(IR.R_HARD.T).reshape(4)
        out = np.full(4, 7.0)
        snap, snapo = snapshot(st, fe), snapshot(other, fo)
        for fn in (lib.slam_ekf_wide_update, lib.slam_ekf_wide_nis):
            assert fn(st._h, fo._f, _p(zp), _p(ii, C.c_int32), 3, _p(rr), _p(out)) == L.SLAM_E_BADARG
            assert "belongs to another state" in L.last_error()
            bad = ii.copy()
            bad[1] = 71
            assert fn(st._h, fe._f, _p(zp), _p(bad, C.c_int32), 3, _p(rr), _p(out)) == L.SLAM_E_BADARG and "idf" in L.last_error()
        assert unchanged(st, fe, snap) and unchanged(other, fo, snapo) and np.all(out == 7.0)
        new_index = st.remove_landmarks([5, 40])
        snap = snapshot(st, fe)
        assert st.N == 68 and snap[5] == 70
        for fn in (lib.slam_ekf_wide_update, lib.slam_ekf_wide_nis):
            assert fn(st._h, fe._f, _p(zp), _p(ii, C.c_int32), 3, _p(rr), _p(out)) == L.SLAM_E_BADARG
            assert "the map changed outside the object" in L.last_error()
        assert unchanged(st, fe, snap) and np.all(out == 7.0)
        fe.remap(np.flatnonzero(new_index) + 1)
        xb, Pb = rounded(st)
        lin, first, count = fe.get()
        ids2 = new_index[ids - 1]
        assert count == 68 and np.all(ids2 > 0)
        got = fe.update_joint(z, IR.R_HARD, ids2)
        xr, Pr, ref, _ = W.update(xb, Pb, lin, first, z, IR.R_HARD, ids2)
        ex, eP, _, _ = errors(st, xr, Pr, Pb, "after remap")
        print(f"wide after remap {dtype}: x {ex:.3e} P {eP:.3e}")
        assert got[0, 3] == -1 == ref[3] and ex <= TOL[dtype]["x"] and eP <= TOL[dtype]["P"]
    finally:
        st.close()
        other.close()


# ---- 4. the bindings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_seventy_observations_go_as_sixty_four_and_six(pkg, dtype):
    x, P, z, ids = W.scene(70, 70, dtype, SEED)
    st, fe, xb, Pb, lin, first = upload(pkg, dtype, x, P)
    b = st.copy()
    try:
        fb = b.fej()
        fb.set(lin, first)
        outs = fe.update_joint(z, IR.R_HARD, ids)
        o1 = fb.update_joint(z[:, :64], IR.R_HARD, ids[:64])
        o2 = fb.update_joint(z[:, 64:], IR.R_HARD, ids[64:])
        assert outs.shape == (2, 4) and np.all(outs[:, 3] == -1)
        assert _bits_eq(outs[0:1], o1) and _bits_eq(outs[1:2], o2)
        (xa, Pa), (xc, Pc) = st.download(), b.download()
        assert _bits_eq(xa, xc) and _bits_eq(Pa, Pc)
        _, _, refs = W.update_batches(xb, Pb, lin, first, z, IR.R_HARD, ids)
        assert np.all(np.abs(outs[0, :3] - refs[0][:3]) / np.abs(refs[0][:3]) <= OUT_BAR), (outs, refs)
        with pytest.raises(ValueError):
            fe.joint_nis(z, IR.R_HARD, ids)
    finally:
        st.close()
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_observe_with_joint_is_associate_update_joint_add_features(pkg, dtype):
    x, P, z, ids = W.scene(70, 17, dtype, SEED)
    z = np.hstack([z, [[12.0, 25.0], [0.3, -2.0]]])                         # two readings of nothing in the map
    st, fe, xb, Pb, lin, first = upload(pkg, dtype, x, P)
    b = st.copy()
    try:
        fb = b.fej()
        fb.set(lin, first)
        g1, g2 = pkg.sim.GATE1, pkg.sim.GATE2
        assoc = np.asarray(fe.observe(z, IR.R_HARD, g1, g2, joint=True))
        assoc_b = np.asarray(b.associate_vector(z, IR.R_HARD, g1, g2))
        assert np.array_equal(assoc, assoc_b) and np.count_nonzero(assoc > 0) >= 1, assoc
        fb.update_joint(z[:, assoc > 0], IR.R_HARD, assoc[assoc > 0])
        fb.add_features(z[:, assoc < 0], IR.R_HARD)
        (xa, Pa), (xc, Pc) = st.download(), b.download()
        assert st.N == b.N and _bits_eq(xa, xc) and _bits_eq(Pa, Pc)
        assert all(_bits_eq(p, q) for p, q in zip(fe.get()[:2], fb.get()[:2]))
    finally:
        st.close()
        b.close()


@pytest.mark.parametrize("grow", [False, True])
def test_sim_with_the_joint_update_completes_and_is_another_filter(pkg, golden_dir, grow):
    """300 steps of the golden course with every step's update routed through update_joint: it completes with a finite NEES and a
    positive definite covariance, and it is not the run of the batched form."""
    Sm = pkg.sim
    wp = Sm.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    got = {}
    for joint in (False, True):
        st = pkg.EKFSlamState(Sm.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=4 if grow else 64, grow=grow)
        try:
            log = Sm.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=2, max_steps=300, fej=True, fej_joint=joint, nees_every=100)
            assert len(log.true_track) == 300 and len(log.nees) == 3
            xg, Pg = st.download()
            assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg)) and st.is_positive_definite()[0]
            assert all(np.isfinite(v) for _, v, _ in log.nees)
            assert not getattr(st, "_fej", None)
            got[joint] = (np.array(log.true_track), max(len(a[0]) for a in log.assoc), xg, [v for _, v, _ in log.nees])
        finally:
            st.close()
    print(f"wide sim (grow={grow}): NEES {got[False][3]} (batched) / {got[True][3]} (joint); at most {got[True][1]} matched a step")
    assert np.array_equal(got[False][0], got[True][0]) and got[True][1] >= 1
    assert not np.array_equal(got[False][2], got[True][2])


# ---- 5. what it is for: no information along the unobservable directions ------------------------------------------------------------
def test_the_chained_run_through_the_joint_update_gains_no_information_along_the_three_directions(pkg):
    """tests/test_gpu_ekf_fej.py's chained run, drive(seed = 0, steps = 96, Q = 0) on an fp64 handle, with every update routed
    through update_joint: the drift of N' inv(P) N stays rounding only, under the bar 1e-3 argued there."""
    ops = F.drive(0, 96, np.zeros((2, 2)))
    hist = F.run(ops)
    st = pkg.EKFSlamState(F.X0_DRIVE, F.P0_DRIVE, dtype="f64", max_landmarks=64)
    try:
        fe = st.fej()
        lin, first, _ = fe.get()
        M0 = F.information(F.N_matrix(lin, first), F.P0_DRIVE)
        for op in ops:
            if op[0] == "predict":
                fe.predict(*op[1:])
            elif op[0] == "update":
                assert fe.update_joint(op[1], F.R_DRIVE, op[2])[0, 3] == -1
            else:
                fe.add_features(op[1], F.R_DRIVE)
        _, xo, Po, lo, fo, _, _ = hist[-1]
        ex, eP, xg, Pg = errors(st, xo, Po, Po, "chained run")
        lg, fg, _ = fe.get()
        d = F.drift(F.information(F.N_matrix(lg, fg), Pg), M0)
        print(f"wide chained run: drift of N' inv(P) N over {len(ops)} calls through update_joint: {d:.3e}; x {ex:.3e} P {eP:.3e}")
        assert ex <= len(ops) * TOL["f64"]["x"] and eP <= len(ops) * TOL["f64"]["P"]
        assert d <= 1e-3
        assert st.is_positive_definite()[0]
    finally:
        st.close()
