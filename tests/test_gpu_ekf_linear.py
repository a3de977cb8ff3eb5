"""libslamhip_linear.so on the device, both dtypes: slam_ekf_update_linear / linear_nis / predict_linear / predict_odometry
(include/ext/slamhip_linear.h) against tests/linear_ref.py and against the existing kernels.

Every cell is re-anchored: the reference repeats the call from the device's own state, downloaded right before it.
  * update_linear: x and P entrywise inside the project's per-call bars (fp64 1e-9 max|x| and 1e-9 sqrt(s_i s_j),
    fp32 5e-6 for both; tests/test_gpu_ekf.py: TOL, relerr, relerr_cov), `out` to 1e-9 relative, linear_nis the same `out` with
    the state bit-identical, the packed diagonal blocks equal to the matrix, P bit-symmetric.
  * the predicts: every owned entry inside  u_T |ref| + c 2^-53 mag  with the c of the existing predict tests
    (tests/strip_ref.py: 16 strip and x, 32 P_vv), everything else bit-identical.
Shapes: N = 0, 1, 70, 200 landmarks in handles of 256, i.e. n = 3, 5, 143, 403 over tile edges 128 (fp32) / 64 (fp64): one and
several tile rows, n no multiple of the edge, two workgroups of the panel and strip kernels at N = 200.  Landmark 63 (fp32) /
31 (fp64) straddles a tile edge."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import copy_ref as CR
from tests import linear_ref as LR
from tests import merge_ref as MR
from tests import strip_ref as S
from tests import update_records as UR
from tests.test_gpu_ekf import DTYPES, TOL, check_side, relerr, relerr_cov, rounded

pytestmark = pytest.mark.gpu

CAP = 256
EDGE = {"f32": 128, "f64": 64}
STRADDLER = {"f32": 63, "f64": 31}
R2 = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
QF = np.array([[0.5 ** 2, -0.3 * 0.5 * (3 * math.pi / 180)], [-0.3 * 0.5 * (3 * math.pi / 180), (3 * math.pi / 180) ** 2]])
Q3 = np.array([[0.04, 0.01, 0.002], [0.01, 0.09, 0.003], [0.002, 0.003, 0.0025]])


def _bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_state(pkg, N, dtype, heading=None):
    """The designed `slam` state of the record tests (tests/update_records.py) for N >= 70; a small dense one below."""
    if N >= 70:
        x, P = UR.designed_state("slam", N, dtype, 1000 + N)
        x = np.array(x)
    else:
        rng = np.random.default_rng(40 + N)
        n = 3 + 2 * N
        x = np.concatenate([[3.0, -2.0, 0.4], rng.uniform(-20, 20, 2 * N)])
        A = rng.normal(0, 0.3, (n, n))
        P = A @ A.T + 0.05 * np.eye(n)
        P = (P + P.T) / 2
    if heading is not None:
        x[2] = heading
    return pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=CAP)


def dense_R(k, seed, scale=0.05):
    """k x k, symmetric bit for bit, positive definite, NOT diagonal."""
    B = np.random.default_rng(seed).normal(0, scale, (k, k))
    Rm = B @ B.T + scale ** 2 * np.eye(k)
    return (Rm + Rm.T) / 2


def row_cases(dtype):
    """name -> (N, rows, wrap): the row patterns of the issue."""
    s = STRADDLER[dtype]
    E = EDGE[dtype]
    assert s in CR.straddlers(70, E) and s in CR.straddlers(200, E)
    fs, fl70, fl200 = LR.f(s), LR.f(70), LR.f(200)
    assert fs // E != (fs + 1) // E
    rng = np.random.default_rng(17)

    def scattered(n, k):
        rows = []
        for _ in range(k):
            cols = rng.choice(n, size=int(rng.integers(1, 4)), replace=False)
            rows.append({int(c): float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5)) for c in cols})
        return rows

    n200 = 3 + 2 * 200
    # eight non-zeros over three tile rows, columns on both sides of every row the panel kernel walks: for a row r of the
    # panel some of these columns lie in a tile row above r's (the transposed side of the symmetric view) and some below
    wide = {1: 0.5, E - 2: -1.0, E: 0.7, E + 9: 1.2, 2 * E + 1: -0.6, 2 * E + 40: 0.9, fs: 0.3, n200 - 1: -0.8}
    assert len({c // E for c in wide}) >= 3 and len(wide) == 8
    k16 = [{0: 1.0}, {1: 1.0}, {2: 1.0}, wide, {fs: 1.0, fs + 1: -0.5}, {fl200: 1.0}, {fl200 + 1: 1.0, 0: -1.0}] + scattered(n200, 9)
    return {
        "N0-k2-vehicle": (0, [{0: 1.0}, {1: 1.0, 2: 0.25}], ()),
        "N0-k1-heading": (0, [{2: 1.0}], (0,)),
        "N1-k2": (1, [{3: 1.0, 0: -1.0}, {4: 1.0, 1: -1.0}], ()),
        "N70-k1-straddler": (70, [{fs: 1.0, fs + 1: -0.5, 2: 0.3}], ()),
        "N70-k15": (70, [{fl70: 1.0}, {fl70 + 1: 1.0}, {2: 1.0}] + scattered(143, 12), (2,)),
        "N200-k2-last": (200, [{fl200: 1.0}, {fl200 + 1: 1.0}], ()),
        "N200-k16": (200, k16, (2,)),
    }


CASES = ["N0-k2-vehicle", "N0-k1-heading", "N1-k2", "N70-k1-straddler", "N70-k15", "N200-k2-last", "N200-k16"]


def held_to_the_bars(st, xo, Po, prior, dtype, what):
    xg, Pg = st.download()
    check_side(st, Pg, what)
    assert _bits_eq(Pg, Pg.T), f"{what}: P is not symmetric"
    ex, eP = relerr(xg, xo), relerr_cov(Pg, Po, np.diag(prior))
    print(f"linear {what} {dtype}: x {ex:.3e} P {eP:.3e}")
    assert ex <= TOL[dtype]["x"], f"{what}: x rel err {ex:.3e}"
    assert eP <= TOL[dtype]["P"], f"{what}: P rel err {eP:.3e}"
    return xg, Pg


def out_close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got[3] == ref[3], (what, got, ref)
    err = np.abs(got[:3] - ref[:3]) / np.maximum(np.abs(ref[:3]), 1e-300)
    print(f"linear out {what}: rel {err}")
    assert np.all(err <= 1e-9), (what, got, ref)


# ---- 1. update_linear against linear_ref ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_update_linear_against_the_reference(pkg, dtype, case):
    N, rows, wrap = row_cases(dtype)[case]
    k = len(rows)
    assert k == {"N0-k2-vehicle": 2, "N0-k1-heading": 1, "N1-k2": 2, "N70-k1-straddler": 1, "N70-k15": 15, "N200-k2-last": 2,
                 "N200-k16": 16}[case]
    st = make_state(pkg, N, dtype, heading=3.1 if wrap else None)
    try:
        xb, Pb = rounded(st)
        H = LR.dense_H(len(xb), rows)
        z = H @ xb + np.random.default_rng(k).normal(0, 0.05, k)
        mask = 0
        for i in wrap:                                                    # the compass reads the same heading from across the cut
            z[i] -= 2 * math.pi
            mask |= 1 << i
        Rm = dense_R(k, 100 + k)
        x0, P0, side0 = st.download("x"), st.download("cov"), st.landmark_blocks()
        nis = st.linear_nis(rows, z, Rm, wrap=wrap)
        assert _bits_eq(st.download("x"), x0) and _bits_eq(st.download("cov"), P0) and _bits_eq(st.landmark_blocks(), side0)
        out = st.update_linear(rows, z, Rm, wrap=wrap)
        xo, Po, ref = LR.update(xb, Pb, H, z, Rm, wrap_mask=mask)
        assert ref[3] == -1 and _bits_eq(nis, out)
        out_close(out, ref, case)
        held_to_the_bars(st, xo, Po, Pb, dtype, case)
        if wrap:                                                          # the wrap bit was honoured: without it v is 2 pi off
            assert abs(LR.innovation(xb, H, z, wrap_mask=mask)[wrap[0]]) < 1.0 < abs(LR.innovation(xb, H, z)[wrap[0]])
        # the dense form of H is the same call
        if case == "N70-k1-straddler":
            xb2, Pb2 = rounded(st)
            out2 = st.update_linear(H, z, Rm)
            xo2, Po2, ref2 = LR.update(xb2, Pb2, H, z, Rm)
            out_close(out2, ref2, case + " dense")
            held_to_the_bars(st, xo2, Po2, Pb2, dtype, case + " dense")
    finally:
        st.close()


# ---- 2. against the existing kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 4, 8])
def test_innovation_mode_agrees_with_the_update_kernels(pkg, dtype, m):
    a = make_state(pkg, 70, dtype)
    b = a.copy()
    try:
        xb, Pb = rounded(a)
        ids = np.array([STRADDLER[dtype], 70, 1, 12, 45, 33, 64, 5][:m])
        rng = np.random.default_rng(m)
        zp, _, _ = O.obs_blocks(xb, ids)
        z = zp.T + rng.normal(0, [0.1, math.pi / 180], (m, 2)).T
        Hs, v = [], []
        for i, j in enumerate(ids):
            zpj, Hj = b.predict_observation(j)                           # slam_ekf_predict_observation: Hv, Hf as the device forms them
            Hs.append(Hj)
            v += [z[0, i] - zpj[0], O.mpi_to_pi(z[1, i] - zpj[1])]
        H = np.vstack(Hs)
        b.update_linear(H, v, np.kron(np.eye(m), R2), innovation=True)
        a.update(z, R2, ids)
        xa, Pa = rounded(a)
        xg, Pg = held_to_the_bars(b, xa, Pa, Pb, dtype, f"innovation m={m}")
        xo, Po = O.update_sparse(xb, Pb, z, R2, ids)                     # and both agree with the oracle
        assert relerr(xg, xo) <= TOL[dtype]["x"] and relerr_cov(Pg, Po, np.diag(Pb)) <= TOL[dtype]["P"]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_difference_rows_agree_with_merge_landmarks_on_the_survivors(pkg, dtype):
    s = STRADDLER[dtype]
    pairs = [(3, 40), (7, s), (1, 70)]
    x, P = UR.designed_state("slam", 70, dtype, 1070)
    x = np.array(x)
    for p, q in pairs:                                                    # near duplicates: the constraint is a sane one
        x[MR.f(q):MR.f(q) + 2] = x[MR.f(p):MR.f(p) + 2] + 0.01
    Rc = np.array([[0.02, 0.005], [0.005, 0.03]])
    a = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=CAP)
    b = a.copy()
    try:
        xb, Pb = rounded(a)
        rows = []
        for p, q in pairs:
            rows += [{MR.f(p): 1.0, MR.f(q): -1.0}, {MR.f(p) + 1: 1.0, MR.f(q) + 1: -1.0}]
        b.update_linear(rows, np.zeros(6), np.kron(np.eye(3), Rc))
        a.merge_landmarks(pairs, Rc)
        gone = np.concatenate([[MR.f(q), MR.f(q) + 1] for _, q in pairs])
        keep = np.setdiff1d(np.arange(len(xb)), gone)
        xa, Pa = rounded(a)
        xg, Pg = b.download()
        check_side(b, Pg, "difference rows")
        ex, eP = relerr(xg[keep], xa), relerr_cov(Pg[np.ix_(keep, keep)], Pa, np.diag(Pb)[keep])
        print(f"linear merge {dtype}: x {ex:.3e} P {eP:.3e}")
        assert ex <= TOL[dtype]["x"] and eP <= TOL[dtype]["P"]
    finally:
        a.close()
        b.close()


# ---- 3. S not positive definite -------------------------------------------------------------------------------------------------
def certain_failure_index(Pb):
    """A state index i for which two identical rows e_i with R = 0 fail in ANY evaluation order: S = [a a; a a], l = a / sqrt(a),
    second pivot a - l^2.  Where l^2 >= a exactly, the pivot is <= 0 with or without a fused multiply-add; where l^2 < a by a
    rounding, a fused evaluation would leave a tiny positive pivot.  Decided in exact rational arithmetic."""
    for i in range(3, Pb.shape[0]):
        a = float(Pb[i, i])
        l = a / math.sqrt(a)
        if Fraction(l) ** 2 >= Fraction(a):
            return i
    raise AssertionError("no diagonal entry whose square root rounds up")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_singular_s_is_refused_and_leaves_the_state_bit_identical(pkg, dtype):
    st = make_state(pkg, 70, dtype)
    try:
        xb, Pb = rounded(st)
        good = [{0: 1.0}, {1: 1.0}]
        st.update_linear(good, xb[:2] + 0.05, np.eye(2) * 0.01)          # a valid call first: its panel is what a stale W1 would be
        xb, Pb = rounded(st)
        i = certain_failure_index(Pb)
        rows = [{i: 1.0}, {i: 1.0}]
        x0, P0, side0 = st.download("x"), st.download("cov"), st.landmark_blocks()
        L = pkg._lib
        ptr, idx, val = LR.csr(rows)
        z = np.array([xb[i] + 0.1, xb[i] + 0.1])
        Rz = np.zeros(4)
        out = np.full(4, 7.0)
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        for fn in (L.linear_lib().slam_ekf_linear_nis, L.linear_lib().slam_ekf_update_linear):
            rc = fn(st._h, 2, p(ptr, C.c_int32), p(idx, C.c_int32), p(val), p(z), p(Rz), 0, 0, p(out))
            assert rc == L.SLAM_E_NOTPD and "not positive definite" in L.last_error()
            ref = LR.gate(xb, Pb, LR.dense_H(len(xb), rows), z, np.zeros((2, 2)))[0]
            assert out[3] == 1 == ref[3] and out[0] == 0 and out[1] == 0 and out[2] <= 0
            assert _bits_eq(st.download("x"), x0) and _bits_eq(st.download("cov"), P0) and _bits_eq(st.landmark_blocks(), side0)
        with pytest.raises(pkg.NotPositiveDefinite):
            st.update_linear(rows, z, 0.0)
        assert _bits_eq(st.download("x"), x0) and _bits_eq(st.download("cov"), P0)
        # a following valid call works
        zg = xb[:2] - 0.03
        outg = st.update_linear(good, zg, np.eye(2) * 0.01)
        xo, Po, ref = LR.update(xb, Pb, LR.dense_H(len(xb), good), zg, np.eye(2) * 0.01)
        out_close(outg, ref, "after the refusal")
        held_to_the_bars(st, xo, Po, Pb, dtype, "after the refusal")
    finally:
        st.close()


# ---- 4. after a valid call: the packed blocks and the gating --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gating_follows_a_linear_update_in_grid_and_sweep_mode(pkg, dtype):
    """A grid built BEFORE the call must not be used after it: the means moved.  A landmark is surveyed 3 m from where the map had
    it, the vehicle gets a position fix, and the next association -- grid form and sweep form -- equals the oracle's on the
    downloaded state."""
    results = {}
    j = 120
    for mode in ("grid", "sweep"):
        st = make_state(pkg, 200, dtype)
        try:
            st.set_gate_mode(mode)
            xb, _ = rounded(st)
            ids = np.array([j, 5, 77, 200, STRADDLER[dtype]])
            z0 = O.obs_blocks(xb, ids)[0].T
            st.associate_vector(z0, R2, 4.0, 25.0)                        # the grid exists now
            st.fix_landmark(j, xb[LR.f(j):LR.f(j) + 2] + np.array([3.0, -1.0]), np.eye(2) * 1e-4)
            st.fix_position(xb[:2] + 0.2, np.eye(2) * 0.01)
            xg, Pg = rounded(st)
            check_side(st, st.download("cov"), mode)
            rng = np.random.default_rng(9)
            z = O.obs_blocks(xg, ids)[0].T + rng.normal(0, [0.05, 0.005], (len(ids), 2)).T
            z = np.hstack([z, [[500.0], [0.3]]])                          # and one that is nobody's
            zf, idf, zn = st.associate(z, R2, 4.0, 25.0)
            zfo, idfo, zno = O.associate_sparse(xg, Pg, z, R2, 4.0, 25.0)
            assert np.array_equal(idf, idfo) and np.array_equal(zf, zfo) and np.array_equal(zn, zno), (mode, idf, idfo)
            assert j in np.asarray(idf).reshape(-1).tolist() and zn.shape[1] >= 1      # the moved landmark is found where it is now
            assert st.gate_info()["form"] == mode
            results[mode] = (np.asarray(idf).copy(), st.download())
        finally:
            st.close()
    assert np.array_equal(results["grid"][0], results["sweep"][0])
    assert _bits_eq(results["grid"][1][0], results["sweep"][1][0]) and _bits_eq(results["grid"][1][1], results["sweep"][1][1])


# ---- 5. / 6. the predicts -------------------------------------------------------------------------------------------------------
def bicycle(x3, v, g, w, Q, dt):
    phi = float(x3[2])
    s, c = math.sin(g + phi), math.cos(g + phi)
    vts, vtc = v * dt * s, v * dt * c
    Gv = np.array([[1.0, 0.0, -vts], [0.0, 1.0, vtc], [0.0, 0.0, 1.0]])
    Gu = np.array([[dt * c, -vts], [dt * s, vtc], [dt * math.sin(g) / w, v * dt * math.cos(g) / w]])
    return np.array([x3[0] + vtc, x3[1] + vts, O.mpi_to_pi(phi + v * dt * math.sin(g) / w)]), Gv, Gu @ Q @ Gu.T


def owned_within(st, ref, xb, Pb, dtype, what):
    """The strip, P_vv and the pose inside the bound of the existing predict tests; everything else bit for bit."""
    xg, Pg = st.download()
    assert _bits_eq(xg[3:], xb[3:]), f"{what}: landmark means moved"
    assert _bits_eq(Pg, Pg.T), f"{what}: P is not symmetric"
    assert _bits_eq(Pg[3:, 3:], Pb[3:, 3:]), f"{what}: the map block changed"
    S.assert_within(Pg[3:, 0:3], ref["strip"], dtype, S.C_STRIP, what + " strip")
    S.assert_within(Pg[0:3, 0:3], ref["vv"], dtype, S.C_BLOCK, what + " P_vv")
    S.assert_within(xg[0:3], ref["x"], dtype, S.C_STRIP, what + " x")
    check_side(st, Pg, what)
    return xg, Pg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [0, 1, 70, 200])
def test_predict_linear_with_the_bicycle_jacobians_is_the_predict_kernel(pkg, dtype, N):
    v, g, w, dt = 7.5, 0.4, 4.0, 0.25
    a = make_state(pkg, N, dtype, heading=3.13)                          # crosses +pi
    b = a.copy()
    try:
        xb, Pb = a.download()
        ref = S.predict_ref(xb[:3].astype(np.float64), np.asarray(Pb[:, 0:3], dtype=np.float64), v, g, w, QF, dt)
        assert ref["wrapped"] == 1
        b.predict_linear(*bicycle(xb[:3].astype(np.float64), v, g, w, QF, dt))
        a.predict(v, g, w, QF, dt)
        xl, Pl = owned_within(b, ref, xb, Pb, dtype, f"predict_linear N={N}")
        xp, Pp = owned_within(a, ref, xb, Pb, dtype, f"predict N={N}")
        # two results inside one bound: they differ by at most twice it
        for got, other, key, c in ((Pl[3:, 0:3], Pp[3:, 0:3], "strip", S.C_STRIP), (Pl[0:3, 0:3], Pp[0:3, 0:3], "vv", S.C_BLOCK),
                                   (xl[0:3], xp[0:3], "x", S.C_STRIP)):
            r, mag = ref[key]
            lim = 2 * (S.U_T[dtype] * np.abs(r) + c * S.C_FACTOR * S.EPS53 * mag)
            assert np.all(np.abs(S._ld(got) - S._ld(other)) <= lim), (N, key)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [0, 1, 70, 200])
def test_predict_odometry_against_the_reference(pkg, dtype, N):
    st = make_state(pkg, N, dtype, heading=3.0)
    try:
        for d, wrapped in (([0.8, -0.15, 0.3], 1), ([0.5, 0.1, -0.2], -1), ([-0.4, 0.3, -0.4], 0)):      # across +pi, back across -pi, neither
            xb, Pb = st.download()
            x3, col = xb[:3].astype(np.float64), np.asarray(Pb[:, 0:3], dtype=np.float64)
            ref = LR.odometry_pairs(x3, col, d, Q3)
            assert ref["wrapped"] == wrapped, (d, ref["wrapped"])
            x64, P64 = LR.predict_odometry(xb.astype(np.float64), np.asarray(Pb, dtype=np.float64), d, Q3)
            assert np.max(np.abs(x64[:3] - ref["x"][0].astype(np.float64))) <= 1e-12 * 10
            assert np.max(np.abs(P64[:, 0:3] - np.vstack([ref["vv"][0], ref["strip"][0]]).astype(np.float64))) <= 1e-12 * max(1.0, float(np.max(np.abs(P64))))
            st.predict_odometry(d, Q3)
            owned_within(st, ref, xb, Pb, dtype, f"predict_odometry N={N} d={d}")
    finally:
        st.close()


# ---- the one-line conveniences --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_conveniences_are_update_linear_with_their_rows(pkg, dtype):
    s = STRADDLER[dtype]
    st = make_state(pkg, 70, dtype, heading=-3.1)
    try:
        n = st.n
        steps = [
            ("fix_position", lambda xb: (st.fix_position(xb[:2] + 0.1, R2 * 4), [{0: 1.0}, {1: 1.0}], xb[:2] + 0.1, R2 * 4, 0)),
            ("fix_heading", lambda xb: (st.fix_heading(3.12, 0.01), [{2: 1.0}], [3.12], [[0.01]], 1)),
            ("fix_landmark", lambda xb: (st.fix_landmark(s, xb[LR.f(s):LR.f(s) + 2] - 0.2, R2), [{LR.f(s): 1.0}, {LR.f(s) + 1: 1.0}],
                                         xb[LR.f(s):LR.f(s) + 2] - 0.2, R2, 0)),
            ("constrain_landmarks", lambda xb: (st.constrain_landmarks(3, 70, xb[LR.f(70):LR.f(70) + 2] - xb[LR.f(3):LR.f(3) + 2] + 0.05, 0.0),
                                                [{LR.f(70): 1.0, LR.f(3): -1.0}, {LR.f(70) + 1: 1.0, LR.f(3) + 1: -1.0}],
                                                xb[LR.f(70):LR.f(70) + 2] - xb[LR.f(3):LR.f(3) + 2] + 0.05, np.zeros((2, 2)), 0)),
        ]
        for name, step in steps:
            xb, Pb = rounded(st)
            out, rows, z, Rm, mask = step(xb)
            xo, Po, ref = LR.update(xb, Pb, LR.dense_H(n, rows), z, Rm, wrap_mask=mask)
            out_close(out, ref, name)
            held_to_the_bars(st, xo, Po, Pb, dtype, name)
    finally:
        st.close()


# ---- 7. the simulator with position fixes ---------------------------------------------------------------------------------------
def test_sim_with_position_fixes_is_no_worse_than_without(pkg, golden_dir):
    """30 steps of the golden course, a fix every 5th step from a receiver of sigma 0.05 m -- below the drift the unaided filter
    has by then, so the fixed run ends closer to the truth; the trace of P_vv can only shrink under an update."""
    Sm = pkg.sim
    wp = Sm.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    got = {}
    for fe in (0, 5):
        st = pkg.EKFSlamState(Sm.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=40)
        try:
            log = Sm.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=2, max_steps=30, fix_every=fe, fix_sigma=0.05)
            assert len(log.true_track) == 30 and len(log.fixes) == (6 if fe else 0)
            err = float(np.linalg.norm(log.true_track[-1][:2] - log.slam_track[-1][:2]))
            got[fe] = (err, float(np.trace(st.get_block(0, 0, 3, 3))), np.array(log.true_track), np.array(log.controls))
        finally:
            st.close()
    print(f"linear sim: pose error {got[0][0]:.4f} -> {got[5][0]:.4f}, trace P_vv {got[0][1]:.3e} -> {got[5][1]:.3e}")
    assert np.array_equal(got[0][2], got[5][2]) and np.array_equal(got[0][3], got[5][3])      # the same seeded run
    assert got[5][0] <= got[0][0] and got[5][1] <= got[0][1]
