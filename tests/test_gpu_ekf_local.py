"""Compressed local-area updates on the device (slam_ekf_local_*, include/ext/slamhip_local.h) against tests/local_ref.py and the
fp64 oracle, both dtypes.

Two checks are made wherever an area with steps is closed:
  (1) close against the EXACT five steps of the header applied to close's own inputs -- the global state as uploaded, the local
      state and phi, psi, theta as the device holds them just before close -- entry by entry inside the header's bound
      (LF.close_bound); x_a and P_aa bit for bit.  This is the derived bound; nothing in it is tuned.
  (2) the result against the fp64 oracle's full filter on the same sequence.  What (1) does not cover is the rounding of the local
      steps themselves, which is the PRODUCT's (slam_ekf_predict / _update / _augment on a small handle) and has no per-entry bound
      over a sequence; the allowance for it is the one smoke() makes for the product's own sequence, STEP_TOL[dtype] max|ref|, added
      to the bound of (1).  The product's full path on the same sequence is measured against the same oracle beside it.
phi, psi, theta are held against tests/local_ref.py separately, step by step from the device's own local state, so a failure says
which half is wrong."""
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import local_ref as LF

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
NP = {"f32": np.float32, "f64": np.float64}
STEP_TOL = {"f32": 2e-4, "f64": 1e-9}          # smoke()'s tolerances for a product sequence, relative to max|ref|
ACC_TOL = 1e-8                                  # accumulators: double on both sides (2^-53), amplified by the conditioning of S; 1e-8 leaves it a factor 1e8
R = np.array([[0.01, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.25, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
WB, DT = 4.0, 0.025


def spd_state(N, seed=7):
    """A fully correlated SPD state, as smoke() builds it."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[50.0, 50.0, 0.3], rng.uniform(10, 90, 2 * N)])
    A = rng.normal(0, 0.2, (n, 8))
    return x, A @ A.T + 0.01 * np.eye(n)


def upload(pkg, N, dtype, max_landmarks, seed=7):
    x, P = spd_state(N, seed)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=max_landmarks)
    xr, Pr = st.download()
    return st, xr.astype(np.float64), np.array(Pr, dtype=np.float64)


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def observe(x, ids, rng):
    z = np.zeros((2, len(ids)))
    for i, j in enumerate(ids):
        z[:, i] = O.predict_observation(x, j)[0] + rng.normal(0, [0.05, 0.005])
    return z


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def run_sequence(pkg, dtype, N, ids, steps, max_landmarks, max_local=None, seed=7):
    """The steps -- ("p", v, g), ("u", local ids), ("a", new observations) -- in an area over ids, closed; beside them the product's
    calls on a second global handle and the oracle.  Asserts checks (1) and (2) and the accumulators; returns the ratios."""
    st, x0, P0 = upload(pkg, N, dtype, max_landmarks, seed)
    prod, _, _ = upload(pkg, N, dtype, max_landmarks, seed)
    rng = np.random.default_rng(100 + N)
    xo, Po = np.array(x0), np.array(P0)
    gids = list(ids)
    out = {}
    try:
        area = st.local(ids, max_local=max_local)
        n0 = 3 + 2 * len(ids)
        phi, psi, theta = np.eye(n0), np.zeros((n0, n0)), np.zeros(n0)
        for s in steps:
            xl, Pl = area.state.download()
            xl, Pl = xl.astype(np.float64), np.array(Pl, dtype=np.float64)
            if s[0] == "p":
                area.predict(s[1], s[2], WB, Q, DT)
                prod.predict(s[1], s[2], WB, Q, DT)
                xo, Po = O.predict_sparse(xo, Po, s[1], s[2], WB, Q, DT)
                phi = LF.acc_predict(phi, xl[2], s[1], s[2], DT)
            elif s[0] == "u":
                g = [gids[j - 1] for j in s[1]]
                z = observe(xo, g, rng)
                area.update(z, R, s[1])
                prod.update(z, R, g)
                xo, Po = O.update_sparse(xo, Po, z, R, g)
                phi, psi, theta = LF.acc_update(phi, psi, theta, xl, Pl, z, s[1], R, NP[dtype])
            else:
                zn = np.asarray(s[1], dtype=float).reshape(2, -1)
                area.add_features(zn, R)
                prod.add_features(zn, R)
                xo, Po = O.add_features_sparse(xo, Po, zn, R)
                gids += [(len(xo) - 3) // 2 - zn.shape[1] + 1 + i for i in range(zn.shape[1])]
                phi = LF.acc_augment(phi, xl[2], zn)
            dphi, dpsi, dtheta = area.accumulators()
            for name, got, want in (("phi", dphi, phi), ("psi", dpsi, psi), ("theta", dtheta, theta)):
                assert got.shape == want.shape, (name, s[0], got.shape, want.shape)
                err = float(np.max(np.abs(got - want))) if want.size else 0.0
                assert err <= ACC_TOL * max(1.0, float(np.max(np.abs(want)))), (dtype, name, s[0], err)
        assert np.array_equal(area.global_ids(), np.array(gids, dtype=np.int32))
        xl, Pl = area.state.download()
        dphi, dpsi, dtheta = area.accumulators()
        first = area.close()
        assert first == N + 1 and st.N == len(gids) + (N - len(ids)) and not area.is_open
        xg, Pg = st.download()
        # (1) close against the exact close of its own inputs
        xe, Pe = LF.close(x0, P0, ids, xl.astype(np.float64), np.array(Pl, dtype=np.float64), dphi, dpsi, dtheta)
        Bx, BP = LF.close_bound(x0, P0, ids, len(xl), dphi, dpsi, dtheta, xe, Pe, NP[dtype])
        ex, eP = np.abs(xg.astype(np.float64) - xe), np.abs(np.array(Pg, dtype=np.float64) - Pe)
        l2g = LF.local_to_global(ids, len(x0), len(xl))
        assert bits_eq(xg[l2g], xl) and bits_eq(np.ascontiguousarray(Pg[np.ix_(l2g, l2g)]), np.ascontiguousarray(Pl))
        with np.errstate(divide="ignore", invalid="ignore"):
            rx = np.where(Bx > 0, ex / Bx, np.where(ex > 0, np.inf, 0.0))
            rP = np.where(BP > 0, eP / BP, np.where(eP > 0, np.inf, 0.0))
        out["close_x"], out["close_P"] = float(rx.max()), float(rP.max())
        print(f"local_bounds {dtype} N={N} n0={n0}: close error / bound  x {out['close_x']:.3g}  P {out['close_P']:.3g}")
        assert out["close_x"] <= 1.0 and out["close_P"] <= 1.0, (dtype, out)
        assert np.array_equal(Pg, Pg.T)
        # (2) the whole sequence against the oracle, beside the product's full path
        sx, sP = STEP_TOL[dtype] * np.max(np.abs(xo)), STEP_TOL[dtype] * np.max(np.abs(Po))
        ox, oP = np.abs(xg - xo), np.abs(Pg - Po)
        out["oracle_x"], out["oracle_P"] = float(np.max(ox / (Bx + sx))), float(np.max(oP / (BP + sP)))
        xp, Pp = prod.download()
        out["prod_x"], out["prod_P"] = float(np.max(np.abs(xp - xo) / (Bx + sx))), float(np.max(np.abs(Pp - Po) / (BP + sP)))
        print(f"local_bounds {dtype} N={N} n0={n0}: oracle error / (bound + step allowance)  area x {out['oracle_x']:.3g} P {out['oracle_P']:.3g}"
              f"   product's full path x {out['prod_x']:.3g} P {out['prod_P']:.3g}   (max rel: area {rel(Pg, Po):.3g}, product {rel(Pp, Po):.3g})")
        assert out["oracle_x"] <= 1.0 and out["oracle_P"] <= 1.0, (dtype, out)
        # the side array follows the matrix
        blocks = st.landmark_blocks()
        d = np.diag(Pg)[3:]
        assert bits_eq(np.ascontiguousarray(blocks[0]), np.ascontiguousarray(d[0::2])) and bits_eq(np.ascontiguousarray(blocks[2]), np.ascontiguousarray(d[1::2]))
        area.destroy()
    finally:
        st.close()
        prod.close()
    return out


# ---- no-op and select ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_area_without_steps_and_an_aborted_area_leave_the_global_state_bit_for_bit(pkg, dtype):
    st, _, _ = upload(pkg, 70, dtype, 100)
    try:
        x0, P0 = st.download()
        side0 = st.landmark_blocks()
        ids = [63, 5, 70, 1, 33]
        area = st.local(ids)
        sel = st.select(ids, max_landmarks=area.max_local)
        xs, Ps = sel.download()
        xl, Pl = area.state.download()
        assert bits_eq(xl, xs) and bits_eq(Pl, Ps) and bits_eq(area.state.landmark_blocks(), sel.landmark_blocks())     # open IS select
        sel.close()
        phi, psi, theta = area.accumulators()
        assert np.array_equal(phi, np.eye(13)) and not psi.any() and not theta.any()
        assert area.info() == {"open": 1, "n0": 13, "n_a": 13, "added": 0, "steps": 0, "N_open": 70, "max_local": 69}
        assert area.close() == 71
        x1, P1 = st.download()
        assert bits_eq(x1, x0) and bits_eq(P1, P0) and bits_eq(st.landmark_blocks(), side0) and st.N == 70
        # steps, then abort
        area.open(ids)
        area.predict(7.5, 0.1, WB, Q, DT)
        area.update(observe(x0.astype(np.float64), [63, 70], np.random.default_rng(1)), R, [1, 3])
        area.add_features(np.array([[25.0], [0.3]]), R)
        assert area.info()["steps"] == 3 and area.info()["added"] == 1
        area.abort()
        x1, P1 = st.download()
        assert bits_eq(x1, x0) and bits_eq(P1, P0) and bits_eq(st.landmark_blocks(), side0) and st.N == 70 and not area.is_open
        with st.local(ids) as a2:                                          # the context manager: abort on an exception
            try:
                with st.local([2]) as a3:
                    a3.predict(7.5, 0.1, WB, Q, DT)
                    raise KeyError("leave")
            except KeyError:
                pass
            assert not a3.is_open
        assert not a2.is_open
        x1, P1 = st.download()
        assert bits_eq(x1, x0) and bits_eq(P1, P0)
        area.destroy()
    finally:
        st.close()


# ---- equivalence -----------------------------------------------------------------------------------------------------------------
EQ_STEPS = [("p", 7.5, 0.1), ("u", [2, 5, 7]), ("p", 7.0, -0.05), ("a", [[30.0, 22.0], [0.4, -0.7]]), ("u", [1, 9]), ("p", 7.5, 0.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_area_is_equivalent_to_the_full_filter(pkg, dtype):
    out = run_sequence(pkg, dtype, 24, [19, 3, 11, 24, 1, 8, 15], EQ_STEPS, 64)
    assert out["close_P"] > 0                                             # the bound was exercised: close did arithmetic


# ---- tile edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["63_in_A", "63_in_B", "grow_spare", "grow_exact"])
def test_tile_edges(pkg, dtype, case):
    steps = [("p", 7.5, 0.1), ("u", [1, 3]), ("p", 7.0, 0.05)]
    if case == "63_in_A":      # n = 143: landmark 63 sits at states 127, 128, across the edge of the first 128 (and second 64) tile
        run_sequence(pkg, dtype, 70, [63, 10, 64, 2], steps, 100)
    elif case == "63_in_B":
        run_sequence(pkg, dtype, 70, [62, 10, 64, 2], steps, 100)
    else:                      # n = 127 -> 129: close grows the state across a tile row; the capacity has a spare tile row, or fits exactly
        grow = [("p", 7.5, 0.1), ("a", [[28.0], [0.5]]), ("u", [4, 2]), ("p", 7.0, 0.0)]
        run_sequence(pkg, dtype, 62, [62, 7, 31], grow, 200 if case == "grow_spare" else 63)


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_accumulator_kernels_at_their_threshold(pkg, dtype):
    """k = 2m <= 128 takes the LDS form of the accumulator launch, k > 128 the form with its scratch in global memory (and the
    local update itself leaves the fused factor launch at the same k): 64 and 65 observations in one area."""
    ids = [int(j) for j in np.random.default_rng(9).permutation(70) + 1]
    run_sequence(pkg, dtype, 70, ids, [("p", 7.5, 0.1), ("u", list(range(1, 65))), ("u", list(range(1, 66))), ("p", 7.0, 0.0)], 100)


# ---- edge sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_sets(pkg, dtype):
    # the vehicle alone, predicts only: P_vb follows the chain of Gv (run_sequence holds phi against it and close against the oracle)
    run_sequence(pkg, dtype, 12, [], [("p", 7.5, 0.1), ("p", 7.0, -0.2), ("p", 6.0, 0.3)], 64, max_local=4)
    # A = every landmark, B empty
    run_sequence(pkg, dtype, 9, list(range(9, 0, -1)), EQ_STEPS, 64)
    # two areas in sequence with overlapping ids, the second over what the first left (its appended landmark included)
    st, x0, P0 = upload(pkg, 24, dtype, 64)
    try:
        rng = np.random.default_rng(3)
        xo, Po = np.array(x0), np.array(P0)
        for ids in ([4, 9, 17], [17, 25, 2, 9]):
            with st.local(ids) as area:
                area.predict(7.5, 0.1, WB, Q, DT)
                xo, Po = O.predict_sparse(xo, Po, 7.5, 0.1, WB, Q, DT)
                z = observe(xo, [ids[0], ids[1]], rng)
                area.update(z, R, [1, 2])
                xo, Po = O.update_sparse(xo, Po, z, R, [ids[0], ids[1]])
                if len(ids) == 3:
                    area.add_features(np.array([[26.0], [-0.4]]), R)
                    xo, Po = O.add_features_sparse(xo, Po, np.array([[26.0], [-0.4]]), R)
        xg, Pg = st.download()
        assert st.N == 25 and rel(xg, xo) <= STEP_TOL[dtype] and rel(Pg, Po) <= STEP_TOL[dtype]
    finally:
        st.close()


# ---- not positive definite -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_failed_local_update_leaves_the_local_state_and_the_accumulators_bit_for_bit(pkg, dtype):
    """The construction of tests/test_gpu_ekf_linear.py -- the same row twice -- in the only form a range-bearing update can take
    it: one landmark observed twice, with the slightly negative R of tests/test_gpu_ekf.py making the failing pivot certain."""
    st, x0, _ = upload(pkg, 24, dtype, 64)
    try:
        area = st.local([19, 3, 11])
        area.predict(7.5, 0.1, WB, Q, DT)
        area.update(observe(x0, [19], np.random.default_rng(2)), R, [1])      # the accumulators are not trivial
        xl, Pl = area.state.download()
        acc = area.accumulators()
        zp = O.predict_observation(xl.astype(np.float64), 2)[0]
        z = np.stack([zp + [0.01, 0.0005], zp - [0.01, 0.0005]], axis=1)
        with pytest.raises(pkg.NotPositiveDefinite):
            area.update(z, -1e-5 * np.eye(2), [2, 2])
        x1, P1 = area.state.download()
        assert bits_eq(x1, xl) and bits_eq(P1, Pl)
        assert all(bits_eq(a, b) for a, b in zip(area.accumulators(), acc))
        area.update(z[:, :1], R, [2])                                        # a following valid update works
        assert not bits_eq(area.accumulators()[0], acc[0])
        area.abort()
        area.destroy()
    finally:
        st.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _code(pkg, fn, *args):
    with pytest.raises(pkg.SlamHipError) as ei:
        fn(*args)
    return ei.value.code


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(pkg, dtype):
    L = pkg._lib
    BAD, CAP = L.SLAM_E_BADARG, L.SLAM_E_CAPACITY
    st, x0, _ = upload(pkg, 24, dtype, 25)
    try:
        area = pkg.LocalArea(st, None, max_local=4)
        z1 = np.array([[20.0], [0.1]])
        # nothing open
        assert _code(pkg, area.predict, 7.5, 0.1, WB, Q, DT) == BAD and "no area is open" in L.last_error()
        assert _code(pkg, area.update, z1, R, [1]) == BAD
        assert _code(pkg, area.add_features, z1, R) == BAD
        assert _code(pkg, area.close) == BAD and _code(pkg, area.abort) == BAD and _code(pkg, area.accumulators) == BAD
        # open
        assert _code(pkg, area.open, [1, 2, 2]) == BAD and _code(pkg, area.open, [0]) == BAD and _code(pkg, area.open, [25]) == BAD
        assert _code(pkg, area.open, [1, 2, 3, 4, 5]) == BAD and "max_local" in L.last_error()
        assert not area.is_open
        area.open([7, 9, 11])
        assert _code(pkg, area.open, [1]) == BAD and "already open" in L.last_error()
        # update
        xl, Pl = area.state.download()
        acc = area.accumulators()
        assert _code(pkg, area.update, z1, R, [4]) == BAD and _code(pkg, area.update, z1, R, [0]) == BAD
        assert _code(pkg, area.update, z1, R, [1], "joseph") == BAD and "CHOLESKY" in L.last_error()
        # capacity, the local one: 3 + 2 > 4
        assert _code(pkg, area.add_features, np.array([[20.0, 21.0], [0.1, 0.2]]), R) == CAP and "max_local" in L.last_error()
        area.add_features(z1, R)                                             # 4 of 4 locally, 25 of 25 globally
        assert _code(pkg, area.add_features, z1, R) == CAP
        x1, P1 = area.state.download()
        assert area.info()["added"] == 1 and x1.shape == (11,)
        area.abort()
        # capacity, the global one: room locally, none in the global handle
        big = pkg.LocalArea(st, [7], max_local=8)
        big.add_features(z1, R)
        xl, Pl = big.state.download()
        acc = big.accumulators()
        assert _code(pkg, big.add_features, z1, R) == CAP and "global capacity" in L.last_error()
        x1, P1 = big.state.download()
        assert bits_eq(x1, xl) and bits_eq(P1, Pl) and all(bits_eq(a, b) for a, b in zip(big.accumulators(), acc))
        # the global N changed under the area
        st.remove_landmarks([24])
        assert _code(pkg, big.close) == BAD and "N changed" in L.last_error() and big.is_open
        big.abort()
        big.destroy()
        area.destroy()
    finally:
        st.close()


# ---- sim -------------------------------------------------------------------------------------------------------------------------
def seeded_start(S, wp):
    """The course's initial pose plus six landmarks 80 m away (never in sensor range, never inside an area), correlated with the
    vehicle: B is not empty and close has work to do from the first area on."""
    p0 = S.initial_pose(wp)
    rng = np.random.default_rng(4)
    far = np.array([[p0[0] + 80 * math.cos(a), p0[1] + 80 * math.sin(a)] for a in np.linspace(0, 2 * math.pi, 6, endpoint=False)])
    A = rng.normal(0, 0.05, (15, 6))
    return np.concatenate([p0, far.reshape(-1)]), A @ A.T + 1e-4 * np.eye(15)


_ORACLE_SIM = {}


def oracle_sim(S, golden_dir):
    """The oracle's two runs (without and with the area), made once for both dtypes and left unchanged."""
    if not _ORACLE_SIM:
        wp = S.get_waypoints(os.path.join(golden_dir, "course1.txt"))
        cfg = np.load(os.path.join(golden_dir, "config1.npz"))
        lms, seed = cfg["landmarks"], int(cfg["seed"][1])
        x0, P0 = seeded_start(S, wp)
        ra, rb = LF.RefFilter(x0, P0), LF.RefFilter(x0, P0)
        la = S.sim(ra, wp, lms, seed=seed, nlaps=1, max_steps=60)
        lb = S.sim(rb, wp, lms, seed=seed, nlaps=1, max_steps=60, local_radius=34.0)
        _ORACLE_SIM.update(wp=wp, lms=lms, seed=seed, x0=x0, P0=P0, ra=ra, la=la, lb=lb)
    return _ORACLE_SIM


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_with_a_local_radius_makes_the_plain_loop_s_decisions(pkg, golden_dir, dtype):
    """60 steps of course1 from seeded_start, radius 34 m (areas are closed and reopened on the way).  The condition on the inputs
    -- the oracle alone makes the same decisions with and without the area -- is checked here on the CPU as well."""
    S = pkg.sim
    o = oracle_sim(S, golden_dir)
    wp, lms, seed, x0, P0, ra, la, lb = (o[k] for k in ("wp", "lms", "seed", "x0", "P0", "ra", "la", "lb"))
    assert la.assoc == lb.assoc and len(lb.areas) >= 3 and sum(len(a[0]) for a in la.assoc) > 20
    ga = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=40)
    gb = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=40)
    try:
        ka = S.sim(ga, wp, lms, seed=seed, nlaps=1, max_steps=60)
        kb = S.sim(gb, wp, lms, seed=seed, nlaps=1, max_steps=60, local_radius=34.0)
        assert ka.assoc == kb.assoc == la.assoc and kb.areas == lb.areas
        assert np.array_equal(np.array(ka.controls), np.array(kb.controls)) and np.array_equal(np.array(ka.true_track), np.array(kb.true_track))
        xa, Pa = ga.download()
        xb, Pb = gb.download()
        assert ga.N == gb.N == ra.N
        for got in ((xa, Pa), (xb, Pb)):                                   # both runs against the oracle, under the sequence allowance
            assert rel(got[0], ra.x) <= STEP_TOL[dtype] and rel(got[1], ra.cov) <= STEP_TOL[dtype]
        assert rel(np.array(kb.slam_track), np.array(ka.slam_track)) <= STEP_TOL[dtype]
    finally:
        ga.close()
        gb.close()
