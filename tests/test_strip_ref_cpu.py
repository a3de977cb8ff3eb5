"""Pins tests/strip_ref.py (the entry-wise reference and bound the GPU tests of csrc/ekf_strip.hip use) without a GPU:
against the literal dense oracle and its sparse twin, against the hand-derived KAT-3 / 4 / 10 / 12, with a NumPy emulation
of the kernels' arithmetic (the bound holds for fp64 arithmetic rounded once, and does NOT hold for `float` arithmetic),
and the storage layout against a direct enumeration of the tiles."""
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import kat_vectors as KV
from tests import strip_ref as S

# full symmetric matrices with non-zero off-diagonals (correlation 0.4 / -0.3)
RF = np.array([[0.1 ** 2, 0.4 * 0.1 * (math.pi / 180)], [0.4 * 0.1 * (math.pi / 180), (math.pi / 180) ** 2]])
QF = np.array([[0.5 ** 2, -0.3 * 0.5 * (3 * math.pi / 180)], [-0.3 * 0.5 * (3 * math.pi / 180), (3 * math.pi / 180) ** 2]])


def _state(rng, N, rank=6):
    n = 3 + 2 * N
    x = np.concatenate([[50.0, 50.0, rng.uniform(-3, 3)], rng.uniform(5, 95, 2 * N)])
    A = rng.normal(0, 0.2, (n, rank))
    P = A @ A.T + 0.01 * np.eye(n)
    return x, (P + P.T) / 2


def test_extended_precision_is_what_the_bound_assumes():
    """The fallback to a float64 reference is explicit: it doubles the slack.  Here long double has a 64-bit significand."""
    assert S.EXTENDED == (np.finfo(np.longdouble).nmant >= 63)
    assert S.C_FACTOR == (1.0 if S.EXTENDED else 2.0)
    assert S.C_STRIP == 16.0 and S.C_BLOCK == 32.0 and S.C_BLOCK <= S.C_LIMIT == 64.0


@pytest.mark.parametrize("N", [0, 1, 35, 200])
def test_predict_ref_against_the_oracles(N):
    rng = np.random.default_rng(100 + N)
    for case, (v, g, dt) in enumerate([(7.5, 0.1, 0.025), (-3.0, -0.4, 0.1), (0.0, 0.3, 0.025), (8.0, 0.0, 0.025)]):
        x, P = _state(rng, N)
        ref = S.predict_ref(x[:3], P[:, 0:3], v, g, 4.0, QF, dt)
        for fn in (O.predict, O.predict_sparse):
            xo, Po = fn(x.copy(), P.copy(), v, g, 4.0, QF, dt)
            what = f"{fn.__name__} N={N} case {case}"
            S.assert_within(Po[3:, 0:3], ref["strip"], "f64", S.C_STRIP, "strip: " + what)
            S.assert_within(Po[0:3, 3:].T, ref["strip"], "f64", S.C_STRIP, "strip: mirror " + what)
            S.assert_within(Po[0:3, 0:3], ref["vv"], "f64", S.C_BLOCK, "vv: " + what)
            S.assert_within(xo[0:3], ref["x"], "f64", S.C_STRIP, "x: " + what)
            # ... and predict owns nothing else
            assert np.array_equal(xo[3:], x[3:]) and np.array_equal(Po[3:, 3:], P[3:, 3:]), what


@pytest.mark.parametrize("nn", [1, 2, 23])
@pytest.mark.parametrize("N", [0, 1, 35, 200])
def test_add_features_ref_against_the_oracles(N, nn):
    rng = np.random.default_rng(1000 * N + nn)
    x, P = _state(rng, N)
    n0 = 3 + 2 * N
    zn = np.vstack([rng.uniform(5, 400, nn), rng.uniform(-4, 4, nn)])
    ref = S.add_features_ref(x[:3], P[:, 0:3], zn, RF)
    for fn in (O.add_features, O.add_features_sparse):
        xo, Po = fn(x, P, zn, RF)
        what = f"{fn.__name__} N={N} nn={nn}"
        assert xo.shape == (n0 + 2 * nn,) and Po.shape == (n0 + 2 * nn,) * 2
        S.assert_within(Po[n0:, :n0], ref["cross"], "f64", S.C_STRIP, "cross: " + what)
        S.assert_within(Po[:n0, n0:].T, ref["cross"], "f64", S.C_STRIP, "cross: mirror " + what)
        S.assert_within(Po[n0:, n0:], ref["new"], "f64", S.C_BLOCK, "new: " + what)
        S.assert_within(xo[n0:], ref["x"], "f64", S.C_STRIP, "x: " + what)
        assert np.array_equal(xo[:n0], x) and np.array_equal(Po[:n0, :n0], P), what


def test_hand_derived_known_answers_through_the_reference():
    """KAT-3, KAT-4, KAT-10, KAT-12 (tests/kat_vectors.py, tests/test_oracle_kat.py): closed forms worked on paper.  Their
    own float64 evaluation is a handful of roundings, so they sit inside the same bound."""
    s3 = (3 * math.pi / 180) ** 2
    Q3 = np.diag([0.25, s3])
    # KAT-3: predict from x = 0, P = 0
    ref = S.predict_ref(np.zeros(3), np.zeros((3, 3)), 8.0, 0.0, 4.0, Q3, 0.025)
    S.assert_within(np.array([[0.025 ** 2 * 0.25, 0, 0], [0, 0.2 ** 2 * s3, 0.2 * 0.05 * s3], [0, 0.2 * 0.05 * s3, 0.05 ** 2 * s3]]),
                    ref["vv"], "f64", S.C_BLOCK, "vv: KAT-3")
    S.assert_within(np.array([0.2, 0.0, 0.0]), ref["x"], "f64", S.C_STRIP, "x: KAT-3")
    assert ref["strip"][0].shape == (0, 3) and ref["wrapped"] == 0
    # KAT-4: add_features from x = 0, P = 0, z = (10, 0)
    ref = S.add_features_ref(np.zeros(3), np.zeros((3, 3)), np.array([[10.0], [0.0]]), KV.R)
    S.assert_within(np.diag([KV.R[0, 0], 100 * KV.R[1, 1]]), ref["new"], "f64", S.C_BLOCK, "new: KAT-4")
    S.assert_within(np.array([10.0, 0.0]), ref["x"], "f64", S.C_STRIP, "x: KAT-4")
    assert np.all(ref["cross"][0] == 0) and np.all(ref["cross"][1] == 0)       # mag 0: the entries must be exactly zero
    # KAT-10: add_features with a vehicle covariance and an existing landmark
    x, P, zn, xp, Pp = KV.kat10()
    ref = S.add_features_ref(x[:3], P[:, 0:3], zn, KV.R)
    S.assert_within(Pp[5:, :5], ref["cross"], "f64", S.C_STRIP, "cross: KAT-10")
    S.assert_within(Pp[5:, 5:], ref["new"], "f64", S.C_BLOCK, "new: KAT-10")
    S.assert_within(xp[5:], ref["x"], "f64", S.C_STRIP, "x: KAT-10")
    # KAT-12: predict with heading, steering, coupled covariance and a landmark
    x, P, (v, g, w, Qk, dtk), xp, Pp = KV.kat12()
    ref = S.predict_ref(x[:3], P[:, 0:3], v, g, w, Qk, dtk)
    S.assert_within(Pp[3:, 0:3], ref["strip"], "f64", S.C_STRIP, "strip: KAT-12")
    S.assert_within(Pp[0:3, 0:3], ref["vv"], "f64", S.C_BLOCK, "vv: KAT-12")
    S.assert_within(xp[0:3], ref["x"], "f64", S.C_STRIP, "x: KAT-12")


def test_heading_wraps_exactly_once():
    for phi, g, sign in ((math.pi - 5e-4, 0.3, 1), (-math.pi + 5e-4, -0.3, -1), (3.0, 0.3, 0), (math.pi - 5e-4, -0.3, 0)):
        ref = S.predict_ref(np.array([1.0, 2.0, phi]), np.zeros((3, 3)), 8.0, g, 4.0, QF, 0.025)
        want = O.mpi_to_pi(phi + 8.0 * 0.025 * math.sin(g) / 4.0)
        assert ref["wrapped"] == sign and -math.pi <= float(ref["x"][0][2]) <= math.pi
        S.assert_within(np.array([want]), (ref["x"][0][2:], ref["x"][1][2:]), "f64", S.C_STRIP, "x: wrap")


# ---- the bound's selectivity: a NumPy emulation of predict_kernel's strip ---------------------------------------------------
def _emulated_strip(x3, col, v, g, dt, arith, store):
    """predict_kernel's strip (ekf_strip.hip:281-294) with ALL its arithmetic -- the heading's sine and cosine, v dt, the
    products and the sums -- in `arith`, and ONE rounding to `store`."""
    phi, v, g, dt = arith(x3[2]), arith(v), arith(g), arith(dt)
    sn, cs = np.sin(g + phi), np.cos(g + phi)
    vts, vtc = v * dt * sn, v * dt * cs
    assert vts.dtype == arith
    p0, p1, p2 = (col[3:, k].astype(arith) for k in range(3))
    out = np.stack([p0 - vts * p2, p1 + vtc * p2, p2], axis=1)
    assert out.dtype == arith
    return out.astype(store)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_bound_admits_fp64_arithmetic_and_rejects_float_arithmetic(dtype):
    """200 random predict calls at N = 500.  The kernel's arithmetic (double, one rounding to the state type) stays inside
    the bound with the committed c; the same strip computed in `float` leaves it on at least 10 % of the entries, even
    with c at its limit of 64."""
    rng = np.random.default_rng(7 + (dtype == "f64"))
    T = S.NP_DTYPE[dtype]
    N = 500
    worst, total, outside = 0.0, 0, 0
    for _call in range(200):
        x, P = _state(rng, N, rank=4)
        x3 = x[:3].astype(T).astype(np.float64)
        col = P[:, 0:3].astype(T).astype(np.float64)                  # the state as the device holds it
        # speed and steering over the vehicle's range; dt from one control step of the sim (0.025 s) to a coarse one-second
        # step, log-uniform: the arithmetic type enters through the term v dt sin() p2 alone, so its size against the
        # entry decides how often `float` shows
        v, g, dt = rng.uniform(-10, 10), rng.uniform(-0.5, 0.5), float(np.exp(rng.uniform(math.log(0.025), 0.0)))
        ref = S.predict_ref(x3, col, v, g, 4.0, QF, dt)
        good = _emulated_strip(x3, col, v, g, dt, np.float64, T)
        worst = max(worst, S.assert_within(good, ref["strip"], dtype, S.C_STRIP, "strip: fp64 emulation"))
        bad = _emulated_strip(x3, col, v, g, dt, np.float32, T)
        q = S.ratio(bad, ref["strip"][0], ref["strip"][1], dtype)      # all three columns (the third is a plain copy)
        total += q.size
        outside += int(np.sum(q > S.C_LIMIT))
    print(f"{dtype}: fp64 emulation needs c = {worst:.2f}; float arithmetic outside c = 64 on {100.0 * outside / total:.1f} %")
    assert worst <= S.C_STRIP
    assert outside >= 0.10 * total


# ---- storage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 128])
def test_p_off_against_a_direct_enumeration_of_the_tiles(E):
    """device_math.h:106-139: band after band, inside a band tile I = J, J + 1, ..., each tile E x E column-major."""
    L = E.bit_length() - 1
    T = 3
    ld = T * E
    nxt = 0
    seen = np.zeros(T * (T + 1) // 2 * E * E, dtype=bool)
    for J in range(T):
        for I in range(J, T):
            for c in range(E):
                got = S.p_off(ld, L, I * E + np.arange(E), J * E + c)
                assert np.array_equal(got, nxt + np.arange(E)), (I, J, c)
                nxt += E
            seen[int(S.tile_base(I, J, T, L)):int(S.tile_base(I, J, T, L)) + E * E] = True
    assert nxt == seen.size and seen.all()
    # one entry by hand: (r, c) = (E + 5, 7) lies in tile (1, 0), the second block of band 0
    assert int(S.p_off(ld, L, E + 5, 7)) == E * E + 7 * E + 5
    # and (2E + 1, E + 2) in tile (2, 1): band 0 holds T tiles, band 1 starts with (1, 1)
    assert int(S.p_off(ld, L, 2 * E + 1, E + 2)) == (T + 1) * E * E + 2 * E + 1


@pytest.mark.parametrize("E", [64, 128])
def test_expected_storage_on_a_two_by_two_tile_example(E):
    L = E.bit_length() - 1
    ld = 2 * E
    n = E + 3
    rng = np.random.default_rng(E)
    A = rng.normal(size=(n, n))
    P = A + A.T
    buf = S.expected_storage(P, ld, E)
    assert buf.shape == (3 * E * E,)
    t00 = buf[:E * E].reshape(E, E).T                # column-major tile -> [row, column]
    t10 = buf[E * E:2 * E * E].reshape(E, E).T
    t11 = buf[2 * E * E:].reshape(E, E).T
    assert np.array_equal(t00, P[:E, :E]) and np.array_equal(t00, t00.T)
    assert np.array_equal(t10[:3, :], P[E:, :E]) and not t10[3:, :].any()
    assert np.array_equal(t11[:3, :3], P[E:, E:]) and not t11[3:, :].any() and not t11[:, 3:].any()
    for r, c in ((0, 0), (E - 1, 2), (E, E - 1), (E + 2, E + 1), (E + 1, E + 2)):
        assert buf[int(S.p_off(ld, L, max(r, c), min(r, c)))] == P[r, c]
    # what p_store_sym writes: both copies inside a diagonal tile, one below it
    assert len(S.stored_offsets(ld, L, 5, 2)) == 2 and len(S.stored_offsets(ld, L, E + 1, 2)) == 1
    assert len(S.stored_offsets(ld, L, 2, E + 1)) == 1 and len(S.stored_offsets(ld, L, 7, 7)) == 1
    assert np.array_equal(S.stored_offsets(ld, L, 2, E + 1), S.stored_offsets(ld, L, E + 1, 2))
    # the offsets predict / add_features own
    own = S.predict_owned_offsets(n, ld, L)
    assert len(own) == 9 + 2 * 3 * (E - 3) + 3 * 3             # P_vv, strip + mirror in tile (0, 0), strip rows in tile (1, 0)
    own = S.add_owned_offsets(n - 2, 1, ld, L)               # the last landmark (rows E + 1, E + 2) as the new one
    assert len(own) == 2 * E + 8                           # two rows of tile (1, 0); in tile (1, 1) the 2 x 3 corner and its mirror
