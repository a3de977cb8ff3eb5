"""Duplicate search and merge on the device (slam_ekf_find_duplicates, slam_ekf_merge_landmarks, csrc/ekf_merge.hip) against
tests/merge_ref.py, the dense fp64 restatement that tests/test_merge_ref_cpu.py pins.

Scenes are built from the state AS DOWNLOADED from the device: landmark b is planted at x_a + L u sqrt(t) with D = L L' the
covariance of the pair's difference, |u| = 1, so that its d2 is t.  Before the GPU is asked anything the fp64 reference must
show that no pair of the scene lies within 1 % of the gate and that every planted D has a condition number below 1e3:
conditions on the INPUT, after which the search has to equal the exhaustive reference exactly.

Merge tolerance: the bounds of the full-P parity tests of slam_ekf_update (tests/test_gpu_ekf.py: TOL, relerr, relerr_cov),
imported.  A merge may exceed them only up to 4 x the error an ordinary 8-observation update has on the same state."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import merge_ref as MR
from tests import strip_ref as SR
from tests.test_gpu_ekf import DTYPES, TOL, check_side, noisy_obs, random_state, relerr, relerr_cov, rounded

pytestmark = pytest.mark.gpu

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
GATE = 9.0
TARGETS = (0.25, 0.9, 1.1, 4.0)
RC = np.array([[0.02, 0.005], [0.005, 0.03]])
IP = C.POINTER(C.c_int32)


def _eq_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(a), SR._bits(b))


def edge_of(dtype):
    return 128 if dtype == "f32" else 64


def straddlers(dtype, N):
    """Landmarks whose two state indices lie in two tiles: f(j) + 1 a multiple of the tile edge."""
    E = edge_of(dtype)
    return [k * E // 2 - 1 for k in range(1, 2 * N // E + 2) if 2 <= k * E // 2 - 1 <= N]


def grid_state(rng, N, scale=0.25):
    """random_state's covariance (scaled), the means on a jittered 5 m grid: no two landmarks are close by accident."""
    x, P = random_state(rng, N)
    side = int(math.ceil(math.sqrt(N)))
    cells = rng.permutation(side * side)[:N]
    x[3::2] = 5.0 * (cells % side) + rng.uniform(-0.5, 0.5, N)
    x[4::2] = 5.0 * (cells // side) + rng.uniform(-0.5, 0.5, N)
    return x, P * scale


def plant(x, P, plants, rng):
    """x with landmark b of every (a, b, t) moved to d2 = t from a; the planted Ds' condition numbers."""
    x = np.array(x, dtype=np.float64)
    conds = []
    for a, b, t in plants:
        _delta, D = MR.difference(x, P, a, b)
        conds.append(np.linalg.cond(D))
        phi = rng.uniform(0, 2 * math.pi)
        x[MR.f(b):MR.f(b) + 2] = x[MR.f(a):MR.f(a) + 2] + np.linalg.cholesky(D) @ np.array([math.cos(phi), math.sin(phi)]) * math.sqrt(t)
    return x, conds


def tie_far_pair(P, a, b, s=6.0, eps=0.01):
    """Landmarks a, b made large (x s) and almost perfectly correlated: the cheap bound keeps the pair, D = eps I rejects it."""
    n = P.shape[0]
    T = np.eye(n)
    fa, fb = MR.f(a), MR.f(b)
    T[fa:fa + 2, fa:fa + 2] *= s
    T[fb:fb + 2, fb:fb + 2] = 0.0
    T[fb:fb + 2, fa:fa + 2] = s * np.eye(2)
    P2 = T @ P @ T.T
    P2[fb:fb + 2, fb:fb + 2] += eps * np.eye(2)
    return (P2 + P2.T) / 2


def input_is_clear_of_the_gate(x, P, gate, conds):
    t = MR.d2_table(x, P)
    near = np.isfinite(t) & (np.abs(t - gate) <= 0.01 * gate)
    assert not near.any(), ("a pair of the scene lies within 1 % of the gate", np.argwhere(near) + 1, t[near])
    assert all(c < 1e3 for c in conds), conds


def make_scene(pkg, dtype, N, plants, seed, far=None):
    """A handle holding the scene, the scene as the device holds it in fp64, and the reference's answer."""
    rng = np.random.default_rng(seed)
    x, P = grid_state(rng, N)
    if far is not None:                                     # 3.5 m apart, between the grid's cells
        P = tie_far_pair(P, *far)
        x[MR.f(far[1]):MR.f(far[1]) + 2] = x[MR.f(far[0]):MR.f(far[0]) + 2] + 2.5
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    xd, Pd = st.download()
    x2, conds = plant(xd.astype(np.float64), np.array(Pd, dtype=np.float64), plants, rng)
    st.set_state(x2, Pd)
    xo, Po = rounded(st)
    input_is_clear_of_the_gate(xo, Po, GATE, conds)
    return st, xo, Po, MR.find(xo, Po, GATE)


def scenes(dtype, N):
    """name -> (plants, far pair)."""
    out = {"none planted": ([], None)}
    if N == 2:
        for t in TARGETS:
            out[f"t = {t} gate"] = ([(1, 2, t * GATE)], None)
        return out
    out["one pair at each target"] = ([(3, 8, TARGETS[0] * GATE), (5, 11, TARGETS[1] * GATE), (13, 21, TARGETS[2] * GATE),
                                       (15, 24, TARGETS[3] * GATE)], None)
    out["first and last"] = ([(1, N, 0.25 * GATE), (2, N - 1, 1.1 * GATE)], None)
    out["far pair kept by the bound"] = ([(3, 8, 0.9 * GATE)], (17, 30))
    if N >= 200:
        S = straddlers(dtype, N)
        E = edge_of(dtype)
        in_band1 = E // 2 + 10                                            # f = E + 21: second tile row
        assert len(S) >= 3 and MR.f(S[0]) + 1 == E and (MR.f(in_band1) // E) == 1
        out["one diagonal tile, and band 0 with band 1"] = ([(4, 9, 0.25 * GATE), (6, 12, 1.1 * GATE), (10, in_band1, 0.9 * GATE),
                                                             (14, in_band1 + 3, 4.0 * GATE)], None)
        out["straddler as a and as b"] = ([(S[0], 140, 0.9 * GATE), (20, S[1], 0.25 * GATE), (S[0] + 1, 150, 1.1 * GATE),
                                           (25, S[1] + 1, 4.0 * GATE)], None)
        out["straddlers as both"] = ([(S[0], S[1], 0.25 * GATE), (S[0] + 1, S[2], 0.9 * GATE), (S[0] - 1, S[2] + 1, 1.1 * GATE)], None)
    return out


def dev_find(st, cap=1024):
    pairs, count = st.find_duplicates(GATE, cap)
    assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2
    return pairs, count


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [2, 35, 200])
def test_find_equals_the_exhaustive_reference(pkg, dtype, N):
    for k, (what, (plants, far)) in enumerate(scenes(dtype, N).items()):
        st, xo, Po, (want, count) = make_scene(pkg, dtype, N, plants, 9000 + 10 * N + k, far)
        tag = f"{dtype} N={N} {what}"
        planted_in = sorted([min(a, b), max(a, b)] for a, b, t in plants if t < GATE)
        assert all(p in want.tolist() for p in planted_in), tag            # the scene is what it says
        assert not any([a, b] in want.tolist() for a, b, t in plants if t > GATE), tag
        if far is not None:                                                 # kept by the cheap bound, rejected by the exact test
            delta, D = MR.difference(xo, Po, *far)
            fa, fb = MR.f(far[0]), MR.f(far[1])
            assert MR.prefilter_keeps(delta, Po[fa:fa + 2, fa:fa + 2], Po[fb:fb + 2, fb:fb + 2], GATE) and MR.d2_of(delta, D) > 2 * GATE
            assert list(far) not in want.tolist()
        snap = SR.snapshot(st)
        x0, blk0 = st.download("x"), st.landmark_blocks()
        got = {}
        for mode in ("sweep", "grid", "auto"):
            st.set_gate_mode(mode)
            pairs, cnt = dev_find(st)
            got[mode] = pairs
            assert cnt == count and np.array_equal(pairs, want), (tag, mode, pairs.tolist(), want.tolist())
        # the state is bit-identical after the calls
        assert SR.changed_offsets(st, snap).size == 0 and _eq_bits(st.download("x"), x0) and _eq_bits(st.landmark_blocks(), blk0), tag
        # cap < count: the first cap pairs and the full count; cap = 0 with NULL pairs: the count alone
        if count >= 2:
            pairs, cnt = dev_find(st, cap=count - 1)
            assert cnt == count and np.array_equal(pairs, want[:count - 1]), tag
        out = C.c_int(-1)
        assert pkg._lib.lib.slam_ekf_find_duplicates(st._h, GATE, None, 0, C.byref(out)) == 0 and out.value == count, tag
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_with_64_pairs_and_several_workgroups_per_axis(pkg, dtype):
    N = 1000
    rng = np.random.default_rng(64)
    order = rng.permutation(np.arange(1, N + 1))
    plants = [(int(min(p)), int(max(p)), TARGETS[i % 2] * GATE) for i, p in enumerate(order[:128].reshape(64, 2))]
    plants += [(int(min(p)), int(max(p)), TARGETS[2 + i % 2] * GATE) for i, p in enumerate(order[128:160].reshape(16, 2))]
    st, _xo, _Po, (want, count) = make_scene(pkg, dtype, N, plants, 777)
    assert count >= 64 and N > 256 * 3                                      # more than one workgroup along a and along b
    p1, c1 = dev_find(st, cap=4096)
    p2, c2 = dev_find(st, cap=4096)
    assert c1 == c2 == count and np.array_equal(p1, want) and p1.tobytes() == p2.tobytes()
    st.close()


def test_find_bad_arguments(pkg):
    rng = np.random.default_rng(1)
    x, P = grid_state(rng, 10)
    st = pkg.EKFSlamState(x, P, dtype="f64", max_landmarks=12)
    lib, out, buf = pkg._lib.lib, C.c_int(-3), (C.c_int32 * 8)()
    snap = SR.snapshot(st)
    for what, rc in (("null count", lib.slam_ekf_find_duplicates(st._h, GATE, buf, 4, None)),
                     ("cap < 0", lib.slam_ekf_find_duplicates(st._h, GATE, buf, -1, C.byref(out))),
                     ("pairs NULL with cap > 0", lib.slam_ekf_find_duplicates(st._h, GATE, None, 4, C.byref(out))),
                     ("gate 0", lib.slam_ekf_find_duplicates(st._h, 0.0, buf, 4, C.byref(out))),
                     ("gate < 0", lib.slam_ekf_find_duplicates(st._h, -1.0, buf, 4, C.byref(out))),
                     ("gate inf", lib.slam_ekf_find_duplicates(st._h, math.inf, buf, 4, C.byref(out))),
                     ("gate nan", lib.slam_ekf_find_duplicates(st._h, math.nan, buf, 4, C.byref(out)))):
        assert rc == pkg._lib.SLAM_E_BADARG and out.value == -3, what
    assert SR.changed_offsets(st, snap).size == 0
    st.close()


# ---- merge -----------------------------------------------------------------------------------------------------------------
def merge_pairs(dtype, N, cnt):
    """cnt disjoint pairs (a_p, b_p): tile-edge landmarks as survivor and as removed, the last landmark removed, the first one
    surviving, and a pair given with b < a."""
    if N == 2:
        return [(1, 2)]
    S = straddlers(dtype, N)
    base = [(1, N)]                                                          # survivor first, removed last
    if N >= 200:
        base += [(S[0], 90), (150, S[1]), (S[2], S[0] + 1), (170, 33), (7, 12), (40, 41), (100, 180)]     # (170, 33): b < a
    else:
        base += [(30, 4), (7, 12), (16, 9), (20, 21), (25, 26), (27, 33), (31, 2)]                         # (30, 4), (16, 9), (31, 2): b < a
    return base[:cnt]


def close_pairs(st, pairs, rng):
    """The pairs' second landmarks moved next to the first ones (a merge of landmarks 50 m apart is not the use case)."""
    xd, Pd = st.download()
    x2 = xd.astype(np.float64)
    for a, b in pairs:
        x2[MR.f(b):MR.f(b) + 2] = x2[MR.f(a):MR.f(a) + 2] + rng.uniform(-0.3, 0.3, 2)
    st.set_state(x2, Pd)
    return rounded(st)


def update_error(pkg, dtype, xo, Po, N, rng):
    """An ordinary update of min(8, N) observations on the same state: its error against the oracle, measured as check_state does."""
    st = pkg.EKFSlamState(xo, Po, dtype=dtype, max_landmarks=N + 4)
    ids = rng.choice(np.arange(1, N + 1), size=min(8, N), replace=False)
    z = noisy_obs(rng, xo, ids)
    st.update(z, R, ids.reshape(1, -1))
    xu, Pu = O.update_sparse(xo, Po, z, R, ids.reshape(1, -1))
    xg, Pg = st.download()
    st.close()
    return relerr(xg, xu), relerr_cov(Pg, Pu, np.diag(Po))


def lib_merge(pkg, st, pairs, Rc=None, null_pairs=False, cnt=None):
    """slam_ekf_merge_landmarks as it is: (status, new_index)."""
    arr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    ni = np.full(st.N, -7, dtype=np.int32)
    rc = None if Rc is None else np.ascontiguousarray(np.asarray(Rc, dtype=np.float64).T).reshape(4)
    code = pkg._lib.lib.slam_ekf_merge_landmarks(st._h, None if null_pairs else arr.ctypes.data_as(IP), len(arr) if cnt is None else cnt,
                                                 None if rc is None else rc.ctypes.data_as(C.POINTER(C.c_double)), ni.ctypes.data_as(IP))
    return code, ni


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,cnt", [(2, 1), (35, 1), (35, 3), (35, 8), (200, 1), (200, 3), (200, 8)])
def test_merge_against_the_reference(pkg, dtype, N, cnt, noisy):
    rng = np.random.default_rng(500 * N + 10 * cnt + noisy)
    x, P = grid_state(rng, N, scale=1.0)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    pairs = merge_pairs(dtype, N, cnt)
    xo, Po = close_pairs(st, pairs, rng)
    Rc = RC if noisy else None
    xr, Pr, nir = MR.merge(xo, Po, pairs, Rc)
    code, ni = lib_merge(pkg, st, pairs, Rc)
    assert code == 0 and st.N == N - len(pairs)
    assert np.array_equal(ni, nir), (ni.tolist(), nir.tolist())
    xg, Pg = st.download()
    assert xg.shape == xr.shape and Pg.shape == Pr.shape
    rm = np.asarray(pairs)[:, 1]
    keep = np.delete(np.arange(len(xo)), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))
    ex, eP = relerr(xg, xr), relerr_cov(Pg, Pr, np.diag(Po)[keep])
    ux, uP = update_error(pkg, dtype, xo, Po, N, rng)
    print(f"merge {dtype} N={N} cnt={len(pairs)} Rc={'set' if noisy else '0'}: x {ex:.3e} P {eP:.3e}; 8-observation update: x {ux:.3e} P {uP:.3e}")
    assert ex <= max(TOL[dtype]["x"], 4 * ux), (ex, ux)
    assert eP <= max(TOL[dtype]["P"], 4 * uP), (eP, uP)
    assert np.array_equal(Pg, Pg.T)
    check_side(st, Pg, "after the merge")                                     # landmark_blocks() are the matrix's own entries
    SR.check_storage(st, pkg, Pg, what=f"merge {dtype} N={N} cnt={cnt}")
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_filter_goes_on_from_the_merged_state(pkg, dtype):
    """associate + update after a merge equal the oracle run from the merged state, in sweep and in grid mode: the side
    array, the variance bound and the grid were invalidated."""
    N = 200
    outs = []
    for mode in ("sweep", "grid"):
        rng = np.random.default_rng(4242)
        x, P = grid_state(rng, N, scale=1.0)
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
        st.set_gate_mode(mode)
        seen0 = rng.choice(np.arange(1, N + 1), size=6, replace=False)
        st.associate_vector(noisy_obs(rng, x, seen0), R, 4.0, 25.0)          # the grid / the variance bound exist before the merge
        pairs = merge_pairs(dtype, N, 5)
        close_pairs(st, pairs, rng)
        st.associate_vector(noisy_obs(rng, x, seen0), R, 4.0, 25.0)
        st.merge_landmarks(pairs)
        xm, Pm = rounded(st)
        seen = rng.choice(np.arange(1, st.N + 1), size=10, replace=False)
        z = np.hstack([noisy_obs(rng, xm, seen), np.array([[400.0], [0.4]])])
        a = st.associate_vector(z, R, 4.0, 25.0)
        nis, nd = O.association_table_sparse(xm, Pm, z, R)
        ao = O.assoc_vector(nis, nd, 4.0, 25.0)
        assert np.array_equal(a, ao) and int((a > 0).sum()) >= 5, mode
        zf, idf, _zn = O.split_assoc(z, ao)
        st.update(zf, R, idf)
        xu, Pu = O.update_sparse(xm, Pm, zf, R, idf)
        xg, Pg = st.download()
        assert relerr(xg, xu) <= TOL[dtype]["x"] and relerr_cov(Pg, Pu, np.diag(Pm)) <= TOL[dtype]["P"], mode
        check_side(st, Pg, mode)
        outs.append((a, xg, Pg))
        st.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and _eq_bits(outs[0][1], outs[1][1]) and _eq_bits(outs[0][2], outs[1][2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_then_merge_end_to_end(pkg, dtype):
    N = 200
    S = straddlers(dtype, N)
    st, _xo, _Po, (want, count) = make_scene(pkg, dtype, N, [(S[0], 140, 0.25 * GATE), (9, 77, 4.0 * GATE)], 31337)
    pairs, cnt = st.find_duplicates(GATE)
    assert cnt == count == 1 and pairs.tolist() == [[S[0], 140]] == want.tolist()
    ni = st.merge_landmarks(pairs, Rc=RC * 1e-3)
    assert st.N == N - 1 and ni[139] == ni[S[0] - 1] == S[0] and ni[140] == 140
    pairs, cnt = st.find_duplicates(GATE)
    assert cnt == 0 and pairs.shape == (0, 2)
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_the_state_bit_identical(pkg, dtype):
    N = 40
    rng = np.random.default_rng(77)
    x, P = grid_state(rng, N, scale=1.0)
    # landmarks 5 and 6 identical and perfectly correlated: D = 0 exactly
    fa, fb = MR.f(5), MR.f(6)
    P[fb:fb + 2, :] = P[fa:fa + 2, :]
    P[:, fb:fb + 2] = P[:, fa:fa + 2]
    P[fb:fb + 2, fb:fb + 2] = P[fa:fa + 2, fa:fa + 2]
    P[fa:fa + 2, fb:fb + 2] = P[fa:fa + 2, fa:fa + 2]
    P[fb:fb + 2, fa:fa + 2] = P[fa:fa + 2, fa:fa + 2]
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    BAD, NOTPD = pkg._lib.SLAM_E_BADARG, pkg._lib.SLAM_E_NOTPD
    snap, x0, blk0 = SR.snapshot(st), st.download("x"), st.landmark_blocks()

    def untouched(what):
        assert st.N == N, what
        assert SR.changed_offsets(st, snap).size == 0 and _eq_bits(st.download("x"), x0) and _eq_bits(st.landmark_blocks(), blk0), what

    nine = [(2 * i + 1, 2 * i + 2) for i in range(9)]
    cases = (("cnt < 0", lib_merge(pkg, st, [(1, 2)], cnt=-1)), ("cnt > SLAM_MERGE_MAX", lib_merge(pkg, st, nine)),
             ("pairs NULL", lib_merge(pkg, st, [(1, 2)], null_pairs=True)), ("id 0", lib_merge(pkg, st, [(0, 2)])),
             ("id N + 1", lib_merge(pkg, st, [(3, N + 1)])), ("a == b", lib_merge(pkg, st, [(4, 4)])),
             ("a landmark in two pairs", lib_merge(pkg, st, [(1, 2), (2, 3)])), ("the same as a and as b", lib_merge(pkg, st, [(1, 2), (9, 1)])),
             ("Rc not symmetric", lib_merge(pkg, st, [(1, 2)], Rc=[[0.1, 0.02], [0.01, 0.1]])),
             ("Rc negative diagonal", lib_merge(pkg, st, [(1, 2)], Rc=[[-0.1, 0.0], [0.0, 0.1]])))
    for what, (code, ni) in cases:
        assert code == BAD and np.all(ni == -7), what
        untouched(what)
    assert pkg._lib.lib.slam_ekf_merge_landmarks(None, None, 0, None, None) == BAD
    code, ni = lib_merge(pkg, st, np.zeros((0, 2)))                        # cnt == 0: nothing happens
    assert code == 0 and ni.tolist() == list(range(1, N + 1))
    untouched("cnt == 0")
    # S = D = 0 with Rc = 0: the definition rejects it
    code, ni = lib_merge(pkg, st, [(5, 6)])
    assert code == NOTPD and "positive definite" in pkg._lib.last_error()
    untouched("not positive definite")
    with pytest.raises(pkg.NotPositiveDefinite):
        st.merge_landmarks([[5, 6], [10, 11]])
    untouched("not positive definite, two pairs")
    # a correct merge on the same handle succeeds afterwards: the same pair with constraint noise, and another pair
    xo, Po = rounded(st)
    xr, Pr, nir = MR.merge(xo, Po, [(5, 6), (20, 3)], RC)
    code, ni = lib_merge(pkg, st, [(5, 6), (20, 3)], RC)
    assert code == 0 and np.array_equal(ni, nir) and st.N == N - 2
    xg, Pg = st.download()
    keep = np.delete(np.arange(len(xo)), [MR.f(6), MR.f(6) + 1, MR.f(3), MR.f(3) + 1])
    ux, uP = update_error(pkg, dtype, xo + 0.0, Po + 1e-6 * np.eye(len(xo)), N, rng)
    assert relerr(xg, xr) <= max(TOL[dtype]["x"], 4 * ux) and relerr_cov(Pg, Pr, np.diag(Po)[keep]) <= max(TOL[dtype]["P"], 4 * uP)
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_is_ordered_behind_async_updates(pkg, dtype):
    N = 120
    rng = np.random.default_rng(66)
    x, P = grid_state(rng, N, scale=1.0)
    pairs = [(3, 70), (64, 5), (100, 101)]
    for a, b in pairs:
        x[MR.f(b):MR.f(b) + 2] = x[MR.f(a):MR.f(a) + 2] + rng.uniform(-0.3, 0.3, 2)
    ids = rng.choice(np.arange(1, N + 1), size=8, replace=False)
    z = noisy_obs(rng, x, ids)
    out = []
    for use_async in (False, True):
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
        st.set_async(use_async)
        st.update(z, R, ids.reshape(1, -1))
        ni = st.merge_landmarks(pairs, Rc=RC)
        st.sync()
        out.append((ni, st.N) + st.download())
        st.close()
    s, a = out
    assert np.array_equal(s[0], a[0]) and s[1] == a[1] == N - 3 and _eq_bits(s[2], a[2]) and _eq_bits(s[3], a[3])


# ---- headless sim ------------------------------------------------------------------------------------------------------------
class DuplicatingFilter:
    """The GPU filter behind sim()'s entry points; at ONE fixed observation step it enters a matched landmark a second time, from
    a perturbed copy of that landmark's own observation -- what gated association does after a long loop."""

    def __init__(self, st, at_step, seed=5):
        self.st, self.at_step, self.steps, self.rng, self.forced = st, at_step, 0, np.random.default_rng(seed), None

    def __getattr__(self, name):
        return getattr(self.st, name)

    def add_features(self, zn, R_):
        self.st.add_features(zn, R_)
        self.steps += 1
        if self.steps == self.at_step:
            assert self._last_zf.shape[1] >= 1
            z = self._last_zf[:, :1] + np.array([[0.05], [0.002]]) * self.rng.standard_normal((2, 1))
            self.st.add_features(z, R_)
            self.forced = (int(self._last_idf[0]), self.st.N)

    def associate(self, z, R_, gate1, gate2):
        zf, idf, zn = self.st.associate(z, R_, gate1, gate2)
        self._last_zf, self._last_idf = zf, np.asarray(idf).reshape(-1)
        return zf, idf, zn


def test_sim_with_merge_gate(pkg, golden_dir):
    S = pkg.sim
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    wp = S.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    lms, seed = cfg["landmarks"], int(cfg["seed"][1])
    runs = {}
    for what, kw, force in (("plain", {}, None), ("gate none", {"merge_gate": None}, None), ("merge", {"merge_gate": GATE}, 12),
                            ("merge, nothing forced", {"merge_gate": GATE}, None)):
        st = pkg.EKFSlamState(S.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=120)
        f = DuplicatingFilter(st, force) if force else st
        log = S.sim(f, wp, lms, seed=seed, nlaps=1, max_steps=400, **kw)
        runs[what] = (log, st.N, st.download(), f)
        st.close()
    (l0, n0, s0, _), (l1, n1, s1, _) = runs["plain"], runs["gate none"]
    assert n0 == n1 and l0.assoc == l1.assoc and l1.merged == [] and _eq_bits(s0[0], s1[0]) and _eq_bits(s0[1], s1[1])
    log, nf, _s, f = runs["merge"]
    assert f.forced is not None and len(log.obs_steps) >= 30
    assert (11, [list(f.forced)]) in [(t, p) for t, p in log.merged], (log.merged, f.forced)     # merged in the step that entered it
    # the same landmark count as the run without the forced duplicate, and nothing else was merged that is not merged there too
    unforced = runs["merge, nothing forced"]
    assert nf == unforced[1] and len(log.merged) == len(unforced[0].merged) + 1
