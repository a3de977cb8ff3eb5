"""Copy, grow and select between EKF handles on the device (slam_ekf_copy / slam_ekf_select, csrc/ekf_copy.hip,
libslamhip_copy.so): dst's raw buffer against tests/copy_ref.py bit for bit, the storage invariants, src untouched, stale data
cleared, the copy as a working filter, errors, the ordering between the two handles' streams, and a state that grows.

Bars where a filter step is compared with the fp64 oracle (per call, the oracle started from the device's own state
before the call): association decisions identical, x 1e-9 / 5e-6 of max|x|, P entry-wise against sqrt(s_i s_j) 1e-9 / 5e-6
(tests/test_gpu_ekf.check_state); a single nis / nd, formed in double from the stored values, at the same 1e-9 / 5e-6.

Not exercised: two handles on different devices (SLAM_E_BADARG by a comparison of two integers ahead of any HIP call; these tests
see one device), and offsets past 2^31 elements."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import copy_ref as CR
from tests import join_ref as JR
from tests import strip_ref as SR
from tests.strip_ref import check_storage
from tests.test_gpu_ekf import DTYPES, Q, R, TOL, check_state, noisy_obs, random_state, rounded

pytestmark = pytest.mark.gpu

GATE1, GATE2 = 4.0, 25.0
# (dtype, source N) -> destination capacities; n = 3 + 2 N is 143 / 263 (2 / 3 tile rows of 128) and 83 / 203 (2 / 4 of 64)
SHAPES = {("f32", 70): (70, 130, 300), ("f32", 130): (130, 300), ("f64", 40): (40, 100, 300), ("f64", 100): (100, 300)}
COPY_CASES = [(d, N, cap) for (d, N), caps in SHAPES.items() for cap in caps]
BIG = {"f32": 130, "f64": 100}            # the sources the selections are taken from
SMALL = {"f32": 70, "f64": 40}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(a), SR._bits(b))


def _raw(st):
    view, ld, E = SR.raw_view(st)
    return view.cpu().numpy(), ld, E


def _blank(pkg, dtype, cap):
    return pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype=dtype, max_landmarks=cap)


def _step(rng, st, k, m=5, ids=None):
    """One predict + observe of m known landmarks (no new feature can arise: the observations lie within a few sigma)."""
    st.predict(1.5 + 0.2 * k, 0.05 - 0.03 * k, 4.0, Q, 0.1)
    x = st.download("x").astype(np.float64)
    if ids is None:
        ids = rng.choice(np.arange(1, st.N + 1), size=m, replace=False)
    z = noisy_obs(rng, x, ids)
    a = st.observe(z, R, GATE1, GATE2)
    assert np.all(a >= 0)
    return z


def lived_in(pkg, rng, dtype, N, cap, steps=2):
    """A random SPD state uploaded, then a few predict / observe steps: dense cross-covariances, a side array, a variance
    bound and an update workspace that have all been used."""
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=cap)
    for k in range(steps):
        _step(rng, st, k)
    st.sync()
    return st


class Source:
    def __init__(self, st):
        self.st = st
        self.x, self.P = st.download()
        self.raw, self.ld, self.E = _raw(st)
        self.snap = SR.snapshot(st)

    def untouched(self):
        return SR.changed_offsets(self.st, self.snap).size == 0 and _bits_equal(self.st.download("x"), self.x)


@pytest.fixture(scope="module")
def sources(pkg):
    """One lived-in source per (dtype, N), shared and never written by the tests below (each of them checks that)."""
    out = {}
    for (dtype, N) in SHAPES:
        E = SR.TILE[dtype]
        assert (3 + 2 * N + E - 1) // E == {("f32", 70): 2, ("f32", 130): 3, ("f64", 40): 2, ("f64", 100): 4}[(dtype, N)]
        out[(dtype, N)] = Source(lived_in(pkg, np.random.default_rng(100 + N), dtype, N, N))
        assert out[(dtype, N)].raw.any()
    yield out
    for s in out.values():
        s.st.close()


def _check_dst(pkg, dst, src, s, what):
    """dst against the rule: raw buffer, x, N, storage invariants."""
    got, ld, E = _raw(dst)
    want = CR.expected_select(src.P, s, ld, E)
    if not _bits_equal(got, want):
        bad = np.flatnonzero(SR._bits(got) != SR._bits(want))
        raise AssertionError(f"{what}: {bad.size} raw offsets differ from the rule, first {bad[:8].tolist()} (ld {ld})")
    assert dst.N == (s.size - 3) // 2 and _bits_equal(dst.download("x"), src.x[s]), what
    check_storage(dst, pkg, what=what)
    assert src.untouched(), f"{what}: the source changed"


# ---- 1. copy, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,cap", COPY_CASES)
def test_copy_is_bit_for_bit_into_every_capacity(pkg, sources, dtype, N, cap):
    src = sources[(dtype, N)]
    dst = _blank(pkg, dtype, cap)
    assert dst.capacity == cap and src.st.capacity == N
    dst.copy_from(src.st)
    got, ld, E = _raw(dst)
    assert ld == src.ld if cap == N else ld > src.ld                # equal capacity: equal block numbers, the same kernel
    assert _bits_equal(got, SR.expected_storage(src.P, ld, E))
    _check_dst(pkg, dst, src, CR.index_map(N), f"{dtype} copy {N} -> capacity {cap}")
    xg, Pg = dst.download()
    assert _bits_equal(Pg, src.P) and _bits_equal(xg, src.x)
    dst.close()


def test_copy_of_3000_landmarks_strides_over_more_work_items_than_workgroups(pkg):
    """N = 3000 fp32: n = 6003 = 47 tile rows of 128, 47 * 48 / 2 = 1128 tiles (74 MB), 4 slices each = 4512 work items on a grid
    capped at 2048 workgroups: every workgroup takes a second item and some a third.  Into another capacity (49 tile rows), and
    a shuffled selection of 2990 landmarks through the gather kernel's stride loop."""
    N, dtype = 3000, "f32"
    Tw, _Tn, items, grid = CR.plan(3, 3 + 2 * N, 6272, 128)
    assert (Tw, Tw * (Tw + 1) // 2, items, grid) == (47, 1128, 4512, 2048) and items > 2 * grid
    rng = np.random.default_rng(3000)
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    _step(rng, st, 0, m=6)
    src = Source(st)
    dst = _blank(pkg, dtype, 3100)
    dst.copy_from(st)
    got, ld, E = _raw(dst)
    assert ld == 6272 and src.ld == 6016
    assert _bits_equal(got, SR.expected_storage(src.P, ld, E)) and dst.N == N and _bits_equal(dst.download("x"), src.x)
    check_storage(dst, pkg, what="copy of 3000 landmarks")
    ids = rng.permutation(np.arange(1, N + 1))[:2990]
    dst.select_from(st, ids)
    s = CR.index_map(N, ids)
    got, ld, E = _raw(dst)
    assert _bits_equal(got, CR.expected_select(src.P, s, ld, E)) and dst.N == 2990 and _bits_equal(dst.download("x"), src.x[s])
    check_storage(dst, pkg, what="selection of 2990 landmarks")
    assert src.untouched()
    dst.close()
    st.close()


# ---- 2. stale data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_larger_state_left_in_dst_is_cleared(pkg, sources, dtype):
    rng = np.random.default_rng(2)
    N = SMALL[dtype]
    src = sources[(dtype, N)]
    n_old = 3 + 2 * 200
    A = rng.normal(0, 1.0, (n_old, n_old))
    dense = A @ A.T / n_old + np.eye(n_old)                          # no zero anywhere
    x_old = random_state(rng, 200)[0]
    dst = pkg.EKFSlamState(x_old, dense, dtype=dtype, max_landmarks=300)
    _step(rng, dst, 0)                                               # ... and an update workspace with 403 live panel rows
    dst.copy_from(src.st)
    _check_dst(pkg, dst, src, CR.index_map(N), f"{dtype} copy over a larger state")
    z = _step(rng, dst, 1, ids=np.array([1, 2, 3]))                  # the panel rows beyond n are zero again: an update works
    assert z.shape == (2, 3)
    check_storage(dst, pkg, what=f"{dtype} update after the copy over a larger state")
    dst.set_state(x_old, dense)
    ids = rng.permutation(np.arange(1, N + 1))[:N // 2]
    dst.select_from(src.st, ids)
    _check_dst(pkg, dst, src, CR.index_map(N, ids), f"{dtype} selection over a larger state")
    dst.close()


# ---- 3. select ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["shuffled", "reversed", "none", "straddler_in", "straddler_out"])
def test_select_against_the_rule_and_the_filter_on_the_selection(pkg, sources, dtype, which):
    N, E = BIG[dtype], SR.TILE[dtype]
    src = sources[(dtype, N)]
    rng = np.random.default_rng(33)
    subsets = {"shuffled": rng.permutation(np.arange(1, N + 1))[:N // 2], "reversed": np.arange(N, 0, -1),
               "none": np.zeros(0, dtype=np.int64), **CR.straddle_subsets(N, E)}
    ids = subsets[which]
    assert CR.straddlers(N, E)[0] == (63 if dtype == "f32" else 31)   # 0-based j = 62 / 30
    s = CR.index_map(N, ids)
    dst = src.st.select(ids, max_landmarks=max(ids.size, 1) if which != "shuffled" else 300)
    _check_dst(pkg, dst, src, s, f"{dtype} select {which}")
    if ids.size:
        xs, Ps = src.x[s].astype(np.float64), np.array(src.P[np.ix_(s, s)], dtype=np.float64)
        k = ids.size
        pick = np.unique(np.concatenate([[1, k], rng.choice(np.arange(1, k + 1), size=min(6, k), replace=False)]))
        if which.startswith("straddler"):
            pick = np.unique(np.concatenate([pick, [2, CR.straddlers(N, E)[0]]]))     # the pairs the subset is aimed at
        z = np.hstack([noisy_obs(rng, xs, pick), np.array([[400.0], [0.4]])])
        nis, nd = O.association_table_sparse(xs, Ps, z, R)
        with np.errstate(invalid="ignore"):
            rel = min(float(np.nanmin(np.abs(nis - GATE1) / GATE1)), float(np.nanmin(np.abs(np.nanmin(nis, axis=1) - GATE2) / GATE2)))
        want = O.assoc_vector(nis, nd, GATE1, GATE2)
        if rel >= 1e-3:                                               # (a decision on a gate's edge is not this test's subject)
            for mode in ("sweep", "grid"):
                dst.set_gate_mode(mode)
                got = dst.associate_vector(z, R, GATE1, GATE2)
                assert np.array_equal(got, want), (which, mode, got.tolist(), want.tolist())
        rt = TOL[dtype]["x"]
        for i, j in enumerate(pick):
            g_nis, g_nd = dst.compute_association(z[:, i], R, int(j))
            o_nis, o_nd = O.compute_association_sparse(xs, Ps, z[:, i], R, int(j))
            assert g_nis == pytest.approx(o_nis, rel=rt, abs=rt) and g_nd == pytest.approx(o_nd, rel=rt, abs=rt), (which, j)
    else:
        assert dst.N == 0 and dst.n == 3
    dst.close()


# ---- 4. the copy is a working filter -------------------------------------------------------------------------------------------------
def _drive(rng, states, steps, dtype, oracle):
    """The same predict / observe sequence on every state; the observations come from the first one's mean.  Returns per step the
    association vectors and the downloads.  oracle: every state is held to the fp64 oracle started from its own state."""
    out = []
    for k in range(steps):
        x0 = states[0].download("x").astype(np.float64)
        ids = rng.choice(np.arange(1, states[0].N + 1), size=6, replace=False)
        z = np.hstack([noisy_obs(rng, x0, ids), np.array([[300.0 + 20 * k], [0.5 * k - 0.7]])])     # six known, one new
        v, g = 2.0 + 0.3 * k, 0.04 * k - 0.05
        row = []
        for st in states:
            if oracle:
                xo, Po = rounded(st)
                xo, Po = O.predict_sparse(xo, Po, v, g, 4.0, Q, 0.1)
            st.predict(v, g, 4.0, Q, 0.1)
            if oracle:
                check_state(st, xo, Po, dtype, f"{dtype} predict, step {k}")
                xo, Po = rounded(st)
                nis, nd = O.association_table_sparse(xo, Po, z, R)
                want = O.assoc_vector(nis, nd, GATE1, GATE2)
                zf, idf, _zn = O.split_assoc(z, want)
                # the update half alone: the new feature's lever arm is add_features' business (tests/test_gpu_ekf.py)
                a = st.associate_vector(z, R, GATE1, GATE2)
                assert np.array_equal(a, want), (k, a.tolist(), want.tolist())
                st.update(zf, R, idf)
                xo2, Po2 = O.update_sparse(xo, Po, zf, R, idf)
                check_state(st, xo2, Po2, dtype, f"{dtype} update, step {k}", prior=Po)
                st.add_features(z[:, a < 0], R)
            else:
                a = st.observe(z, R, GATE1, GATE2)
            row.append((a, *st.download()))
        out.append(row)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["sweep", "grid"])
def test_the_copy_runs_on_bit_identical_at_equal_capacity(pkg, dtype, mode):
    rng = np.random.default_rng(41)
    N = BIG[dtype]
    src = lived_in(pkg, rng, dtype, N, N + 8)
    if mode == "sweep":
        dst = src.copy()
    else:                                                             # dst carried the grid of another map
        xo, Po = random_state(np.random.default_rng(5), N - 20, spread=40.0)
        dst = pkg.EKFSlamState(xo, Po, dtype=dtype, max_landmarks=N + 8)
        dst.set_gate_mode("grid")
        dst.associate_vector(noisy_obs(rng, xo, [1, 2, 3]), R, GATE1, GATE2)
        assert dst.gate_info()["form"] == "grid"
        dst.copy_from(src)
    for st in (src, dst):
        st.set_gate_mode(mode)
    for k, row in enumerate(_drive(rng, [src, dst], 3, dtype, oracle=False)):
        (a0, x0, P0), (a1, x1, P1) = row
        assert np.array_equal(a0, a1) and (a0 > 0).sum() >= 4 and (a0 < 0).sum() == 1, (k, a0.tolist(), a1.tolist())
        assert _bits_equal(x0, x1) and _bits_equal(P0, P1), f"step {k}: the copy left the source's path"
    assert src.gate_info()["form"] == mode and dst.gate_info()["form"] == mode and src.N == dst.N == N + 3
    check_storage(dst, pkg, what=f"{dtype} {mode}: the copy after three steps")
    for st in (src, dst):
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_copy_runs_on_within_the_bars_at_another_capacity(pkg, dtype):
    rng = np.random.default_rng(43)
    N = BIG[dtype]
    src = lived_in(pkg, rng, dtype, N, N + 8)
    dst = src.copy(max_landmarks=300)
    assert dst.capacity == 300 and dst.device_ptrs()[2] != src.device_ptrs()[2]
    same = True
    for k, row in enumerate(_drive(rng, [src, dst], 3, dtype, oracle=True)):
        (a0, x0, P0), (a1, x1, P1) = row
        assert np.array_equal(a0, a1), (k, a0.tolist(), a1.tolist())
        same = same and _bits_equal(x0, x1) and _bits_equal(P0, P1)
    print(f"{dtype}: source (ld {src.device_ptrs()[2]}) and copy (ld {dst.device_ptrs()[2]}) bit-identical after three steps: {same}")
    check_storage(dst, pkg, what=f"{dtype}: the larger copy after three steps")
    for st in (src, dst):
        st.close()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_refusal_leaves_both_states_bit_identical(pkg, sources, dtype):
    N = SMALL[dtype]
    src = sources[(dtype, N)]
    rng = np.random.default_rng(6)
    x, P = random_state(rng, 20)
    dst = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N - 1)
    other = pkg.EKFSlamState(x, P, dtype="f32" if dtype == "f64" else "f64", max_landmarks=N)
    d_snap, d_x, d_blk = SR.snapshot(dst), dst.download("x"), dst.landmark_blocks()
    lib = pkg._lib.copy_lib()
    BAD, CAP = pkg._lib.SLAM_E_BADARG, pkg._lib.SLAM_E_CAPACITY
    ids = lambda *v: (C.c_int32 * len(v))(*v)                         # noqa: E731
    assert lib.slam_ekf_copy(dst._h, src.st._h) == CAP                # N landmarks into a capacity of N - 1
    assert lib.slam_ekf_select(dst._h, src.st._h, ids(*range(1, N + 1)), N) == CAP
    for d, s in ((None, src.st._h), (dst._h, None), (dst._h, dst._h), (other._h, src.st._h), (dst._h, other._h)):
        assert lib.slam_ekf_copy(d, s) == BAD, (d, s)
        assert lib.slam_ekf_select(d, s, ids(1), 1) == BAD, (d, s)
    assert lib.slam_ekf_select(dst._h, src.st._h, ids(1), -1) == BAD
    assert lib.slam_ekf_select(dst._h, src.st._h, None, 2) == BAD
    for bad in ((0,), (N + 1,), (3, 5, 3), (-2, 1), (1, 2, N + 1)):
        assert lib.slam_ekf_select(dst._h, src.st._h, ids(*bad), len(bad)) == BAD, bad
    with pytest.raises(pkg.SlamHipError) as ei:
        dst.copy_from(src.st)
    assert ei.value.code == CAP
    with pytest.raises(pkg.SlamHipError) as ei:
        dst.select_from(src.st, [1, 1])
    assert ei.value.code == BAD
    with pytest.raises(pkg.SlamHipError) as ei:
        src.st.copy(max_landmarks=N - 1)
    assert ei.value.code == CAP
    assert SR.changed_offsets(dst, d_snap).size == 0 and _bits_equal(dst.download("x"), d_x) and dst.N == 20
    assert _bits_equal(dst.landmark_blocks(), d_blk) and src.untouched() and src.st.N == N
    dst.select_from(src.st, np.arange(1, N))                          # ... and the largest selection that fits goes through
    assert dst.N == N - 1
    for h in (dst, other):
        h.close()


# ---- 6. ordering -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_is_ordered_between_two_async_updates_of_the_source(pkg, dtype):
    rng = np.random.default_rng(61)
    N = BIG[dtype]
    x, P = random_state(rng, N)
    xs = np.asarray(x, dtype=SR.NP_DTYPE[dtype]).astype(np.float64)
    ids1, ids2 = np.array([3, 40, 64, 77]), np.array([5, 12, 63, 90])
    z1, z2 = noisy_obs(rng, xs, ids1), noisy_obs(rng, xs, ids2)
    # the run with syncs: the state between the two updates
    ref = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    ref.update(z1, R, ids1)
    ref.sync()
    x_mid, P_mid = ref.download()
    ref.update(z2, R, ids2)
    x_end, P_end = ref.download()
    ref.close()
    assert not _bits_equal(P_mid, P_end)
    src = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    dst = _blank(pkg, dtype, 300)
    src.set_async(True)
    src.update(z1, R, ids1)                                           # enqueued, status deferred
    dst.copy_from(src)                                                # resolves the status, waits on the device only
    src.update(z2, R, ids2)                                           # behind the copy's last read of src
    xd, Pd = dst.download()
    assert _bits_equal(xd, x_mid) and _bits_equal(Pd, P_mid), "the copy is not the state between the two updates"
    src.sync()
    xe, Pe = src.download()
    assert _bits_equal(xe, x_end) and _bits_equal(Pe, P_end)
    check_storage(dst, pkg, what=f"{dtype} copy between two async updates")
    # the source destroyed right after the call
    dst2 = _blank(pkg, dtype, N)
    dst2.copy_from(src)
    src.close()
    assert _bits_equal(dst2.download("cov"), P_end)
    for h in (dst, dst2):
        h.close()


# ---- 7. growth -------------------------------------------------------------------------------------------------------------------------
def _new_obs(rng, k, r0):
    return np.vstack([rng.uniform(r0, r0 + 15, k), np.linspace(-2.5, 2.5, k) + rng.uniform(-0.05, 0.05, k)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_growing_state_passes_8_16_and_32_landmarks(pkg, dtype):
    rng = np.random.default_rng(71)
    x0 = np.array([50.0, 50.0, 0.4])
    P0 = np.diag([0.02, 0.02, 0.001])
    st = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=8, grow=True)
    st.set_gate_mode("grid")
    st.set_async(False)
    assert st.capacity == 8 and st.grow

    def add(k, r0):
        xs, Ps = rounded(st)
        zn = _new_obs(rng, k, r0)
        st.add_features(zn, R)
        xo, Po = O.add_features_sparse(xs, Ps, zn, R)
        check_state(st, xo, Po, dtype, f"{dtype} add_features to {st.N}", prior=Ps)

    add(6, 10.0)
    assert (st.capacity, st.N) == (8, 6)
    st.associate_joint_vector(noisy_obs(rng, rounded(st)[0], [2, 5]), R, GATE1, GATE2)     # a joint workspace on the OLD handle
    ptr_before = st.device_ptrs()[1]
    add(5, 30.0)                                                      # 11 > 8: capacity max(16, 11)
    assert (st.capacity, st.N, st.max_landmarks) == (16, 11, 16) and st.device_ptrs()[1] != ptr_before
    # observe: four known landmarks and seven new ones, 18 > 16: the update is applied, then the state grows and the seven follow
    st.predict(1.0, 0.02, 4.0, Q, 0.1)
    xs, Ps = rounded(st)
    z = np.hstack([noisy_obs(rng, xs, [1, 4, 7, 10]), _new_obs(rng, 7, 50.0)])[:, rng.permutation(11)]
    nis, nd = O.association_table_sparse(xs, Ps, z, R)
    want = O.assoc_vector(nis, nd, GATE1, GATE2)
    assert (want < 0).sum() == 7 and (want > 0).sum() >= 3
    got = st.observe(z, R, GATE1, GATE2)
    assert np.array_equal(got, want) and (st.capacity, st.N) == (32, 18)
    zf, idf, zn = O.split_assoc(z, want)
    xu, Pu = O.update_sparse(xs, Ps, zf, R, idf)
    xo, Po = O.add_features_sparse(xu, Pu, zn, R)
    check_state(st, xo, Po, dtype, f"{dtype} observe across a growth", prior=Ps)
    st.associate_vector(z[:, :2], R, GATE1, GATE2)
    assert st.gate_info()["form"] == "grid"                          # the gate mode came along (auto would sweep 18 landmarks)
    check_storage(st, pkg, what=f"{dtype} grown to 32")
    # one join: a local map of 20 landmarks, 38 > 32: capacity max(64, 38)
    sub = st.submap(20)
    sub.add_features(_new_obs(rng, 20, 70.0), R)
    xa, Pa = rounded(st)
    xb, Pb = rounded(sub)
    first = st.join(sub)
    sub.close()
    assert first == 19 and (st.capacity, st.N) == (64, 38)
    xj, Pj = JR.join(xa, Pa, xb, Pb)
    check_state(st, np.asarray(xj, dtype=np.float64), np.asarray(Pj, dtype=np.float64), dtype, f"{dtype} join across a growth")
    check_storage(st, pkg, what=f"{dtype} grown to 64")
    a, info = st.associate_joint_vector(noisy_obs(rng, rounded(st)[0], [3, 21, 38]), R, GATE1, GATE2)   # a workspace on the new handle
    assert all(int(v) in (0, j) for v, j in zip(a, (3, 21, 38))) and info["pairings"] == int((a > 0).sum()) >= 1
    st.reserve(10)                                                    # nothing to do
    assert st.capacity == 64
    st.close()
    # the same drive with the default: the capacity error, as before
    st = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=8)
    st.add_features(_new_obs(rng, 6, 10.0), R)
    with pytest.raises(pkg.SlamHipError) as ei:
        st.add_features(_new_obs(rng, 5, 30.0), R)
    assert ei.value.code == pkg._lib.SLAM_E_CAPACITY and (st.capacity, st.N) == (8, 6)
    with pytest.raises(pkg.SlamHipError) as ei:
        st.observe(_new_obs(rng, 5, 50.0), R, GATE1, GATE2)
    assert ei.value.code == pkg._lib.SLAM_E_CAPACITY and st.N == 6
    sub = st.submap(4)
    sub.add_features(_new_obs(rng, 4, 8.0), R)
    with pytest.raises(pkg.SlamHipError) as ei:
        st.join(sub)
    assert ei.value.code == pkg._lib.SLAM_E_CAPACITY and st.N == 6
    st.reserve(10)                                                    # ... and reserve by hand lets the join through
    assert st.join(sub) == 7 and (st.capacity, st.N) == (10, 10)
    for h in (st, sub):
        h.close()
