"""Landmark removal on the device (slam_ekf_remove_landmarks, csrc/ekf_compact.hip).

Removal does no arithmetic -- x <- x[keep], P <- P[keep, keep] -- so every comparison here is BIT FOR BIT (`_eq_bits`);
there is no tolerance to choose.  The reference is three lines of NumPy (`reduced`)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import strip_ref as SR
from tests.test_gpu_ekf import DTYPES, noisy_obs, random_state

pytestmark = pytest.mark.gpu

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])


def _eq_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(a), SR._bits(b))


def reduced(x, P, ids):
    """The reference: the state without the landmarks `ids` (1-based), and the index map."""
    N = (len(x) - 3) // 2
    rm = np.unique(np.asarray(ids, dtype=np.int64))
    keep = np.delete(np.arange(len(x)), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))
    new_index = np.zeros(N, dtype=np.int32)
    left = np.delete(np.arange(N), rm - 1)
    new_index[left] = np.arange(1, len(left) + 1)
    return x[keep], P[np.ix_(keep, keep)], new_index


def blocks_of(P):
    f = 3 + 2 * np.arange((P.shape[0] - 3) // 2)
    return np.stack([P[f, f], P[f + 1, f], P[f + 1, f + 1]])


def removal_sets(N, dtype, rng):
    edge = 128 if dtype == "f32" else 64
    sets = {"first": [1], "last": [N], "middle": [(N + 1) // 2], "all": list(range(1, N + 1)), "none": [],
            "random 10 %": sorted(rng.choice(np.arange(1, N + 1), size=max(1, N // 10), replace=False).tolist()),
            "descending": list(range(N, 0, -max(1, N // 7)))}
    for k in (1, 2):                                   # three consecutive landmarks whose state indices straddle a tile edge
        j = (k * edge - 3) // 2 + 1                    # f = 3 + 2 (j - 1) = k edge - 1 or k edge - 2: landmark j ends at / on the edge
        if j + 1 <= N:
            sets[f"tile edge {k * edge}"] = [j - 1, j, j + 1]
    return sets


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 2, 35, 200, 1000])
def test_removal_is_exact(pkg, dtype, N):
    rng = np.random.default_rng(7000 + N)
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 5)
    xd, Pd = st.download()                                # the state as the device holds it
    sets = removal_sets(N, dtype, rng)
    if N >= 200:
        assert any(k.startswith("tile edge") for k in sets)
    for what, ids in sets.items():
        st.set_state(xd, Pd)
        xr, Pr, ni = reduced(xd, Pd, ids)
        got = st.remove_landmarks(ids)
        assert st.N == N - len(ids), what
        assert got.dtype == np.int32 and np.array_equal(got, ni), what
        xg, Pg = st.download()
        assert _eq_bits(xg, xr) and _eq_bits(Pg, np.asfortranarray(Pr)), f"{dtype} N={N} {what}"
        SR.check_storage(st, pkg, Pg, what=f"{dtype} N={N} {what}")
        assert _eq_bits(st.landmark_blocks(), blocks_of(Pr)), what
    # the edge sets are what they say: landmarks 62-64 / 30-32 around the first edge
    if N >= 200:
        assert sets["tile edge 128" if dtype == "f32" else "tile edge 64"] == ([62, 63, 64] if dtype == "f32" else [30, 31, 32])
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,j", [(200, 200), (200, 150), (200, 70), (200, 33), (35, 20)])
def test_nothing_below_the_first_removed_landmark_changes(pkg, dtype, N, j):
    """Only landmarks with id >= j go: no stored entry with row AND column below 3 + 2 (j - 1) changes in the raw buffer
    (necessary for the skipped prefix, not sufficient)."""
    rng = np.random.default_rng(100 * N + j)
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 5)
    ids = np.unique(np.concatenate([[j], rng.choice(np.arange(j, N + 1), size=min(5, N - j + 1), replace=False)]))
    snap = SR.snapshot(st)
    st.remove_landmarks(ids)
    changed = SR.changed_offsets(st, snap)
    _view, ld, E = SR.raw_view(st)
    f0 = 3 + 2 * (j - 1)
    r, c = np.meshgrid(np.arange(f0), np.arange(f0), indexing="ij")
    below = SR.stored_offsets(ld, E.bit_length() - 1, r, c)
    assert changed.size > 0
    assert np.intersect1d(changed, below).size == 0
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_the_state_alone(pkg, dtype):
    N = 40
    rng = np.random.default_rng(5)
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 5)
    snap = SR.snapshot(st)
    x0 = st.download("x")
    lib = pkg._lib.lib
    ip = C.POINTER(C.c_int32)

    def call(ids, cnt, null=False):
        arr = np.asarray(ids, dtype=np.int32)
        ni = np.full(N, -7, dtype=np.int32)
        return lib.slam_ekf_remove_landmarks(st._h, None if null else arr.ctypes.data_as(ip), cnt, ni.ctypes.data_as(ip))

    for what, rc in (("id 0", call([3, 0], 2)), ("id N + 1", call([N + 1], 1)), ("duplicate", call([4, 9, 4], 3)),
                     ("cnt = -1", call([1], -1)), ("ids = NULL", call([], 1, null=True))):
        assert rc == pkg._lib.SLAM_E_BADARG, what
        assert st.N == N, what
        assert SR.changed_offsets(st, snap).size == 0, what
        assert _eq_bits(st.download("x"), x0), what
    for bad in ([0], [N + 1], [2, 2]):
        with pytest.raises(pkg.SlamHipError) as ei:
            st.remove_landmarks(bad)
        assert ei.value.code == pkg._lib.SLAM_E_BADARG
    assert SR.changed_offsets(st, snap).size == 0 and st.N == N
    st.close()


def _cycle(st, z1, z2, zn, assocs):
    """predict, associate (sweep and grid), observe, add_features, predict, observe; the association vectors go to `assocs`."""
    st.predict(7.0, 0.05, 4.0, Q, 0.025)
    st.set_gate_mode("sweep")
    assocs.append(st.associate_vector(z1, R, 4.0, 25.0))
    st.set_gate_mode("grid")
    assocs.append(st.associate_vector(z1, R, 4.0, 25.0))
    st.set_gate_mode("auto")
    assocs.append(st.observe(z1, R, 4.0, 25.0))
    st.add_features(zn, R)
    st.predict(8.0, -0.1, 4.0, Q, 0.025)
    assocs.append(st.observe(z2, R, 4.0, 25.0))
    return st.download()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [35, 300])
def test_the_filter_goes_on_as_if_it_had_never_known_them(pkg, dtype, N):
    """Handle A removes a scattered set; handles B and B2 are uploaded with the NumPy-reduced state.  B and B2 (no removal
    anywhere) first confirm that two handles with the same state agree bit for bit over the cycle; then A equals B bit
    for bit, association vectors included, and the association after the removal equals the fp64 oracle's on the
    reduced state."""
    rng = np.random.default_rng(31 * N)
    x, P = random_state(rng, N)
    cap = N + 16
    A = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=cap)
    xd, Pd = A.download()
    ids = rng.choice(np.arange(1, N + 1), size=max(3, N // 6), replace=False)
    xr, Pr, ni = reduced(xd, Pd, ids)
    assert np.array_equal(A.remove_landmarks(ids), ni)
    B = pkg.EKFSlamState(xr, Pr, dtype=dtype, max_landmarks=cap)
    B2 = pkg.EKFSlamState(xr, Pr, dtype=dtype, max_landmarks=cap)
    Nr = N - len(ids)
    # observations of the reduced map after the first predict (oracle on the state the device holds), two clutter points
    xo, Po = O.predict_sparse(xr.astype(np.float64), Pr.astype(np.float64), 7.0, 0.05, 4.0, Q, 0.025)
    seen1 = rng.choice(np.arange(1, Nr + 1), size=min(12, Nr), replace=False)
    z1 = np.hstack([noisy_obs(rng, xo, seen1), np.array([[350.0, 420.0], [0.3, -0.8]])])
    seen2 = rng.choice(np.arange(1, Nr + 1), size=min(9, Nr), replace=False)
    z2 = np.hstack([noisy_obs(rng, xo, seen2), np.array([[500.0], [1.1]])])
    zn = np.array([[610.0, 640.0], [0.2, -0.4]])
    aA, aB, aB2 = [], [], []
    xB, PB = _cycle(B, z1, z2, zn, aB)
    xB2, PB2 = _cycle(B2, z1, z2, zn, aB2)
    assert all(np.array_equal(p, q) for p, q in zip(aB, aB2)) and _eq_bits(xB, xB2) and _eq_bits(PB, PB2), \
        "two handles with the same state do not agree bit for bit even without a removal"
    xA, PA = _cycle(A, z1, z2, zn, aA)
    assert len(aA) == len(aB) == 4 and all(np.array_equal(p, q) for p, q in zip(aA, aB)), (aA, aB)
    assert _eq_bits(xA, xB) and _eq_bits(PA, PB)
    assert A.N == B.N == Nr + 2 + 2 + 1
    # the first association after the removal against the oracle on the reduced state (as the device holds it after predict)
    C2 = pkg.EKFSlamState(xr, Pr, dtype=dtype, max_landmarks=cap)
    C2.predict(7.0, 0.05, 4.0, Q, 0.025)
    xc, Pc = C2.download()
    zf_o, idf_o, zn_o = O.associate_sparse(xc.astype(np.float64), np.array(Pc, dtype=np.float64), z1, R, 4.0, 25.0)
    for a in aA[:3]:
        zf, idf, znn = O.split_assoc(z1, a)
        assert np.array_equal(idf, idf_o) and np.array_equal(zf, zf_o) and np.array_equal(znn, zn_o)
    assert int((aA[0] > 0).sum()) >= len(seen1) // 2 and int((aA[0] < 0).sum()) == 2
    SR.check_storage(A, pkg, PA, what="after the cycle")
    for s in (A, B, B2, C2):
        s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_comes_back(pkg, dtype):
    rng = np.random.default_rng(8)
    x, P = random_state(rng, 8)
    A = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=8)
    xd, Pd = A.download()
    with pytest.raises(pkg.SlamHipError) as ei:
        A.add_features(np.array([[20.0], [0.1]]), R)
    assert ei.value.code == pkg._lib.SLAM_E_CAPACITY and A.N == 8
    A.remove_landmarks([3, 7])
    zn = np.array([[20.0, 31.0], [0.1, -0.6]])
    A.add_features(zn, R)
    xr, Pr, _ = reduced(xd, Pd, [3, 7])
    B = pkg.EKFSlamState(xr, Pr, dtype=dtype, max_landmarks=8)
    B.add_features(zn, R)
    xA, PA = A.download()
    xB, PB = B.download()
    assert A.N == B.N == 8 and _eq_bits(xA, xB) and _eq_bits(PA, PB)
    SR.check_storage(A, pkg, PA, what="capacity")
    assert _eq_bits(A.landmark_blocks(), B.landmark_blocks())
    with pytest.raises(pkg.SlamHipError):
        A.add_features(np.array([[20.0], [0.1]]), R)
    A.close()
    B.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_removal_is_ordered_behind_async_updates(pkg, dtype):
    N = 120
    rng = np.random.default_rng(66)
    x, P = random_state(rng, N)
    ids = rng.choice(np.arange(1, N + 1), size=15, replace=False)
    z1 = np.hstack([noisy_obs(rng, x, rng.choice(np.arange(1, N + 1), size=10, replace=False)), np.array([[400.0], [0.5]])])
    xr, _Pr, _ni = reduced(x, P, ids)
    z2 = noisy_obs(rng, xr, rng.choice(np.arange(1, N - 15 + 1), size=8, replace=False))
    out = []
    for use_async in (False, True):
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 8)
        st.set_async(use_async)
        a1 = st.observe(z1, R, 4.0, 25.0)
        ni = st.remove_landmarks(ids)
        a2 = st.observe(z2, R, 4.0, 25.0)
        st.sync()
        out.append((a1, ni, a2, st.N) + st.download())
        st.close()
    s, a = out
    assert np.array_equal(s[0], a[0]) and np.array_equal(s[1], a[1]) and np.array_equal(s[2], a[2]) and s[3] == a[3] == N + 1 - 15
    assert int((s[0] > 0).sum()) >= 5 and int((s[2] > 0).sum()) >= 4
    assert _eq_bits(s[4], a[4]) and _eq_bits(s[5], a[5])


def test_full_size_10k_landmarks_several_staging_groups(pkg):
    """fp32, N = 10 000 (BASELINE config 3's shape): landmark 1 (everything moves) plus 100 seeded ids.  The stored tiles
    that move exceed the 256 MiB staging bound, so the schedule runs in at least two band groups."""
    rng = np.random.default_rng(20241016)
    N = 10000
    n = 3 + 2 * N
    x = rng.uniform(0, 1000, n).astype(np.float32)
    A = rng.normal(0, 0.05, (n, 8)).astype(np.float32)
    P = A @ A.T
    del A
    P[np.diag_indices(n)] += np.float32(0.01)
    P = np.maximum(P, P.T)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
    E = 128
    T = -(-n // E)                                          # tile rows that hold state: all of them move (f0 = 3)
    assert T * (T + 1) // 2 * E * E * 4 > 2 * (256 << 20)  # more than two staging buffers' worth: >= 3 groups
    xd, Pd = st.download()
    assert _eq_bits(xd, x) and _eq_bits(Pd, np.asfortranarray(P))
    del Pd
    ids = np.concatenate([[1], rng.choice(np.arange(2, N + 1), size=100, replace=False)])
    xr, Pr, ni = reduced(x, P, ids)
    del P
    got = st.remove_landmarks(ids)
    assert np.array_equal(got, ni) and st.N == N - 101
    xg, Pg = st.download()
    assert _eq_bits(xg, xr) and _eq_bits(Pg, np.asfortranarray(Pr))
    del Pr
    SR.check_storage(st, pkg, Pg, what="N = 10k, 101 removed")
    st.close()


# ---- headless sim with clutter ---------------------------------------------------------------------------------------------
class ClutterFilter:
    """The GPU filter behind sim()'s four entry points, with ONE seeded false detection appended to every observation
    step.  A false detection is drawn (seeded rejection sampling) so that the fp64 oracle's association on the filter's
    current state calls it a new feature with a wide margin (smallest nis over the map > 4 gate2) and so that it lies
    at least `clear` metres from every true landmark and from the false detections of the last steps (estimated pose) --
    no later observation of a true landmark can fall inside its gate.  It also keeps its own per-landmark books
    (true / false, matches after creation), renumbered through new_index, to check what gets removed."""

    def __init__(self, st, landmarks, seed, clear=6.0):
        self.st, self.lm, self.rng, self.clear = st, np.asarray(landmarks, dtype=np.float64), np.random.default_rng(seed), clear
        self.false = np.zeros(0, dtype=bool)
        self.hits = np.zeros(0, dtype=np.int64)
        self.recent = []                       # world positions of the last false detections
        self.false_decisions = []              # the filter's decision for each false detection
        self.oracle_margin = []                # smallest nis of the false detection over the map (oracle)
        self.removed_true_with_hits = 0
        self.removed = 0

    def __getattr__(self, name):              # predict, update, add_features, pose, ...
        return getattr(self.st, name)

    def _draw(self):
        x, P = self.st.download()
        x, P = x.astype(np.float64), np.array(P, dtype=np.float64)
        for _ in range(10000):
            r, b = self.rng.uniform(5.0, 30.0), self.rng.uniform(-1.4, 1.4)
            w = np.array([x[0] + r * math.cos(x[2] + b), x[1] + r * math.sin(x[2] + b)])
            if np.min(np.hypot(self.lm[0] - w[0], self.lm[1] - w[1])) < self.clear:
                continue
            if any(np.hypot(*(w - q)) < self.clear for q in self.recent):
                continue
            z = np.array([[r], [b]])
            nis, _nd = O.association_table_sparse(x, P, z, R_SIM)
            m = float(np.min(nis)) if nis.size else math.inf
            if m > 4 * 25.0:
                self.recent = (self.recent + [w])[-7:]
                self.oracle_margin.append(m)
                return z
        raise AssertionError("no admissible false detection found")

    def associate(self, z, R_, gate1, gate2):
        z = np.hstack([np.asarray(z, dtype=np.float64).reshape(2, -1), self._draw()])
        a = self.st.associate_vector(z, R_, gate1, gate2)
        self.false_decisions.append(int(a[-1]))
        zf, idf, zn = O.split_assoc(z, a)
        np.add.at(self.hits, idf.reshape(-1) - 1, 1)
        newf = np.zeros(int((a < 0).sum()), dtype=bool)
        if a[-1] < 0:
            newf[-1] = True
        self.false = np.concatenate([self.false, newf])
        self.hits = np.concatenate([self.hits, np.zeros(len(newf), dtype=np.int64)])
        return zf, idf, zn

    def remove_landmarks(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self.removed += len(ids)
        self.removed_true_with_hits += int(np.sum(~self.false[ids - 1] & (self.hits[ids - 1] >= 1)))
        ni = self.st.remove_landmarks(ids)
        left = ni > 0
        self.false, self.hits = self.false[left], self.hits[left]
        return ni


R_SIM = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])


def test_headless_sim_prunes_false_detections(pkg, golden_dir):
    S = pkg.sim
    assert np.array_equal(S.default_QR()[1], R_SIM)
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    wp = S.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    lms, seed = cfg["landmarks"], int(cfg["seed"][1])
    assert lms.shape[1] == 35
    runs = {}
    # (the two runs that keep every false detection are cut short: their maps fill up with one landmark per step)
    for what, kw in (("plain", {"max_steps": 900}), ("none", {"max_steps": 900, "prune_after": None}), ("prune", {"prune_after": 5})):
        st = pkg.EKFSlamState(S.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=1200)
        f = ClutterFilter(st, lms, seed=99)
        log = S.sim(f, wp, lms, seed=seed, nlaps=2, **kw)
        track, truth = np.array(log.slam_track), np.array(log.true_track)
        rms = float(np.sqrt(np.mean(np.sum((track[:, :2] - truth[:, :2]) ** 2, axis=1))))
        print(f"sim with one false detection per observation step, {what}: N_final {st.N}, "
              f"{len(log.obs_steps)} observation steps, {f.removed} removed, track RMS {rms:.3f} m")
        runs[what] = (log, f, st.N, st.download(), track)
        if what == "prune":
            SR.check_storage(st, pkg, runs[what][3][1], what="after the pruned run")
        st.close()
    # prune_after=None is exactly the run without the argument
    (l0, f0, n0, s0, t0), (l1, f1, n1, s1, t1) = runs["plain"], runs["none"]
    assert n0 == n1 and np.array_equal(t0, t1) and l0.assoc == l1.assoc and l1.pruned == [] and f1.removed == 0
    assert _eq_bits(s0[0], s1[0]) and _eq_bits(s0[1], s1[1])
    assert n0 > len(l0.obs_steps) >= 90                           # the reference's rule: every false detection stays a landmark
    log, f, nf, _s, _t = runs["prune"]
    steps = len(log.obs_steps)
    # the premise, asserted: every false detection lies outside the gate of every landmark for the oracle, and the
    # device decided the same (a new feature)
    assert len(f.false_decisions) == steps and all(d == -1 for d in f.false_decisions)
    assert min(f.oracle_margin) > 4 * 25.0
    assert nf <= 35 + 5, nf                                       # 35 true landmarks + the false detections of the last 5 steps
    assert int(f.false.sum()) <= 5 and int((~f.false).sum()) <= 35
    assert f.removed_true_with_hits == 0                          # no true landmark that was matched again is ever removed
    assert f.removed >= steps - 5 and len(log.pruned) > 0
