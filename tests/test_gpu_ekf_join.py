"""Map joining on the device (slam_ekf_join, csrc/ekf_join.hip) against the dense restatement of tests/join_ref.py, entry by entry
within its DERIVED bound, from the two states as the device held them before the call; the storage invariants; what must not
change at all; the filter going on from the joined state; join followed by find-and-merge; errors; the ordering between the two
handles' streams; and sim(submap_steps=k)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import join_ref as JR
from tests import merge_ref as MR
from tests import strip_ref as SR
from tests.strip_ref import check_storage
from tests.test_gpu_ekf import DTYPES, R, check_state, noisy_obs, random_state, rounded

pytestmark = pytest.mark.gpu

SHAPES = [(0, 0), (0, 1), (1, 0), (2, 3), (35, 40), (62, 2), (30, 2), (100, 130)]
GATE1, GATE2 = 4.0, 25.0


def _eq_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(np.ascontiguousarray(a)), SR._bits(np.ascontiguousarray(b)))


def local_state(rng, N, rank=6):
    """A local map: the vehicle a few metres from its origin, landmarks within sensor range of it."""
    n = 3 + 2 * N
    x = np.concatenate([[rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.6, 0.6)], rng.uniform(-30, 30, 2 * N)])
    A = rng.normal(0, 0.1, (n, rank))
    P = A @ A.T + 0.004 * np.eye(n)
    return x, (P + P.T) / 2


@pytest.fixture(scope="module")
def pairs_of_states():
    """One seeded (global, local) pair per shape, shared (and never written) by the tests below."""
    out = {}
    for NA, NB in SHAPES:
        rng = np.random.default_rng(7000 + 131 * NA + NB)
        out[(NA, NB)] = (random_state(rng, NA), local_state(rng, NB))
    return out


def _join_and_check(pkg, dtype, A, B, what, cap_extra=4):
    (xA, PA), (xB, PB) = A, B
    NA, NB = (len(xA) - 3) // 2, (len(xB) - 3) // 2
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=NA + NB + cap_extra)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=max(NB, 1))
    xa0, Pa0 = rounded(a)
    xb0, Pb0 = rounded(b)
    xab, Pab = a.download()
    xbb, Pbb = b.download()
    first = a.join(b)
    assert first == NA + 1 and a.N == NA + NB, what
    xo, Po = JR.join(xa0, Pa0, xb0, Pb0)
    xg, Pg = a.download()
    rx = JR.worst_ratio(xg, xo, JR.bound_x(xa0, xb0, dtype))
    rP = JR.worst_ratio(Pg, Po, JR.bound_P(xa0, Pa0, xb0, Pb0, dtype))
    print(f"{what}: worst error / bound  x {rx:.3f}  P {rP:.3f}")
    if rP > 1.0:                                        # where: the entry, its group pair, got and reference
        bP = JR.bound_P(xa0, Pa0, xb0, Pb0, dtype)
        q = np.abs(np.asarray(Pg, dtype=JR.LD) - Po) / np.where(bP > 0, bP, 1)
        for i in np.argsort(q.reshape(-1))[::-1][:6]:
            r, cc = divmod(int(i), q.shape[1])
            print(f"  P[{r}, {cc}] ratio {float(q[r, cc]):.3f}  got {float(Pg[r, cc])!r}  ref {float(Po[r, cc])!r}  bound {bP[r, cc]:.3e}")
    assert rx <= 1.0 and rP <= 1.0, f"{what}: x {rx:.3f} P {rP:.3f} of the bound"
    check_storage(a, pkg, Pg, what=what)
    assert np.array_equal(Pg, Pg.T), what
    nA = 3 + 2 * NA
    assert _eq_bits(Pg[3:nA, 3:nA], Pab[3:nA, 3:nA]) and _eq_bits(xg[3:nA], xab[3:nA]), f"{what}: a's landmark part changed"
    xb1, Pb1 = b.download()
    assert _eq_bits(xb1, xbb) and _eq_bits(Pb1, Pbb), f"{what}: b changed"
    check_storage(b, pkg, Pb1, what=what + " (b)")
    b.close()
    return a, xg, Pg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("NA,NB", SHAPES)
def test_join_against_the_restatement_entry_by_entry(pkg, pairs_of_states, dtype, NA, NB):
    E = SR.TILE[dtype]
    n2 = 3 + 2 * (NA + NB)
    strad = lambda N: [j for j in range(1, N + 1) if (MR.f(j) + 1) % E == 0]           # noqa: E731
    if (NA, NB) == (100, 130):                          # the shape holds what it is chosen for
        assert n2 == 463 and (n2 - 1) // E + 1 == (4 if dtype == "f32" else 8) and (2 * NA) % E != 0
    if (NA, NB) == (35, 40) and dtype == "f64":         # straddlers in the source and in the destination, and they do not coincide
        assert strad(NB) == [31] and strad(NA + NB) == [31, 63] and 31 + NA not in strad(NA + NB) and (2 * NA) % E != 0
    if (NA, NB) == (35, 40) and dtype == "f32":         # E = 128: b has no straddler; the destination's is b's landmark 28, which lies
        assert strad(NB) == [] and strad(NA + NB) == [63] and 63 - NA == 28 and (2 * NA) % E != 0       # inside a tile of b
    if (NA, NB) == (100, 130) and dtype == "f32":       # fp32 straddlers on BOTH sides that do not coincide: b's 63, 127; a's 63 (old), 127, 191
        assert strad(NB) == [63, 127] and strad(NA + NB) == [63, 127, 191] and not {63 + NA, 127 + NA} & set(strad(NA + NB))
    if (NA, NB) == ((62, 2) if dtype == "f32" else (30, 2)):
        assert strad(NA + NB) == [NA + 1]               # b's first landmark becomes the straddling pair
    A, B = pairs_of_states[(NA, NB)]
    a, _xg, _Pg = _join_and_check(pkg, dtype, A, B, f"{dtype} ({NA}, {NB})")
    a.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_filter_goes_on_from_the_joined_state(pkg, dtype):
    """a's landmarks lie in [5, 95]^2; b's are sent 150 m out (other grid cells) and one of them carries a variance above every
    old one.  The association on the joined state equals the oracle's in sweep and in grid mode, then an update follows it."""
    rng = np.random.default_rng(31)
    NA, NB = 60, 12
    xA, PA = random_state(rng, NA)
    xB, PB = local_state(rng, NB)
    xB[3:] = rng.uniform(120, 180, 2 * NB) * rng.choice([-1, 1], 2 * NB)
    PB[MR.f(5), MR.f(5)] += 4.0
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=NA + NB + 4)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=NB)
    a.set_gate_mode("grid")
    ids0 = rng.choice(np.arange(1, NA + 1), size=6, replace=False)
    a.associate_vector(noisy_obs(rng, xA, ids0), R, GATE1, GATE2)      # a grid and a variance bound of the OLD map exist
    a.join(b)
    b.close()
    xs, Ps = rounded(a)
    assert np.diag(Ps)[3 + 2 * NA:].max() > np.diag(Ps)[3:3 + 2 * NA].max()
    ids = np.concatenate([rng.choice(np.arange(1, NA + 1), size=5, replace=False), NA + np.array([1, 5, 9, 12])])
    z = np.hstack([noisy_obs(rng, xs, ids), np.array([[400.0], [0.4]])])
    nis, nd = O.association_table_sparse(xs, Ps, z, R)
    with np.errstate(invalid="ignore"):
        rel = min(float(np.nanmin(np.abs(nis - GATE1) / GATE1)), float(np.nanmin(np.abs(np.nanmin(nis, axis=1) - GATE2) / GATE2)))
    assert rel >= 0.01, f"a decision lies within 1 % of a gate ({rel:.4f})"
    want = O.assoc_vector(nis, nd, GATE1, GATE2)
    assert (want[:-1] > 0).sum() >= 6
    for mode in ("sweep", "grid"):
        a.set_gate_mode(mode)
        got = a.associate_vector(z, R, GATE1, GATE2)
        assert a.gate_info()["form"] == mode and np.array_equal(got, want), (mode, got.tolist(), want.tolist())
    zf, idf, _zn = O.split_assoc(z, want)
    a.update(zf, R, idf)
    xo, Po = O.update_sparse(xs, Ps, zf, R, idf)
    check_state(a, xo, Po, dtype, f"{dtype} update after the join", prior=Ps)
    check_storage(a, pkg, what="update after the join")
    a.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_join_then_find_and_merge(pkg, dtype):
    """b re-observes five of a's landmarks (their means expressed in b's frame, a little noise, small covariance): after the join
    exactly those five pairs are duplicates, and merging them equals tests/merge_ref.py on the joined state."""
    rng = np.random.default_rng(57)
    NA, NB = 40, 9
    xA = np.concatenate([[50.0, 50.0, 0.7], (np.stack(np.meshgrid(np.arange(8) * 11.0 + 8, np.arange(5) * 17.0 + 9), -1).reshape(-1, 2)).reshape(-1)])
    A = rng.normal(0, 0.02, (3 + 2 * NA, 5))
    PA = A @ A.T + 0.003 * np.eye(3 + 2 * NA)
    seen = np.array([3, 11, 18, 26, 37])
    c, s = math.cos(0.7), math.sin(0.7)
    xB, PB = local_state(rng, NB)
    xB[:3] = [1.0, -0.5, 0.1]
    PB *= 0.05
    for k, j in enumerate(seen):
        d = xA[MR.f(j):MR.f(j) + 2] - xA[:2]
        xB[MR.f(k + 1):MR.f(k + 1) + 2] = [c * d[0] + s * d[1] + rng.normal(0, 0.01), -s * d[0] + c * d[1] + rng.normal(0, 0.01)]
    xB[MR.f(6):] = rng.uniform(200, 260, 2 * (NB - 5))
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=NA + NB + 4)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=NB)
    a.join(b)
    b.close()
    xs, Ps = rounded(a)
    gate = 9.0
    pairs_ref, cnt_ref = MR.find(xs, Ps, gate)
    assert pairs_ref.tolist() == [[int(j), NA + k + 1] for k, j in enumerate(seen)]
    t = MR.d2_table(xs, Ps)
    assert np.min(np.abs(t[np.isfinite(t)] - gate) / gate) >= 0.01
    pairs, cnt = a.find_duplicates(gate)
    assert cnt == cnt_ref and np.array_equal(pairs, pairs_ref)
    ni = a.merge_landmarks(pairs)
    xr, Pr, nir = MR.merge(xs, Ps, pairs_ref)
    assert np.array_equal(ni, nir) and a.N == NA + NB - 5
    rm = pairs_ref[:, 1].astype(np.int64)
    keep = np.delete(np.arange(len(xs)), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))
    # measured as tests/test_gpu_ekf_merge.py measures a merge: every entry against the larger of its posterior and PRIOR scale (the
    # constraint takes the re-observed landmarks' variance from range^2 x heading variance down to b's), four times an update's tolerance
    check_state(a, xr, Pr, dtype, f"{dtype} join then merge", fx=4.0, fP=4.0, prior=Ps[np.ix_(keep, keep)])
    check_storage(a, pkg, what="join then merge")
    a.close()
    # the same through join(merge_gate=...)
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=NA + NB + 4)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=NB)
    first, new_index = a.join(b, merge_gate=gate)
    assert first == NA + 1 and np.array_equal(new_index, nir) and a.N == NA + NB - 5
    b.close()
    a.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_overflow_and_bad_arguments_leave_both_states_bit_identical(pkg, pairs_of_states, dtype):
    (xA, PA), (xB, PB) = pairs_of_states[(35, 40)]
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=35 + 39)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=40)
    other = pkg.EKFSlamState(xB, PB, dtype="f32" if dtype == "f64" else "f64", max_landmarks=40)
    snaps = [(SR.snapshot(h), h.download("x"), h.landmark_blocks(), h.N) for h in (a, b)]
    lib = pkg._lib.join_lib()
    first = C.c_int32(-7)
    assert lib.slam_ekf_join(a._h, b._h, C.byref(first)) == pkg._lib.SLAM_E_CAPACITY
    for args in ((None, b._h), (a._h, None), (a._h, a._h), (a._h, other._h)):
        assert lib.slam_ekf_join(args[0], args[1], C.byref(first)) == pkg._lib.SLAM_E_BADARG, args
    assert first.value == -7
    with pytest.raises(pkg.SlamHipError) as ei:
        a.join(b)
    assert ei.value.code == pkg._lib.SLAM_E_CAPACITY
    for h, (snap, x0, blk0, N0) in zip((a, b), snaps):
        assert SR.changed_offsets(h, snap).size == 0 and _eq_bits(h.download("x"), x0) and _eq_bits(h.landmark_blocks(), blk0) and h.N == N0
    for h in (a, b, other):
        h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_join_is_ordered_behind_bs_async_update_and_survives_bs_destruction(pkg, pairs_of_states, dtype):
    (xA, PA), (xB, PB) = pairs_of_states[(35, 40)]
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=80)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=40)
    xa0, Pa0 = rounded(a)
    xb0, Pb0 = rounded(b)
    rng = np.random.default_rng(8)
    ids = np.array([2, 9, 17, 33])
    z = noisy_obs(rng, xb0, ids)
    b.set_async(True)
    b.update(z, R, ids)                                  # enqueued on b's stream, status deferred
    a.join(b)
    b.close()                                            # destroyed right after the call
    xb1, Pb1 = O.update_sparse(xb0, Pb0, z, R, ids.reshape(1, -1))
    xo, Po = JR.join(xa0, Pa0, xb1, Pb1)
    check_state(a, xo.astype(np.float64), Po.astype(np.float64), dtype, f"{dtype} join behind b's async update")
    check_storage(a, pkg, what="join behind an async update")
    a.close()
    # a failed asynchronous update of b is returned by the join; a is untouched
    a = pkg.EKFSlamState(xA, PA, dtype=dtype, max_landmarks=80)
    b = pkg.EKFSlamState(xB, PB, dtype=dtype, max_landmarks=40)
    snap, x0, N0 = SR.snapshot(a), a.download("x"), a.N
    zp, _ = O.predict_observation(xb0, 3)
    zz = np.stack([zp + [0.01, 0.0005], zp - [0.01, 0.0005]], axis=1)
    b.set_async(True)
    b.update(zz, -1e-5 * np.eye(2), [3, 3])
    with pytest.raises(pkg.NotPositiveDefinite):
        a.join(b)
    assert SR.changed_offsets(a, snap).size == 0 and _eq_bits(a.download("x"), x0) and a.N == N0
    b.sync()
    assert a.join(b) == N0 + 1                           # ... and the status was consumed: the join now goes through
    for h in (a, b):
        h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_with_submaps_on_the_golden_course(pkg, golden_dir, dtype):
    S = pkg.sim
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    wp = S.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    st = pkg.EKFSlamState(S.initial_pose(wp), np.zeros((3, 3)), dtype=dtype, max_landmarks=400)
    k = 25
    log = S.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=1, submap_steps=k, merge_gate=9.0, fused=True)
    assert st is not None and len(log.joined) == len(log.obs_steps) // k + 1
    assert all(j[1] >= 1 for j in log.joined) and log.joined[-1][3] == st.N and st.N >= 1
    assert len(log.slam_track) == len(log.true_track) == len(log.controls)
    xg, Pg = st.download()
    check_storage(st, pkg, Pg, what=f"{dtype} sim with submaps")
    np.linalg.cholesky(np.asarray(Pg, dtype=np.float64))
    err = np.linalg.norm(np.array(log.slam_track)[:, :2] - np.array(log.true_track)[:, :2], axis=1)
    print(f"{dtype} submaps: {len(log.joined)} joins, {st.N} landmarks, track error mean {err.mean():.3f} max {err.max():.3f} m")
    st.close()
