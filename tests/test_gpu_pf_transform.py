"""The FastSLAM filter expressed in another frame on the device (slam_pf_transform, csrc/pf_transform.hip) against the
restatement of tests/transform_ref.py (`records`, `poses`): every value of every record in use within the per-record bound
(one rounding to the dtype, a handful of double operations), every record NOT in use and every log-weight bit for bit; the map
read-out before and after; after lazy resampling (live ancestor tables: the call must materialise); with a normalisation
shift pending; the record whose Pxx would round to zero; the filter going on afterwards against the fp64 oracle; and two
in-process shards with peers attached against the one-shard filter."""
import math
import threading

import numpy as np
import pytest

from oracle import pf_ref as F
from tests import transform_ref as X
from tests.test_gpu_pf import Q, R, TOL, close, observe, scene
from tests.test_gpu_pf_map import BOUND, _ThreadComm, advance

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
SIZES = [1, 255, 4097]
NSLOTS = 6
G = (12.0, -7.0, 2.4)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def known_filter(pkg, n, dtype, steps=4):
    """Landmarks 1..4 initialised and observed (5 first seen on the way), 6 never seen: its records are all zero."""
    lm = scene(NSLOTS, 3)
    sh = pkg.PFShard(n, NSLOTS, 31, dtype=dtype)
    sh.set_pose([1.0, -2.0, 3.0])                      # (a heading that wraps under theta = 2.4)
    sh.init_landmarks(lm[:4], 0.01, 0.1)
    rng = np.random.default_rng(2)
    pose = np.array([1.0, -2.0, 3.0])
    for t in range(steps):
        sh.predict(6.0, 0.05 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.6, 0.05 * t)
        ids = np.array([1 + t % 4, 1 + (t + 1) % 4, 5])
        sh.update_known(observe(lm, pose, ids, rng), ids, R)
    return sh, np.array([1, 1, 1, 1, 1, 0], dtype=bool), steps, pose, lm


def unknown_filter(pkg, n, dtype):
    """Every slot emptied by clear_landmarks, some refilled by update_unknown, slot 1 then overwritten by init_landmarks with
    var = 0: a used record with Pxx == 0, in use only because the landmark is `seen`."""
    lm = np.array([[12.0, 3.0], [6.0, -9.0], [-10.0, 4.0], [15.0, -2.0]])
    sh = pkg.PFShard(n, NSLOTS, 11, dtype=dtype)
    sh.set_pose([0.5, -0.5, 0.3])
    sh.clear_landmarks()
    rng = np.random.default_rng(5)
    pose = np.array([0.5, -0.5, 0.3])
    for t in range(3):
        sh.predict(3.0, 0.02 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.3, 0.02 * t)
        sh.update_unknown(observe(lm, pose, np.array([1, 2, 3, 4][:2 + t % 3]), rng), R, 4.0, 25.0)
    sh.init_landmarks(np.array([[2.0, 3.0]]), 0.0, 0.0)
    return sh, np.array([1, 0, 0, 0, 0, 0], dtype=bool), 3


def check_transform(sh, seen, g, dtype, what, pending=False, peek=False):
    """download, transform, download: the restatement's bounds; unused records, log-weights, map counts and masses unchanged; the
    map read-out moves with the frame.  Returns the download after.  `peek`: the state before is read particle by particle
    (slam_pf_get_particle: through the ancestor tables, nothing is materialised or flushed by looking), and so are the map
    read-outs before the call; `pending`: the same, right after a normalize whose shift is still pending."""
    if pending:                                        # the shift is PENDING now and stays so
        gm, s1, _ = sh.weight_stats()
        sh.normalize(gm, s1)
    if pending or peek:
        p0, w0, l0 = _peek(sh)
    else:
        p0, w0, l0 = sh.download()
    sums0 = sh.map_sums()
    whole = sh.n == sh.n_global
    map0 = sh.get_map() if whole else None
    sh.transform(*g)
    p1, w1, l1 = sh.download()
    want_l, bound_l, use = X.records(l0, seen, *g, dtype)
    want_p, bound_p = X.poses(p0, *g, dtype)
    rl = X.worst_ratio(l1, want_l, bound_l)
    rp = X.worst_ratio(p1, want_p, bound_p)
    print(f"{what}: worst error / bound  records {rl:.3f}  poses {rp:.3f}  ({int(use.sum())} of {use.size} records in use)")
    assert rl <= 1.0 and rp <= 1.0, what
    keep = np.broadcast_to(~use[:, None, :], l0.shape)
    assert _bits_equal(l1[keep], l0[keep]), f"{what}: a record not in use changed"
    assert _bits_equal(w1, w0), f"{what}: log-weights changed"
    assert np.array_equal(X.in_use(l1[:, 2, :], seen), use), f"{what}: a record changed sides"
    sums1 = sh.map_sums()
    assert np.array_equal(sums1[:, 9], sums0[:, 9]) and np.array_equal(sums1[:, 0], sums0[:, 0]), f"{what}: counts / masses"
    if whole:
        _check_map(sh.get_map(), map0, l0, bound_l, use, sh.weights(), g, what)
    return p1, w1, l1


def _peek(sh):
    """The state with a normalisation shift PENDING, without flushing it: a twin download would apply it.  The pending shift only
    concerns the log-weights, which the transform must not touch; poses and records are read through one particle at a time."""
    n, nl = sh.n, sh.nl
    pose = np.empty((3, n), dtype=sh.np_dtype)
    lm = np.empty((nl, 5, n), dtype=sh.np_dtype)
    logw = np.empty(n, dtype=sh.np_dtype)
    for i in range(n):
        _gid, lw, p, rec = sh.particle(i)
        pose[:, i], lm[:, :, i], logw[i] = p, rec, lw
    return pose, logw, lm


def _check_map(m1, m0, l0, bound_l, use, w, g, what):
    """get_map after = the transformed get_map before: mean' = R mean + t, C' = R C R'.  Tolerance: the records' bounds summed over
    the contributors with their weights (a mean moves by at most the weighted mean of its contributors' errors; the spread
    term of C by 2 |m - mean| times that), plus the read-out's own summation bound (tests/test_gpu_pf_map.py) on both calls."""
    c, s = X.cs_of(g[2])
    Rm = np.array([[c, -s], [s, c]])
    for l in range(m0.shape[0]):
        u = use[l]
        assert m1[l, 6] == m0[l, 6] == u.sum() and m1[l, 0] == m0[l, 0]
        if not u.any():
            assert not m1[l].any()
            continue
        wl = np.where(u, w, 0.0)
        W = wl.sum()
        mean = Rm @ m0[l, 1:3] + np.array(g[:2])
        C0 = np.array([[m0[l, 3], m0[l, 4]], [m0[l, 4], m0[l, 5]]])
        C = Rm @ C0 @ Rm.T
        rec = l0[l].astype(np.float64)
        eb = (wl * bound_l[l]).sum(axis=1) / W                                  # [5]: weighted mean of the per-value bounds
        mag = (wl * (np.abs(rec[0]) + np.abs(rec[1]) + abs(g[0]) + abs(g[1]))).sum() / W
        mag2 = (wl * (np.abs(rec[0]) + np.abs(rec[1]) + abs(g[0]) + abs(g[1])) ** 2).sum() / W
        tol_m = eb[:2].max() + 4 * BOUND * mag
        assert np.all(np.abs(m1[l, 1:3] - mean) <= tol_m), (what, l, m1[l, 1:3], mean, tol_m)
        tol_C = eb[2:].max() + 4 * mag * eb[:2].max() + 8 * BOUND * mag2 + 4 * BOUND * np.abs(C0).max()
        got = np.array([m1[l, 3], m1[l, 4], m1[l, 5]])
        assert np.all(np.abs(got - [C[0, 0], C[0, 1], C[1, 1]]) <= tol_C), (what, l, got, C, tol_C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_mixed_filters_against_the_restatement(pkg, dtype, n):
    for build in (known_filter, unknown_filter):
        sh, seen = build(pkg, n, dtype)[:2]
        _p, _w, l = sh.download()
        use = X.in_use(l[:, 2, :], seen)
        if build is known_filter:
            assert use[:5].all() and not use[5].any() and not l[5].any()          # five in use, one never seen: all zero
        else:
            assert use[0].all() and not l[0, 2:].any() and np.any(l[1:, 2, :] == -1) and np.any(l[1:, 2, :] > 0)
        check_transform(sh, seen, G, dtype, f"{build.__name__} {dtype} n={n}")
        check_transform(sh, seen, (0.0, 0.0, 7.0), dtype, f"{build.__name__} {dtype} n={n} theta=7")
        sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_after_lazy_resampling_and_with_a_pending_shift(pkg, dtype, n):
    sh, seen, _steps, pose, lm = known_filter(pkg, n, dtype)
    rng = np.random.default_rng(17)
    for k in range(2):                                 # two resamplings: composed ancestor tables, maps not yet moved
        gm, _s1, _s2 = sh.weight_stats()
        sh.resample_local(gm, pkg.philox_uniform(k, 2, 31))
        if k == 0:                                     # an update in between: some landmarks move, others stay behind tables
            sh.predict(6.0, 0.0, 4.0, Q, 0.1)
            pose = advance(pose, 0.6)
            sh.update_known(observe(lm, pose, np.array([2]), rng), np.array([2]), R)
    # the SAME checks as everywhere else, map read-out included: here the read-out before the call goes through the live tables
    # and the one after it through the records the call has materialised
    check_transform(sh, seen, G, dtype, f"lazy tables {dtype} n={n}", peek=True)
    # ... and once more with a normalisation shift pending
    sh.predict(6.0, 0.1, 4.0, Q, 0.1)
    c, s_ = X.cs_of(G[2])
    lmT = (np.array([[c, -s_], [s_, c]]) @ lm.T).T + np.array(G[:2])          # the scene and the pose in the new frame
    poseT = np.array([c * pose[0] - s_ * pose[1] + G[0], s_ * pose[0] + c * pose[1] + G[1], pose[2] + G[2]])
    sh.update_known(observe(lmT, advance(poseT, 0.6, 0.1), np.array([3]), rng), np.array([3]), R)
    check_transform(sh, seen, (-3.0, 8.0, -1.1), dtype, f"pending shift {dtype} n={n}", pending=True)
    sh.close()


@pytest.mark.parametrize("dtype,var", [("f32", 1e-30), ("f64", 1e-300)])
def test_a_record_whose_variance_rounds_to_zero_stays_in_use(pkg, dtype, var):
    """P = diag(var, 0) turned by pi/2: Pxx' = c^2 var underflows; the record keeps the smallest positive normal number as its
    in-use mark.  The records are brought in as a resampling step's remote records."""
    import torch
    n = 255
    sh = pkg.PFShard(n, NSLOTS, 3, dtype=dtype, first=0, n_global=2 * n)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.clear_landmarks()
    rec = np.zeros((3 + 5 * NSLOTS, n), dtype=sh.np_dtype)
    rec[5:3 + 5 * NSLOTS:5] = -1.0                    # every slot empty ...
    rec[3:8] = np.array([4.0, -2.0, var, 0.0, 0.0], dtype=sh.np_dtype)[:, None]      # ... but slot 1
    ids = torch.arange(n, 2 * n, dtype=torch.int32, device="cuda")
    sh.resample_apply(ids.clone(), ids, torch.as_tensor(rec, device="cuda"))
    seen = np.zeros(NSLOTS, dtype=bool)
    _p, _w, l0 = sh.download()
    assert np.all(l0[0, 2] == sh.np_dtype(var)) and np.all(l0[1:, 2] == -1)
    cnt0 = sh.map_sums()[:, 9].copy()
    assert cnt0[1] == n and not cnt0[2:].any()
    sh.transform(1.0, 1.0, math.pi / 2)
    _p, _w, l1 = sh.download()
    want, bound, use = X.records(l0, seen, 1.0, 1.0, math.pi / 2, dtype)
    assert np.all(l1[0, 2] == sh.np_dtype(X.TINY[dtype])) and np.all(l1[0, 4] == sh.np_dtype(var))
    assert X.worst_ratio(l1, want, bound) <= 1.0 and _bits_equal(l1[1:], l0[1:])
    assert np.array_equal(sh.map_sums()[:, 9], cnt0)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_filter_goes_on_after_the_transform(pkg, dtype):
    """step_fused after the transform against the fp64 oracle started from the downloaded, transformed state -- with the RNG step
    the filter had BEFORE the transform: the call consumed none."""
    n = 4097
    sh, seen, steps, _pose, _lm = known_filter(pkg, n, dtype)
    sh.transform(*G)
    p, w, l = sh.download()
    orc = F.OraclePF(n, NSLOTS, 31)
    orc.pose, orc.logw, orc.lm = p.astype(np.float64), w.astype(np.float64), l.astype(np.float64)
    orc.seen, orc.step = seen.copy(), steps
    lm = scene(NSLOTS, 3)
    c, s = X.cs_of(G[2])
    lmT = (np.array([[c, -s], [s, c]]) @ lm.T).T + np.array(G[:2])               # the scene in the new frame
    pose = orc.pose[:, 0].copy()
    ids = np.array([2, 4, 6, 2])                       # a repeat and the first sighting of landmark 6
    z = observe(lmT, advance(pose, 0.6, 0.02), ids, np.random.default_rng(8))
    sh.step_fused(6.0, 0.02, 4.0, Q, 0.1, z, ids, R)
    orc.predict(6.0, 0.02, 4.0, Q, 0.1)
    orc.update_known(z, ids, R)
    p1, w1, l1 = sh.download()
    tol = TOL[dtype]
    assert close(p1, orc.pose, tol) and close(l1[:, 0:2], orc.lm[:, 0:2], tol)
    assert close(l1[:, 2:5], orc.lm[:, 2:5], tol * 10, scale=float(np.max(np.abs(orc.lm[:, 2:5]))))
    assert close(w1, orc.logw, tol * 10, scale=max(1.0, float(np.max(np.abs(orc.logw)))))
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_align_fits_the_map_means_back_onto_surveyed_positions(pkg, dtype):
    """FastSLAM.align from map() means: after a transform by g, fitting landmarks 1..4 onto their means of before returns g^-1
    (1e-9 in fp64, 1e-4 in fp32 as for the EKF: rounded means at a scale of tens of metres); applied, the means move by exactly the
    returned transform, at rounding level (the distance to the surveyed positions, which holds the fit's own error, is printed)."""
    sh = known_filter(pkg, 255, dtype)[0]
    f = pkg.FastSLAM(sh, None)
    ids = [1, 2, 3, 4]
    before = f.map(ids)[:, 1:3]
    f.transform(*G)
    tol = 1e-9 if dtype == "f64" else 1e-4
    want = X.inverse(*G)
    got = f.align(ids, before, apply=False)
    assert all(abs(p - q) <= tol for p, q in zip(got[:2], want[:2])) and abs(math.remainder(got[2] - want[2], 2 * math.pi)) <= tol, (got, want)
    # what is applied is what is returned: the means after against the returned transform of the means just before, within the
    # records' bound of one call (weighted means of values of size M, each within (u + slack) M) and the read-out's summation bound
    moved = f.map(ids)[:, 1:3]
    assert f.align(ids, before.T) == got                # [2, k] as well; applies
    c, s_ = X.cs_of(got[2])
    expect = (np.array([[c, -s_], [s_, c]]) @ moved.T).T + np.array(got[:2])
    M = 2.0 * float(np.max(np.abs(moved))) + abs(got[0]) + abs(got[1])
    after = f.map(ids)[:, 1:3]
    bound = (X.U[dtype] + X.SLACK) * M + 8 * BOUND * M
    print(f"{dtype} FastSLAM align: means after against the returned transform / bound {float(np.max(np.abs(after - expect))) / bound:.3f}; "
          f"against the surveyed positions {float(np.max(np.abs(after - before))):.3e} m")
    assert np.all(np.abs(after - expect) <= bound)
    with pytest.raises(ValueError):
        f.align([1], before[:1])
    with pytest.raises(ValueError):
        f.align([6, 1], before[:2])                     # landmark 6 was never seen: nothing to fit
    sh.close()


def test_bad_arguments_leave_the_filter_alone(pkg):
    sh = known_filter(pkg, 255, "f32")[0]
    before = sh.download()
    for bad in ((math.nan, 0.0, 0.0), (0.0, -math.inf, 0.0), (0.0, 0.0, math.nan)):
        assert pkg._lib.frame_lib().slam_pf_transform(sh._h, *bad) == pkg._lib.SLAM_E_BADARG
    after = sh.download()
    assert all(_bits_equal(a, b) for a, b in zip(before, after))
    sh.close()


@pytest.mark.parametrize("dtype,world", [("f32", 2), ("f64", 3)])
def test_shards_with_peers_equal_the_one_shard_filter(pkg, dtype, world):
    """The collective call on every rank after steps that resampled (remote ancestors behind the tables) against the one-shard
    filter: bit for bit."""
    per, nl, seed = 2048, NSLOTS, 77
    n = per * world
    lm = scene(nl, 19)
    ref_shard = pkg.PFShard(n, nl, seed, dtype=dtype)
    shards = [pkg.PFShard(per, nl, seed, dtype=dtype, first=r * per, n_global=n) for r in range(world)]
    for sh in shards + [ref_shard]:
        sh.set_pose([0.5, 1.5, -0.2])
        sh.init_landmarks(lm[:4], 0.01, 0.1)
    pkg.attach_local_peers(shards)
    comm = _ThreadComm(world)
    ref = pkg.FastSLAM(ref_shard, None, neff_frac=0.75)
    ranks = [pkg.FastSLAM(sh, comm.view(r), neff_frac=0.75) for r, sh in enumerate(shards)]
    rng = np.random.default_rng(6)
    pose = np.array([0.5, 1.5, -0.2])
    steps = []
    for t in range(6):
        pose = advance(pose, 0.6)
        ids = np.array([1 + t % 4, 1 + (t + 2) % 4, 5])
        steps.append((0.01 * (t % 5), observe(lm, pose, ids, rng), ids, None if t % 3 == 2 else True))
    for g, z, ids, force in steps:
        ref.step_async(6.0, g, 4.0, Q, 0.1, z, ids, R, force_resample=force)
    ref.flush()
    assert ref.resamples >= 3
    ref.transform(*G)
    want = ref_shard.download()
    got, errs = [None] * world, []

    def drive(r):
        try:
            f = ranks[r]
            assert f.shard.peer_selftest(10000)
            for g, z, ids, force in steps:
                f.step_async(6.0, g, 4.0, Q, 0.1, z, ids, R, force_resample=force)
            f.flush()
            f.transform(*G)                            # collective: the remote records come home first
            got[r] = f.shard.download()
        except BaseException as e:                     # noqa: BLE001 -- reported by the main thread
            errs.append((r, e))
            comm.bar.abort()

    th = [threading.Thread(target=drive, args=(r,)) for r in range(world)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not errs, errs
    assert all(g is not None for g in got)
    assert _bits_equal(np.hstack([g[0] for g in got]), want[0]) and _bits_equal(np.concatenate([g[1] for g in got]), want[1])
    assert _bits_equal(np.concatenate([g[2] for g in got], axis=2), want[2])
    th = [threading.Thread(target=sh.detach_peers) for sh in shards]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    for sh in shards + [ref_shard]:
        sh.close()
