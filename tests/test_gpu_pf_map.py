"""GPU tests of the FastSLAM map read-out (slam_pf_map_sums / slam_pf_get_map / slam_pf_get_particle via slam.jl_amd/pf.py).

The expectations are formed in this file, in extended precision, from what the device itself reports about its state
(download() and weights()), and -- one case -- from the independent fp64 oracle (oracle/pf_ref.py).

Tolerance of a sum: 4096 * 2^-53 * 2 * sum w |v| with the absolute-value sum formed here -- the standard bound of a
floating-point sum whose longest chain of additions has at most 4096 terms (the kernel's: 16 per thread, 9 in the workgroup,
slabs / 64 + 6 in the fold), doubled for the rounding of the products.  Counts are exact.
"""
import ctypes
import math
import threading

import numpy as np
import pytest

from oracle import pf_ref as F

pytestmark = pytest.mark.gpu

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
TOL = {"f64": 1e-9, "f32": 2e-4}
LD = np.longdouble
BOUND = 4096 * 2.0 ** -53 * 2


def scene(nl, seed):
    return np.random.default_rng(seed).uniform(-40, 40, (nl, 2))


def observe(lm, pose, ids, rng):
    dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
    return np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))


def advance(pose, d, g=0.0):
    return np.array([pose[0] + d * math.cos(g + pose[2]), pose[1] + d * math.sin(g + pose[2]), pose[2] + d * math.sin(g) / 4.0])


def expected_sums(pose, w, lm, ids):
    """(rows [1 + cnt, 10], tolerance of every entry) in extended precision from a download: pose [3, n], w [n] (the
    weights()), lm [nl, 5, n], ids 1-based.  A record is in use when Pxx > 0."""
    w = w.astype(LD)
    rows, tol = np.zeros((1 + len(ids), 10), dtype=LD), np.zeros((1 + len(ids), 10))

    def put(r, cols, used):
        wu = np.where(used, w, LD(0))
        for k, v in enumerate(cols):
            if v is None:
                continue
            v = v.astype(LD)
            rows[r, k] = (wu * v).sum()
            tol[r, k] = BOUND * float((wu * np.abs(v)).sum())
        rows[r, 9] = used.sum()

    x, y, phi = (pose[k].astype(np.float64) for k in range(3))
    one = np.ones_like(x)
    put(0, [one, x, y, x * x, x * y, y * y, np.sin(phi), np.cos(phi), None], np.ones(len(x), bool))
    # (sin / cos in double, as on the device: their own rounding, one ulp of a value below 1, is far inside the bound)
    for i, l1 in enumerate(ids):
        rec = lm[l1 - 1].astype(np.float64)
        mx, my = rec[0], rec[1]
        put(1 + i, [one, mx, my, mx * mx, mx * my, my * my, rec[2], rec[3], rec[4]], rec[2] > 0)
    return rows, tol


def check_sums(got, pose, w, lm, ids, what):
    want, tol = expected_sums(pose, w, lm, ids)
    assert got.shape == want.shape, what
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    print(f"{what}: largest error / tolerance {float(np.max(err[:, :9] / np.maximum(tol[:, :9], 1e-300))):.3g}")
    assert np.all(err[:, :9] <= tol[:, :9]), (what, np.argwhere(err[:, :9] > tol[:, :9])[:5], err.max())
    assert np.array_equal(got[:, 9], want[:, 9].astype(np.float64)), (what, "counts")
    return want, tol


def check_map(got_map, sums, pkg, what):
    """get_map against the finalisation of the sums; entries of C to 1e-11 * sum w |m|^2 / W_l (the cancellation scale)."""
    want = pkg.pf.finalise_map(sums)
    assert got_map.shape == want.shape
    r = sums[1:]
    has = r[:, 0] > 0
    assert not got_map[~has].any(), what
    scale = np.where(has, (r[:, 3] + r[:, 5]) / np.where(has, r[:, 0], 1.0), 0.0)
    assert np.allclose(got_map[:, :3], want[:, :3], rtol=1e-13, atol=0), what
    assert np.all(np.abs(got_map[:, 3:6] - want[:, 3:6]) <= 1e-11 * scale[:, None]), what
    assert np.array_equal(got_map[:, 6:], want[:, 6:]), what


# ---- 1: against the device's own state ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3001, 70000])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_map_sums_against_the_devices_own_state(pkg, dtype, n):
    """update_known steps with first sightings; landmarks 11 and 12 are never seen.  n = 3001 is no multiple of the vector
    width (every landmark takes the particle-by-particle kernel), 70000 takes the 16-byte loads."""
    nl, seed = 12, 77
    lm = scene(nl, 1)
    sh = pkg.PFShard(n, nl, seed, dtype=dtype)
    sh.set_pose([1.0, -2.0, 0.4])
    sh.init_landmarks(lm[:7], 0.01, 0.1)
    rng = np.random.default_rng(2)
    pose = np.array([1.0, -2.0, 0.4])
    for t in range(6):
        sh.predict(6.0, 0.05 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.6, 0.05 * t)
        ids = np.array([(2 * t) % 10 + 1, (2 * t + 1) % 10 + 1, 8 + t % 3, (2 * t) % 10 + 1])
        sh.update_known(observe(lm, pose, ids, rng), ids, R)
    every = list(range(1, nl + 1))
    for stage in ("unnormalised", "right after normalize"):
        if stage != "unnormalised":
            gm, s1, _ = sh.weight_stats()
            sh.normalize(gm, s1)                     # the shift is PENDING now: the query must honour it
        sums = sh.map_sums()
        again = sh.map_sums()
        assert sums.tobytes() == again.tobytes(), "two calls, different bytes"
        sub = sh.map_sums([12, 3, 9, 3])
        gmap = sh.get_map()
        best = sh.particle(-1)
        w = sh.weights()                             # (flushes the pending shift: the same weights, now stored)
        p, lw, l = sh.download()
        check_sums(sums, p, w, l, every, f"{dtype} n={n} {stage}")
        check_sums(sub, p, w, l, [12, 3, 9, 3], f"{dtype} n={n} {stage} subset")
        assert np.array_equal(sub[2], sums[3]) and np.array_equal(sub[4], sub[2])
        assert not sums[11].any() and not sums[12].any(), "a landmark never seen is ten zeros"
        assert sums[0, 9] == n
        if stage != "unnormalised":
            assert sums[0, 0] == pytest.approx(1.0, rel=1e-5 if dtype == "f32" else 1e-12)
        check_map(gmap, sums, pkg, stage)
        check_map(pkg.FastSLAM(sh).map(), sums, pkg, stage + " (driver)")
        k = int(np.argmax(lw))
        assert best[0] == k and best[1] == float(lw[k])
        assert np.array_equal(best[2], p[:, k].astype(np.float64)) and np.array_equal(best[3], l[:, :, k].astype(np.float64))
        some = sh.particle(n - 1, landmarks=False)
        assert some[0] == n - 1 and some[1] == float(lw[n - 1]) and some[3] is None
    sh.close()


# ---- 2, 5, 6: through live ancestor tables; the query is read-only -------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [("f64", 5000), ("f32", 8192 + 4), ("f32", 4099)])
def test_map_through_live_tables_and_the_query_changes_nothing(pkg, dtype, n):
    nl, seed = 20, 5
    lm = scene(nl, 9)
    f = [pkg.FastSLAM(pkg.PFShard(n, nl, seed, dtype=dtype)) for _ in range(2)]          # [queried, twin]
    for g in f:
        g.shard.set_pose([0.0, 0.0, 0.1])
        g.shard.init_landmarks(lm[:15], 0.01, 0.1)
    rng = np.random.default_rng(4)
    pose = np.array([0.0, 0.0, 0.1])

    def step(t, force):
        nonlocal pose
        pose = advance(pose, 0.5)
        ids = np.array([1 + (3 * t) % 15, 1 + (3 * t + 1) % 15, 16 + t % 4])            # landmark 20 is never seen
        z = observe(lm, pose, ids, rng)
        for g in f:
            g.step_async(5.0, 0.0, 4.0, Q, 0.1, z, ids, R, force_resample=force)

    for t in range(12):
        step(t, True)
    q = f[0].shard
    subset = [2, 19, 7, 20, 11]
    sub = q.map_sums(subset)                        # the FIRST legacy call after the auto steps: it sees the lazy state
    sums = q.map_sums()
    assert sums.tobytes() == q.map_sums().tobytes()
    best = q.particle(-1)
    mid = q.particle(n // 2)
    gmap = q.get_map()
    w = q.weights()
    p, lw, l = q.download()                         # (materialises)
    check_sums(sums, p, w, l, list(range(1, nl + 1)), f"{dtype} n={n} live tables")
    check_sums(sub, p, w, l, subset, f"{dtype} n={n} live tables, subset")
    check_map(gmap, sums, pkg, "live tables")
    assert not sums[20].any()
    check_sums(q.map_sums(), p, w, l, list(range(1, nl + 1)), f"{dtype} n={n} after the download materialised the maps")
    # right after a resampling all weights are equal: the best particle is index 0
    assert best[0] == 0 and best[1] == float(lw[0])
    assert np.array_equal(best[3], l[:, :, 0].astype(np.float64)) and np.array_equal(best[2], p[:, 0].astype(np.float64))
    assert mid[0] == n // 2 and np.array_equal(mid[3], l[:, :, n // 2].astype(np.float64))
    # now query in the middle of further steps (no download in between: the tables stay alive) and compare with the twin
    for t in range(12, 20):
        step(t, None if t % 2 else True)
        if t in (14, 17):
            q.map_sums(subset)
            q.particle(-1)
            f[0].map()
    a, b = f[0].shard.download(), f[1].shard.download()
    for x, y, name in zip(a, b, ("poses", "log-weights", "records")):
        assert np.array_equal(x, y), f"the queried filter's {name} differ from its twin's"
    for g in f:
        g.shard.close()


# ---- 3: unknown correspondences -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_map_of_an_unknown_correspondence_run(pkg, dtype):
    """Gates (2, 6) make the particles disagree about the use of the last slot (checked on the oracle alone first)."""
    n, nslots, seed = 1500 + 13, 6, 11
    lm = np.array([[12.0, 3.0], [6.0, -9.0], [-10.0, 4.0], [15.0, -2.0], [-4.0, -12.0], [9.0, 11.0], [-13.0, -6.0]])
    sh = pkg.PFShard(n, nslots, seed, dtype=dtype)
    orc = F.OraclePF(n, nslots, seed)
    for g in (sh, orc):
        g.set_pose([0.5, -0.5, 0.3])
        g.clear_landmarks()
    assert not sh.map_sums()[1:].any(), "an empty map"
    rng = np.random.default_rng(5)
    pose = np.array([0.5, -0.5, 0.3])
    for t, ids in enumerate([[1, 2], [2, 1, 3], [1, 3, 4, 2], [5, 1]]):
        for g in (sh, orc):
            g.predict(3.0, 0.02 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.3, 0.02 * t)
        z = observe(lm, pose, np.array(ids), rng)
        sh.update_unknown(z, R, 2.0, 6.0)
        orc.update_unknown(z, R, 2.0, 6.0)
    cnt_o = (orc.lm[:, 2, :] > 0).sum(axis=1)
    assert np.any((cnt_o > 0) & (cnt_o < n)), "the inputs must leave a slot that only some particles use"
    sums = sh.map_sums()
    w = sh.weights()
    p, _lw, l = sh.download()
    cnt = (l[:, 2, :] > 0).sum(axis=1)
    assert np.any((cnt > 0) & (cnt < n))
    assert np.array_equal(sums[1:, 9], cnt.astype(np.float64))
    check_sums(sums, p, w, l, list(range(1, nslots + 1)), f"{dtype} unknown correspondences")
    check_map(sh.get_map(), sums, pkg, "unknown correspondences")
    sh.close()


# ---- 4: against the independent oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_map_against_the_oracle(pkg, dtype):
    n, nl, seed = 3000, 10, 77
    lm = scene(nl, 1)
    sh = pkg.PFShard(n, nl, seed, dtype=dtype)
    orc = F.OraclePF(n, nl, seed)
    for g in (sh, orc):
        g.set_pose([1.0, -2.0, 0.4])
        g.init_landmarks(lm[:7], 0.01, 0.1)
    rng = np.random.default_rng(2)
    pose = np.array([1.0, -2.0, 0.4])
    for t in range(6):
        for g in (sh, orc):
            g.predict(6.0, 0.05 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.6, 0.05 * t)
        ids = np.array([(2 * t) % nl + 1, (2 * t + 1) % nl + 1, 8 + t % 3, (2 * t) % nl + 1])
        z = observe(lm, pose, ids, rng)
        for g in (sh, orc):
            g.update_known(z, ids, R)
    got = sh.get_map()
    w = np.exp(orc.logw - orc.logw.max())
    w /= w.sum()
    mean = (orc.lm[:, 0:2, :] * w).sum(axis=2)                                   # [nl, 2]
    d = orc.lm[:, 0:2, :] - mean[:, :, None]
    cov = np.stack([(w * (orc.lm[:, 2] + d[:, 0] ** 2)).sum(axis=1), (w * (orc.lm[:, 3] + d[:, 0] * d[:, 1])).sum(axis=1),
                    (w * (orc.lm[:, 4] + d[:, 1] ** 2)).sum(axis=1)], axis=1)
    tol = TOL[dtype] * 50
    assert np.all(got[:, 0] == pytest.approx(1.0, rel=tol)) and np.all(got[:, 6] == n)
    assert np.max(np.abs(got[:, 1:3] - mean)) <= tol * np.max(np.abs(mean))
    assert np.max(np.abs(got[:, 3:6] - cov)) <= 10 * tol * np.max(np.abs(cov))
    s0 = sh.map_sums([])[0]                                                      # the pose row against the oracle's sums
    assert np.allclose(s0[[1, 2, 6, 7]] / s0[0], orc.mean_pose_sums() / np.exp(orc.logw).sum(), rtol=0, atol=tol)
    sh.close()


# ---- 7: shards -----------------------------------------------------------------------------------------------------------
class _ThreadComm:
    """The collectives FastSLAM.map / best_particle use, among the threads of one process."""
    def __init__(self, world):
        self.world, self.slots, self.bar = world, [None] * world, threading.Barrier(world)

    def view(self, rank):
        outer = self

        class View:
            world = outer.world

            def __init__(self):
                self.rank = rank

            def _gather(self, vec):
                outer.slots[rank] = list(vec)
                outer.bar.wait(timeout=120)
                table = [list(s) for s in outer.slots]
                outer.bar.wait(timeout=120)
                return table

            def all_gather_scalars(self, vec):
                return self._gather(vec)

            def allreduce_sum(self, vec):
                return np.sum(np.array(self._gather(vec), dtype=np.float64), axis=0).tolist()
        return View()


@pytest.mark.parametrize("dtype,world", [("f32", 2), ("f64", 3)])
def test_shards_map_sums_add_up_to_the_one_rank_filter(pkg, dtype, world):
    per, nl, seed = 2048, 14, 77             # (slices of a multiple of 1024 particles: the ranks' log-weights are the one-rank filter's bit for bit)
    n = per * world
    lm = scene(nl, 19)
    ref_shard = pkg.PFShard(n, nl, seed, dtype=dtype)
    shards = [pkg.PFShard(per, nl, seed, dtype=dtype, first=r * per, n_global=n) for r in range(world)]
    for sh in shards + [ref_shard]:
        sh.set_pose([0.5, 1.5, -0.2])
        sh.init_landmarks(lm[:9], 0.01, 0.1)
    pkg.attach_local_peers(shards)
    comm = _ThreadComm(world)
    ref = pkg.FastSLAM(ref_shard, None, neff_frac=0.75)
    ranks = [pkg.FastSLAM(sh, comm.view(r), neff_frac=0.75) for r, sh in enumerate(shards)]
    rng = np.random.default_rng(6)
    pose = np.array([0.5, 1.5, -0.2])
    steps = []
    for t in range(14):
        pose = advance(pose, 0.6)
        ids = np.array([1 + t % 9, 1 + (t + 4) % 9, 10 + t % 4, 3])                    # landmark 14 is never seen
        steps.append((0.01 * (t % 5), observe(lm, pose, ids, rng), ids, False if t >= 12 else (None if t % 3 == 2 else True)))
    for g, z, ids, force in steps:
        ref.step_async(6.0, g, 4.0, Q, 0.1, z, ids, R, force_resample=force)
    ref.flush()
    assert ref.resamples >= 8
    want_sums = ref_shard.map_sums()
    want_best = ref.best_particle()
    w = ref_shard.weights()
    p, lw, l = ref_shard.download()
    _, tol = check_sums(want_sums, p, w, l, list(range(1, nl + 1)), "one-rank filter")
    assert want_best[0] == int(np.argmax(lw))
    got, errs = [None] * world, []

    def drive(r):
        try:
            f = ranks[r]
            assert f.shard.peer_selftest(10000)
            for g, z, ids, force in steps:
                f.step_async(6.0, g, 4.0, Q, 0.1, z, ids, R, force_resample=force)
            f.flush()
            local = f.shard.map_sums()                    # collective: the remote records come home first
            got[r] = (local, f.map_sums(), f.map(), f.best_particle(), f.shard.download())
        except BaseException as e:                        # noqa: BLE001 -- reported by the main thread
            errs.append((r, e))
            comm.bar.abort()

    th = [threading.Thread(target=drive, args=(r,)) for r in range(world)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not errs, errs
    assert all(g is not None for g in got)
    assert np.array_equal(np.hstack([g[4][0] for g in got]), p) and np.array_equal(np.concatenate([g[4][1] for g in got]), lw)
    assert np.array_equal(np.concatenate([g[4][2] for g in got], axis=2), l), "the shards are the one-rank filter bit for bit"
    total = np.sum([g[0] for g in got], axis=0)
    assert np.all(np.abs(total[:, :9] - want_sums[:, :9]) <= tol[:, :9]), "shards' sums against the one-rank filter's"
    assert np.array_equal(total[:, 9], want_sums[:, 9])
    for g in got:
        assert np.array_equal(g[1], got[0][1]) and np.array_equal(g[2], pkg.pf.finalise_map(g[1]))
        assert np.all(np.abs(g[1][:, :9] - want_sums[:, :9]) <= tol[:, :9])
        assert g[3][0] == want_best[0] and g[3][1] == want_best[1]
        assert np.array_equal(g[3][2], want_best[2]) and np.array_equal(g[3][3], want_best[3])
    th = [threading.Thread(target=sh.detach_peers) for sh in shards]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    for sh in shards + [ref_shard]:
        sh.close()


# ---- 8: more than one chunk of landmark storage ---------------------------------------------------------------------------
def test_full_size_config4_map_of_landmarks_across_a_chunk_boundary(pkg):
    """262144 particles x 512 landmarks, fp32: the records live in chunks of 128 landmarks.  24 landmarks around the first
    boundary, after steps with a forced resampling (live tables), against the download."""
    n, nl, seed = 262144, 512, 20240602
    rng = np.random.default_rng(seed)
    lm = rng.uniform(-200, 200, (nl, 2))
    pf = pkg.PFSlamState(n, nl, seed=seed, dtype="f32", distributed=False)
    pf.shard.set_pose([0.0, 0.0, 0.3])
    pf.shard.init_landmarks(lm, 0.01, 0.1)
    pose = np.array([0.0, 0.0, 0.3])
    for t in range(4):
        pose = np.array([pose[0] + 0.2 * math.cos(pose[2]), pose[1] + 0.2 * math.sin(pose[2]), pose[2]])
        ids = 113 + (np.arange(16) + 16 * t) % 32                                    # landmarks 113..144
        pf.step_async(8.0, 0.0, 4.0, Q, 0.025, observe(lm, pose, ids, rng), ids, R, force_resample=(t == 2))
    subset = list(range(117, 141))
    sums = pf.shard.map_sums(subset)
    best = pf.shard.particle(-1)
    w = pf.shard.weights()
    p, lw, l = pf.shard.download()
    check_sums(sums, p, w, l, subset, "C4 shape, chunk boundary")
    assert np.all(sums[1:, 9] == n)
    k = int(np.argmax(lw))
    assert best[0] == k and np.array_equal(best[3], l[:, :, k].astype(np.float64))
    mp = pf.pose()
    assert np.hypot(*(mp[:2] - pose[:2])) < 0.5 and pf.N == nl
    assert pf.feature_ellipses().shape == (5, nl) and pf.vehicle_ellipse().shape == (6,)
    pf.close()


# ---- a zero-variance prior: used records with Pxx == 0 ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [("f32", 4096), ("f64", 3001)])
def test_records_of_a_zero_variance_prior_count_through_the_seen_flag(pkg, dtype, n):
    """slam_pf_init_landmarks with var = 0 writes used records with Pxx == 0: they count because the landmark is marked seen;
    the all-zero record of a landmark never seen (Pxx == 0 as well) still gives ten zeros."""
    nl = 6
    lm = scene(nl, 3)
    sh = pkg.PFShard(n, nl, 9, dtype=dtype)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.init_landmarks(lm[:4], 0.0, 0.1)
    sums = sh.map_sums()
    w = sh.weights()
    p, _lw, l = sh.download()
    assert np.all(l[:4, 2] == 0) and np.all(l[4:] == 0)
    l_marked = l.astype(np.float64)
    l_marked[:4, 2] = np.finfo(np.float64).tiny       # expected_sums takes Pxx > 0 as "in use": mark the seen landmarks' records
    want, tol = expected_sums(p, w, l_marked, list(range(1, nl + 1)))
    assert np.all(np.abs(sums.astype(LD) - want).astype(np.float64)[:, :9] <= tol[:, :9] + 1e-300)
    assert np.all(sums[1:5, 9] == n) and not sums[5:].any() and np.all(sums[1:5, 6:9] == 0)
    m = sh.get_map()
    assert np.all(m[:4, 0] == pytest.approx(1.0, rel=1e-12)) and not m[4:].any()
    assert np.max(np.abs(m[:4, 1:3] - lm[:4])) < 0.02 and np.all(m[:4, 3] > 0)      # the jitter's spread is the covariance
    sh.close()


# ---- 9: bad arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_status_codes_and_leave_the_handle_usable(pkg):
    lib, BAD = pkg._lib.lib, pkg._lib.SLAM_E_BADARG
    sh = pkg.PFShard(1000, 5, 1, dtype="f32")
    part = pkg.PFShard(500, 5, 1, dtype="f32", first=0, n_global=1000)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.init_landmarks(scene(5, 1), 0.01, 0.1)
    out = np.zeros(10 * 6)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    po = out.ctypes.data_as(dp)

    def ids(*v):
        a = np.array(v, dtype=np.int32)
        return a, a.ctypes.data_as(ip)

    assert lib.slam_pf_map_sums(None, None, 0, po) == BAD
    assert lib.slam_pf_map_sums(sh._h, None, 0, None) == BAD
    for bad in ((0,), (6,), (1, -3)):
        a, pa = ids(*bad)
        assert lib.slam_pf_map_sums(sh._h, pa, len(bad), po) == BAD and "landmark id" in pkg._lib.last_error()
        assert lib.slam_pf_get_map(sh._h, pa, len(bad), po) == BAD
    a, pa = ids(1, 2)
    assert lib.slam_pf_map_sums(sh._h, pa, -1, po) == BAD
    assert lib.slam_pf_get_map(None, None, 0, po) == BAD
    assert lib.slam_pf_get_map(part._h, None, 0, po) == BAD and "whole filter" in pkg._lib.last_error()
    assert lib.slam_pf_get_particle(None, 0, None, None, None, None) == BAD
    assert lib.slam_pf_get_particle(sh._h, 1000, None, None, None, None) == BAD
    assert lib.slam_pf_get_particle(sh._h, -2, None, None, None, None) == BAD
    assert lib.slam_pf_get_particle(sh._h, 999, None, None, None, None) == 0
    s = sh.map_sums()
    assert s[0, 9] == 1000 and np.all(s[1:, 9] == 1000) and s[0, 0] == pytest.approx(1.0, rel=1e-5)
    assert part.map_sums([])[0, 9] == 500
    sh.close()
    part.close()
