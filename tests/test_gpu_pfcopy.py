"""A particle set uploaded, copied, selected and resized on the device (include/slamhip_pfcopy.h, csrc/pf_copy.hip,
libslamhip_pfcopy.so) against tests/pfcopy_ref.py, the rules run literally in NumPy.

Everything is compared BIT FOR BIT through download / meta (uint views: a negative zero is not a zero); no tolerance is picked
anywhere in this file.  Only the ancestor table of a resize is compared through ExactInto.check (exact Python-integer reference,
decided and undecided slots: tests/pfcopy_ref.py), and the one comparison with the fp64 oracle uses the tolerances of
tests/test_gpu_pf.py unchanged.

Where src has a normalisation shift pending or records behind lazy tables, the copy comes FIRST and src.download() after it: the
download flushes the shift and materialises the maps, the copy must have read the records where they lay.

Shapes: n in {1, 3, 64, 65, 1023, 1025, 5013} -- one thread, no multiple of 4 (scalar stores, particles 256 apart), a full and a
partial wave, one slab of 1024 and one particle more, several slabs; 1 and 7 landmarks (one group) and 17 / 33 where a second
landmark group matters; and ONE shape whose records lie in two chunks (see test_two_chunks)."""
import math

import numpy as np
import pytest

from oracle import pf_ref as F
from tests import pfcopy_ref as PR
from tests import resample_ref as RR
from tests.test_gpu_pf import TOL as PF_TOL, close

pytestmark = pytest.mark.gpu

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
CTL = (6.0, 0.03, 4.0, 0.1)                                          # V, G, wheelbase, dt
SIZES = (1, 3, 64, 65, 1023, 1025, 5013)
DTYPES = ("f32", "f64")
eq = PR.bits_equal


def scene(nl, seed):
    return np.random.default_rng(seed).uniform(-40, 40, (nl, 2))


def observe(lm, pose, ids, rng):
    dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
    return np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))


def snapshot(sh):
    pose, logw, lm = sh.download()
    m = sh.meta()
    return dict(pose=pose, logw=logw, lm=lm, seen=m["seen"], seed=m["seed"], step=m["step"], resamples=m["resamples"])


def assert_same(got, want, what):
    for k in ("pose", "logw", "lm", "seen"):
        assert eq(got[k], want[k]), f"{what}: {k} differs"
    for k in ("seed", "step", "resamples"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"


def source_of(snap):
    return PR.LazySource.from_plain(snap["pose"], snap["logw"], snap["lm"], snap["seen"], seed=snap["seed"], step=snap["step"],
                                    resamples=snap["resamples"])


def designed_set(n, nl, dtype, seed):
    rng = np.random.default_rng(seed)
    return PR.designed((3, n), dtype, seed), PR.designed((n,), dtype, seed + 1), PR.designed((nl, 5, n), dtype, seed + 2), rng.integers(0, 2, nl)


def normalise(sh):
    """weight_stats + normalize as FastSLAM.normalize does; returns the largest normalised log-weight as stored."""
    gm, s1, _ = sh.weight_stats()
    sh.normalize(gm, s1)
    T = sh.np_dtype
    return float(T(gm) - T(gm + math.log(s1)))


def lazy_filter(pkg, n, nl, dtype, seed, pending=False):
    """A filter run so that records lie behind ancestor tables AND in the other buffer: all landmarks initialised with jitter, then
    twice (predict, update of a subset, normalise, resample_local) and one more update of another subset.  `pending`: a
    normalisation shift is left pending at the end."""
    lm = scene(nl, seed)
    sh = pkg.PFShard(n, nl, seed, dtype=dtype)
    pose = np.array([1.0, -2.0, 0.4])
    sh.set_pose(pose)
    sh.init_landmarks(lm, 0.04, 0.3)
    rng = np.random.default_rng(seed + 1)
    V, G, wb, dt = CTL
    for t in range(3):
        sh.predict(V, G, wb, Q, dt)
        pose = np.array([pose[0] + V * dt * math.cos(G + pose[2]), pose[1] + V * dt * math.sin(G + pose[2]), pose[2] + V * dt * math.sin(G) / wb])
        ids = np.array(sorted({1 + (2 * t) % nl, 1 + (2 * t + 3) % nl}))
        sh.update_known(observe(lm, pose, ids, rng), ids, R)
        if t < 2:
            gmax = normalise(sh)
            sh.resample_local(gmax, pkg.philox_uniform(t, 2, seed))
            sh.set_resample_count(t + 1)
    if pending:
        normalise(sh)
    return sh, lm, pose


# ---- upload / download ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nl", (1, 7))
def test_upload_download_round_trip(pkg, dtype, nl):
    for n in SIZES:
        sh = pkg.PFShard(n, nl, 5, dtype=dtype)
        pose, logw, lm, seen = designed_set(n, nl, dtype, n + nl)
        sh.upload(pose, logw, lm, seen)
        p, w, l = sh.download()
        assert eq(p, pose) and eq(w, logw) and eq(l, lm), (n, nl, dtype)
        assert sh.meta()["seen"].tolist() == seen.tolist()
        # partial uploads: that part only
        pose2, logw2 = PR.designed((3, n), dtype, 900 + n), PR.designed((n,), dtype, 901 + n)
        sh.upload(pose=pose2)
        p, w, l = sh.download()
        assert eq(p, pose2) and eq(w, logw) and eq(l, lm), ("pose only", n)
        sh.upload(logw=logw2)
        p, w, l = sh.download()
        assert eq(p, pose2) and eq(w, logw2) and eq(l, lm), ("logw only", n)
        with pytest.raises(ValueError):
            sh.upload(lm=lm)
        m = sh.meta()
        assert (m["n"], m["n_global"], m["first"], m["max_landmarks"], m["dtype"], m["step"], m["resamples"], m["seed"]) == (n, n, 0, nl, dtype, 0, 0, 5)
        sh.set_rng(2 ** 63 + 12345, 4000000000)
        m = sh.meta()
        assert m["seed"] == 2 ** 63 + 12345 and m["step"] == 4000000000
        sh.close()


def test_upload_drops_a_pending_shift_only_with_logw(pkg):
    sh = pkg.PFShard(65, 2, 1, dtype="f32")
    pose, logw, lm, seen = designed_set(65, 2, "f32", 3)
    sh.upload(pose, logw, lm, seen)
    sh.normalize(0.25, 1.0)                                         # a shift of 0.25 pending
    sh.upload(pose=pose)
    assert eq(sh.download()[1], (logw - np.float32(0.25)).astype(np.float32))         # still applied
    sh.upload(logw=logw)
    sh.normalize(0.25, 1.0)
    sh.upload(logw=logw)
    assert eq(sh.download()[1], logw)                               # dropped
    sh.close()


def test_upload_on_a_shard_without_peers(pkg):
    sh = pkg.PFShard(65, 3, 1, dtype="f64", first=65, n_global=195)
    pose, logw, lm, seen = designed_set(65, 3, "f64", 8)
    sh.upload(pose, logw, lm, seen)
    p, w, l = sh.download()
    assert eq(p, pose) and eq(w, logw) and eq(l, lm)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_upload_onto_live_tables_gives_plain_maps(pkg, dtype):
    """After an upload onto a filter with live tables the tables are gone: a following update_known gives, bit for bit, what a
    fresh filter with the same upload gives, and equals the fp64 oracle within the tolerances of tests/test_gpu_pf.py."""
    n, nl = 1025, 7
    sh, lm, pose = lazy_filter(pkg, n, nl, dtype, 21)
    donor, _, _ = lazy_filter(pkg, n, nl, dtype, 22)
    snap = snapshot(donor)
    sh.upload(snap["pose"], snap["logw"], snap["lm"], snap["seen"])
    fresh = pkg.PFShard(n, nl, 21, dtype=dtype)
    fresh.upload(snap["pose"], snap["logw"], snap["lm"], snap["seen"])
    orc = F.OraclePF(n, nl, 21)
    orc.pose, orc.logw, orc.lm = (snap[k].astype(np.float64) for k in ("pose", "logw", "lm"))
    orc.seen = snap["seen"].astype(bool)
    ids = np.array([2, 5, 7])
    z = observe(scene(nl, 22), np.array([2.7, -1.3, 0.45]), ids, np.random.default_rng(0))
    for f in (sh, fresh, orc):
        f.update_known(z, ids, R)
    a, b = snapshot(sh), snapshot(fresh)
    for k in ("pose", "logw", "lm", "seen"):
        assert eq(a[k], b[k]), k
    tol = PF_TOL[dtype]
    assert close(a["lm"][:, 0:2], orc.lm[:, 0:2], tol) and close(a["lm"][:, 2:5], orc.lm[:, 2:5], tol * 10, scale=float(np.max(np.abs(orc.lm[:, 2:5]))))
    assert close(a["logw"], orc.logw, tol * 10, scale=max(1.0, float(np.max(np.abs(orc.logw)))))
    for f in (sh, fresh, donor):
        f.close()


# ---- checkpoint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_and_restore_continue_bit_for_bit(pkg, dtype):
    n, nl, seed = 3000, 8, 31
    lm = scene(nl, 4)
    V, G, wb, dt = CTL
    rng = np.random.default_rng(9)
    pose, obs = np.array([1.0, -2.0, 0.4]), []
    for t in range(12):
        pose = np.array([pose[0] + V * dt * math.cos(G + pose[2]), pose[1] + V * dt * math.sin(G + pose[2]), pose[2] + V * dt * math.sin(G) / wb])
        ids = np.array([1 + t % nl, 1 + (t + 3) % nl])
        obs.append((observe(lm, pose, ids, rng), ids))

    def start():
        pf = pkg.FastSLAM(pkg.PFShard(n, nl, seed, dtype=dtype), neff_frac=0.75)
        pf.shard.set_pose([1.0, -2.0, 0.4])
        pf.shard.init_landmarks(lm, 0.04, 0.3)
        return pf

    def steps(pf, lo, hi):
        for t in range(lo, hi):
            pf.step_async(V, G, wb, Q, dt, obs[t][0], obs[t][1], R)
        pf.flush()

    whole = start()
    steps(whole, 0, 12)
    want = snapshot(whole.shard)
    part = start()
    steps(part, 0, 6)
    assert part.shard.resample_count() >= 1, "the first six steps must resample at least once"
    d = pkg.save_particles(part.shard)
    part.shard.close()
    back = pkg.FastSLAM(pkg.load_particles(d), neff_frac=0.75)
    assert back.shard.resample_count() == d["resamples"] and back.shard.meta()["step"] == d["step"]
    steps(back, 6, 12)
    assert_same(snapshot(back.shard), want, f"checkpoint {dtype}")
    assert back.shard.resample_count() == whole.shard.resample_count()
    whole.shard.close()
    back.shard.close()


# ---- copy and select ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (3, 64, 1025, 5013))
def test_copy_and_select_with_lazy_tables_live(pkg, dtype, n):
    nl = 17                                                          # a second landmark group of one landmark
    src, _, _ = lazy_filter(pkg, n, nl, dtype, 40 + n)
    dsts = {}
    cases = [("copy equal", nl, None, 0), ("copy equal fill 1", nl, None, 1), ("copy larger fill 0", 33, None, 0), ("copy larger fill 1", 20, None, 1),
             ("select shuffled", 9, [16, 3, 17, 1, 8, 2, 11], 1), ("select shuffled fill 0", 7, [5, 4, 12, 17, 1, 2, 3], 0),
             ("select none", 3, [], 1), ("select one", 1, [17], 0)]
    for what, cap, ids, fill in cases:
        d = pkg.PFShard(n, cap, 999, dtype=dtype)
        junk = designed_set(n, cap, dtype, 77)
        d.upload(*junk)                                              # (whatever dst held must be gone)
        if ids is None:
            d.copy_from(src, fill=fill)
        else:
            d.select_from(src, ids, fill=fill)
        dsts[what] = d
    snap = snapshot(src)                                             # AFTER the copies: this materialises src
    ref = source_of(snap)
    for what, cap, ids, fill in cases:
        assert_same(snapshot(dsts[what]), PR.select(ref, ids, cap, fill), f"{what} n={n} {dtype}")
        assert dsts[what].seed == src.seed
        dsts[what].close()
    src.close()


def test_errors_leave_dst_unchanged(pkg):
    n, nl = 65, 5
    src, _, _ = lazy_filter(pkg, n, nl, "f32", 50)
    dst = pkg.PFShard(n, nl, 3, dtype="f32")
    dst.upload(*designed_set(n, nl, "f32", 51))
    dst.set_rng(17, 9)
    dst.normalize(0.5, 1.0)                                          # a pending shift is part of the state
    E = pkg._lib

    def refused(code, call):
        with pytest.raises(pkg.SlamHipError) as ei:
            call()
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    other = pkg.PFShard(n, nl, 3, dtype="f64")
    refused(E.SLAM_E_BADARG, lambda: dst.copy_from(other))                                   # dtype
    refused(E.SLAM_E_BADARG, lambda: dst.copy_from(dst))                                     # dst == src
    refused(E.SLAM_E_BADARG, lambda: dst.select_from(src, [1, 2, 1]))                        # a duplicate id
    refused(E.SLAM_E_BADARG, lambda: dst.select_from(src, [0]))                              # an id out of range
    refused(E.SLAM_E_BADARG, lambda: dst.select_from(src, [nl + 1]))
    refused(E.SLAM_E_BADARG, lambda: dst.copy_from(src, fill=2))
    small = pkg.PFShard(n, nl - 1, 3, dtype="f32")
    refused(E.SLAM_E_CAPACITY, lambda: small.copy_from(src))                                 # capacity
    small2 = pkg.PFShard(n, 2, 3, dtype="f32")
    refused(E.SLAM_E_CAPACITY, lambda: small2.select_from(src, [1, 2, 3]))
    refused(E.SLAM_E_CAPACITY, lambda: small.resize_from(src, 0.0, 0.5))
    wrong_n = pkg.PFShard(n + 1, nl, 3, dtype="f32")
    refused(E.SLAM_E_BADARG, lambda: wrong_n.copy_from(src))                                 # counts differ: that is resize
    shard = pkg.PFShard(n, nl, 3, dtype="f32", first=0, n_global=2 * n)                      # a sharded handle, either side
    refused(E.SLAM_E_BADARG, lambda: dst.copy_from(shard))
    refused(E.SLAM_E_BADARG, lambda: shard.copy_from(src))
    refused(E.SLAM_E_BADARG, lambda: dst.resize_from(src, 0.0, 1.0))                         # u0 out of range
    if pkg.device_count() >= 2:                                                              # (needs a second card)
        far = pkg.PFShard(n, nl, 3, dtype="f32", device=1)
        refused(E.SLAM_E_BADARG, lambda: far.copy_from(src))
        far.close()
    # dst: the uploaded values minus the pending shift, the RNG state as set; src as it was
    pose, logw, lm, seen = designed_set(n, nl, "f32", 51)
    got = snapshot(dst)
    assert eq(got["pose"], pose) and eq(got["lm"], lm) and eq(got["logw"], (logw - np.float32(0.5)).astype(np.float32))
    assert got["seen"].tolist() == seen.tolist() and (got["seed"], got["step"], got["resamples"]) == (17, 9, 0)
    for f in (src, dst, other, small, small2, wrong_n, shard):
        f.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clone_stays_equal(pkg, dtype):
    n, nl = 1025, 7
    sh, lm, pose = lazy_filter(pkg, n, nl, dtype, 60)
    pf = pkg.FastSLAM(sh, neff_frac=0.75)
    pf.resamples = 2
    twin = pf.clone()
    assert twin.shard is not pf.shard and twin.resamples == 2 and twin.shard.seed == sh.seed
    rng = np.random.default_rng(1)
    V, G, wb, dt = CTL
    for t in range(3):
        ids = np.array([1 + t, 4 + t])
        z = observe(lm, pose, ids, rng)
        for f in (pf, twin):
            f.step_async(V, G, wb, Q, dt, z, ids, R)
    a, b = pf.flush(), twin.flush()
    assert a == b
    assert_same(snapshot(twin.shard), snapshot(sh), f"clone {dtype}")
    twin.shard.close()
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pending_shift_is_applied_on_the_way(pkg, dtype):
    n, nl = 1023, 3
    src, _, _ = lazy_filter(pkg, n, nl, dtype, 70, pending=True)
    dst = pkg.PFShard(n, nl, 1, dtype=dtype)
    dst.copy_from(src)
    got = snapshot(dst)
    want = snapshot(src)                                             # the download applies src's shift only now
    assert_same(got, want, "pending shift")
    assert abs(float(np.log(np.exp(got["logw"].astype(np.float64)).sum()))) < 1e-3      # (the shift was indeed applied: normalised weights)
    dst.close()
    src.close()


def test_fastslam_refuses_what_does_not_follow(pkg):
    sh = pkg.PFShard(64, 2, 1)
    pf = pkg.FastSLAM(sh)
    pf.track_path(4)
    for call in (pf.clone, lambda: pf.reserve(4), lambda: pf.resize(32), lambda: pf.adapt(0.5, 0.1)):
        with pytest.raises(ValueError, match="PathHistory"):
            call()
    pf.path_history.close()
    pf.path_history = None
    ev = pkg.LandmarkEvidence(sh, 30.0, math.pi / 2)
    with pytest.raises(ValueError, match="LandmarkEvidence"):
        pf.clone()
    ev.close()
    pf.clone().shard.close()
    sh.close()


# ---- two chunks -----------------------------------------------------------------------------------------------------------------------
def test_two_chunks(pkg):
    """The smallest shape whose records slam_pf_create cuts into two chunks.  pf_create_impl (csrc/pf_legacy.hip) takes the largest
    shift with (esz 5 n) << shift <= 2^30 bytes and allocates ceil(nl / 2^shift) chunks (PF_LM_MAXC = 16 only matters above 16
    chunks), so two chunks need nl = 2^shift + 1 and the buffer is smallest where esz 5 n 2^shift is just above 2^29: fp32,
    shift 8, n = 104864 (20 n 2^8 = 2^29 + 32768; a multiple of 8), nl = 257 -- 539 MB a buffer.  Half the particles give
    shift 9 and ONE chunk for the same 257 landmarks: the resize below moves between two chunkings that differ in shift and
    count; the copy goes into three chunks (513 landmarks) and the select takes landmarks from both sides of the boundary."""
    n, nl, dtype = 104864, 257, "f32"
    assert 20 * n * 256 > 2 ** 29 and 20 * n * 512 > 2 ** 30 >= 20 * n * 256 and 20 * (n // 2) * 512 <= 2 ** 30
    src = pkg.PFShard(n, nl, 7, dtype=dtype)
    lm = (np.arange(nl * 5 * n, dtype=np.uint32) + np.uint32(0x3F000000)).view(np.float32).reshape(nl, 5, n)
    pose = PR.designed((3, n), dtype, 1)
    logw = np.full(n, -math.log(n), dtype=np.float32)
    seen = np.arange(nl) % 3 == 0
    src.upload(pose, logw, lm, seen)
    ref = PR.LazySource.from_plain(pose, logw, lm, seen.astype(np.uint8), seed=7, step=0, resamples=0)
    # select across the boundary (landmarks 256 | 257 are the last of chunk 0 and the only one of chunk 1)
    ids = [257, 1, 256, 2]
    d = pkg.PFShard(n, 5, 1, dtype=dtype)
    d.select_from(src, ids, fill=1)
    assert_same(snapshot(d), PR.select(ref, ids, 5, 1), "select across the chunk boundary")
    d.close()
    # resize into half the particles: shift 9, one chunk
    m = n // 2
    d = pkg.PFShard(m, nl, 1, dtype=dtype)
    anc = d.resize_from(src, float(logw[0]), 0.37)
    PR.ExactInto(logw, float(logw[0]), 0.37, m).check(anc, "two chunks")
    got = snapshot(d)
    assert eq(got["lm"], lm[:, :, anc]) and eq(got["pose"], pose[:, anc]) and got["resamples"] == 1
    d.close()
    # copy into three chunks
    d = pkg.PFShard(n, 513, 1, dtype=dtype)
    d.copy_from(src, fill=1)
    got = snapshot(d)
    assert eq(got["lm"][:nl], lm) and np.all(got["lm"][nl:, 2] == -1) and not got["lm"][nl:, [0, 1, 3, 4]].any()
    assert eq(got["pose"], pose) and eq(got["logw"], logw) and got["seen"][:nl].tolist() == seen.astype(np.uint8).tolist() and not got["seen"][nl:].any()
    d.close()
    src.close()


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", PR.RESIZE_NS)
def test_resize_on_the_resampling_scenes(pkg, dtype, n):
    """Scenes of tests/resample_ref.py as log-weights over designed records: the returned table passes ExactInto.check with at
    most max(2, 1e-4 m) undecided slots, dst is the gather of src by THE RETURNED table bit for bit, the weights are (T)(-log m),
    the meta follows the rule, src is untouched and the call is reproducible."""
    nl = 3
    T = PR.NP_DTYPE[dtype]
    pose, _, lm, seen = designed_set(n, nl, dtype, 80 + n)
    src = pkg.PFShard(n, nl, 11, dtype=dtype)
    src.upload(pose, np.zeros(n, dtype=T), lm, seen)
    src.set_rng(11, 5)
    src.set_resample_count(3)
    dsts = {m: pkg.PFShard(m, nl + (m % 2), 1, dtype=dtype) for m in PR.resize_ms(n)}
    worst = 0
    for name in RR.SCENES:
        if not RR.fits(name, n):
            continue
        sc = RR.scene(name, n, dtype)
        src.upload(logw=sc.logw)
        ref = PR.LazySource.from_plain(pose, sc.logw, lm, seen, seed=11, step=5, resamples=3)
        for m, d in dsts.items():
            for u0 in RR.U0S:
                what = f"{name} n={n} m={m} {dtype} u0={u0}"
                anc = d.resize_from(src, sc.gmax, u0, fill=m % 2)
                ex = PR.ExactInto(sc.logw, sc.gmax, u0, m)
                assert ex.n_undecided <= PR.undecided_cap(m), what
                worst = max(worst, ex.check(anc, what))
                assert_same(snapshot(d), PR.resize(ref, anc, d.nl, m % 2), what)
        assert_same(snapshot(src), PR.select(ref, None, nl, 0), f"src after {name}")
    # reproducible from call to call
    d = dsts[n + 1]
    a1 = d.resize_from(src, sc.gmax, 0.37)
    s1 = snapshot(d)
    a2 = d.resize_from(src, sc.gmax, 0.37)
    assert np.array_equal(a1, a2) and all(eq(s1[k], v) for k, v in snapshot(d).items() if isinstance(v, np.ndarray))
    print(f"resize n={n} {dtype}: undecided slots that differ from the exact table, worst scene: {worst}")
    # total == 0 is refused before dst is written
    before = snapshot(d)
    src.upload(logw=np.full(n, RR.DEAD_LOGW, dtype=T))
    with pytest.raises(pkg.SlamHipError) as ei:
        d.resize_from(src, 0.0, 0.37)
    assert ei.value.code == pkg._lib.SLAM_E_BADARG
    assert_same(snapshot(d), before, "total == 0")
    for f in list(dsts.values()) + [src]:
        f.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_with_tables_live_and_a_shift_pending(pkg, dtype):
    n, nl = 1025, 17
    # the largest normalised log-weight as stored: read from a twin (the run is deterministic), src itself stays lazy and pending
    twin, _, _ = lazy_filter(pkg, n, nl, dtype, 90, pending=True)
    gmax = float(twin.download()[1].max())
    twin.close()
    for m in (64, 1023, n, 2 * n + 1):
        src, _, _ = lazy_filter(pkg, n, nl, dtype, 90, pending=True)
        d = pkg.PFShard(m, nl + 1, 1, dtype=dtype)
        anc = d.resize_from(src, gmax, 0.37, fill=1)
        snap = snapshot(src)                                         # after the resize
        PR.ExactInto(snap["logw"], gmax, 0.37, m).check(anc, f"lazy resize m={m}")
        assert_same(snapshot(d), PR.resize(source_of(snap), anc, nl + 1, 1), f"lazy resize m={m} {dtype}")
        d.close()
        src.close()


def test_fastslam_resize_and_adapt(pkg):
    sh, lm, pose = lazy_filter(pkg, 1025, 7, "f32", 95)
    pf = pkg.FastSLAM(sh)
    pf.resamples = 2
    k = sh.pose_bins(0.05, 0.02)
    want = pkg.kld_particle_count(k, n_min=64, n_max=4096)
    got = pf.adapt(0.05, 0.02, n_min=64, n_max=4096)
    assert got == want and pf.shard.n == want and (want == 1025 or (pf.resamples == 3 and pf.shard.resample_count() == 3))
    anc = pf.resize(300)
    assert pf.shard.n == 300 and anc.shape == (300,) and np.all(np.diff(anc) >= 0)
    assert np.all(pf.shard.download()[1] == np.float32(-math.log(300)))
    pf.shard.close()


# ---- bins -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (1, 65, 5013))
def test_pose_bins(pkg, dtype, n):
    """Designed poses on and beside cell edges, at +-pi, negative coordinates; the count equals np.unique over the header's rule."""
    T = PR.NP_DTYPE[dtype]
    cell_xy, cell_phi = 0.5, 0.1
    rng = np.random.default_rng(n)
    k = rng.integers(-40, 40, (2, n)).astype(np.float64)
    edge = (k * cell_xy).astype(T)
    side = rng.integers(0, 3, (2, n))
    xy = np.where(side == 0, edge, np.where(side == 1, np.nextafter(edge, T(np.inf)), np.nextafter(edge, T(-np.inf)))).astype(T)
    phi = rng.uniform(-math.pi, math.pi, n).astype(T)
    phi[::5] = T(math.pi)
    phi[1::5] = T(-math.pi)
    phi[2::5] = (rng.integers(0, 63, phi[2::5].shape) * cell_phi - math.pi).astype(T)
    pose = np.vstack([xy, phi[None]]).astype(T)
    sh = pkg.PFShard(n, 1, 1, dtype=dtype)
    sh.upload(pose=pose)
    for cxy, cphi in ((cell_xy, cell_phi), (0.125, math.pi / 2), (1000.0, 7.0)):
        assert sh.pose_bins(cxy, cphi) == PR.pose_bins(pose, cxy, cphi), (n, dtype, cxy, cphi)
    assert sh.pose_bins(1000.0, 7.0) <= 4 and eq(sh.download()[0], pose)      # (the four quadrants, one heading cell; the poses are only read)
    # out of range, not finite, a bad cell
    for bad in (2.0 ** 19, -2.0 ** 19 - 0.5, np.nan, np.inf):
        p2 = pose.copy()
        p2[0, n // 2] = T(bad)
        sh.upload(pose=p2)
        with pytest.raises(ValueError):
            PR.pose_bins(p2, cell_xy, cell_phi)
        with pytest.raises(pkg.SlamHipError) as ei:
            sh.pose_bins(cell_xy, cell_phi)
        assert ei.value.code == pkg._lib.SLAM_E_BADARG
    with pytest.raises(pkg.SlamHipError):
        sh.pose_bins(0.0, 0.1)
    with pytest.raises(pkg.SlamHipError):
        sh.pose_bins(0.5, -1.0)
    sh.close()


# ---- FastSLAM.reserve, unknown correspondences -----------------------------------------------------------------------------------------
def test_reserve_gives_a_full_filter_room_for_a_new_landmark(pkg):
    """A filter whose slots are all used drops a new landmark; after reserve(2 nl, unknown=True) the same observation starts it.
    In d_assoc the library writes -1 ("new") for that observation BOTH times -- -2 is its code for an observation between the
    two gates, and a particle without a free slot drops the new landmark silently (slam_pf_update_unknown: "none left:
    dropped") -- so the drop is read off the records: before, every record stays as it was, bit for bit; after, the record
    appears in the first new slot of every particle."""
    n, nl = 257, 2
    pf = pkg.FastSLAM(pkg.PFShard(n, nl, 3, dtype="f32"))
    pf.shard.set_pose([0.0, 0.0, 0.0])
    pf.shard.clear_landmarks()
    z2 = np.array([[10.0, 12.0], [0.5, -0.6]])
    a = pf.shard.update_unknown(z2, R, 4.0, 25.0, want_assoc=True).cpu().numpy()
    assert np.all(a == -1)                                           # both slots taken in every particle
    full = pf.shard.download()
    assert np.all(full[2][:, 2] > 0)
    z_new = np.array([[20.0], [1.4]])
    a = pf.shard.update_unknown(z_new, R, 4.0, 25.0, want_assoc=True).cpu().numpy()
    assert np.all(a == -1)                                           # a new landmark ...
    before = pf.shard.download()
    assert eq(before[2], full[2])                                    # ... with no slot left: dropped, no record changed
    pf.reserve(2 * nl, unknown=True)
    assert pf.shard.nl == 4
    after = pf.shard.download()
    assert eq(after[0], before[0]) and eq(after[1], before[1]) and eq(after[2][:nl], before[2])
    assert np.all(after[2][nl:, 2] == -1) and not after[2][nl:, [0, 1, 3, 4]].any()
    a = pf.shard.update_unknown(z_new, R, 4.0, 25.0, want_assoc=True).cpu().numpy()
    assert np.all(a == -1)                                           # the same observation starts the landmark now
    got = pf.shard.download()[2]
    assert np.all(got[nl, 2] > 0) and np.all(got[nl + 1, 2] == -1) and eq(got[:nl], before[2])     # in the first new slot
    pf.shard.close()
