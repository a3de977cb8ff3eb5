"""GPU tests of the per-particle trajectory history (include/slamhip_path.h, libslamhip_path.so; PFShard + PathHistory,
FastSLAM.track_path).

The oracle is tests/path_ref.py fed with DOWNLOADS only: the poses after every step, and for every resampling the ancestors
recovered by matching each particle's pose triple after it to the pose triples before it (asserted pairwise distinct: a seed
that collides is replaced, the assertion stays).  So the records, the ancestors, the traces, the best path and the survivor
counts are compared exactly.  The mean path is held to the bound tests/path_ref.mean_bounds derives for ANY order of additions
in double, against sums formed with math.fsum.

Each step is predict + update_known with one observation whose R decides how skewed the weights get: "mild" leaves most
particles alive, "depleted" a handful (R and the landmarks' variance are small against the spread of the poses)."""
import itertools
import math

import numpy as np
import pytest

import path_ref as PR

pytestmark = pytest.mark.gpu

LM = np.array([[20.0, 5.0], [-8.0, 15.0]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
V, G, WB, DT = 5.0, 0.02, 4.0, 0.1
STEPS = 12
SIZES = (1, 64, 65, 1023, 1025, 4099)          # a wave, a wave + 1, a scan block - 1 / + 1, four scan blocks with a ragged tail
CAPS = (1, 3, 8)
SCHEDULES = ("never", "every", "twice", "first", "last")
SKEW = {"mild": (0.08, 1e-4), "depleted": (0.004, 1e-8)}       # rho of R = diag(rho^2, (rho / 5)^2), the landmarks' variance


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_download(a, b, what):
    for x, y, part in zip(a, b, ("pose", "logw", "landmarks")):
        assert _same_bits(x, y), f"{what}: {part} differ"


def _obs(step, phi0, rho):
    """One observation of landmark 1 or 2 from about where the vehicle is after step + 1 moves, the range 2 rho off."""
    lid = 1 + step % 2
    px, py = V * DT * (step + 1) * math.cos(phi0), V * DT * (step + 1) * math.sin(phi0)
    dx, dy = LM[lid - 1, 0] - px, LM[lid - 1, 1] - py
    z = np.array([[math.hypot(dx, dy) + 2.0 * rho], [math.atan2(dy, dx) - phi0]])
    return z, np.array([lid]), np.diag([rho ** 2, (rho / 5.0) ** 2])


def _shard(pkg, n, dtype, seed, skew, phi0):
    sh = pkg.PFShard(n, 2, seed, dtype=dtype)
    sh.set_pose([0.0, 0.0, phi0])
    sh.init_landmarks(LM, SKEW[skew][1], 0.05)
    return sh


def _step(sh, step, skew, phi0):
    z, ids, R = _obs(step, phi0, SKEW[skew][0])
    sh.predict(V, G, WB, Q, DT)
    sh.update_known(z, ids, R)


def _resample(pkg, sh, resample, ref, count):
    """One resampling through `resample` (PathHistory.resample or PFShard.resample_local); the reference gets the ancestors
    recovered from the downloads."""
    pre, logw, _ = sh.download(landmarks=False)
    resample(float(logw.max()), pkg.philox_uniform(count, 2, sh.seed))
    post = sh.download(landmarks=False)[0]
    if ref is not None:
        ref.resample(PR.recover_ancestors(pre, post))


def _run(pkg, n, dtype, cap, schedule, skew, phi0=0.3, seed=5):
    """The filter, its path object and the reference after STEPS steps of `schedule`:
    never / every  no resampling / one before every record;
    twice          one at every step, a record at every second: two resamplings between two records, and they compose;
    first          one before the first record only;   last  one after the last record only."""
    sh = _shard(pkg, n, dtype, seed, skew, phi0)
    ph = pkg.PathHistory(sh, cap)
    ref = PR.PathRef(n, cap)
    count = 0
    for s in range(STEPS):
        _step(sh, s, skew, phi0)
        if schedule in ("every", "twice") or (schedule == "first" and s == 0):
            _resample(pkg, sh, ph.resample, ref, count)
            count += 1
        if schedule != "twice" or s % 2 == 1:
            ph.record()
            ref.record(sh.download(landmarks=False)[0])
    if schedule == "last":
        _resample(pkg, sh, ph.resample, ref, count)
    return sh, ph, ref


def _trace_all(ph, n):
    return np.concatenate([ph.trace(np.arange(a, min(a + 4096, n))) for a in range(0, n, 4096)])


def _check_mean(ph, ref, n, logw, what):
    dev = ph.mean()
    want, detail = ref.mean(logw)
    bounds = PR.mean_bounds(n, detail)
    worst = 0.0
    for t, (d, w, b, dt) in enumerate(zip(dev, want, bounds, detail)):
        R = math.hypot(dt["S"], dt["C"])
        assert R >= 0.5, f"{what}: the scene's headings are too spread at record {t} (R = {R})"
        errs = dict(x=abs(d[0] - w[0]), y=abs(d[1] - w[1]), phi=abs(d[2] - w[2]), R=abs(d[3] - w[3]))
        for key, e in errs.items():
            worst = max(worst, e / b[key] if b[key] > 0 else (0.0 if e == 0 else math.inf))
            assert e <= b[key], f"{what}: record {t} {key}: |dev - ref| = {e:.3e} > {b[key]:.3e} (dev {d}, ref {w})"
    again = ph.mean()
    assert _same_bits(dev, again), f"{what}: two mean calls differ"
    print(f"{what}: mean error / bound at most {worst:.3f}")
    return dev


def _check_everything(pkg, sh, ph, ref, n, schedule, what):
    before = sh.download()
    info = ph.info()
    assert info == ref.info(), (what, info, ref.info())
    L = info["L"]
    assert L == min(cap_records(schedule), ph.cap)
    T = sh.np_dtype
    slots = []
    for k in range(L):
        pose, anc, has = ph.get(k)
        rp, ra, rh = ref.get(k)
        assert np.array_equal(pose, rp) and _same_bits(pose.astype(T), rp.astype(T)), f"{what}: record {k} back: poses"
        assert has == rh and anc.dtype == np.int32 and np.array_equal(anc, ra), f"{what}: record {k} back: ancestors"
        slots.append((pose, anc, has))
    tr = _trace_all(ph, n)
    want = ref.trace(np.arange(n))
    assert tr.shape == want.shape == (n, L, 3) and np.array_equal(tr, want), f"{what}: trace"
    b, path = ph.best()
    rb, rpath = ref.best(before[1])
    assert b == rb and np.array_equal(path, rpath), f"{what}: best {b} {rb}"
    sv = ph.survivors()
    rsv = ref.survivors()
    assert sv.dtype == np.int64 and np.array_equal(sv, rsv), f"{what}: survivors {sv} {rsv}"
    assert sv[-1] <= n and np.all(np.diff(sv) >= 0)
    if schedule == "never":
        assert np.all(sv == n)
    _check_mean(ph, ref, n, before[1], what)
    # the read-outs changed neither the filter nor the ring
    _same_download(before, sh.download(), what + ": after the read-outs")
    assert ph.info() == info
    for k, (pose, anc, has) in enumerate(slots):
        p2, a2, h2 = ph.get(k)
        assert np.array_equal(p2, pose) and np.array_equal(a2, anc) and h2 == has, f"{what}: record {k} back changed"
    return sv


def cap_records(schedule):
    return STEPS // 2 if schedule == "twice" else STEPS


# every (schedule, cap, dtype) once; the sizes and the two kinds of weights take turns: every size meets every schedule, both
# dtypes and at least two of the three capacities
CASES = [(SIZES[(i + i // 6) % len(SIZES)], dtype, cap, schedule, ("mild", "depleted")[(i // 2) % 2])
         for i, (schedule, cap, dtype) in enumerate(itertools.product(SCHEDULES, CAPS, ("f32", "f64")))]


@pytest.mark.parametrize("n,dtype,cap,schedule,skew", CASES)
def test_history_against_the_reference(pkg, n, dtype, cap, schedule, skew):
    """Records, ancestors, traces, the best path and the survivors exactly, the mean within its bound, for every schedule of
    resamplings with the ring wrapping (cap 1 and 3 against 6 or 12 records) and not (cap 8 against 6)."""
    what = f"n={n} {dtype} cap={cap} {schedule} {skew}"
    sh, ph, ref = _run(pkg, n, dtype, cap, schedule, skew)
    sv = _check_everything(pkg, sh, ph, ref, n, schedule, what)
    print(f"{what}: survivors {sv.tolist()}")
    if n >= 64 and schedule in ("every", "twice") and cap > 1:
        assert sv[0] < sv[-1] or sv[-1] < n, f"{what}: no resampling removed a particle: the scene tests nothing"
    ph.close()
    sh.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [65, 4099])
def test_depleted_filter_keeps_a_handful_of_ancestors(pkg, dtype, n):
    """Depleted weights, a resampling before every record: a few records back a handful of particles is all that is left."""
    sh, ph, ref = _run(pkg, n, dtype, 8, "every", "depleted", seed=9)
    sv = _check_everything(pkg, sh, ph, ref, n, "every", f"depleted n={n} {dtype}")
    assert sv[0] <= max(4, n // 16), sv
    ph.close()
    sh.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("schedule", ["never", "every"])
def test_headings_across_pi(pkg, dtype, schedule):
    """The vehicle drives along heading pi: the stored headings of a held record lie on both sides of +-pi, the mean heading
    near pi.  (The steering angle G turns the vehicle by about 0.03 in twelve steps; with a resampling at every step the bearing
    observations hold the cloud within about 0.006 of the start heading + 0.013.)"""
    n, phi0 = 1025, math.pi - (0.03 if schedule == "never" else 0.012)
    sh, ph, ref = _run(pkg, n, dtype, 8, schedule, "mild", phi0=phi0)
    sides = [min(int((poses[2] > 3.0).sum()), int((poses[2] < -3.0).sum())) for poses, _ in ref.held]
    assert max(sides) > n // 20, f"no held record has headings on both sides of +-pi: {sides}"
    _check_everything(pkg, sh, ph, ref, n, schedule, f"across pi {dtype} {schedule}")
    m = ph.mean()
    assert np.all(np.abs(np.abs(m[:, 2]) - math.pi) < 0.05) and np.all(m[:, 3] > 0.99)
    ph.close()
    sh.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [65, 1025])
def test_filter_is_the_same_with_and_without_a_path_object(pkg, dtype, n):
    """Same seed, one filter resampled through resample_local, the other through PathHistory.resample with records in between:
    the downloads are bit-identical after every step, and so is the next step (it draws from the RNG)."""
    a = _shard(pkg, n, dtype, 5, "mild", 0.3)
    b = _shard(pkg, n, dtype, 5, "mild", 0.3)
    ph = pkg.PathHistory(b, 3)
    for s in range(6):
        _step(a, s, "mild", 0.3)
        _step(b, s, "mild", 0.3)
        if s % 2 == 0:
            _resample(pkg, a, a.resample_local, None, s)
            _resample(pkg, b, ph.resample, None, s)
        ph.record()
        _same_download(a.download(), b.download(), f"step {s}")
    ph.mean(), ph.survivors(), ph.best(), ph.trace([0]), ph.get(0)
    _step(a, 6, "mild", 0.3)
    _step(b, 6, "mild", 0.3)
    _same_download(a.download(), b.download(), "the step after the read-outs")
    ph.close()
    a.close()
    b.close()


def test_bad_arguments_change_nothing(pkg):
    BAD = pkg._lib.SLAM_E_BADARG
    n = 65

    def refused(call, *args):
        with pytest.raises(pkg.SlamHipError) as e:
            call(*args)
        assert e.value.code == BAD, e.value

    part = pkg.PFShard(64, 2, 5, dtype="f32", first=0, n_global=128)      # a shard of a larger filter
    refused(pkg.PathHistory, part, 4)
    part.close()
    sh = _shard(pkg, n, "f32", 5, "mild", 0.3)
    refused(pkg.PathHistory, sh, 0)
    refused(pkg.PathHistory, sh, -3)
    ph = pkg.PathHistory(sh, 4)
    _step(sh, 0, "mild", 0.3)
    before = sh.download()
    # L == 0: the five read-outs that need a record, and nothing else
    assert ph.info() == dict(L=0, records=0, cap=4, resamples=0)
    for call, args in ((ph.get, (0,)), (ph.trace, ([0],)), (ph.best, ()), (ph.mean, ()), (ph.survivors, ())):
        refused(call, *args)
    _same_download(before, sh.download(), "L == 0")
    assert ph.info() == dict(L=0, records=0, cap=4, resamples=0)
    refused(ph.resample, float(before[1].max()), 1.5)                    # slam_pf_resample_local's own check: u0 outside [0, 1)
    assert ph.info()["resamples"] == 0
    ph.record()
    _step(sh, 1, "mild", 0.3)
    ph.record()
    before = sh.download()
    info, slots = ph.info(), [ph.get(k) for k in range(2)]
    assert info == dict(L=2, records=2, cap=4, resamples=0)
    refused(ph.get, 2)
    refused(ph.get, -1)
    refused(ph.trace, [n])
    refused(ph.trace, [0, -1])
    refused(ph.trace, [])
    refused(ph.trace, np.zeros(4097, dtype=np.int64))
    assert ph.trace(np.zeros(4096, dtype=np.int64)).shape == (4096, 2, 3)
    lib = pkg._lib.path_lib()
    assert lib.slam_pf_path_mean(ph._p, None) == BAD and lib.slam_pf_path_survivors(ph._p, None) == BAD
    assert lib.slam_pf_path_best(ph._p, None, None) == BAD and lib.slam_pf_path_info(ph._p, None) == BAD
    _same_download(before, sh.download(), "after the refused calls")
    assert ph.info() == info
    for k, (pose, anc, has) in enumerate(slots):
        p2, a2, h2 = ph.get(k)
        assert np.array_equal(p2, pose) and np.array_equal(a2, anc) and h2 == has
    ph.close()
    sh.close()


# ---- FastSLAM.track_path ---------------------------------------------------------------------------------------------------------
def _filter(pkg, n, dtype, seed=7):
    st = pkg.PFSlamState(n, 2, seed=seed, dtype=dtype, neff_frac=0.75, distributed=False)
    st.shard.set_pose([0.0, 0.0, 0.3])
    st.shard.init_landmarks(LM, SKEW["mild"][1], 0.05)
    return st


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_track_path_end_to_end(pkg, dtype):
    """Twelve step() calls under the Neff rule on three filters of one seed: `a` tracks its path, `b` does not and has its
    resample_local wrapped so that the reference sees the poses before and after every resampling, `c` is left alone.  The three
    end bit-identical (tracking changes nothing, and neither does watching), a.path() is the reference's best path, and the
    untracked filter has no path."""
    n, cap = 1025, 8
    a, b, c = (_filter(pkg, n, dtype) for _ in range(3))
    assert a.track_path(cap) is a.path_history and b.path_history is None
    ref = PR.PathRef(n, cap)
    plain = b.shard.resample_local

    def watched(gmax, u0):
        pre = b.shard.download(landmarks=False)[0]
        plain(gmax, u0)
        ref.resample(PR.recover_ancestors(pre, b.shard.download(landmarks=False)[0]))

    b.shard.resample_local = watched
    did = []
    for s in range(STEPS):
        # every third observation is tight (Neff falls far below 0.75 n: a resampling), the others so wide that the weights stay
        # close to what they were (uniform after a resampling: none)
        z, ids, R = _obs(s, 0.3, 0.05 if s % 3 == 0 else 2.0)
        out = [f.step(V, G, WB, Q, DT, z, ids, R) for f in (a, b, c)]
        assert out[0] == out[1] == out[2]
        did.append(out[0][1])
        ref.record(b.shard.download(landmarks=False)[0])
    print(f"track_path {dtype}: the Neff rule resampled at {[s for s, d in enumerate(did) if d]}")
    assert any(did) and not all(did), f"the Neff rule resampled at {did}: the run tests one branch only"
    assert a.resamples == b.resamples == c.resamples == sum(did) == ref.resamples
    assert a.path_history.info() == ref.info()
    path, mean = a.path(), a.mean_path()
    final = a.shard.download()
    _same_download(final, b.shard.download(), "tracked against watched")
    _same_download(final, c.shard.download(), "tracked against untracked")
    rb, rpath = ref.best(final[1])
    assert path.shape == (cap, 3) and np.array_equal(path, rpath)
    assert a.path_history.best()[0] == rb == a.best_particle()[0]
    assert np.array_equal(a.path_history.survivors(), ref.survivors())
    # (a normalisation shift may still be deferred in `a`: the downloaded log-weights then carry one more rounding of the storage
    #  type than the stored ones the mean was formed from, 6e-8 of |logw| in fp32 on every weight -- far below 1e-6 on the means)
    assert mean.shape == (cap, 4) and np.allclose(mean[:, :3], ref.mean(final[1])[0][:, :3], rtol=0, atol=1e-6)
    with pytest.raises(RuntimeError):
        c.path()
    with pytest.raises(RuntimeError):
        c.mean_path()
    # while tracking: the enqueued steps and the evidence step are refused before anything is enqueued
    z, ids, R = _obs(0, 0.3, SKEW["mild"][0])
    with pytest.raises(RuntimeError):
        a.step_async(V, G, WB, Q, DT, z, ids, R)
    with pytest.raises(RuntimeError):
        a.step_async_batch(pkg.PFShard.prepare_batch([(V, G)], [(z, ids)]), WB, Q, DT, R)
    with pytest.raises(RuntimeError):
        a.step_unknown_pruned(V, G, WB, Q, DT, z, R, 4.0, 25.0, None)
    _same_download(final, a.shard.download(), "after the refused steps")
    for f in (a, b, c):
        f.close()


def test_track_path_refuses_a_sharded_filter(pkg):
    class TwoRanks:
        rank, world = 0, 2

    sh = pkg.PFShard(64, 2, 5, dtype="f32", first=0, n_global=128)
    f = pkg.FastSLAM(sh, TwoRanks())
    with pytest.raises(ValueError):
        f.track_path(4)
    assert f.path_history is None
    sh.close()
