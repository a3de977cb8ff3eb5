"""GPU tests of the FastSLAM kernels on the scenes of tests/wrap_scenes.py: headings that cross +-pi and bearings reported in
[-pi, pi], so that every wrap_pi of csrc/pf_device.h, pf_legacy.hip, pf_batch.hip and pf_unknown.hip changes values that
matter (the scenes of tests/test_gpu_pf.py never make one do so; tests/test_wrap_scenes_cpu.py pins that and shows that the
scenes here are as hard as they claim).

a. The calls the suite checks against the fp64 oracle -- predict + update_known + weight_stats, step_proposal, update_unknown,
   step_unknown_fused (up to 40 observations) -- against the oracle on both mirrored starts, at the suite's tolerances
   (wrap_scenes.compare_with_oracle; a wrong wrap is an error of 2 pi against 1e-9 or 2e-4).
b. Every other form of the step bit for bit against the form the suite already compares it with, on the same scene, at the
   smallest particle count that selects the form.
c. The read-outs of the pose (mean_pose_sums, FastSLAM.mean_pose, the pose row of map_sums) in the step in which about half of
   the particles have crossed the seam: the mean heading is near +-pi, not near 0.
d. The sharded instantiations of the step kernels: two shards of one process against the one-rank filter, bit for bit.

Each test prints a line "wrap-record ..." with the shares the scene had and the largest error as a fraction of its bound.
"""
import math
import threading

import numpy as np
import pytest

import wrap_scenes as W
from test_gpu_pf import TOL, _compare, _Rank
from test_gpu_pf_batch import drive
from wrap_scenes import GATE1, GATE2, Q, QF, R, WHEELBASE

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
KV, KDT = W.KNOWN_MOTION["V"], W.KNOWN_MOTION["dt"]
UV, UDT = W.SMALL_MOTION["V"], W.SMALL_MOTION["dt"]


def _record(what, sc, recs, **extra):
    rows = sc.rows
    worst = {k: float(f"{v:.2g}") for k, v in W.worst(recs).items()}
    print(f"wrap-record {what}: crossing {[round(r['cross'], 3) for r in rows]} wrapped-matched {[round(r['v1'], 3) for r in rows]} "
          f"error/bound {worst} {extra if extra else ''}")


def _same_state(a, b, what):
    for x, y, part in zip(a.download(), b.download(), ("pose", "logw", "landmarks")):
        assert np.array_equal(x, y), f"{what}: {part} differ"


# ---- a. against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_update_weights_against_oracle_across_the_seam(pkg, dtype, sign):
    """predict + update_known + weight_stats, normalised after every step, with a repeat and first sightings; at the step with the
    population astride the seam also the pose read-outs (c)."""
    sc = W.known_scene(sign, False)
    sh = pkg.PFShard(sc.n, W.RING_N, sc.seed, dtype=dtype)
    W.fresh_known(sh, sign)
    tol = TOL[dtype]
    recs = []
    for t, ((V, G, z, ids, _), s) in enumerate(zip(sc.steps, sc.run)):
        sh.predict(V, G, WHEELBASE, Q, KDT)
        sh.update_known(z, ids, R)
        try:
            recs.append(W.compare_with_oracle(sh.download(), s, dtype))
        except AssertionError as e:
            raise AssertionError(f"step {t}: {e}") from None
        gm, s1, s2 = sh.weight_stats()
        om, o1, o2 = s.stats
        assert gm == pytest.approx(om, abs=tol * 50) and s1 == pytest.approx(o1, rel=tol * 50) and s2 == pytest.approx(o2, rel=tol * 50)
        sh.normalize(gm, s1)
        if t == sc.astride:
            _pose_read_outs(pkg, sh, s, tol, sign)
    _record(f"known ids {dtype} sign {sign:+d}", sc, recs)
    sh.close()


def _pose_read_outs(pkg, sh, s, tol, sign):
    """(c) at the tolerances test_predict_update_weights_against_oracle and test_map_against_the_oracle use for them."""
    assert 0.10 <= np.mean(np.sign(s.pose[2]) == -sign) <= 0.90                    # the oracle's population is astride the seam
    assert W.close(sh.mean_pose_sums(), s.sums, tol * 50, scale=1.0)[0]
    want = math.atan2(s.sums[2], s.sums[3])
    assert abs(want) > 3.0
    mp = pkg.FastSLAM(sh, None).mean_pose()
    assert abs(mp[2]) > 3.0 and abs(float(W.wrap(mp[2] - want))) <= tol * 50, (mp, want)
    assert W.close(mp[:2], s.sums[:2], tol * 50, scale=1.0)[0]
    s0 = sh.map_sums([])[0]
    assert np.allclose(s0[[1, 2, 6, 7]] / s0[0], s.sums / np.exp(s.logw_norm).sum(), rtol=0, atol=tol * 50)
    assert abs(math.atan2(s0[6], s0[7])) > 3.0


@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_proposal_step_against_oracle_across_the_seam(pkg, dtype, sign):
    """step_proposal with the full Q on odd steps: the wraps of the proposal's mean heading, of its innovations, of the sampled
    heading and of the update from the sampled pose."""
    sc = W.known_scene(sign, True)
    sh = pkg.PFShard(sc.n, W.RING_N, sc.seed, dtype=dtype)
    W.fresh_known(sh, sign)
    tol = TOL[dtype]
    recs = []
    for t, ((V, G, z, ids, _), s) in enumerate(zip(sc.steps, sc.run)):
        stats = sh.step_proposal(V, G, WHEELBASE, QF if t % 2 else Q, KDT, z, ids, R)
        state = sh.download()
        try:
            recs.append(W.compare_with_oracle(state, s, dtype))
        except AssertionError as e:
            raise AssertionError(f"step {t}: {e}") from None
        om, o1, _ = s.stats
        assert stats[0] == float(state[1].max())
        assert stats[0] == pytest.approx(om, abs=tol * 50) and stats[1] == pytest.approx(o1, rel=tol * 200)
        sh.normalize(stats[0], stats[1])
    _record(f"proposal {dtype} sign {sign:+d}", sc, recs)
    sh.close()


def _unknown_against_oracle(pkg, dtype, sign, which, fused, nsteps=None):
    sc = W.unknown_scene(sign, which)
    sh = pkg.PFShard(sc.n, W.UNKNOWN_SLOTS, sc.seed, dtype=dtype)
    W.fresh_unknown(sh, sign)
    recs = []
    run = sc.run[:nsteps]
    for t, s in enumerate(run):
        if fused:
            stats, a = sh.step_unknown_fused(UV, sign * W.STEER, WHEELBASE, Q, UDT, s.z, R, GATE1, GATE2, want_assoc=True)
        else:
            sh.predict(UV, sign * W.STEER, WHEELBASE, Q, UDT)
            a = sh.update_unknown(s.z, R, GATE1, GATE2, want_assoc=True)
        state = sh.download()
        try:
            recs.append(W.compare_with_oracle(state, s, dtype, assoc=(a.cpu().numpy(), s.assoc)))
        except AssertionError as e:
            raise AssertionError(f"step {t}: {e}") from None
        if fused:
            assert stats[0] == float(state[1].max())
    agree, total = sum(r["agree"] for r in recs), sum(r["total"] for r in recs)
    assert agree >= 0.999 * total
    _record(f"unknown {which} {'fused' if fused else 'legacy'} {dtype} sign {sign:+d}", sc, recs, agreement=f"{agree}/{total}",
            gate_margin=round(min(s.gate_margin for s in run), 3))
    sh.close()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_unknown_correspondences_against_oracle_across_the_seam(pkg, dtype, sign, fused):
    """predict + update_unknown, and step_unknown_fused, from an empty map: every matched pair's bearing innovation is wrapped for
    about half of the ring; the decisions (fp64 identical, fp32 at least 0.999 of them) and the state where they agree."""
    _unknown_against_oracle(pkg, dtype, sign, "m16", fused)


@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_unknown_step_with_two_sightings_of_every_landmark(pkg, dtype, sign):
    """m = 32, twice (two sightings of each ring landmark: the second LDS group of 16 scores wrapped innovations, too) and, in
    fp64, m = 40 for the second sweep over the observations."""
    _unknown_against_oracle(pkg, dtype, sign, "m40", True, nsteps=4 if dtype == "f64" else 3)


# ---- b. the other forms, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_equals_the_separate_calls_across_the_seam(pkg, dtype, sign):
    steps = W.driver_scene(sign, 8, False, 3)
    a = pkg.PFShard(W.N_ORACLE, W.RING_N, 5, dtype=dtype)
    b = pkg.PFShard(W.N_ORACLE, W.RING_N, 5, dtype=dtype)
    for f in (a, b):
        W.fresh_known(f, sign)
    for t, (V, G, z, ids, _) in enumerate(steps):
        sa = a.step_fused(V, G, WHEELBASE, Q, KDT, z, ids, R)
        b.predict(V, G, WHEELBASE, Q, KDT)
        b.update_known(z, ids, R)
        sb = b.weight_stats()
        _same_state(a, b, f"step {t}")
        assert sa[0] == sb[0] and abs(sa[1] - sb[1]) <= 1e-12 * sb[1] and abs(sa[2] - sb[2]) <= 1e-12 * sb[2]
    heading = a.download()[0][2].astype(np.float64)
    assert np.all(np.sign(heading) == -sign) and np.all(np.abs(heading) <= math.pi * (1 + 1e-6))     # every particle has crossed
    a.close()
    b.close()


@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_proposal_without_information_is_the_fused_step_across_the_seam(pkg, dtype, sign):
    """No observation, or first sightings only, over the steps in which the heading crosses the seam."""
    lm = W.ring()
    a = pkg.PFShard(W.N_ORACLE, W.RING_N, 17, dtype=dtype)
    b = pkg.PFShard(W.N_ORACLE, W.RING_N, 17, dtype=dtype)
    for f in (a, b):
        W.fresh_known(f, sign)
    rng = np.random.default_rng(3)
    pose = W.start_pose(sign, KV, KDT)
    first = {1: [13, 14], 2: [15], 4: [16]}
    for t in range(6):
        pose = W.advance(pose, KV, sign * W.STEER, KDT)
        ids = np.array(first.get(t, []), dtype=np.int32)
        z = W.observe_wrapped(lm, pose, ids, rng) if len(ids) else np.zeros((2, 0))
        sa = a.step_proposal(KV, sign * W.STEER, WHEELBASE, Q, KDT, z, ids, R)
        sb = b.step_fused(KV, sign * W.STEER, WHEELBASE, Q, KDT, z, ids, R)
        assert sa == sb, f"step {t}"
        _same_state(a, b, f"step {t}")
    heading = a.download()[0][2].astype(np.float64)
    assert np.all(np.sign(heading) == -sign)
    a.close()
    b.close()


@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_unknown_step_equals_the_three_calls_across_the_seam(pkg, dtype, sign):
    sc = W.unknown_scene(sign, "m16")
    a = pkg.PFShard(sc.n, W.UNKNOWN_SLOTS, sc.seed, dtype=dtype)
    b = pkg.PFShard(sc.n, W.UNKNOWN_SLOTS, sc.seed, dtype=dtype)
    for f in (a, b):
        W.fresh_unknown(f, sign)
    for t, z in enumerate(sc.steps):
        a.predict(UV, sign * W.STEER, WHEELBASE, Q, UDT)
        assoc_a = a.update_unknown(z, R, GATE1, GATE2, want_assoc=True).cpu().numpy()
        sa = a.weight_stats()
        sb, assoc_b = b.step_unknown_fused(UV, sign * W.STEER, WHEELBASE, Q, UDT, z, R, GATE1, GATE2, want_assoc=True)
        assert np.array_equal(assoc_a, assoc_b.cpu().numpy()), f"step {t}: decisions differ"
        _same_state(a, b, f"step {t}")
        assert sa == sb, f"step {t}: statistics {sa} {sb}"
    a.close()
    b.close()


def _known_pair(pkg, names, n, seed, dtype, sign):
    f = {}
    for name in names:
        sh = pkg.PFShard(n, W.RING_N, seed, dtype=dtype)
        W.fresh_known(sh, sign)
        f[name] = pkg.FastSLAM(sh, None, neff_frac=0.75)
    return f


# the kernel FastSLAM.step_async takes: the sequential one for a step with a repeated landmark (here the step in which the seam is
# crossed; the other steps of that run take the observation-parallel one), the observation-parallel one, the 4-way and the 2-way one
AUTO_FORMS = [("sequential", "f64", W.N_ORACLE, 2), ("sequential", "f32", W.N_ORACLE, 2), ("parallel", "f64", 5013, 5),
              ("parallel", "f32", 5013, 5), ("4-way", "f32", 60000, 5), ("2-way", "f64", 65536, 5)]


@pytest.mark.parametrize("proposal", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("form,dtype,n,repeat_at", AUTO_FORMS)
def test_auto_mode_equals_the_synchronous_driver_across_the_seam(pkg, form, dtype, n, repeat_at, sign, proposal):
    steps = W.driver_scene(sign, 8, False, repeat_at)
    f = _known_pair(pkg, ("auto", "sync"), n, 58, dtype, sign)
    hist = []
    for t, (V, G, z, ids, force) in enumerate(steps):
        f["auto"].step_async(V, G, WHEELBASE, Q, KDT, z, ids, R, force_resample=force, proposal=proposal)
        hist.append(f["sync"].step(V, G, WHEELBASE, Q, KDT, z, ids, R, force_resample=force, proposal=proposal))
        if t in (W.CROSS_AT - 1, W.CROSS_AT, len(steps) - 1):
            neff, did = f["auto"].flush()
            assert did == hist[-1][1], f"step {t}"
            assert neff == pytest.approx(hist[-1][0], rel=1e-12 if dtype == "f64" else 1e-6)
            assert f["auto"].resamples == f["sync"].resamples
            _compare(f["auto"].shard, f["sync"].shard, f"{form} n {n} step {t}", exact_logw=False)
    assert hist[W.CROSS_AT + 2][1] and f["sync"].resamples >= 1
    heading = f["auto"].shard.download(landmarks=False)[0][2].astype(np.float64)
    assert np.all(np.sign(heading) == -sign)
    for g in f.values():
        g.shard.close()


# (n, the step with a repeated landmark): 8 / 4 / 2 observation ways, and the sequential form -- the repeat is in the first launch
# of four steps, in which the seam is crossed
BATCH_FORMS = [("8 ways", 5013, 5), ("4 ways", 40005, 5), ("2 ways", 70000, 5), ("sequential", 5013, 1)]


@pytest.mark.parametrize("proposal", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,n,repeat_at", BATCH_FORMS)
def test_batch_equals_the_steps_one_by_one_across_the_seam(pkg, form, n, repeat_at, dtype, sign, proposal):
    """K = 4 steps per call with persistent launches allowed, as FastSLAM.drive does (fp64 and the FastSLAM-2.0 step take the
    steps one by one: still the same filter)."""
    K = 4
    steps = W.driver_scene(sign, 2 * K + 8, True, repeat_at)
    f = _known_pair(pkg, ("batch", "single"), n, 58, dtype, sign)
    drive(pkg, f, list(steps), K, (K - 1, len(steps) - 1), f"{form} n {n} {dtype} sign {sign:+d}", proposal=proposal)
    assert f["single"].resamples >= 1
    heading = f["batch"].shard.download(landmarks=False)[0][2].astype(np.float64)
    assert np.all(np.sign(heading) == -sign)
    for g in f.values():
        g.shard.close()


# ---- d. the sharded instantiations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proposal", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
def test_sharded_filter_equals_the_one_rank_filter_across_the_seam(pkg, sign, proposal):
    """The pattern of test_sharded_filter_resamples_on_the_device (two shards of this process with peers attached, one host thread
    each) on the wrap scene: the shards together are the one-rank synchronous filter bit for bit, with no halt."""
    dtype, world, per = "f32", 2, 1365
    n = per * world
    steps = W.driver_scene(sign, 8, False, 3)
    ref_shard = pkg.PFShard(n, W.RING_N, 77, dtype=dtype)
    W.fresh_known(ref_shard, sign)
    ref = pkg.FastSLAM(ref_shard, None, neff_frac=0.75)
    shards = [pkg.PFShard(per, W.RING_N, 77, dtype=dtype, first=r * per, n_global=n) for r in range(world)]
    for sh in shards:
        W.fresh_known(sh, sign)
    pkg.attach_local_peers(shards)
    ranks = [pkg.FastSLAM(sh, _Rank(r, world), neff_frac=0.75) for r, sh in enumerate(shards)]
    hist = [ref.step(V, G, WHEELBASE, Q, KDT, z, ids, R, force_resample=force, proposal=proposal) for V, G, z, ids, force in steps]
    want = ref_shard.download()
    got, errs = [None] * world, []

    def run(r):
        try:
            f = ranks[r]
            assert f.shard.peer_selftest(10000)      # (collective) every peer's inbox write arrives
            for t, (V, G, z, ids, force) in enumerate(steps):
                f.step_async(V, G, WHEELBASE, Q, KDT, z, ids, R, force_resample=force, proposal=proposal)
                if t == W.CROSS_AT - 1:
                    neff, did = f.flush()
                    assert did == hist[t][1] and neff == pytest.approx(hist[t][0], rel=1e-6), f"step {t}"
            neff, did = f.flush()
            assert did == hist[-1][1] and neff == pytest.approx(hist[-1][0], rel=1e-6)
            assert f.resamples == ref.resamples
            got[r] = f.shard.download()              # collective: remote records come home first
        except BaseException as e:                    # noqa: BLE001 -- reported by the main thread
            errs.append((r, e))

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not errs, errs
    assert all(g is not None for g in got)
    assert ref.resamples >= 1
    info = [sh.comm_info() for sh in shards]
    assert all(i["halts"] == 0 and i["peers"] and i["world"] == world and i["resamples"] == ref.resamples for i in info), info
    assert np.array_equal(np.hstack([g[0] for g in got]), want[0]), "poses differ"
    assert np.array_equal(np.concatenate([g[2] for g in got], axis=2), want[2]), "landmarks differ"
    wa = np.concatenate([g[1] for g in got])
    assert np.allclose(wa, want[1], rtol=0, atol=4 * np.finfo(wa.dtype).eps * max(1.0, float(np.abs(want[1]).max())))
    assert np.all(np.sign(want[0][2].astype(np.float64)) == -sign)
    th = [threading.Thread(target=sh.detach_peers) for sh in shards]          # collective, too
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    for sh in shards + [ref_shard]:
        sh.close()
