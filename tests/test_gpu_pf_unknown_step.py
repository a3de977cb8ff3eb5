"""GPU tests of the fused unknown-correspondence step (slam_pf_step_unknown via PFShard.step_unknown_fused /
FastSLAM.step_unknown_fused): predict + per-particle association + updates / new landmarks + weight statistics in one
sweep, for up to 64 observations per call.

Up to 16 observations the call must leave the filter BIT for bit as slam_pf_predict + slam_pf_update_unknown +
slam_pf_weight_stats do (same decisions, same three statistics); beyond 16 the reference is the fp64 oracle
(oracle/pf_ref.py::OraclePF.predict + update_unknown) with the tolerances of tests/test_gpu_pf.py."""
import functools
import math

import numpy as np
import pytest

from oracle import pf_ref as F
from test_gpu_pf import Q, R, TOL, close, observe

pytestmark = pytest.mark.gpu

GATE1, GATE2 = 4.0, 25.0
LM7 = np.array([[12.0, 3.0], [6.0, -9.0], [-10.0, 4.0], [15.0, -2.0], [-4.0, -12.0], [9.0, 11.0], [-13.0, -6.0]])


def _same_state(a, b, what):
    for x, y, part in zip(a.download(), b.download(), ("pose", "logw", "landmarks")):
        assert np.array_equal(x, y), f"{what}: {part} differ"


# ---- 1. m <= 16: the three calls, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1500 + 13, 70])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_equals_the_three_calls_bit_for_bit(pkg, dtype, n):
    """The plan of test_unknown_correspondences_against_oracle (empty map at the start, revisits, capacity overflow, one
    observation inside gate2 only) on two shards with the same seed: predict + update_unknown + weight_stats against
    step_unknown_fused.  After every step the decisions, the whole state and the three statistics are identical; step 2
    carries a pending normalisation shift.  n = 1513: six workgroups of 256 particles, the last one ragged; n = 70: more
    than one wave, less than one workgroup."""
    nslots, seed = 6, 11
    a = pkg.PFShard(n, nslots, seed, dtype=dtype)
    b = pkg.PFShard(n, nslots, seed, dtype=dtype)
    for f in (a, b):
        f.set_pose([0.5, -0.5, 0.3])
        f.clear_landmarks()
    rng = np.random.default_rng(5)
    pose = np.array([0.5, -0.5, 0.3])
    plan = [[1, 2], [2, 1, 3], [1, 3, 4, 2], [5, 1], [6, 2, 3], [7, 4, 6]]          # 7 > 6 slots: the last new one is dropped
    seen_drop = seen_new = seen_match = False
    for t, ids in enumerate(plan):
        pose = np.array([pose[0] + 0.3 * math.cos(0.02 * t + pose[2]), pose[1] + 0.3 * math.sin(0.02 * t + pose[2]),
                         pose[2] + 0.3 * math.sin(0.02 * t) / 4.0])
        z = observe(LM7, pose, np.array(ids), rng)
        if t == 3:
            z = np.hstack([z, z[:, 1:2] + np.array([[0.35], [0.0]])])      # 3.5 sigma off in range: inside gate2 only
        if t == 2:                                                         # a pending shift on the way into the step
            a.normalize(sa[0], sa[1])
            b.normalize(sb[0], sb[1])
        a.predict(3.0, 0.02 * t, 4.0, Q, 0.1)
        assoc_a = a.update_unknown(z, R, GATE1, GATE2, want_assoc=True).cpu().numpy()
        sa = a.weight_stats()
        sb, assoc_b = b.step_unknown_fused(3.0, 0.02 * t, 4.0, Q, 0.1, z, R, GATE1, GATE2, want_assoc=True)
        assoc_b = assoc_b.cpu().numpy()
        assert np.array_equal(assoc_a, assoc_b), f"step {t}: decisions differ"
        _same_state(a, b, f"step {t}")
        assert sa == sb, f"step {t}: statistics {sa} {sb}"
        seen_drop |= bool((assoc_b == -2).any())
        seen_new |= bool((assoc_b == -1).any())
        seen_match |= bool((assoc_b >= 0).any())
    assert seen_drop and seen_new and seen_match
    assert int((b.download()[2][:, 2, :] >= 0).sum(axis=0).max()) == nslots          # the capacity was reached
    a.close()
    b.close()


# ---- 2. m beyond 16: the oracle ----------------------------------------------------------------------------------------------
N2, SLOTS2, SEED2, DT2 = 600 + 7, 80, 23, 0.02
POSE2 = np.array([0.0, 0.0, 0.3])


def _scene2():
    """84 landmarks on a 12 x 7 grid of 10 m cells, jittered by at most 1 m per axis: spacing at least 8 m, none closer than
    4 m to the vehicle.  (More than the 80 slots: the step of 33 observations has to overflow them.)"""
    g = np.random.default_rng(61)
    xs, ys = np.meshgrid(-55.0 + 10.0 * np.arange(12), -30.0 + 10.0 * np.arange(7), indexing="ij")
    lm = np.stack([xs.ravel(), ys.ravel()], axis=1) + g.uniform(-1.0, 1.0, (84, 2))
    return lm[g.permutation(84)]


def _observe_quiet(lm, pose, ids, rng):
    """(range, bearing) of landmarks `ids` (0-based) from `pose` with 0.3 sigma of sensor noise: a revisit's NIS stays far
    below gate1, so no decision of the scene sits at a gate (asserted from the oracle's own numbers below)."""
    dx, dy = lm[ids, 0] - pose[0], lm[ids, 1] - pose[1]
    return np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + 0.3 * rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))


def _plan2():
    lm = _scene2()
    rng = np.random.default_rng(62)
    pose = POSE2.copy()
    steps = []
    first64 = np.arange(64)
    mixed = np.empty(33, dtype=np.int64)                        # 13 revisits between 20 new landmarks: 16 fit, 4 are dropped
    mixed[0::5] = [3, 40, 63, 17, 58, 9, 31]
    rest = np.setdiff1d(np.arange(33), np.arange(0, 33, 5))
    mixed[rest[:20]] = np.arange(64, 84)
    mixed[rest[20:]] = [22, 47, 5, 60, 12, 35]
    last = np.array([7, 33, 50, 2, 61, 19, 33, 44, 28, 11, 56, 39, 0, 24, 62, 15])      # landmark 33 twice
    for ids in (first64, first64, mixed, last):
        pose = np.array([pose[0] + 3.0 * DT2 * math.cos(0.02 + pose[2]), pose[1] + 3.0 * DT2 * math.sin(0.02 + pose[2]),
                         pose[2] + 3.0 * DT2 * math.sin(0.02) / 4.0])
        z = _observe_quiet(lm, pose, ids, rng)
        steps.append(z)
    z = steps[3]
    steps[3] = np.hstack([z, z[:, 4:5] + np.array([[0.35], [0.0]])])        # m = 17: 3.5 sigma off in range, inside gate2 only
    return steps


def _scores(orc, z):
    """nis, nd [m, slots, n] of every (observation, slot) pair and the used mask [slots, n]: the arithmetic of
    OraclePF.associate_unknown on the oracle's state, kept whole so that the margins can be asserted."""
    x, y, phi = orc.pose
    lx, ly, pxx, pxy, pyy = (orc.lm[:, k, :] for k in range(5))
    used = pxx >= 0.0
    with np.errstate(all="ignore"):
        dx, dy = lx - x, ly - y
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2)
        zp1 = np.arctan2(dy, dx) - phi
        h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
        t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
        t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
        s00 = h00 * t00 + h01 * t10 + R[0, 0]
        s01 = h00 * t01 + h01 * t11 + R[0, 1]
        s10 = h10 * t00 + h11 * t10 + R[1, 0]
        s11 = h10 * t01 + h11 * t11 + R[1, 1]
        det = s00 * s11 - s01 * s10
        qa, qb, qc = s11 / det, -(s01 + s10) / det, s00 / det
        v0 = z[0][:, None, None] - d[None]
        v1 = z[1][:, None, None] - zp1[None]
        v1 = np.where(v1 > math.pi, v1 - 2 * math.pi, np.where(v1 < -math.pi, v1 + 2 * math.pi, v1))
        nis = qa[None] * v0 * v0 + qb[None] * v0 * v1 + qc[None] * v1 * v1
        nd = nis + np.log(det)[None]
    return nis, nd, used


@functools.lru_cache(maxsize=1)
def _oracle_run2():
    """The oracle's run over the four steps, computed once: per step the observations, the decisions, the state after the
    step, and the smallest relative distance of any (observation, used slot) NIS from a gate / the smallest gap between the
    best and the second-best candidate of a matched observation."""
    orc = F.OraclePF(N2, SLOTS2, SEED2)
    orc.set_pose(POSE2)
    orc.clear_landmarks()
    out = []
    for z in _plan2():
        orc.predict(3.0, 0.02, 4.0, Q, DT2)
        nis, nd, used = _scores(orc, z)
        u = np.broadcast_to(used[None], nis.shape)
        gate_margin = min(float(np.min(np.abs(nis[u] - g) / g)) if u.any() else np.inf for g in (GATE1, GATE2))
        cand = np.where(u & (nis < GATE1), nd, np.inf)
        two = np.sort(cand, axis=1)[:, :2, :]
        matched = np.isfinite(two[:, 0, :])
        nd_gap = float(np.min(two[:, 1, :][matched] - two[:, 0, :][matched])) if matched.any() else np.inf
        free_before = (~used).sum(axis=0)
        assoc = orc.update_unknown(z, R, GATE1, GATE2)
        # a decision of -1 that found no slot is returned as -1 by the association and dropped by the update: what the
        # library reports as its decision is the association's value, so compare those
        out.append(dict(z=z, assoc=assoc.copy(), pose=orc.pose.copy(), lm=orc.lm.copy(), logw=orc.logw.copy(),
                        gate_margin=gate_margin, nd_gap=nd_gap, near_only=(assoc == -2), free_before=free_before))
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_more_than_16_observations_against_the_oracle(pkg, dtype):
    """80 slots, 84 landmarks all in view.  m = 64 all new; m = 64 the same landmarks (matched, slots far beyond 16);
    m = 33 revisits and new ones until the 80 slots overflow; m = 17 with one landmark observed twice in the call and one
    observation 3.5 sigma off in range (inside gate2 only: dropped).  fp64: identical decisions.  fp32: at least 0.999 of
    them -- and the scene itself leaves no decision near an edge: from the oracle's numbers alone, no (observation, slot)
    NIS lies within 1e-3 (relative) of a gate and the two best candidates of a matched observation are more than 1e-3
    apart, so the cap only guards against rounding in the fp32 geometry."""
    run = _oracle_run2()
    for t, s in enumerate(run):
        assert s["gate_margin"] > 1e-3, f"step {t}: a NIS sits at a gate ({s['gate_margin']:.2e})"
        assert s["nd_gap"] > 1e-3, f"step {t}: two candidates tie ({s['nd_gap']:.2e})"
    assert [s["z"].shape[1] for s in run] == [64, 64, 33, 17]
    sh = pkg.PFShard(N2, SLOTS2, SEED2, dtype=dtype)
    sh.set_pose(POSE2)
    sh.clear_landmarks()
    tol = TOL[dtype]
    agree = total = 0
    for t, s in enumerate(run):
        stats, a = sh.step_unknown_fused(3.0, 0.02, 4.0, Q, DT2, s["z"], R, GATE1, GATE2, want_assoc=True)
        a = a.cpu().numpy()
        ao = s["assoc"]
        agree += int(np.sum(a == ao))
        total += a.size
        if dtype == "f64":
            assert np.array_equal(a, ao), f"step {t}"
        same = np.all(a == ao, axis=0)                    # compare the state where the decisions agree
        pose_g, logw_g, lm_g = sh.download()
        assert close(pose_g[:, same], s["pose"][:, same], tol, scale=20.0), f"pose step {t}"
        used_o = s["lm"][:, 2, :] >= 0
        assert np.array_equal((lm_g[:, 2, :] >= 0)[:, same], used_o[:, same]), f"slot usage step {t}"
        mask = np.broadcast_to(used_o[:, None, :] & same[None, None, :], s["lm"].shape)
        assert close(np.where(mask, lm_g, 0.0), np.where(mask, s["lm"], 0.0), 10 * tol, scale=20.0), f"landmarks step {t}"
        assert close(logw_g[same], s["logw"][same], 10 * tol, scale=max(1.0, float(np.max(np.abs(s["logw"]))))), f"logw step {t}"
        assert stats[0] == float(logw_g.max())
    assert agree >= 0.999 * total
    assert np.all(run[0]["assoc"] == -1) and np.all(run[1]["assoc"] >= 0) and int(run[1]["assoc"].max()) == 63
    assert int((run[2]["lm"][:, 2, :] >= 0).sum(axis=0).max()) == SLOTS2          # the capacity was reached
    # step 2: 20 new landmarks met 16 unused slots -- the last four found none (the association says -1, the slot count says
    # dropped); step 3: the observation inside gate2 only is a -2 of the association itself
    new2 = (run[2]["assoc"] == -1).sum(axis=0)
    assert np.all(new2 == 20) and np.all(run[2]["free_before"] == 16)
    assert np.all(run[3]["assoc"][16] == -2) and np.all(run[3]["assoc"][:16] >= 0)
    assert np.all(run[3]["assoc"][1] == run[3]["assoc"][6])                         # the landmark observed twice
    sh.close()


# ---- 3. an observation index beyond 31 in the "near" set ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gate2_only_observation_beyond_index_31(pkg, dtype):
    """m = 40 with observation 37 the one inside gate2 only: it must be dropped by every particle and open no slot (a 32-bit
    `near` mask would lose it and start a landmark)."""
    n, nslots = 300, 48
    lm = _scene2()
    sh = pkg.PFShard(n, nslots, 7, dtype=dtype)
    sh.set_pose(POSE2)
    sh.clear_landmarks()
    rng = np.random.default_rng(8)
    ids = np.arange(40)
    pose = np.array([POSE2[0] + 3.0 * DT2 * math.cos(0.02 + POSE2[2]), POSE2[1] + 3.0 * DT2 * math.sin(0.02 + POSE2[2]),
                     POSE2[2] + 3.0 * DT2 * math.sin(0.02) / 4.0])
    _, a0 = sh.step_unknown_fused(3.0, 0.02, 4.0, Q, DT2, _observe_quiet(lm, pose, ids, rng), R, GATE1, GATE2, want_assoc=True)
    assert bool((a0 == -1).all())
    z = _observe_quiet(lm, pose, ids, rng)
    z[0, 37] += 0.35                                           # 3.5 sigma off in range: inside gate2 only
    _, a1 = sh.step_unknown_fused(0.0, 0.0, 4.0, Q, DT2, z, R, GATE1, GATE2, want_assoc=True)
    a1 = a1.cpu().numpy()
    assert np.all(a1[37] == -2)
    assert np.all(np.delete(a1, 37, axis=0) >= 0)
    assert np.all((sh.download()[2][:, 2, :] >= 0).sum(axis=0) == 40)
    sh.close()


# ---- 4. after a lazy resampling -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_unknown_step_after_lazy_resampling(pkg, monkeypatch, dtype):
    """Live ancestor tables (three known-id auto steps with forced resamplings) must be materialised before the sweep: a
    lazy and an eager (SLAMHIP_PF_EAGER=1) shard stay bit-identical through two fused unknown steps, the known-id steps
    and a fused unknown step of 20 observations."""
    n, nslots, seed = 2048, 12, 19
    lm = _scene2()
    f = {}
    for name, flag in (("lazy", "0"), ("eager", "1")):
        monkeypatch.setenv("SLAMHIP_PF_EAGER", flag)
        sh = pkg.PFShard(n, nslots, seed, dtype=dtype)
        sh.set_pose(POSE2)
        sh.clear_landmarks()
        f[name] = pkg.FastSLAM(sh, None)
    monkeypatch.delenv("SLAMHIP_PF_EAGER", raising=False)
    rng = np.random.default_rng(20)
    zs = [_observe_quiet(lm, POSE2, np.arange(0, 5), rng), _observe_quiet(lm, POSE2, np.arange(2, 9), rng)]
    zk = [_observe_quiet(lm, POSE2, np.array([0, 3, 6]) + k, rng) for k in range(3)]
    z20 = _observe_quiet(lm, POSE2, np.arange(0, 20), rng)
    outs = {}
    for name, g in f.items():
        o = [g.shard.step_unknown_fused(0.5, 0.02, 4.0, Q, DT2, z, R, GATE1, GATE2) for z in zs]
        for k in range(3):
            g.step_async(0.5, 0.02, 4.0, Q, DT2, zk[k], np.array([1, 4, 7]) + k, R, force_resample=True)
        o.append(g.flush())
        st, a = g.shard.step_unknown_fused(0.5, 0.02, 4.0, Q, DT2, z20, R, GATE1, GATE2, want_assoc=True)
        o += [st, a.cpu().numpy().tobytes()]
        outs[name] = o
    assert outs["lazy"] == outs["eager"]
    _same_state(f["lazy"].shard, f["eager"].shard, "after the fused unknown step")
    for g in f.values():
        g.shard.close()


# ---- 5. arguments -------------------------------------------------------------------------------------------------------------
def test_arguments_of_the_fused_unknown_step(pkg):
    import ctypes as C
    BAD = pkg._lib.SLAM_E_BADARG
    n, nslots, seed = 500, 6, 3
    a = pkg.PFShard(n, nslots, seed, dtype="f32")
    twin = pkg.PFShard(n, nslots, seed, dtype="f32")
    rng = np.random.default_rng(4)
    z2 = observe(LM7, np.array([0.5, -0.5, 0.3]), np.array([1, 2]), rng)
    for f in (a, twin):
        f.set_pose([0.5, -0.5, 0.3])
        f.clear_landmarks()
    for f in (a, twin):
        f.step_unknown_fused(3.0, 0.02, 4.0, Q, 0.1, z2, R, GATE1, GATE2)
    before = a.download()
    with pytest.raises(pkg.SlamHipError) as ei:                                     # m = 65
        a.step_unknown_fused(3.0, 0.02, 4.0, Q, 0.1, np.ones((2, 65)), R, GATE1, GATE2)
    assert ei.value.code == BAD
    q, r, out = np.ascontiguousarray(Q.T.reshape(-1)), np.ascontiguousarray(R.T.reshape(-1)), np.empty(3)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    lib = pkg._lib.lib
    assert lib.slam_pf_step_unknown(a._h, 3.0, 0.02, 4.0, dp(q), 0.1, None, 3, dp(r), GATE1, GATE2, None, dp(out)) == BAD    # null z
    assert lib.slam_pf_step_unknown(a._h, 3.0, 0.02, 4.0, dp(q), 0.1, dp(out), -1, dp(r), GATE1, GATE2, None, dp(out)) == BAD
    for x, y in zip(before, a.download()):
        assert np.array_equal(x, y)
    a.predict(3.0, 0.02, 4.0, Q, 0.1)                                               # the RNG step counter did not move
    twin.predict(3.0, 0.02, 4.0, Q, 0.1)
    assert np.array_equal(a.download()[0], twin.download()[0])
    with pytest.raises(pkg.SlamHipError) as ei:                                     # the legacy call keeps its cap
        a.update_unknown(np.ones((2, 17)), R, GATE1, GATE2)
    assert ei.value.code == BAD
    # m = 0: predict + statistics, i.e. step_fused without observations
    none = np.zeros((2, 0))
    s0 = a.step_unknown_fused(3.0, 0.01, 4.0, Q, 0.1, none, R, GATE1, GATE2)
    s1 = twin.step_fused(3.0, 0.01, 4.0, Q, 0.1, none, np.zeros(0, dtype=np.int32), R)
    assert s0 == s1
    _same_state(a, twin, "m = 0")
    for f in (a, twin):
        f.close()


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------
def test_driver_fused_unknown_step_equals_step_unknown(pkg):
    """FastSLAM.step_unknown_fused against FastSLAM.step_unknown on twin fp64 filters over the seven steps of
    test_unknown_correspondence_driver_against_oracle: the same Neff, the same resampling decisions, identical particles."""
    n, nslots, seed = 2048, 8, 41
    lm = LM7[:6]
    f = {name: pkg.FastSLAM(pkg.PFShard(n, nslots, seed, dtype="f64"), None) for name in ("calls", "fused")}
    for g in f.values():
        g.shard.set_pose([0.0, 0.0, 0.2])
        g.shard.clear_landmarks()
    rng = np.random.default_rng(3)
    pose = np.array([0.0, 0.0, 0.2])
    did = []
    for t in range(7):
        pose = np.array([pose[0] + 0.3 * math.cos(0.02 + pose[2]), pose[1] + 0.3 * math.sin(0.02 + pose[2]),
                         pose[2] + 0.3 * math.sin(0.02) / 4.0])
        ids = np.array([1 + t % 6, 1 + (t + 2) % 6, 1 + (t + 4) % 6])
        z = observe(lm, pose, ids, rng)
        n1, d1 = f["calls"].step_unknown(3.0, 0.02, 4.0, Q, 0.1, z, R, GATE1, GATE2, force_resample=(t == 4))
        n2, d2 = f["fused"].step_unknown_fused(3.0, 0.02, 4.0, Q, 0.1, z, R, GATE1, GATE2, force_resample=(t == 4))
        assert n1 == n2 and d1 == d2, f"step {t}: Neff {n1} {n2}, resampled {d1} {d2}"
        _same_state(f["calls"].shard, f["fused"].shard, f"step {t}")
        did.append(d1)
    assert did[4]
    for g in f.values():
        g.shard.close()
