"""GPU tests of FastSLAM 2.0 with unknown correspondences (include/ext/slamhip_proposal.h, libslamhip_proposal.so;
PFShard.step_proposal_unknown / associate_proposal, FastSLAM.step_unknown(proposal=True) / step_unknown_pruned(proposal=True)).

The reference is tests/proposal_unknown_ref.py (fp64, the header's rule run literally) on the scene that
tests/test_proposal_unknown_ref_cpu.py asserts conditions about: 10 of its 72 624 decisions (10 of 1513 particles, 0.66 %) move
when the gates are scaled by +-0.2 %, a thousand times the relative error of an fp32 nis.  fp64 must make the reference's decisions
everywhere; fp32 may lose at most 1 % of the particles to a decision at a gate edge, and the particles that made the reference's
decisions all along are held to the tolerances of tests/test_gpu_pf.py::test_proposal_step_against_oracle (the arithmetic that
moves state is the same).  Beside that: identities, bit for bit, with the product library's step calls on clones."""
import math

import numpy as np
import pytest

from oracle import pf_ref as F
from tests import evidence_ref as E
from tests import proposal_unknown_ref as P
from test_gpu_pf import TOL, close

pytestmark = pytest.mark.gpu

QFULL = np.array([[0.25, 0.004], [0.004, math.radians(3.0) ** 2]])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_state(a, b, what):
    for x, y, part in zip(a.download(), b.download(), ("pose", "logw", "landmarks")):
        assert _same_bits(x, y), f"{what}: {part} differ"


def _shard(pkg, dtype, n=P.N, slots=P.SLOTS, seed=P.SEED, cleared=True):
    sh = pkg.PFShard(n, slots, seed, dtype=dtype)
    sh.set_pose(P.START)
    if cleared:
        sh.clear_landmarks()
    return sh


def _clone(pkg, src, dtype):
    c = pkg.PFShard(src.n, src.nl, src.seed, dtype=dtype)
    c.copy_from(src)
    return c


def _model_of(sh):
    """The reference filter holding exactly what the shard holds."""
    pose, lw, lm = sh.download()
    m = P.ProposalUnknownPF(sh.n, sh.nl, sh.seed)
    m.pose, m.logw, m.lm = pose.astype(np.float64), lw.astype(np.float64), lm.astype(np.float64)
    m.step = sh.meta()["step"]
    return m


def _step_both(sh, orc, G, z, dtype, good, what, q=P.Q, gates=(P.GATE1, P.GATE2)):
    """One step on the shard and on the reference; ``good`` (particles whose every decision so far was the reference's) is
    narrowed and the state of those particles compared.  Returns (statistics, decisions, the reference's decisions)."""
    tol = TOL[dtype]
    stats, a = sh.step_proposal_unknown(P.V, G, P.WHEELBASE, q, P.DT, z, P.R, *gates, want_assoc=True)
    assert stats == sh.weight_stats(), f"{what}: out is not what weight_stats returns"
    a = a.cpu().numpy()
    ref = orc.step_proposal_unknown(P.V, G, P.WHEELBASE, q, P.DT, z, P.R, *gates)
    wrong = (a != ref).any(axis=0) if a.shape[0] else np.zeros(sh.n, dtype=bool)
    print(f"{what} [{dtype}]: {int((a != ref).sum())} of {a.size} decisions differ, in {int(wrong.sum())} particles")
    if dtype == "f64":
        assert not wrong.any(), f"{what}: {int((a != ref).sum())} decisions differ from the reference's"
    good &= ~wrong
    p, lw, l = sh.download()
    g = good
    assert close(p[:, g], orc.pose[:, g], tol), f"{what}: pose"
    assert np.array_equal(l[:, 2, g] >= 0, orc.lm[:, 2, g] >= 0), f"{what}: slot usage"
    assert close(l[:, 0:2, g], orc.lm[:, 0:2, g], tol), f"{what}: landmark means"
    assert close(l[:, 2:5, g], orc.lm[:, 2:5, g], tol * 10, scale=float(np.max(np.abs(orc.lm[:, 2:5, g])))), f"{what}: landmark cov"
    assert close(lw[g], orc.logw[g], tol * 10, scale=max(1.0, float(np.max(np.abs(orc.logw[g]))))), f"{what}: log-weights"
    assert stats[0] == float(lw.max())
    return stats, a, ref


# ---- 1. the scene against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scene_against_the_reference(pkg, dtype):
    """n = 1513 (six workgroups, the last partly filled), 8 slots, 12 steps, normalised every step (every step but the first
    enters with a pending shift), a ninth landmark from step 9 on: the slots are exhausted and the observation is reported -2.
    Measured on one MI355X: 0 of the 77 163 decisions differ from the reference's in fp64 and in fp32."""
    sh, orc = _shard(pkg, dtype), P.fresh()
    good = np.ones(P.N, dtype=bool)
    capacity = 0
    for t, (G, z) in enumerate(P.scene(ninth_from=9)):
        stats, a, ref = _step_both(sh, orc, G, z, dtype, good, f"step {t}")
        capacity += int((a[orc.last_capacity] == -2).sum())
        om, o1, _ = orc.weight_stats()
        sh.normalize(stats[0], stats[1])
        orc.normalize(om, o1)
    print(f"[{dtype}] particles that made the reference's decisions throughout: {int(good.sum())} of {P.N}")
    assert (~good).sum() <= 0.01 * P.N
    assert orc.last_capacity.any() and capacity > 0
    assert int((sh.download()[2][:, 2, :] >= 0).sum(axis=0).max()) == P.SLOTS          # the capacity was reached
    assert sh.meta()["step"] == P.STEPS
    sh.close()


# ---- 2. identities with the product library's steps, on clones ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_without_observations_it_is_the_fused_unknown_step_bit_for_bit(pkg, dtype):
    a = _shard(pkg, dtype)
    for t, (G, z) in enumerate(P.scene(3)):                                # a map and uneven weights to start from
        a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    b = _clone(pkg, a, dtype)
    none = np.zeros((2, 0))
    sa, da = a.step_proposal_unknown(P.V, 0.02, P.WHEELBASE, P.Q, P.DT, none, P.R, P.GATE1, P.GATE2, want_assoc=True)
    sb = b.step_unknown_fused(P.V, 0.02, P.WHEELBASE, P.Q, P.DT, none, P.R, P.GATE1, P.GATE2)
    assert sa == sb and da.shape == (0, a.n)
    _same_state(a, b, "m = 0")
    ma, mb = a.meta(), b.meta()
    assert ma["step"] == mb["step"] == 4 and ma["seed"] == mb["seed"]
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_on_a_cleared_map_it_is_the_fused_unknown_step_bit_for_bit(pkg, dtype):
    a = _shard(pkg, dtype)
    b = _clone(pkg, a, dtype)
    G, z = P.scene(1)[0]
    z = z[:, :3]
    sa, da = a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_assoc=True)
    sb, db = b.step_unknown_fused(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_assoc=True)
    da, db = da.cpu().numpy(), db.cpu().numpy()
    assert sa == sb and np.array_equal(da, db) and (da == -1).all()
    _same_state(a, b, "cleared map")
    assert a.meta()["step"] == b.meta()["step"] == 1
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_with_wide_gates_it_is_the_known_id_proposal_step(pkg, dtype):
    """Six landmarks from init_landmarks, five observations (landmark 3 twice), a full Q, gates so wide that the nearest
    landmark always matches: the decisions are ids - 1 and the step is slam_pf_step_proposal with those ids.  The arithmetic
    is copied term for term, so the two agree bit for bit (asserted; TOL is what the issue asks for at least)."""
    n = 1513
    ids = np.array([1, 3, 6, 3, 2])
    lms = P.LANDMARKS[:6]
    a = pkg.PFShard(n, 6, 3, dtype=dtype)
    a.set_pose(P.START)
    a.init_landmarks(lms, 0.04, 0.1)
    a.predict(P.V, 0.0, P.WHEELBASE, P.Q, P.DT)                            # the particles spread
    b = _clone(pkg, a, dtype)
    rng = np.random.default_rng(4)
    pose = np.array(P.START) + [2 * P.V * P.DT * math.cos(P.START[2]), 2 * P.V * P.DT * math.sin(P.START[2]), 0.0]
    dx, dy = lms[ids - 1, 0] - pose[0], lms[ids - 1, 1] - pose[1]
    z = np.vstack([np.hypot(dx, dy) + 0.05 * rng.standard_normal(5), np.arctan2(dy, dx) - pose[2] + 0.008 * rng.standard_normal(5)])
    sa, da = a.step_proposal_unknown(P.V, 0.03, P.WHEELBASE, QFULL, P.DT, z, P.R, 1e6, 1e9, want_assoc=True)
    sb = b.step_proposal(P.V, 0.03, P.WHEELBASE, QFULL, P.DT, z, ids, P.R)
    assert np.array_equal(da.cpu().numpy(), np.repeat((ids - 1)[:, None], n, axis=1).astype(np.int32))
    tol = TOL[dtype]
    (pa, wa, la), (pb, wb, lb) = a.download(), b.download()
    assert close(pa, pb, tol) and close(la[:, 0:2], lb[:, 0:2], tol)
    assert close(la[:, 2:5], lb[:, 2:5], tol * 10, scale=float(np.max(np.abs(lb[:, 2:5]))))
    assert close(wa, wb, tol * 10, scale=max(1.0, float(np.max(np.abs(wb)))))
    assert sa[0] == pytest.approx(sb[0], abs=tol * 50) and sa[1] == pytest.approx(sb[1], rel=tol * 200)
    bitwise = all(_same_bits(x, y) for x, y in ((pa, pb), (wa, wb), (la, lb))) and sa == sb
    print(f"[{dtype}] bit for bit with slam_pf_step_proposal: {bitwise}")
    assert bitwise
    a.close()
    b.close()


# ---- 3. the association alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_associate_proposal_reads_only_and_announces_the_step(pkg, dtype):
    a = _shard(pkg, dtype)
    sc = P.scene(5, ninth_from=4)                                          # the last step: two new landmarks, one slot free
    for G, z in sc[:4]:
        s = a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    a.normalize(s[0], s[1])
    G, z = sc[4]
    orc = _model_of(a)
    before, meta = a.download(), a.meta()
    b = _clone(pkg, a, dtype)
    dec, nis = a.associate_proposal(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_nis=True)
    only = a.associate_proposal(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    dec, nis = dec.cpu().numpy(), nis.cpu().numpy()
    assert np.array_equal(dec, only.cpu().numpy())
    after, meta2 = a.download(), a.meta()
    assert all(_same_bits(x, y) for x, y in zip(before, after))
    assert {k: v for k, v in meta.items() if k != "seen"} == {k: v for k, v in meta2.items() if k != "seen"}
    _, stepped = b.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_assoc=True)
    # the step reports -2 where a new landmark finds no unused slot: the particle's k-th new one with fewer than k slots free
    free = (before[2][:, 2, :] < 0).sum(axis=0)
    full = (dec == -1) & (np.cumsum(dec == -1, axis=0) > free[None, :])
    assert full.any() and (~full & (dec == -1)).any()
    assert np.array_equal(np.where(full, -2, dec), stepped.cpu().numpy())
    ref = orc.associate_proposal(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    agree = dec == ref
    print(f"[{dtype}] associate: {int((~agree).sum())} of {dec.size} decisions differ from the reference on the same state")
    assert agree.all() if dtype == "f64" else (~agree).any(axis=0).sum() <= 0.01 * a.n
    hit = agree & (ref >= 0)
    assert hit.sum() > a.n and np.isnan(nis[agree & (ref < 0)]).all() and (ref < 0).any()
    rel = np.abs(nis[hit] - orc.last_nis[hit]) / np.maximum(np.abs(orc.last_nis[hit]), 1.0)
    print(f"[{dtype}] nis: largest relative error {float(rel.max()):.3e}")
    assert float(rel.max()) <= 10 * TOL[dtype]
    a.close()
    b.close()


# ---- 4. small shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("n", [5, 256, 257])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_small_shapes_against_the_reference(pkg, dtype, n, m):
    """Less than a wave, exactly one workgroup, one workgroup and one particle; one observation and sixteen (every landmark
    looked at twice in one call: a slot matched twice, new landmarks between matches)."""
    sh, orc = _shard(pkg, dtype, n=n), P.fresh(n=n)
    good = np.ones(n, dtype=bool)
    sc = P.scene(4)
    for t, (G, z) in enumerate(sc[:3]):
        stats, _, _ = _step_both(sh, orc, G, z, dtype, good, f"warm-up {t}")
        sh.normalize(stats[0], stats[1])
        orc.normalize(*orc.weight_stats()[:2])
    G, z4 = sc[3]
    if m == 1:
        z = z4[:, :1]
    else:
        # the truth's pose after four steps is not kept by the scene: the second looks are the first with fresh noise
        rng = np.random.default_rng(3)
        first = np.hstack([sc[3][1], sc[2][1][:, :1], sc[1][1][:, :1], sc[0][1][:, :1], sc[3][1][:, :1]])
        z = np.hstack([first, first + np.vstack([0.02 * rng.standard_normal(8), 0.003 * rng.standard_normal(8)])])
    assert z.shape[1] == m
    _, a, ref = _step_both(sh, orc, G, z, dtype, good, f"m = {m}")
    assert good.sum() >= n - max(1, n // 100) if dtype == "f32" else good.all()
    assert (ref >= 0).any()
    sh.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_behind_a_lazy_resampling_it_is_the_step_on_materialised_maps(pkg, dtype):
    a = _shard(pkg, dtype)
    f = pkg.FastSLAM(a, None)
    sc = P.scene(5)
    for G, z in sc[:3]:
        f.step_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, force_resample=False, proposal=True)
    G, z = sc[3]
    _, did = f.step_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, force_resample=True, proposal=True)
    assert did and f.resamples == 1                                        # the records now sit behind ancestor tables
    b = _clone(pkg, a, dtype)                                              # ... and here in their particles' slots
    G, z = sc[4]
    sa, da = a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_assoc=True)
    sb, db = b.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2, want_assoc=True)
    assert sa == sb and np.array_equal(da.cpu().numpy(), db.cpu().numpy()) and (da >= 0).any()
    _same_state(a, b, "behind the resampling")
    a.close()
    b.close()


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bad_arguments_leave_state_and_rng_alone(pkg, dtype):
    BAD = pkg._lib.SLAM_E_BADARG
    a = _shard(pkg, dtype, n=300)
    G, z = P.scene(1)[0]
    a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    before, meta = a.download(), a.meta()
    z17 = np.tile(z, (1, 5))[:, :17]
    znan = z.copy()
    znan[1, 2] = float("nan")
    qbad = np.array([[0.25, 0.3], [0.3, 0.1]])
    for zz, q in ((z17, P.Q), (znan, P.Q), (z, qbad)):
        for call in (a.step_proposal_unknown, a.associate_proposal):
            with pytest.raises(pkg._lib.SlamHipError) as e:
                call(P.V, G, P.WHEELBASE, q, P.DT, zz, P.R, P.GATE1, P.GATE2)
            assert e.value.code == BAD
    after, meta2 = a.download(), a.meta()
    assert all(_same_bits(x, y) for x, y in zip(before, after))
    assert {k: v for k, v in meta.items() if k != "seen"} == {k: v for k, v in meta2.items() if k != "seen"} and meta2["step"] == 1
    part = pkg.PFShard(128, P.SLOTS, P.SEED, dtype=dtype, first=128, n_global=256)      # a shard of a larger filter
    part.set_pose(P.START)
    part.clear_landmarks()
    before, meta = part.download(), part.meta()
    for call in (part.step_proposal_unknown, part.associate_proposal):
        with pytest.raises(pkg._lib.SlamHipError) as e:
            call(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
        assert e.value.code == BAD and "whole filter" in str(e.value)
    assert all(_same_bits(x, y) for x, y in zip(before, part.download())) and part.meta()["step"] == meta["step"] == 0
    part.close()
    a.close()


# ---- 6. the driver --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_driver_with_the_neff_rule_and_evidence(pkg, dtype):
    """Ten steps of the scene with the Neff rule.  `plain`: FastSLAM.step_unknown(proposal=True); `blind`:
    step_unknown_pruned(proposal=True) with an evidence that never has a landmark in view (r_max = 0.5 m): bit-identical to
    `plain`, resamplings included; `pruned`: step_unknown_pruned(proposal=True) with a field of view that prunes, beside a
    shadow that takes the step in pieces (step_proposal_unknown, LandmarkEvidence.update, normalize, the resampling): the
    counters and counts are those of tests/evidence_ref.py driven by the shadow's decisions on the shadow's downloaded state, the
    ancestors of a resampling come from PFShard.ancestors, and the driver stays bit-identical to the shadow."""
    n, nl, seed = P.N, P.SLOTS, P.SEED
    rule = dict(r_max=40.0, half_fov=1.75, inc=1, dec=1, init=1, cap=5)
    sh = {k: _shard(pkg, dtype) for k in ("plain", "blind", "pruned", "shadow")}
    f = {k: pkg.FastSLAM(s, None) for k, s in sh.items()}
    ev = {"blind": pkg.LandmarkEvidence(sh["blind"], 0.5, math.pi / 2), "pruned": pkg.LandmarkEvidence(sh["pruned"], **rule),
          "shadow": pkg.LandmarkEvidence(sh["shadow"], **rule)}
    c_ref = np.full((nl, n), E.EMPTY, dtype=np.int8)
    resampled = pruned_total = 0
    for t, (G, z) in enumerate(P.scene(10)):
        args = (P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
        n0, d0 = f["plain"].step_unknown(*args, proposal=True)
        n1, d1, _ = f["blind"].step_unknown_pruned(*args, ev["blind"], proposal=True)
        assert n0 == n1 and d0 == d1
        _same_state(sh["plain"], sh["blind"], f"step {t}: plain and blind")
        neff, did, counts = f["pruned"].step_unknown_pruned(*args, ev["pruned"], proposal=True)
        # the shadow, in pieces
        stats, a = sh["shadow"].step_proposal_unknown(*args, want_assoc=True)
        pose, _, rec = sh["shadow"].download()
        c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec, pose, a.cpu().numpy(), rule["r_max"], rule["half_fov"], 1, 1, 1, 5)
        assert float(mg["range"].min()) > 1e-5 and float(mg["bearing"].min()) > 1e-5, "a pair sits at the edge of the field of view"
        counts_s = ev["shadow"].update(a)
        assert counts.tolist() == counts_ref == counts_s.tolist(), f"step {t}: counts {counts.tolist()} {counts_ref}"
        assert _same_bits(sh["shadow"].download()[2], rec_ref), f"step {t}: pruned records"
        neff_s = f["shadow"].normalize(stats)
        do = neff_s < f["shadow"].neff_frac * n
        assert neff == neff_s and did == do
        if do:
            u0 = pkg.philox_uniform(f["shadow"].resamples, 2, seed)
            gmax = f["shadow"]._gmax_norm
            anc = sh["shadow"].ancestors(sh["shadow"].logw_tensor(), gmax, u0).cpu().numpy().astype(np.int64)
            ev["shadow"].resample(gmax, u0)
            f["shadow"]._gmax_norm = None
            f["shadow"]._count_resampling()
            c_ref = c_ref[:, anc]
            resampled += 1
        pruned_total += counts_ref[3]
        _same_state(sh["pruned"], sh["shadow"], f"step {t}: driver and shadow")
        assert np.array_equal(ev["pruned"].counters(), c_ref) and np.array_equal(ev["shadow"].counters(), c_ref), f"step {t}: counters"
    assert resampled > 0 and f["pruned"].resamples == resampled and pruned_total > 0
    assert f["plain"].resamples == f["blind"].resamples > 0
    for e in ev.values():
        e.close()
    for s in sh.values():
        s.close()
