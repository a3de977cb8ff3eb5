"""GPU tests of the landmark evidence of the unknown-correspondence particle filter (include/slamhip_evidence.h,
libslamhip_evidence.so; PFShard + LandmarkEvidence, FastSLAM.step_unknown_pruned).

The reference is tests/evidence_ref.py on the DOWNLOADED state (fp64 geometry from exactly the stored values, integer counters),
so everything is compared exactly: counters, counts, and records bit for bit.  What makes that legitimate is a condition on the
inputs, asserted in every test that has a field of view: no pair in use lies within 1e-5 (relative range / radians) of a
boundary -- ten times the few-ulp error of fp32 sqrt / atan2 at these magnitudes -- so the kernel's dtype cannot decide otherwise."""
import ctypes as C
import math

import numpy as np
import pytest

import evidence_ref as E
from oracle import pf_ref as F
from test_evidence_ref_cpu import check_scenario_outcome, scenario_gate_margins, scenario_run

pytestmark = pytest.mark.gpu

EMPTY = E.EMPTY


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_state(a, b, what):
    for x, y, part in zip(a.download(), b.download(), ("pose", "logw", "landmarks")):
        assert _same_bits(x, y), f"{what}: {part} differ"


def _dev(sh, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(sh.device)


def _margins_ok(mg):
    assert float(mg["range"].min()) > 1e-5, f"a pair sits at r_max ({float(mg['range'].min()):.2e})"
    assert float(mg["bearing"].min()) > 1e-5, f"a pair sits at the edge of the field of view ({float(mg['bearing'].min()):.2e})"


# ---- 1. the rule on real states ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [6, 130])
@pytest.mark.parametrize("n", [70, 1513, 2052])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rule_on_real_states(pkg, dtype, n, nl):
    """The state of three fused unknown-correspondence steps (tests/evidence_ref.rule_plan: all but a few slots filled), then
    four updates with hand-made decisions (-1, -2, slots of every group of 64, a slot index past the map, 2^30, the most
    negative int32, one slot named twice; 3, 5, 40 and 0 observations) and one more fused step between the second and the
    third, which starts a landmark in the lowest free slot.  Before each update the field of view is picked from the
    downloaded state (evidence_ref.pick_fov): it splits one slot's particles into in view and out of view and keeps every pair
    in use more than 1e-5 away from both boundaries -- asserted, no pair excluded.  After each update: counters and counts equal
    the reference, every record is bit-identical to before or the empty record exactly where the reference prunes, poses and
    log-weights untouched.
    n = 70: less than a workgroup; 1513: two slabs of 1024 particles, the last ragged, n % 4 = 1 (the path without vector
    loads); 2052: three slabs, the last ragged, n % 4 = 0 (the vector path).  nl = 6: one group of slots; 130: three groups of
    64, the last ragged."""
    P = E.RULE
    _, fill, between = E.rule_plan(nl)
    sh = pkg.PFShard(n, nl, 11, dtype=dtype)
    sh.set_pose(P["pose"])
    sh.clear_landmarks()
    for z in fill:
        sh.step_unknown_fused(P["V"], P["G"], P["wheelbase"], E.RULE_Q, P["dt"], z, E.SCN_R, P["gate1"], P["gate2"])
    ev = pkg.LandmarkEvidence(sh, 30.0, 1.5, P["inc"], P["dec"], P["init"], P["cap"])
    c_ref = np.full((nl, n), EMPTY, dtype=np.int8)
    assert np.array_equal(ev.counters(), c_ref)
    total = np.zeros(4, dtype=np.int64)
    split_seen = False
    for u, m in enumerate((3, 5, 40, 0)):
        if u == 2:
            sh.step_unknown_fused(P["V"], P["G"], P["wheelbase"], E.RULE_Q, P["dt"], between, E.SCN_R, P["gate1"], P["gate2"])
        pose, logw, rec = sh.download()
        ev.r_max, ev.half_fov, slot = E.pick_fov(pose, rec)
        a = E.hand_decisions(u, m, n, nl) if m else None
        c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec, pose, a, ev.r_max, ev.half_fov, P["inc"], P["dec"],
                                                           P["init"], P["cap"])
        _margins_ok(mg)
        used = ~(rec[slot, 2, :] < 0)
        split_seen |= bool(mg["in_view"][slot][used].any() and (~mg["in_view"][slot][used]).any())
        counts = ev.update(_dev(sh, a))
        pose2, logw2, rec2 = sh.download()
        c = ev.counters()
        assert np.array_equal(c, c_ref), f"update {u}: {int((c != c_ref).sum())} counters differ"
        assert counts.tolist() == counts_ref, f"update {u}: counts {counts.tolist()} {counts_ref}"
        assert _same_bits(rec2, rec_ref), f"update {u}: records"
        changed = np.any(_bits(rec2) != _bits(rec), axis=1)
        assert np.array_equal(changed, mg["pruned"]), f"update {u}: a record changed where nothing was pruned"
        assert _same_bits(pose2, pose) and _same_bits(logw2, logw)
        total += counts
    assert split_seen and total[1] > 0 and total[2] > 0 and total[3] > 0
    assert (c_ref == P["cap"]).any() and (c_ref == 0).any() and (c_ref == EMPTY).any()
    ev.close()
    sh.close()


# ---- 2. the counters follow the records without a hook -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_counters_follow_clear_and_init_landmarks(pkg, dtype):
    """Records made by slam_pf_init_landmarks receive `init` at the next pass; slam_pf_clear_landmarks followed by a pass leaves
    every counter EMPTY."""
    n, nl = 300, 6
    sh = pkg.PFShard(n, nl, 5, dtype=dtype)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.clear_landmarks()
    ev = pkg.LandmarkEvidence(sh, 0.5, math.pi / 2, inc=1, dec=1, init=2, cap=4)         # r_max = 0.5: nothing is in view
    assert ev.update(None).tolist() == [0, 0, 0, 0] and np.all(ev.counters() == EMPTY)
    sh.init_landmarks(np.array([[10.0, 0.0], [0.0, 12.0], [-9.0, 3.0], [5.0, -14.0]]), 0.01, 0.1)
    assert ev.update(None).tolist() == [4 * n, 4 * n, 0, 0]
    want = np.full((nl, n), EMPTY, dtype=np.int8)
    want[:4] = 2
    assert np.array_equal(ev.counters(), want)
    a = np.full((2, n), 1, dtype=np.int32)                     # slot 1 matched twice: one increment
    assert ev.update(_dev(sh, a)).tolist() == [4 * n, 0, 0, 0]
    want[1] = 3
    assert np.array_equal(ev.counters(), want)
    before = sh.download()
    sh.clear_landmarks()
    assert ev.update(_dev(sh, a)).tolist() == [0, 0, 0, 0]     # a decision that names a free slot changes nothing
    assert np.all(ev.counters() == EMPTY)
    after = sh.download()
    assert _same_bits(before[0], after[0]) and np.all(after[2][:, 2, :] == -1)
    ev.close()
    sh.close()


# ---- 3. resampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_counters_follow_their_particles_through_resampling(pkg, dtype):
    """Three filters with the same seed and steps: `a` with evidence through FastSLAM.step_unknown_pruned, `b` through
    FastSLAM.step_unknown_fused, `c` by hand without resampling (it supplies the ancestors: PFShard.ancestors for the same
    weights, gmax, u0).  The evidence of `a` never prunes here (r_max = 0.5 m) and hand-made decisions make its counters differ
    from particle to particle.  At the forced resampling `a` and `b` stay bit-identical and a's counters are the reference gather
    of the counters after that step's pass.  A bare pass directly behind the (lazy) resampling and a further pruned step, with the
    moved records now materialised, still match the reference."""
    n, nl, seed = 1200, 8, 23
    S = E.SCN
    zs = E.scenario_observations()
    step = lambda z: (S["V"], S["G"], S["wheelbase"], E.SCN_Q, S["dt"], z, E.SCN_R, S["gate1"], S["gate2"])
    sh = {k: pkg.PFShard(n, nl, seed, dtype=dtype) for k in "abc"}
    f = {k: pkg.FastSLAM(s, None) for k, s in sh.items()}
    for s in sh.values():
        s.set_pose(S["pose"])
        s.clear_landmarks()
    ev = pkg.LandmarkEvidence(sh["a"], 0.5, math.pi / 2, inc=1, dec=1, init=1, cap=100)
    c_ref = np.full((nl, n), EMPTY, dtype=np.int8)

    def by_hand(z):
        """`c`: the step without resampling; returns its decisions (the reference's input)."""
        stats, a = sh["c"].step_unknown_fused(*step(z), want_assoc=True)
        f["c"].normalize(stats)
        return a.cpu().numpy()

    for t in range(3):
        n1, d1, counts = f["a"].step_unknown_pruned(*step(zs[t]), ev, force_resample=False)
        n2, d2 = f["b"].step_unknown_fused(*step(zs[t]), force_resample=False)
        a = by_hand(zs[t])
        assert n1 == n2 and not d1 and not d2
        pose, _, rec = sh["c"].download()
        c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec, pose, a, 0.5, math.pi / 2, 1, 1, 1, 100)
        _margins_ok(mg)
        assert counts.tolist() == counts_ref and counts_ref[3] == 0 and np.array_equal(ev.counters(), c_ref)
    for u in range(3):                                          # counters that differ from particle to particle
        a = E.hand_decisions(u, 6, n, nl)
        pose, _, rec = sh["c"].download()
        c_ref, _, counts_ref, _ = E.evidence_update(c_ref, rec, pose, a, 0.5, math.pi / 2, 1, 1, 1, 100)
        assert ev.update(_dev(sh["a"], a)).tolist() == counts_ref
    assert np.array_equal(ev.counters(), c_ref) and len(np.unique(c_ref[0])) >= 3
    _same_state(sh["a"], sh["b"], "before the resampling step")

    # the resampling step
    n1, d1, counts = f["a"].step_unknown_pruned(*step(zs[3]), ev, force_resample=True)
    n2, d2 = f["b"].step_unknown_fused(*step(zs[3]), force_resample=True)
    a = by_hand(zs[3])
    assert n1 == n2 and d1 and d2 and f["a"].resamples == f["b"].resamples == 1
    pose, _, rec = sh["c"].download()
    c_mid, _, counts_ref, mg = E.evidence_update(c_ref, rec, pose, a, 0.5, math.pi / 2, 1, 1, 1, 100)
    _margins_ok(mg)
    assert counts.tolist() == counts_ref
    u0 = pkg.philox_uniform(0, 2, seed)
    anc = sh["c"].ancestors(sh["c"].logw_tensor(), f["c"]._gmax_norm, u0).cpu().numpy().astype(np.int64)
    assert (anc != np.arange(n)).any() and anc.min() >= 0 and anc.max() < n
    _same_state(sh["a"], sh["b"], "after the resampling step")
    c_ref = c_mid[:, anc]
    assert np.array_equal(ev.counters(), c_ref), "the counters did not follow their particles"
    # the oracle's resampling of `c`'s records with the same ancestors is what `a` now holds
    pose_c, _, rec_c = sh["c"].download()
    pose_a, _, rec_a = sh["a"].download()
    assert _same_bits(pose_a, pose_c[:, anc]) and _same_bits(rec_a, rec_c[:, :, anc])

    # a bare pass directly behind the lazy resampling: it has to materialise the moved records itself
    # (the scenario's motion noise is a hundredth of the usual: a landmark's ranges lie within millimetres, so the field of view is
    #  put between landmarks here, not across one)
    d, b = E.geometry(pose_a, rec_a)
    in_use = rec_a[:, 2, :] >= 0
    ev.r_max = float(E.gap_midpoint(d[in_use], 11.5, 25.0, 1e-3))
    ev.half_fov = float(E.gap_midpoint(np.abs(b)[in_use], 0.6, 2.2, 1e-3))
    c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec_a, pose_a, None, ev.r_max, ev.half_fov, 1, 1, 1, 100)
    _margins_ok(mg)
    assert ev.update(None).tolist() == counts_ref and counts_ref[2] > 0
    assert np.array_equal(ev.counters(), c_ref) and _same_bits(sh["a"].download()[2], rec_ref)
    _same_state(sh["a"], sh["b"], "after the pass behind the resampling")          # (cap = 100, init = 1: nothing fell below 0)

    # a further pruned step against the reference on the twin's state
    ev.dec = 120                                               # whatever is in view and unmatched is pruned now
    n1, d1, counts = f["a"].step_unknown_pruned(*step(zs[4]), ev, force_resample=False)
    stats, a = sh["b"].step_unknown_fused(*step(zs[4]), want_assoc=True)
    pose, _, rec = sh["b"].download()
    c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec, pose, a.cpu().numpy(), ev.r_max, ev.half_fov, 1, 120, 1, 100)
    _margins_ok(mg)
    assert counts.tolist() == counts_ref and counts_ref[3] > 0
    assert np.array_equal(ev.counters(), c_ref) and _same_bits(sh["a"].download()[2], rec_ref)
    ev.close()
    for s in sh.values():
        s.close()


# ---- 4. the scenario ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scenario_through_the_driver(pkg, dtype):
    """The clutter scenario of tests/test_evidence_ref_cpu.py (step 11 padded to 40 observations: three observation chunks)
    through FastSLAM.step_unknown_pruned, beside a twin without evidence and a shadow that takes the same step in pieces
    (PFShard.step_unknown_fused, LandmarkEvidence.update, normalize), which is where the decisions come from.  No resampling (the
    oracle run has none).  At every step the decisions equal the oracle's, the counters and counts are the oracle's exactly, the
    driver's filter is bit-identical to the shadow; the outcome is the CPU run's: the twin is full from step 2 and never stores
    the sixth landmark, the pruned filter never holds more than seven, holds six at the end and matches the sixth landmark at
    step 13.  From the oracle alone: no NIS within 1e-3 of a gate, no two candidates within 1e-3, no pair within 0.2 of a
    field-of-view boundary."""
    S = E.SCN
    n, nl = S["n"], S["slots"]
    orc = scenario_run(True, 11, 40)
    orc_plain = scenario_run(False, 11, 40)
    for run in (orc, orc_plain):
        gate_margin, nd_gap = scenario_gate_margins(run)
        assert gate_margin > 1e-3 and nd_gap > 1e-3
    assert min(s["margin"] for s in orc) > 0.2 and orc[11]["z"].shape[1] == 40
    sh = {k: pkg.PFShard(n, nl, S["seed"], dtype=dtype) for k in ("driver", "shadow", "plain")}
    f = {k: pkg.FastSLAM(s, None) for k, s in sh.items()}
    for s in sh.values():
        s.set_pose(S["pose"])
        s.clear_landmarks()
    rule = (S["r_max"], S["half_fov"], S["inc"], S["dec"], S["init"], S["cap"])
    ev = {k: pkg.LandmarkEvidence(sh[k], *rule) for k in ("driver", "shadow")}
    got, got_plain = [], []
    for t, o in enumerate(orc):
        args = (S["V"], S["G"], S["wheelbase"], E.SCN_Q, S["dt"], o["z"], E.SCN_R, S["gate1"], S["gate2"])
        free = (sh["shadow"].download()[2][:, 2, :] < 0).sum()
        neff, did, counts = f["driver"].step_unknown_pruned(*args, ev["driver"], force_resample=False)
        stats, a = sh["shadow"].step_unknown_fused(*args, want_assoc=True)
        created = int(free - (sh["shadow"].download()[2][:, 2, :] < 0).sum())
        counts_s = ev["shadow"].update(a)
        neff_s = f["shadow"].normalize(stats)
        a = a.cpu().numpy()
        assert np.array_equal(a, o["assoc"]), f"step {t}: {int((a != o['assoc']).sum())} decisions differ from the oracle's"
        assert neff == neff_s and not did
        _same_state(sh["driver"], sh["shadow"], f"step {t}")
        c = ev["driver"].counters()
        assert np.array_equal(c, o["c"]) and np.array_equal(ev["shadow"].counters(), o["c"]), f"step {t}: counters"
        assert counts.tolist() == o["counts"] == counts_s.tolist(), f"step {t}: counts {counts.tolist()} {o['counts']}"
        lm = sh["driver"].download()[2]
        assert np.array_equal(lm[:, 2, :] >= 0, o["lm"][:, 2, :] >= 0), f"step {t}: slot usage"
        got.append(dict(held=(lm[:, 2, :] >= 0).sum(axis=0), assoc=a, created=created, lm=lm))
        # the twin without evidence
        free = (sh["plain"].download()[2][:, 2, :] < 0).sum()
        stats, ap = sh["plain"].step_unknown_fused(*args, want_assoc=True)
        f["plain"].normalize(stats)
        lm = sh["plain"].download()[2]
        ap = ap.cpu().numpy()
        assert np.array_equal(ap, orc_plain[t]["assoc"]), f"step {t}: the twin's decisions differ from the oracle's"
        got_plain.append(dict(held=(lm[:, 2, :] >= 0).sum(axis=0), assoc=ap, created=int(free - (lm[:, 2, :] < 0).sum()), lm=lm))
    check_scenario_outcome(got_plain, got)
    for e in ev.values():
        e.close()
    for s in sh.values():
        s.close()


# ---- 5. the read-out sees the prune --------------------------------------------------------------------------------------------
def test_map_sums_count_drops_by_the_pruned_particles(pkg):
    """slam_pf_map_sums counts a slot's records in use (Pxx > 0): after a pass that prunes, count_l of every slot has dropped by
    the number of particles the reference prunes there -- for the slot the field of view splits, some but not all."""
    P = E.RULE
    n, nl = 300, 6
    _, fill, _ = E.rule_plan(nl)
    sh = pkg.PFShard(n, nl, 11, dtype="f32")
    sh.set_pose(P["pose"])
    sh.clear_landmarks()
    for z in fill:
        sh.step_unknown_fused(P["V"], P["G"], P["wheelbase"], E.RULE_Q, P["dt"], z, E.SCN_R, P["gate1"], P["gate2"])
    pose, _, rec = sh.download()
    r_max, half_fov, slot = E.pick_fov(pose, rec)
    ev = pkg.LandmarkEvidence(sh, r_max, half_fov, inc=1, dec=1, init=0, cap=5)
    c_ref, _, _, _ = E.evidence_update(np.full((nl, n), EMPTY), rec, pose, None, r_max, half_fov, 1, 1, 0, 5)
    assert ev.update(None).tolist()[1] == int((rec[:, 2, :] >= 0).sum())
    before = sh.map_sums()
    c_ref, rec_ref, counts_ref, mg = E.evidence_update(c_ref, rec, pose, None, r_max, half_fov, 1, 1, 0, 5)
    _margins_ok(mg)
    counts = ev.update(None)
    after = sh.map_sums()
    pruned = mg["pruned"].sum(axis=1)
    assert counts.tolist() == counts_ref and counts_ref[3] == int(pruned.sum()) > 0
    assert 0 < pruned[slot] < int((rec[slot, 2, :] >= 0).sum())
    assert np.array_equal(before[1:, 9] - after[1:, 9], pruned.astype(np.float64))
    assert before[0, 9] == after[0, 9] == n
    ev.close()
    sh.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_unchanged(pkg):
    BAD = pkg._lib.SLAM_E_BADARG
    lib = pkg._lib.evidence_lib()
    S = E.SCN
    n, nl, seed = 500, 6, 3
    # a shard of a larger filter
    part = pkg.PFShard(256, nl, seed, dtype="f32", first=0, n_global=512)
    with pytest.raises(pkg.SlamHipError) as ei:
        pkg.LandmarkEvidence(part, 30.0, 1.0)
    assert ei.value.code == BAD
    part.close()

    a = pkg.PFShard(n, nl, seed, dtype="f32")
    twin = pkg.PFShard(n, nl, seed, dtype="f32")
    zs = E.scenario_observations()
    for s in (a, twin):
        s.set_pose(S["pose"])
        s.clear_landmarks()
    ev = pkg.LandmarkEvidence(a, 30.0, math.pi / 2)
    args = lambda z: (S["V"], S["G"], S["wheelbase"], E.SCN_Q, S["dt"], z, E.SCN_R, S["gate1"], S["gate2"])
    for t in range(2):
        ev.step(*args(zs[t]))
        twin.step_unknown_fused(*args(zs[t]))
    import torch
    dec = torch.zeros((65, n), dtype=torch.int32, device=a.device)
    torch.cuda.synchronize(a.device)
    ptr = C.c_void_p(dec.data_ptr())
    before, c_before = a.download(), ev.counters()
    fov = math.pi / 2
    upd = lambda p, m, r_max, half_fov, inc, dc, init, cap: lib.slam_pf_evidence_update(ev._e, p, m, r_max, half_fov, inc, dc, init,
                                                                                        cap, None)
    assert upd(ptr, 65, 30.0, fov, 1, 1, 1, 5) == BAD                     # m = 65
    assert upd(ptr, -1, 30.0, fov, 1, 1, 1, 5) == BAD
    assert upd(ptr, 3, 30.0, fov, 1, 1, 1, 128) == BAD                    # cap = 128
    assert upd(ptr, 3, 30.0, fov, 1, 1, 6, 5) == BAD                      # init > cap
    assert upd(ptr, 3, 30.0, fov, 1, 1, -1, 5) == BAD
    assert upd(ptr, 3, 30.0, fov, 1, 0, 1, 5) == BAD                      # dec = 0
    assert upd(ptr, 3, 30.0, fov, 0, 1, 1, 5) == BAD                      # inc = 0
    assert upd(None, 3, 30.0, fov, 1, 1, 1, 5) == BAD                     # NULL decisions with m > 0
    assert "null decisions" in pkg._lib.last_error()
    assert upd(ptr, 3, 30.0, 0.0, 1, 1, 1, 5) == BAD                      # half_fov = 0
    assert upd(ptr, 3, 30.0, 3.2, 1, 1, 1, 5) == BAD                      # half_fov > pi
    assert upd(ptr, 3, 0.0, fov, 1, 1, 1, 5) == BAD                       # r_max = 0
    assert upd(ptr, 3, math.inf, fov, 1, 1, 1, 5) == BAD
    assert upd(ptr, 3, math.nan, fov, 1, 1, 1, 5) == BAD
    # the combined call checks the evidence arguments before it takes the step, and the step's own arguments as well
    ev.cap = 128
    with pytest.raises(pkg.SlamHipError) as ei:
        ev.step(*args(zs[2]))
    assert ei.value.code == BAD
    ev.cap = 5
    with pytest.raises(pkg.SlamHipError) as ei:
        ev.step(S["V"], S["G"], S["wheelbase"], E.SCN_Q, S["dt"], np.ones((2, 65)), E.SCN_R, S["gate1"], S["gate2"])
    assert ei.value.code == BAD
    with pytest.raises(pkg.SlamHipError) as ei:                           # u0 outside [0, 1): slam_pf_resample_local's refusal
        ev.resample(0.0, 1.0)
    assert ei.value.code == BAD
    for x, y in zip(before, a.download()):
        assert _same_bits(x, y)
    assert np.array_equal(ev.counters(), c_before)
    _same_state(a, twin, "after the refusals")                            # (no pass has pruned anything yet: still the twin)
    a.predict(3.0, 0.02, 4.0, E.SCN_Q, 0.1)                               # the RNG step counter did not move
    twin.predict(3.0, 0.02, 4.0, E.SCN_Q, 0.1)
    assert _same_bits(a.download()[0], twin.download()[0])
    # m = 0 with NULL decisions is a valid pass
    assert upd(None, 0, 30.0, fov, 1, 1, 1, 5) == 0
    ev.close()
    a.close()
    twin.close()
