"""CPU tests of tests/pf_assoc_records.py: the designed table is what it claims (bands, the conditions on decided and edge pairs,
coverage of chunks, residues and boundaries), the margins follow their rule, the float64 model is the oracle, the comparison
rejects every planted defect on a decided pair -- and the quiet scene of tests/test_gpu_pf_unknown_step.py with its 0.999 quota
accepts most of them (QUIET_SCENE_ACCEPTS below: the gap this closes).  No GPU."""
import math

import numpy as np
import pytest

import pf_assoc_records as A
from oracle import pf_ref as F

DTYPES = ("f64", "f32")
LD = np.longdouble


def test_the_suites_numbers_and_the_observations():
    import lm_records as L
    import test_gpu_pf_unknown_step as U
    assert (A.GATE1, A.GATE2) == (U.GATE1, U.GATE2) and np.array_equal(L.R_DIAG, U.R)
    assert A.N % 64 and A.N % 256 and all(A.NL % g for g in (2, 3, 4))
    for dtype in DTYPES:
        t = A.table(dtype)
        assert t.kind[-1] == A.FULL
        r, b = t.z
        assert r.min() >= 10.0 and r.max() <= 50.0 and np.all(np.abs(b) <= math.pi * (1 + 1e-7))
        first = np.array([i for i in range(A.M) if i not in A.DUP_OF])
        xy = np.stack([r[first] * np.cos(b[first]), r[first] * np.sin(b[first])])
        dist = np.hypot(xy[0][:, None] - xy[0][None], xy[1][:, None] - xy[1][None]) + 1e9 * np.eye(len(first))
        assert dist.min() >= 8.0, dist.min()
        for d, s in A.DUP_OF.items():
            assert np.array_equal(t.z[:, d], t.z[:, s])
        assert all(any(d // 16 == ch for d in A.DUP_OF) for ch in range(4))


@pytest.mark.parametrize("which", list(A.NOISES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_is_what_it_claims(dtype, which):
    c = A.case(dtype, which)
    t = c.t
    assert c.foreign_min > A.FOREIGN_MIN, c.foreign_min                  # situations of different observations do not interfere
    assert A.truth_in_sets(c).all()
    # -- the bands, in units of the pair's own bound (edge: of its fp32 bound)
    c32 = A.case(dtype, which, "f32")
    gate = np.where(np.isin(c.sit, (A.G1IN, A.G1OUT)), A.GATE1, A.GATE2)
    for cc, names in ((c, ("near", "far")), (c32, ("edge",))):
        dist = np.asarray(cc.nis_a - gate, dtype=np.float64)
        assert np.all(dist[np.isin(c.sit, (A.G1IN, A.G2IN))] < 0) and np.all(dist[np.isin(c.sit, (A.G1OUT, A.G2OUT))] > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            k_gate = np.abs(dist) / cc.b_nis_a
            gap = np.asarray(cc.nd_b - cc.nd_a, dtype=np.float64)
            k_rival = gap / (cc.b_nd_a + cc.b_nd_b)
        for name in names:
            lo, hi = A.BAND_RANGE[name]
            bsel = c.band == A.BANDS.index(name)
            for sit in (A.G1IN, A.G1OUT, A.G2IN, A.G2OUT):
                k = k_gate[bsel & (c.sit == sit)]
                assert len(k) > 1000 and lo < k.min() and k.max() < hi, (name, A.SITS[sit], k.min(), k.max())
            k = k_rival[bsel & (c.sit == A.RIVAL)]
            assert len(k) > 1000 and lo < k.min() and k.max() < hi, (name, "rival", k.min(), k.max())
    # the winner of a rival pair has the larger NIS and the smaller log det; both are well inside gate1
    rv = c.sit == A.RIVAL
    assert np.all(c.nis_a[rv] > c.nis_b[rv]) and np.all((c.nd_a - c.nis_a)[rv] < (c.nd_b - c.nis_b)[rv]) and np.all(c.nis_a[rv] < 1.0)
    assert np.all(c.dec[rv] == t.slot_a[A.OBS_LOC][rv])
    assert (t.slot_a[A.OBS_LOC][rv] < t.slot_b[A.OBS_LOC][rv]).sum() > 1000 and (t.slot_a[A.OBS_LOC][rv] > t.slot_b[A.OBS_LOC][rv]).sum() > 1000
    # -- conditions, not measurements: decided classes decided, the edge class open for fp32 and decided for fp64
    decided_cls = ~(c.has_band & (c.band == A.BANDS.index("edge")))
    assert c.decided[decided_cls].all(), int((~c.decided[decided_cls]).sum())
    edge = c.has_band & (c.band == A.BANDS.index("edge"))
    assert np.mean(~c32.decided[edge]) >= 0.9
    if dtype == "f64":
        assert c.decided.all()
    assert np.all(c.count >= 1)
    # -- the truth's decisions are the situations'
    slot_a = t.slot_a[A.OBS_LOC]
    want = {A.NEW: -1, A.G1OUT: -2, A.G2IN: -2, A.G2OUT: -1, A.STALE: -1, A.EXACT: -2}
    for sit, d in want.items():
        assert np.all(c.dec[c.sit == sit] == d), A.SITS[sit]
    for sit in (A.G1IN, A.RIVAL, A.TWIN):
        assert np.all(c.dec[c.sit == sit] == slot_a[c.sit == sit]), A.SITS[sit]
    tw = c.sit == A.TWIN
    sa, sb = slot_a[tw], t.slot_b[A.OBS_LOC][tw]
    P = np.broadcast_to(np.arange(t.n)[None, :], c.sit.shape)[tw]
    assert np.all(sa < sb) and np.array_equal(t.lm[sa, :, P], t.lm[sb, :, P]) and np.all(c.nis_a[tw] < 3.5)
    # stale: unused, exactly on the observation, a stale positive Pyy
    st = t.sit == A.STALE
    K, Pk = np.nonzero(st)
    s = t.slot_a[st]
    i = np.array([int(np.nonzero(A.OBS_LOC == k)[0][0]) for k in range(A.NLOC)])[K]
    T = A.NP_DTYPE[dtype]
    ex = t.pose[0][Pk] + t.z[0, i] * np.cos(t.pose[2][Pk] + t.z[1, i])
    assert len(s) > 5000 and np.all(t.lm[s, 2, Pk] == -1.0) and np.all(t.lm[s, 4, Pk] > 0)
    assert np.array_equal(t.lm[s, 0, Pk], ex.astype(T).astype(np.float64))
    # -- coverage: every situation and attribute in every chunk and at every chunk boundary
    used = t.lm[:, 2, :] >= 0
    free = (~used).sum(axis=0)
    wants_slot = (c.dec == -1).sum(axis=0)
    full = (t.kind == A.FULL)
    assert np.all(free[full] <= 3) and np.all(wants_slot[full] > free[full]) and np.all(wants_slot[t.kind == A.NORMAL] <= free[t.kind == A.NORMAL])
    assert np.all((c.dec[:5] == -1).sum(axis=0)[full & (free == 0)] >= 1) and (full & (free == 0)).sum() > 50      # full already at m = 5
    assert (t.kind == A.EMPTY).sum() >= 10 and not used[:, t.kind == A.EMPTY].any()
    assert used[:, np.isin(t.kind, (A.NORMAL, A.FULL))].any(axis=0).all()
    attrs = {A.SITS[s_]: c.sit == s_ for s_ in range(len(A.SITS))}
    attrs["dup"] = c.dup
    attrs["wrapped"] = c.wrapped & (c.dec >= 0)
    attrs["full"] = np.broadcast_to(full[None, :], c.sit.shape) & (c.dec == -1)
    for name, mask in attrs.items():
        if name == "exact":                                               # (64 particles, one pair each and its repeats: checked with the defects)
            continue
        for ch in range(4):
            assert mask[16 * ch:16 * ch + 16].sum() > 100, (name, ch)
        for i_ in A.BOUNDARY_OBS:
            if name == "dup" and i_ not in A.DUP_OF:
                continue
            if name == "wrapped" and abs(t.z[1, i_]) < 1.0:           # (|phi + b| > pi takes a heading beyond pi - |b|)
                continue
            assert mask[i_].sum() >= 10, (name, i_)
        for bi in range(3):
            if name in ("gate1_in", "gate1_out", "gate2_in", "gate2_out", "rival"):
                for ch in range(4):
                    assert (mask & (c.band == bi))[16 * ch:16 * ch + 16].sum() > 100, (name, A.BANDS[bi], ch)
    assert np.mean(c.wrapped[c.dec >= 0]) > 0.15 and (c.raw_a > math.pi).sum() > 1000 and (c.raw_a < -math.pi).sum() > 1000
    # -- coverage: the slots of every situation in every residue modulo 2, 3 and 4, in the last ragged round, interleaved with holes
    for sit in (A.G1IN, A.G1OUT, A.G2IN, A.G2OUT, A.RIVAL, A.TWIN, A.STALE):
        two = sit in (A.RIVAL, A.TWIN)
        for slots in (np.concatenate([t.slot_a[t.sit == sit], t.slot_b[t.sit == sit]]) if two else t.slot_a[t.sit == sit],):
            for g in (2, 3, 4):
                assert all((slots % g == r_).sum() > 100 for r_ in range(g)), (A.SITS[sit], g)
                assert (slots >= A.NL - A.NL % g).sum() > 20, (A.SITS[sit], g, "last round")
            assert (slots == A.NL - 1).sum() >= 10 and (slots == 0).sum() >= 10
    sa, sb = t.slot_a[t.sit == A.TWIN], t.slot_b[t.sit == A.TWIN]
    for g in (2, 3, 4):
        assert (sa // g == sb // g).sum() >= 20 and (sa // g != sb // g).sum() > 1000, ("twins within / across rounds of", g)
    assert ((sa < 16) & (sb >= 16)).sum() > 100
    holes_between = (~used[:-1] & used[1:]).sum(axis=0)
    assert np.median(holes_between[t.kind == A.NORMAL]) >= 5                          # used and unused slots interleave
    perm_differs = np.mean(t.slot_a[:, 1:] != t.slot_a[:, :-1])
    assert perm_differs > 0.9                                                           # the layout differs from particle to particle


@pytest.mark.parametrize("dtype", DTYPES)
def test_margins_follow_their_rule(dtype):
    rule = A.derive_margins(dtype)
    for cl in A.CLASSES:
        for q in A.QUANT:
            have, want = A.MARGINS[dtype][cl][q], rule[cl][q]
            assert want <= have <= 1.5 * want, f"{dtype} {cl} {q}: committed {have}, the rule gives {want:.3f}"
    rule = A.derive_replay_margins(dtype)
    for q, want in rule.items():
        have = A.REPLAY_MARGINS[dtype][q]
        assert want <= have <= 1.5 * want, f"{dtype} replay {q}: committed {have}, the rule gives {want:.3f}"


@pytest.mark.parametrize("which", list(A.NOISES))
def test_float64_model_is_the_oracle(which):
    """decide(np.float64) against OraclePF.associate_unknown on the f64 table: identical decisions on every decided pair (here: on
    every pair but the edge class in fp32 units -- all of them are decided for fp64), nis to 1e-12 relative."""
    c = A.case("f64", which)
    t = c.t
    orc = F.OraclePF(t.n, A.NL, 1)
    orc.pose, orc.lm = t.pose.copy(), t.lm.copy()
    want = orc.associate_unknown(t.z, t.R, t.gate1, t.gate2)
    got, nis = A.decide(np.float64, t.pose, t.lm, t.z, t.R, t.gate1, t.gate2, want_nis=True)
    assert c.decided.all() and np.array_equal(got, want) and np.array_equal(got, c.dec)
    if which == "diag":
        import test_gpu_pf_unknown_step as U
        ref, _nd, used = U._scores(orc, t.z)
        u = np.broadcast_to(used[None], ref.shape)
        assert np.max(np.abs(nis[u] - ref[u]) / np.abs(ref[u])) <= 1e-12
    for i in (0, 17, 63):                                                 # and the longdouble truth, whole, against the model
        _q, s, used = A.truth(t, [i])
        assert np.max(np.abs(np.asarray(s.nis[0], dtype=np.float64)[used] - nis[i][used]) / nis[i][used]) <= 1e-9


def _verdict(c, T, defect):
    """(pairs outside their admissible set, decided pairs that differ from the truth, state findings) of the model with `defect`;
    the state is replayed only where the decisions say nothing (no defect, or one that leaves them alone)."""
    if defect in A.DECISION_DEFECTS:
        dec = A.decide(T, c.t.pose, c.t.lm, c.t.z, c.t.R, c.t.gate1, c.t.gate2, defect)
        return A.check_decisions(c, dec, A.M) + (None,)
    dec, rp_model = A.model_call(T, c.t, A.M, defect)
    outside, wrong = A.check_decisions(c, dec, A.M)
    if defect == "sequential_map":
        return outside, wrong, None
    rp = A.replay(c.t, dec, A.M)                                          # the truth's state under the SAME decisions
    st = A.check_state(c.t, rp, np.asarray(rp_model.lm, dtype=np.float64), np.asarray(rp_model.inc, dtype=np.float64))
    return outside, wrong, st


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_model_passes_and_every_planted_defect_is_rejected(dtype):
    c = A.case(dtype, "diag")                                             # (the exact pairs need the diagonal R)
    T = A.NP_DTYPE[dtype]
    ex = c.sit == A.EXACT
    assert all(ex[16 * ch:16 * ch + 16].any() for ch in range(4)) and all(((c.nis_a == g) & ex).sum() >= 10 for g in (A.GATE1, A.GATE2))
    assert c.decided[ex].all() and np.all(c.dec[ex] == -2) and np.all(c.b_nis_a[ex] == 0)
    outside, wrong, st = _verdict(c, T, None)
    assert not outside.any() and not wrong.any()
    # (0.25 by the margins' rule on the records the truth's decisions touch; the model's own decisions on edge pairs touch others)
    assert st["used_wrong"] == st["untouched_changed"] == st["out_of_bound"] == 0 and st["worst_lm"] <= 0.5 and st["worst_inc"] <= 0.5, st
    for defect in A.DEFECTS:
        outside, wrong, st = _verdict(c, T, defect)
        by_state = st["used_wrong"] + st["untouched_changed"] if st else 0
        print(f"planted {dtype} {defect}: {int(wrong.sum())} decided pairs wrong, {int(outside.sum())} outside their set, "
              f"{by_state} slots wrong after the call")
        if defect == "new_to_slot0_when_full":                           # decisions untouched: the state check has to see it
            assert not wrong.any() and st["untouched_changed"] > 0
        else:
            assert wrong.any(), defect
            assert np.all(outside[wrong])


# planted defects that the quiet scene of tests/test_gpu_pf_unknown_step.py::test_more_than_16_observations_against_the_oracle
# accepts: the float64 rule with the defect agrees with the oracle on at least 0.999 of its decisions there (the fp32 quota; most
# agree on all of them).  Re-derived and compared by the test below; all of them are rejected above.
QUIET_SCENE_ACCEPTS = ["le_in_minimum", "strict_gate2", "nearest_by_nis", "no_wrap", "unused_ignored", "ragged_round_dropped",
                       "sequential_map"]


def test_the_quiet_scene_accepts_defects_it_cannot_see():
    import test_gpu_pf_unknown_step as U
    orc = F.OraclePF(U.N2, U.SLOTS2, U.SEED2)
    orc.set_pose(U.POSE2)
    orc.clear_landmarks()
    steps = []                                                            # (pose, map before the step, observations, the oracle's decisions)
    for z in U._plan2():
        orc.predict(3.0, 0.02, 4.0, U.Q, U.DT2)
        before = (orc.pose.copy(), orc.lm.copy(), orc.logw.copy())
        steps.append(before + (z, orc.update_unknown(z, U.R, U.GATE1, U.GATE2)))
    total = sum(s[4].size for s in steps)
    accepted = []
    for defect in A.DEFECTS:
        if defect == "new_to_slot0_when_full":                           # (decisions unchanged; the old state comparison sees slot 0)
            continue
        agree = 0
        for pose, lm, logw, z, want in steps:
            if defect == "sequential_map":
                twin = F.OraclePF(U.N2, U.SLOTS2, U.SEED2)
                twin.pose, twin.lm, twin.logw = pose.copy(), lm.copy(), logw.copy()
                got = np.concatenate([twin.update_unknown(z[:, i:i + 1], U.R, U.GATE1, U.GATE2) for i in range(z.shape[1])])
            else:
                got = A.decide(np.float64, pose, lm, z, U.R, U.GATE1, U.GATE2, defect)
            agree += int(np.sum(got == want))
        print(f"quiet scene, {defect}: agreement {agree / total:.6f}")
        if agree >= 0.999 * total:
            accepted.append(defect)
    assert accepted == QUIET_SCENE_ACCEPTS
