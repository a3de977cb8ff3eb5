"""CPU tests of tests/evidence_ref.py, the NumPy restatement of the landmark-evidence rule (include/slamhip_evidence.h): each of
the five cases by hand, their order of precedence, saturation, the two sides of zero, a slot matched twice, a new landmark
that found no slot -- and the clutter scenario on the fp64 oracle: without pruning one false detection per step fills the
eight slots for good and a landmark seen later is never stored; with the rule no particle ever holds more than seven."""
import functools
import math
import os

import numpy as np
import pytest

import evidence_ref as E
from oracle import pf_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = E.EMPTY
POSE1 = np.array([[0.0], [0.0], [0.0]])


def _one(c, rec, assoc=None, pose=POSE1, r_max=30.0, half_fov=math.pi / 2, **kw):
    """One particle, one slot: (counter, record [5], counts)."""
    lm = np.asarray(rec, dtype=np.float64).reshape(1, 5, 1)
    a = None if assoc is None else np.asarray(assoc, dtype=np.int64).reshape(-1, 1)
    cn, ln, counts, _ = E.evidence_update(np.array([[c]]), lm, pose, a, r_max, half_fov, **kw)
    return int(cn[0, 0]), ln[0, :, 0], counts


AHEAD = [10.0, 1.0, 0.5, 0.1, 0.4]            # 10 m ahead: in view
BEHIND = [-10.0, 1.0, 0.5, 0.1, 0.4]          # behind the vehicle: out of the +-90 degree field of view
FAR = [40.0, 1.0, 0.5, 0.1, 0.4]              # beyond r_max
FREE = [0.0, 0.0, -1.0, 0.0, 0.0]


def test_case1_a_free_slot_is_empty_whatever_the_counter_was():
    c, rec, counts = _one(3, FREE)
    assert c == EMPTY and np.array_equal(rec, FREE) and counts == [0, 0, 0, 0]
    # ... also when a decision names it: case 1 comes first
    c, rec, counts = _one(3, FREE, assoc=[0])
    assert c == EMPTY and counts == [0, 0, 0, 0]


def test_case2_a_new_record_gets_init_before_anything_else():
    for rec in (AHEAD, BEHIND, FAR):
        c, out, counts = _one(EMPTY, rec, init=2)
        assert c == 2 and np.array_equal(out, rec) and counts == [1, 1, 0, 0]
    # matched in the same call: still init, not init + inc (case 2 before case 3)
    c, _, counts = _one(EMPTY, AHEAD, assoc=[0], init=2, inc=3, cap=9)
    assert c == 2 and counts == [1, 1, 0, 0]
    # unmatched and in view: not decremented either (case 2 before case 4), even with init = 0
    c, out, counts = _one(EMPTY, AHEAD, init=0)
    assert c == 0 and np.array_equal(out, AHEAD) and counts == [1, 1, 0, 0]
    # Pxx == 0 is in use (the test is !(Pxx < 0))
    c, _, counts = _one(EMPTY, [10.0, 1.0, 0.0, 0.0, 0.0])
    assert c == 1 and counts == [1, 1, 0, 0]


def test_case3_a_match_raises_once_and_saturates():
    assert _one(1, AHEAD, assoc=[0])[0] == 2
    assert _one(1, AHEAD, assoc=[0], inc=3)[0] == 4
    assert _one(4, AHEAD, assoc=[0], inc=3)[0] == 5                  # saturates at cap
    assert _one(5, AHEAD, assoc=[0])[0] == 5
    assert _one(1, AHEAD, assoc=[0, 0, -1, 0])[0] == 2               # matched three times in one call: one increment
    assert _one(2, BEHIND, assoc=[-2, 0])[0] == 3                    # a match counts wherever the landmark lies
    assert _one(126, AHEAD, assoc=[0], inc=100, cap=127)[0] == 127
    # matched and in view: raised, not lowered (case 3 before case 4)
    c, _, counts = _one(0, AHEAD, assoc=[0])
    assert c == 1 and counts == [1, 0, 0, 0]


def test_case4_in_view_and_unmatched_lowers_and_prunes_below_zero():
    c, rec, counts = _one(3, AHEAD)
    assert c == 2 and np.array_equal(rec, AHEAD) and counts == [1, 0, 1, 0]
    c, rec, counts = _one(1, AHEAD)                                  # lands on exactly 0: kept
    assert c == 0 and np.array_equal(rec, AHEAD) and counts == [1, 0, 1, 0]
    c, rec, counts = _one(0, AHEAD)                                  # lands on -1: pruned
    assert c == EMPTY and np.array_equal(rec, FREE) and counts == [0, 0, 1, 1]
    c, rec, counts = _one(2, AHEAD, dec=2)
    assert c == 0 and counts == [1, 0, 1, 0]
    c, rec, counts = _one(2, AHEAD, dec=3)
    assert c == EMPTY and np.array_equal(rec, FREE) and counts == [0, 0, 1, 1]
    # decisions that name other slots, or nothing, do not protect it
    c, _, _ = _one(0, AHEAD, assoc=[-1, -2, 1, 7])
    assert c == EMPTY


def test_case5_out_of_view_and_unmatched_is_left_alone():
    for rec in (BEHIND, FAR):
        c, out, counts = _one(0, rec)
        assert c == 0 and np.array_equal(out, rec) and counts == [1, 0, 0, 0]
    # the boundaries belong to the field of view: d == r_max and |b| == half_fov are in view
    c, _, counts = _one(2, [30.0, 0.0, 0.5, 0.0, 0.5])
    assert c == 1 and counts[2] == 1
    c, _, counts = _one(2, [0.0, 10.0, 0.5, 0.0, 0.5])              # bearing pi / 2 exactly (atan2(10, 0))
    assert c == 1 and counts[2] == 1
    c, _, counts = _one(2, [-1e-3, 10.0, 0.5, 0.0, 0.5])
    assert c == 2 and counts[2] == 0
    # the bearing is relative to the heading, wrapped once
    pose = np.array([[0.0], [0.0], [3.0]])
    assert _one(2, BEHIND, pose=pose)[0] == 1                        # now ahead
    assert _one(2, [-10.0, -1.0, 0.5, 0.1, 0.4], pose=pose)[0] == 1  # atan2 = -3.04, minus 3.0 = -6.04, wrapped to 0.24
    assert _one(2, AHEAD, pose=pose)[0] == 2                         # now behind


def test_several_particles_and_slots_and_a_new_landmark_without_a_slot():
    """Two slots, three particles.  Every slot is in use, the decisions say -1 (new landmark) for all particles: nothing
    was created (no slot left), so no counter may become `init`; the -1 matches nothing and both slots, in view, decay."""
    lm = np.zeros((2, 5, 3))
    lm[0, :, :] = np.array(AHEAD)[:, None]
    lm[1, :, :] = np.array([12.0, -2.0, 0.3, 0.0, 0.3])[:, None]
    c = np.array([[2, 0, 5], [1, 1, 0]])
    cn, ln, counts, mg = E.evidence_update(c, lm, np.zeros((3, 3)), np.full((1, 3), -1), 30.0, math.pi / 2)
    assert np.array_equal(cn, [[1, EMPTY, 4], [0, 0, EMPTY]])
    assert counts == [4, 0, 6, 2]
    assert np.array_equal(ln[0, :, 1], FREE) and np.array_equal(ln[1, :, 2], FREE)
    assert np.array_equal(ln[0, :, 0], AHEAD) and np.array_equal(mg["pruned"], [[False, True, False], [False, False, True]])
    # per-particle decisions: particle 0 matches slot 1, particle 1 slot 0, particle 2 nothing; a slot index past the map is ignored
    a = np.array([[1, 0, -2], [64, 130, -1]])
    cn, _, counts, _ = E.evidence_update(c, lm, np.zeros((3, 3)), a, 30.0, math.pi / 2)
    assert np.array_equal(cn, [[1, 1, 4], [2, 0, EMPTY]]) and counts == [5, 0, 4, 1]


def test_margins_report_every_pair_in_use():
    lm = np.zeros((2, 5, 2))
    lm[:, 2, :] = -1.0
    lm[0, :, 0] = [3.0, 4.0, 0.5, 0.0, 0.5]           # d = 5, b = atan2(4, 3)
    _, _, _, mg = E.evidence_update(np.full((2, 2), EMPTY), lm, np.zeros((3, 2)), None, 10.0, 1.0)
    assert mg["range"][0, 0] == pytest.approx(0.5) and mg["bearing"][0, 0] == pytest.approx(abs(math.atan2(4, 3) - 1.0))
    assert np.isinf(mg["range"][1]).all() and np.isinf(mg["range"][0, 1]) and np.isinf(mg["bearing"][1]).all()
    assert E.gap_midpoint([1.0, 2.0, 5.0, 5.5], 0.0, 6.0, 1.0) == 3.5 and E.gap_midpoint([9.0], 1.0, 2.0, 0.5) == 1.5


# ---- the scenario ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenario_run(prune, pad_step=None, pad_to=0):
    """The scenario on the fp64 oracle: per step the observations, the decisions, the state after the step (and after the
    pruning pass, if any), the counters and counts, the smallest field-of-view margins.  Shared with the GPU test."""
    S = E.SCN
    o = F.OraclePF(S["n"], S["slots"], S["seed"])
    o.set_pose(S["pose"])
    o.clear_landmarks()
    c = np.full((S["slots"], S["n"]), EMPTY, dtype=np.int8)
    out = []
    for z in E.scenario_observations(pad_step, pad_to):
        o.predict(S["V"], S["G"], S["wheelbase"], E.SCN_Q, S["dt"])
        pose_pred, lm_before = o.pose.copy(), o.lm.copy()
        assoc = o.update_unknown(z, E.SCN_R, S["gate1"], S["gate2"])
        created = int(((o.lm[:, 2, :] >= 0) & (lm_before[:, 2, :] < 0)).sum())
        rec = dict(z=z, assoc=assoc.copy(), created=created, pose_pred=pose_pred, lm_before=lm_before)
        if prune:
            c, lm, counts, mg = E.evidence_update(c, o.lm, o.pose, assoc, S["r_max"], S["half_fov"], S["inc"], S["dec"],
                                                  S["init"], S["cap"])
            o.lm = lm
            rec.update(c=c.copy(), counts=counts, margin=min(float(mg["range"].min()), float(mg["bearing"].min())))
        rec.update(lm=o.lm.copy(), pose=o.pose.copy(), held=(o.lm[:, 2, :] >= 0).sum(axis=0))
        out.append(rec)
    return out


def scenario_gate_margins(run):
    """(smallest relative distance of any (observation, slot in use) NIS from a gate, smallest gap between the best and the
    second-best candidate of a matched observation) over all steps of a scenario run, from the oracle's own numbers: the
    margins tests/test_gpu_pf_unknown_step.py asserts before it compares fp32 decisions with the oracle's."""
    from types import SimpleNamespace

    from test_gpu_pf_unknown_step import _scores
    S = E.SCN
    gate_margin = nd_gap = np.inf
    for s in run:
        nis, nd, used = _scores(SimpleNamespace(pose=s["pose_pred"], lm=s["lm_before"]), s["z"])
        u = np.broadcast_to(used[None], nis.shape)
        if u.any():
            gate_margin = min(gate_margin, min(float(np.min(np.abs(nis[u] - g) / g)) for g in (S["gate1"], S["gate2"])))
        two = np.sort(np.where(u & (nis < S["gate1"]), nd, np.inf), axis=1)[:, :2, :]
        matched = np.isfinite(two[:, 0, :])
        if matched.any():
            nd_gap = min(nd_gap, float(np.min(two[:, 1, :][matched] - two[:, 0, :][matched])))
    return gate_margin, nd_gap


def check_scenario_outcome(plain, pruned):
    """The outcome the rule exists for, from the per-step `held` [n] and `assoc` [m, n] of the two runs."""
    S = E.SCN
    n, slots = S["n"], S["slots"]
    # without pruning: full from step 2 on, the sixth landmark (the last observation of steps 12 and 13) is never stored
    for t, s in enumerate(plain):
        assert np.all(s["held"] == (slots if t >= 2 else 6 + t)), f"step {t}"
    for t in (12, 13):
        assert np.all(plain[t]["assoc"][-1] == -1) and plain[t]["created"] == 0
    # with pruning: never more than seven, six at the end, the sixth landmark created at step 12 and matched at step 13
    assert max(int(s["held"].max()) for s in pruned) <= slots - 1
    assert np.all(pruned[-1]["held"] == 6)
    assert np.all(pruned[12]["assoc"][-1] == -1) and pruned[12]["created"] == n
    a13 = pruned[13]["assoc"][-1]
    assert np.all(a13 >= 0)
    assert np.all(pruned[13]["lm"][a13, 2, np.arange(n)] >= 0)


def test_scenario_clutter_fills_the_map_and_pruning_keeps_it_open():
    plain, pruned = scenario_run(False), scenario_run(True)
    check_scenario_outcome(plain, pruned)
    # no record in use anywhere near a field-of-view boundary (relative range, or radians): the smallest margin of this
    # reconstruction of the scenario (G = 0, wheelbase 4, R of the other particle-filter tests, its own noise draws) is 0.2495
    assert min(s["margin"] for s in pruned) > 0.2
    assert sum(s["counts"][3] for s in pruned) == 10 * E.SCN["n"]       # every false landmark was discarded, nothing else
    assert all(s["counts"][0] == int(s["held"].sum()) for s in pruned)
    # the padded form the GPU test uses (step 11 carries 40 observations): the same outcome
    padded = scenario_run(True, 11, 40)
    assert padded[11]["z"].shape[1] == 40
    check_scenario_outcome(plain, padded)
    for a, b in zip(pruned, padded):
        assert np.array_equal(a["c"], b["c"]) and np.array_equal(a["held"], b["held"])
    # ... and no decision of it sits at a gate or between two candidates (what the fp32 GPU run relies on)
    for run in (padded, scenario_run(False, 11, 40)):
        gate_margin, nd_gap = scenario_gate_margins(run)
        assert gate_margin > 1e-3 and nd_gap > 1e-3, (gate_margin, nd_gap)


# ---- the scene of the GPU rule test, checked here on the oracle's state before it goes to the GPU -------------------------------
@pytest.mark.parametrize("nl", [6, 130])
@pytest.mark.parametrize("n", [70, 1513])
def test_rule_scene_has_a_field_of_view_that_splits_a_slot_and_touches_no_pair(n, nl):
    """tests/test_gpu_pf_evidence.py builds its state with three fused steps, then runs updates with hand-made decisions and a
    field of view picked from the state itself (evidence_ref.pick_fov).  The same plan on the fp64 oracle: at every update a
    field of view exists that leaves every pair in use more than 2e-5 (relative range / radians) from its boundaries and
    splits one slot's particles; the decisions reach every case of the rule, prunes included."""
    P = E.RULE
    lm, fill, between = E.rule_plan(nl)
    o = F.OraclePF(n, nl, 11)
    o.set_pose(P["pose"])
    o.clear_landmarks()
    for z in fill:
        o.predict(P["V"], P["G"], P["wheelbase"], E.RULE_Q, P["dt"])
        o.update_unknown(z, E.SCN_R, P["gate1"], P["gate2"])
    held = (o.lm[:, 2, :] >= 0).sum(axis=0)          # (under this motion noise a few particles gate differently: not one number)
    assert held.min() >= nl - 8 and (held < nl).any()
    c = np.full((nl, n), EMPTY, dtype=np.int8)
    total = np.zeros(4, dtype=np.int64)
    split_seen = False
    for u, m in enumerate((3, 5, 40, 0)):
        if u == 2:
            o.predict(P["V"], P["G"], P["wheelbase"], E.RULE_Q, P["dt"])
            o.update_unknown(between, E.SCN_R, P["gate1"], P["gate2"])
        r_max, half_fov, slot = E.pick_fov(o.pose, o.lm)
        a = E.hand_decisions(u, m, n, nl) if m else None
        c, lm_new, counts, mg = E.evidence_update(c, o.lm, o.pose, a, r_max, half_fov, P["inc"], P["dec"], P["init"], P["cap"])
        assert mg["range"].min() > 2e-5 and mg["bearing"].min() > 2e-5
        used = o.lm[slot, 2, :] >= 0
        split_seen |= bool(mg["in_view"][slot][used].any() and (~mg["in_view"][slot][used]).any())
        o.lm = lm_new
        total += counts
    assert split_seen and total[1] > 0 and total[2] > 0 and total[3] > 0
    assert (c == P["cap"]).any() and (c == 0).any() and (c == EMPTY).any()


# ---- the declarations the host layers bind -----------------------------------------------------------------------------------
NAMES = {"slam_pf_evidence_create", "slam_pf_evidence_destroy", "slam_pf_evidence_update", "slam_pf_step_unknown_evidence",
         "slam_pf_evidence_resample", "slam_pf_evidence_get"}


def test_header_python_and_julia_name_the_same_symbols(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    assert set(pkg._lib.EVIDENCE_SIGNATURES) == NAMES
    with open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")) as f:
        src = f.read()
    assert "LandmarkEvidence" in src and "step_unknown_pruned!" in src
    assert callable(pkg.LandmarkEvidence) and callable(pkg.FastSLAM.step_unknown_pruned)


def test_null_arguments_are_status_codes(pkg):
    lib = pkg._lib.evidence_lib()
    BAD = pkg._lib.SLAM_E_BADARG
    assert lib.slam_pf_evidence_create(None, None) == BAD
    assert lib.slam_pf_evidence_destroy(None) == BAD
    assert lib.slam_pf_evidence_update(None, None, 0, 30.0, 1.0, 1, 1, 1, 5, None) == BAD
    assert "null evidence object" in pkg._lib.last_error()
    assert lib.slam_pf_evidence_resample(None, 0.0, 0.5) == BAD
    assert lib.slam_pf_evidence_get(None, None) == BAD
