"""CPU half of tests/test_gpu_pf_wrap.py, with the oracle alone:

1. THE FINDING, pinned.  On the plans of test_predict_update_weights_against_oracle, test_proposal_step_against_oracle and
   test_unknown_correspondences_against_oracle (tests/test_gpu_pf.py) no wrap of the FastSLAM arithmetic changes a value that
   matters: no heading, no innovation of an observation against its own landmark; in the unknown-correspondence plan only
   pairs of an observation and ANOTHER landmark wrap, which the gates reject either way.
2. The scenes of tests/wrap_scenes.py are as hard as they claim, for both mirrored starts.
3. The comparison helper the GPU tests use tells an oracle with a planted wrap defect from the true one on these scenes, at
   the fp32 tolerance as well as at the fp64 one; it accepts the oracle with its state rounded to fp32 after every step, and
   a heading that sits on the other side of the seam.

ONE WRAP IS REDUNDANT, and no comparison of states can see it go: step_proposal's `pm` enters nothing but the bearing innovation
b - (atan2 - pm), which is wrapped itself.  With |b|, |atan2| <= pi and the unwrapped pm within a step of [-pi, pi] the sum is
2 pi k + (something small) with k in {-1, 0, 1} either way, so the single wrap of the innovation returns the same number
(test_the_wrap_of_pm_is_redundant: equal to 1e-12, while the wrap does change `pm` on these scenes).  The heading's wrap in
predict is of the same kind for everything downstream; the helper tells it by the range of the stored heading.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wrap_scenes as W                                            # noqa: E402
from oracle import pf_ref as F                                     # noqa: E402

DTYPES = ["f64", "f32"]


def test_constants_are_the_suites():
    import test_gpu_pf as G
    import test_gpu_pf_unknown_step as U
    assert np.array_equal(W.R, G.R) and np.array_equal(W.Q, G.Q) and W.TOL == G.TOL
    assert (W.GATE1, W.GATE2) == (U.GATE1, U.GATE2)
    assert (W.SMALL_MOTION["V"], W.SMALL_MOTION["dt"]) == (3.0, U.DT2)
    a, b = np.array([1.0, 2.0, 3.5]), np.array([1.0, 2.0, 3.0])
    for tol in (0.1, 0.2):
        assert W.close(a, b, tol)[0] == G.close(a, b, tol) and W.close(a, b, tol, scale=2.0)[0] == G.close(a, b, tol, scale=2.0)


# ---- 1. the finding ------------------------------------------------------------------------------------------------------------
def _count(plan):
    counter = W.WrapCounter()
    with W.replaced_wrap(counter):
        plan()
    return counter


def _plan_known():
    from test_gpu_pf import Q, R, observe, scene
    n, nl, seed = 3000, 10, 77
    lm = scene(nl, 1)
    orc = F.OraclePF(n, nl, seed)
    orc.set_pose([1.0, -2.0, 0.4])
    orc.init_landmarks(lm[:7], 0.01, 0.1)
    rng = np.random.default_rng(2)
    pose = np.array([1.0, -2.0, 0.4])
    for t in range(6):
        orc.predict(6.0, 0.05 * t, 4.0, Q, 0.1)
        pose = np.array([pose[0] + 0.6 * math.cos(0.05 * t + pose[2]), pose[1] + 0.6 * math.sin(0.05 * t + pose[2]),
                         pose[2] + 0.6 * math.sin(0.05 * t) / 4.0])
        ids = np.array([(2 * t) % nl + 1, (2 * t + 1) % nl + 1, 8 + t % 3, (2 * t) % nl + 1])
        orc.update_known(observe(lm, pose, ids, rng), ids, R)


def _plan_proposal():
    from test_gpu_pf import Q, R, observe, scene
    n, nl, seed = 3000 + 11, 10, 91
    lm = scene(nl, 21)
    Qf = np.array([[0.3, 0.004], [0.004, 0.003]])
    orc = F.OraclePF(n, nl, seed)
    orc.set_pose([1.0, -2.0, 0.4])
    orc.init_landmarks(lm[:6], 0.01, 0.1)
    rng = np.random.default_rng(22)
    pose = np.array([1.0, -2.0, 0.4])
    for t in range(6):
        g = 0.04 * t - 0.1
        pose = np.array([pose[0] + 0.6 * math.cos(g + pose[2]), pose[1] + 0.6 * math.sin(g + pose[2]), pose[2] + 0.6 * math.sin(g) / 4.0])
        ids = np.array([1 + t % 6, 1 + (t + 3) % 6, 7 + t % 4, 1 + t % 6, 7 + t % 4])
        orc.step_proposal(6.0, g, 4.0, Qf if t % 2 else Q, 0.1, observe(lm, pose, ids, rng), ids, R)
        om, o1, _ = orc.weight_stats()
        orc.normalize(om, o1)


def _plan_unknown():
    from test_gpu_pf import Q, R, observe
    n, nslots, seed = 1500 + 13, 6, 11
    lm = np.array([[12.0, 3.0], [6.0, -9.0], [-10.0, 4.0], [15.0, -2.0], [-4.0, -12.0], [9.0, 11.0], [-13.0, -6.0]])
    orc = F.OraclePF(n, nslots, seed)
    orc.set_pose([0.5, -0.5, 0.3])
    orc.clear_landmarks()
    rng = np.random.default_rng(5)
    pose = np.array([0.5, -0.5, 0.3])
    for t, ids in enumerate([[1, 2], [2, 1, 3], [1, 3, 4, 2], [5, 1], [6, 2, 3], [7, 4, 6]]):
        orc.predict(3.0, 0.02 * t, 4.0, Q, 0.1)
        pose = np.array([pose[0] + 0.3 * math.cos(0.02 * t + pose[2]), pose[1] + 0.3 * math.sin(0.02 * t + pose[2]),
                         pose[2] + 0.3 * math.sin(0.02 * t) / 4.0])
        z = observe(lm, pose, np.array(ids), rng)
        if t == 3:
            z = np.hstack([z, z[:, 1:2] + np.array([[0.35], [0.0]])])
        orc.update_unknown(z, R, 4.0, 25.0)


def test_the_existing_plans_never_wrap_a_value_that_matters():
    """Elements changed by the oracle's wrap, per call site, on the three plans the suite checks against the oracle."""
    c = _count(_plan_known)
    assert (c.calls("predict.heading"), c.calls("known.v1")) == (6, 21)                # 27 calls in all
    assert c.changed(*W.SITES) == 0
    c = _count(_plan_proposal)
    assert c.calls(*W.SITES) == 60
    assert c.changed(*W.SITES) == 0
    c = _count(_plan_unknown)
    assert c.changed("predict.heading") == 0
    assert c.calls("known.v1") > 0 and c.changed("known.v1") == 0                      # the innovation of every MATCHED pair
    assert c.changed("unknown.v1") > 30000                                             # mismatched (observation, slot) pairs only
    print(f"unknown-correspondence plan: {c.changed('unknown.v1')} wrapped elements, all in mismatched pairs")


# ---- 2. the scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proposal", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
def test_known_id_scene_is_hard(sign, proposal):
    sc = W.known_scene(sign, proposal)                 # (asserts its own conditions)
    rows = sc.rows
    print(f"sign {sign:+d} proposal {proposal}: crossing {[round(r['cross'], 3) for r in rows]} wrapped matched {[round(r['v1'], 3) for r in rows]}"
          f" astern {[r['astern'] for r in rows]}")
    assert rows[sc.astride]["cross"] >= 0.10 and sum(r["cross"] for r in rows) >= 0.99          # ... and in the end every particle has crossed
    assert sum(r["cross"] for r in rows[:W.CROSS_AT - 1]) <= 0.01 and all(r["v1"] >= 0.25 for r in rows)
    # the start heading lies on the side its sign says and the population ends on the other one
    assert np.all(np.sign(sc.run[0].pose[2]) == sign) and np.all(np.sign(sc.run[-1].pose[2]) == -sign)
    # bearings as a sensor reports them; about half of those the scene uses lie more than pi from atan2 - (start heading)
    z = np.hstack([s[2] for s in sc.steps])
    assert np.all(np.abs(z[1]) <= math.pi) and np.abs(z[1]).max() > 3.0
    if proposal:
        c = sum(s.counts["proposal.pm"][2] for s in sc.run)
        assert c >= 0.5 * sc.n, "the wrap of the proposal's mean heading is taken, too"


def test_the_ring_puts_landmarks_where_the_fast_atan2_branches():
    lm = W.ring() - np.array(W.START_XY)
    ang = np.arctan2(lm[:, 1], lm[:, 0])
    assert len(lm) == 16 and np.allclose(np.hypot(lm[:, 0], lm[:, 1]), 15.0)
    assert abs(abs(ang[W.ASTERN - 1]) - math.pi) < 1e-12
    assert sum(np.isclose(np.abs(lm[:, 0]), np.abs(lm[:, 1]))) == 4                    # the diagonals: ay > ax flips with the jitter
    assert sum(np.abs(lm[:, 0]) < 1e-9) == 2 and sum(np.abs(lm[:, 1]) < 1e-9) == 2     # both axes
    assert (lm[:, 0] < -1).sum() >= 6 and (lm[:, 1] < -1).sum() >= 6 and (lm[:, 1] > 1).sum() >= 6      # x < 0, both signs of y


@pytest.mark.parametrize("which", ["m16", "m40"])
@pytest.mark.parametrize("sign", W.SIGNS)
def test_unknown_correspondence_scene_is_hard_and_away_from_the_gates(sign, which):
    sc = W.unknown_scene(sign, which)                  # (asserts its own conditions, the 1e-3 margins among them)
    rows = sc.rows
    print(f"{which} sign {sign:+d}: crossing {[round(r['cross'], 3) for r in rows]} wrapped matched {[round(r['v1'], 3) for r in rows]}"
          f" astern {[r['astern'] for r in rows]} gate margin {min(s.gate_margin for s in sc.run):.3g}")
    assert [s.z.shape[1] for s in sc.run] == ([12, 16, 16, 10, 16, 12] if which == "m16" else [16, 32, 32, 40])
    assert rows[1]["v1_changed"] >= 0.25 * rows[1]["v1_elements"] > 0 and rows[sc.astride]["cross"] >= 0.10
    assert all(np.abs(s.z[1]).max() <= math.pi for s in sc.run)


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("sign", W.SIGNS)
def test_driver_scenes_are_hard(sign, batch):
    """The runs of the bit-for-bit comparisons of tests/test_gpu_pf_wrap.py (driver_scene asserts the conditions)."""
    for repeat_at in ((2, 3, 5) if not batch else (1, 5)):
        steps = W.driver_scene(sign, 16 if batch else 8, batch, repeat_at)
        assert [t for t, s in enumerate(steps) if len(np.unique(s[3])) < len(s[3])] == [repeat_at]
        assert any(s[4] is True for s in steps) and any(s[4] is None for s in steps)


# ---- 3. the comparison helper -------------------------------------------------------------------------------------------------------
def _state(s):
    return s.pose, s.logw, s.lm


def _rejected(true_run, bad_run, dtype, unknown):
    """True when the helper (and, for unknown correspondences, the 0.999 rule on top of it) refuses `bad_run`."""
    agree = total = 0
    for s, b in zip(true_run, bad_run):
        try:
            r = W.compare_with_oracle(_state(b), s, dtype, assoc=(b.assoc, s.assoc) if unknown else None)
        except AssertionError:
            return True
        agree += r.get("agree", 0)
        total += r.get("total", 0)
    return agree < 0.999 * total


KNOWN_DEFECTS = [("predict.heading", "none"), ("known.v1", "none"), ("*", "pos"), ("*", "neg")]
PROPOSAL_DEFECTS = [("proposal.heading", "none"), ("proposal.v1", "none"), ("known.v1", "none"), ("*", "pos"), ("*", "neg")]
UNKNOWN_DEFECTS = [("predict.heading", "none"), ("unknown.v1", "none"), ("known.v1", "none"), ("*", "pos"), ("*", "neg")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sign", W.SIGNS)
def test_helper_rejects_planted_defects_on_the_known_id_scenes(sign, dtype):
    for proposal, defects in ((False, KNOWN_DEFECTS), (True, PROPOSAL_DEFECTS)):
        sc = W.known_scene(sign, proposal)
        assert not _rejected(sc.run, sc.run, dtype, False)
        for defect in defects:
            bad = W.run_known(sign, sc.steps, proposal=proposal, wrap_fn=W.planted(defect))
            assert _rejected(sc.run, bad, dtype, False), f"proposal {proposal}: {defect} passes"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["m16", "m40"])
@pytest.mark.parametrize("sign", W.SIGNS)
def test_helper_rejects_planted_defects_on_the_unknown_correspondence_scenes(sign, which, dtype):
    sc = W.unknown_scene(sign, which)
    assert not _rejected(sc.run, sc.run, dtype, True)
    for defect in UNKNOWN_DEFECTS:
        bad = W.run_unknown(sign, sc.steps, wrap_fn=W.planted(defect))
        assert _rejected(sc.run, bad, dtype, True), f"{defect} passes"


@pytest.mark.parametrize("sign", W.SIGNS)
def test_the_wrap_of_pm_is_redundant(sign):
    """See the header: the issue behind these tests asked for this defect to be rejected; it computes the oracle's numbers."""
    sc = W.known_scene(sign, True)
    assert sum(s.counts["proposal.pm"][2] for s in sc.run) >= 0.5 * sc.n               # the wrap is taken ...
    bad = W.run_known(sign, sc.steps, proposal=True, wrap_fn=W.planted(("proposal.pm", "none")))
    for s, b in zip(sc.run, bad):                                                       # ... and changes nothing
        for x, y in zip(_state(s), _state(b)):
            assert np.max(np.abs(x - y)) <= 1e-12 * max(1.0, float(np.max(np.abs(x))))
    assert not _rejected(sc.run, bad, "f64", False)


@pytest.mark.parametrize("sign", W.SIGNS)
def test_helper_accepts_the_oracle_rounded_to_fp32_after_every_step(sign):
    for proposal in (False, True):
        sc = W.known_scene(sign, proposal)
        rounded = W.run_known(sign, sc.steps, proposal=proposal, round_to="f32")
        recs = [W.compare_with_oracle(_state(b), s, "f32") for s, b in zip(sc.run, rounded)]
        assert all(r["compared"] == sc.n for r in recs)
        assert _rejected(sc.run, rounded, "f64", False)                                 # (fp32 storage is not fp64 accuracy)
    for which in ("m16", "m40"):
        sc = W.unknown_scene(sign, which)
        rounded = W.run_unknown(sign, sc.steps, round_to="f32")
        recs = [W.compare_with_oracle(_state(b), s, "f32", assoc=(b.assoc, s.assoc)) for s, b in zip(sc.run, rounded)]
        assert sum(r["agree"] for r in recs) == sum(r["total"] for r in recs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_helper_and_headings_on_the_other_side_of_the_seam(dtype):
    """A heading within rounding of +-pi may come out as its 2 pi twin: accepted.  The same twin of a heading that is NOT at the
    seam lies outside [-pi, pi]: refused, like a particle left out, a shifted position or a transposed landmark block."""
    sc = W.known_scene(+1, False)
    s = sc.run[sc.astride]
    eps = 0.25 * W.TOL[dtype] * math.pi
    want = W.types.SimpleNamespace(pose=s.pose.copy(), logw=s.logw, lm=s.lm)
    want.pose[2, [3, 500, 1002]] = [math.pi - eps, -math.pi + eps, math.pi]             # a few particles at the seam
    got = want.pose.copy()
    got[2, 3] -= 2 * math.pi
    got[2, 500] += 2 * math.pi
    got[2, 1002] -= 2 * math.pi
    assert np.all(np.abs(got[2, [3, 500, 1002]] - want.pose[2, [3, 500, 1002]]) > 6.28)
    r = W.compare_with_oracle((got, s.logw, s.lm), want, dtype)
    assert r["compared"] == sc.n and r["heading"] <= 1e-3
    far = s.pose.copy()
    k = int(np.argmin(np.abs(far[2])))                                                  # the particle furthest from the seam
    far[2, k] += 2 * math.pi * (1 if far[2, k] > 0 else -1)
    for bad in ((far, s.logw, s.lm), (s.pose[:, :-1], s.logw[:-1], s.lm[:, :, :-1]), (s.pose + [[0.1], [0], [0]], s.logw, s.lm),
                (s.pose, s.logw, s.lm[:, [1, 0, 2, 3, 4], :]), (s.pose, s.logw + 0.1, s.lm)):
        with pytest.raises(AssertionError):
            W.compare_with_oracle(bad, s, dtype)
