"""Seeded FastSLAM scenes in which the angle wraps of the particle-filter kernels (csrc/pf_device.h: wrap_pi) change values
that matter, shared by tests/test_wrap_scenes_cpu.py (CPU: every scene is as hard as it claims, by the oracle alone; the
comparison helper rejects planted defects) and tests/test_gpu_pf_wrap.py (every form of the step on exactly these numbers).
NumPy and the oracle only.

THE SCENE.  A ring of 16 landmarks at 15 m round the start position at the angles k pi / 8 -- on both axes, on the diagonals
(|dy| = |dx|: the `ay > ax` branch of the fp32 atan2), in all four quadrants, and landmark 9 (k = 8) on the negative x axis,
where atan2 flips between +pi and -pi from particle to particle.  The first 12 are known at the start (known-id runs), the
last 4 are first sighted later.  Two mirrored starts: heading +(pi - a) steering left (sign = +1: the heading climbs through
+pi and comes out at -pi) and -(pi - a) steering right (sign = -1), so that both outcomes of both comparisons of the wrap
are taken.  a is CROSS_AT steps of the mean heading advance, so the mean heading lands on the seam after the step of index
CROSS_AT - 1 and about half of the particles have crossed there.  `observe_wrapped` reports bearings in [-pi, pi] as a
sensor does: for about half of the ring the bearing and the particle's own atan2 - phi then differ by 2 pi.

SELF-ASSERTIONS (`assert_hard`, from the oracle alone, on N_ORACLE particles; the random numbers are keyed by the global
particle id, so these are the first N_ORACLE particles of a filter of any size until it first resamples):
  * in at least one step between 10 % and 90 % of the particles cross the seam (the wrap changes their heading);
  * in every step after the first at least 25 % of the (observation, own landmark) pairs have an innovation beyond pi in
    magnitude before the wrap;
  * in one and the same step the particles' atan2 of landmark 9 takes both signs.
The counts come from a counting replacement of oracle/pf_ref.py::_wrap (`WrapCounter`), told apart by call site.

COMPARISON (`compare_with_oracle`).  The tolerances are those of tests/test_gpu_pf.py (TOL, 10 x on covariances and
log-weights, the same scales); nothing new.  Headings are compared as |wrap(got - want)|: a heading within rounding of +-pi
may come out on the other side in fp32, and everything downstream is invariant to that.  The stored heading itself must lie
in [-pi, pi] to the same tolerance: without that a kernel that never wraps the heading would pass (its sines, cosines and
wrapped innovations are the same numbers).  No particle is left out: the helper asserts that it compares all of them, or, in
the unknown-correspondence case, all of those whose decisions agree (fp64: all).
"""
import contextlib
import functools
import math
import sys
import types

import numpy as np

from oracle import pf_ref as F

# the suite's noise and tolerances (tests/test_gpu_pf.py; tests/test_wrap_scenes_cpu.py asserts that they are the same numbers)
R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
QF = np.array([[0.3, 0.004], [0.004, 0.003]])              # the full Q of test_proposal_step_against_oracle
TOL = {"f64": 1e-9, "f32": 2e-4}
GATE1, GATE2 = 4.0, 25.0
NP_DTYPE = {"f64": np.float64, "f32": np.float32}

RING_R, RING_N, RING_KNOWN = 15.0, 16, 12
ASTERN = 9                                                 # 1-based id of the landmark at angle pi
START_XY = (1.0, -2.0)
WHEELBASE, STEER = 4.0, 0.3
CROSS_AT = 3                                               # the mean heading reaches the seam after this many steps
N_ORACLE = 1003                                            # not a multiple of 64
INIT_VAR, INIT_JITTER = 0.01, 0.1
SIGNS = (+1, -1)

KNOWN_MOTION = dict(V=6.0, dt=0.1)                         # the motion of the known-id tests of tests/test_gpu_pf.py
SMALL_MOTION = dict(V=3.0, dt=0.02)                        # the motion of tests/test_gpu_pf_unknown_step.py


def wrap(a):
    return np.where(a > math.pi, a - 2 * math.pi, np.where(a < -math.pi, a + 2 * math.pi, a))


def close(a, b, tol, scale=None):
    """tests/test_gpu_pf.py::close, returning the error as a fraction of the bound as well."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    s = scale if scale is not None else max(float(np.max(np.abs(b))), 1e-30)
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    return err <= tol * s, err / (tol * s)


# ---- the scene -----------------------------------------------------------------------------------------------------------
def ring():
    k = np.arange(RING_N)
    return np.stack([START_XY[0] + RING_R * np.cos(k * math.pi / 8), START_XY[1] + RING_R * np.sin(k * math.pi / 8)], axis=1)


def heading_advance(V, dt):
    return V * dt * math.sin(STEER) / WHEELBASE


def start_pose(sign, V, dt):
    """Heading sign * (pi - a) with a = CROSS_AT mean heading steps."""
    return np.array([START_XY[0], START_XY[1], sign * (math.pi - CROSS_AT * heading_advance(V, dt))])


def advance(pose, V, G, dt):
    """The true vehicle: the motion model without noise, the heading wrapped as a simulator keeps it."""
    return np.array([pose[0] + V * dt * math.cos(G + pose[2]), pose[1] + V * dt * math.sin(G + pose[2]),
                     float(wrap(pose[2] + V * dt * math.sin(G) / WHEELBASE))])


def observe_wrapped(lm, pose, ids, rng, noise=1.0):
    """(range, bearing) of the landmarks `ids` (1-based) from `pose` with `noise` x the sensor's sigma, the bearing brought
    into [-pi, pi] the way a sensor reports it."""
    ids = np.asarray(ids, dtype=np.int64)
    dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
    z = np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + noise * rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))
    z[1] = wrap(z[1])
    assert np.all(np.abs(z[1]) <= math.pi)
    return z


# ---- the counting / replaceable wrap of the oracle ---------------------------------------------------------------------
SITES = ("predict.heading", "proposal.pm", "proposal.v1", "proposal.heading", "known.v1", "unknown.v1")


def _site():
    """Which wrap of oracle/pf_ref.py is being evaluated (the caller of the replaced `_wrap`)."""
    f = sys._getframe(2)
    name = f.f_code.co_name
    if name == "predict":
        return "predict.heading"
    if name == "update_known":
        return "known.v1"
    if name == "associate_unknown":
        return "unknown.v1"
    if name == "step_proposal":
        loc = f.f_locals
        return "proposal.heading" if "e1" in loc else ("proposal.v1" if "pm" in loc else "proposal.pm")
    raise AssertionError(f"_wrap called from {name}: a site this module does not know")


@contextlib.contextmanager
def replaced_wrap(fn):
    """oracle/pf_ref.py::_wrap replaced by fn(site, a) for the duration (the oracle looks `_wrap` up at every call)."""
    saved = F._wrap
    F._wrap = lambda a: fn(_site(), a)
    try:
        yield
    finally:
        F._wrap = saved


class WrapCounter:
    """Per site: calls, elements, elements the wrap changed -- in total and since the last `take()`.  For `replaced_wrap`;
    `inner`: the wrap to count (fn(site, a), e.g. a planted defect) instead of the true one."""

    def __init__(self, inner=None):
        self.total = {s: np.zeros(3, dtype=np.int64) for s in SITES}
        self.since = {s: np.zeros(3, dtype=np.int64) for s in SITES}
        self.inner = inner if inner is not None else (lambda site, a: wrap(a))

    def __call__(self, site, a):
        out = self.inner(site, a)
        inc = np.array([1, np.size(out), int(np.count_nonzero(out != a))])
        self.total[site] += inc
        self.since[site] += inc
        return out

    def take(self):
        out = {s: v.copy() for s, v in self.since.items()}
        for v in self.since.values():
            v[:] = 0
        return out

    def changed(self, *sites):
        return int(sum(self.total[s][2] for s in sites))

    def calls(self, *sites):
        return int(sum(self.total[s][0] for s in sites))


def planted(defect):
    """A `_wrap` with one planted defect, for `replaced_wrap`: (site, "none" | "pos" | "neg") -- no wrap at that site, or a
    wrap for a > pi only / for a < -pi only; site "*" means every site."""
    where, kind = defect

    def fn(site, a):
        if where != "*" and site != where:
            return wrap(a)
        if kind == "none":
            return a
        if kind == "pos":
            return np.where(a > math.pi, a - 2 * math.pi, a)
        if kind == "neg":
            return np.where(a < -math.pi, a + 2 * math.pi, a)
        raise ValueError(kind)
    return fn


# ---- known-id runs ---------------------------------------------------------------------------------------------------------
def known_ids(t, repeat):
    """Step t of a known-id run: landmark 9 (astern), two of the known landmarks of the lower half plane, three of the upper
    one, one of 13..16 (first sighted at t = 0..3, matched afterwards); all distinct unless `repeat` (then the second one again)."""
    lower = (10, 11, 12)
    ids = [ASTERN, lower[t % 3], lower[(t + 1) % 3]] + [1 + (3 * j + t) % 8 for j in range(3)] + [13 + t % 4]
    if repeat:
        ids.append(ids[1])
    return np.array(ids)


def known_steps(sign, nsteps, force=None, repeat_at=3, seed=7):
    """[(V, G, z, ids, force)] of a known-id run from start_pose(sign): constant speed and steering, wrapped observations of the
    true vehicle.  `force`: per-step resampling rule for the drivers (None / False / True each; default: never)."""
    V, dt = KNOWN_MOTION["V"], KNOWN_MOTION["dt"]
    lm = ring()
    rng = np.random.default_rng(seed + (0 if sign > 0 else 1000))
    pose = start_pose(sign, V, dt)
    steps = []
    for t in range(nsteps):
        pose = advance(pose, V, sign * STEER, dt)
        ids = known_ids(t, t == repeat_at)
        steps.append((V, sign * STEER, observe_wrapped(lm, pose, ids, rng), ids, None if force is None else force[t]))
    return steps


def fresh_known(f, sign):
    """Start pose and the 12 known landmarks on anything with the shard's protocol (PFShard, OraclePF)."""
    f.set_pose(start_pose(sign, **KNOWN_MOTION))
    f.init_landmarks(ring()[:RING_KNOWN], INIT_VAR, INIT_JITTER)


def _astern_signs(orc, slot):
    """(particles with atan2 > 0, with atan2 < 0) of the landmark in `slot` as the oracle holds it now."""
    a = np.arctan2(orc.lm[slot, 1] - orc.pose[1], orc.lm[slot, 0] - orc.pose[0])
    return int(np.count_nonzero(a > 0)), int(np.count_nonzero(a < 0))


def _snapshot(orc, **extra):
    return types.SimpleNamespace(pose=orc.pose.copy(), logw=orc.logw.copy(), lm=orc.lm.copy(), **extra)


KNOWN_PF_SEED = 77


def run_known(sign, steps, proposal=False, n=N_ORACLE, seed=KNOWN_PF_SEED, wrap_fn=None, round_to=None, full_q=True):
    """The oracle over a known-id run, normalised after every step as test_proposal_step_against_oracle does: per step a
    snapshot (pose, logw BEFORE the normalisation, lm, stats, sums = mean_pose_sums after it) and the wrap counts of the step.
    `proposal`: step_proposal, with QF on odd steps (`full_q`); otherwise predict + update_known.  `wrap_fn`: a replacement for the
    oracle's wrap (a planted defect).  `round_to`: the state is rounded to that dtype after every step (what a device that
    stores fp32 does at best)."""
    orc = F.OraclePF(n, RING_N, seed)
    fresh_known(orc, sign)
    counter = WrapCounter(wrap_fn)
    out = []
    with replaced_wrap(counter):
        for t, (V, G, z, ids, _force) in enumerate(steps):
            dt = KNOWN_MOTION["dt"]
            if proposal:
                orc.step_proposal(V, G, WHEELBASE, QF if (t % 2 and full_q) else Q, dt, z, ids, R)
            else:
                orc.predict(V, G, WHEELBASE, Q, dt)
                pos, neg = _astern_signs(orc, ASTERN - 1)
                orc.update_known(z, ids, R)
            if proposal:
                pos, neg = _astern_signs(orc, ASTERN - 1)
            if round_to is not None:
                _round_state(orc, round_to)
            snap = _snapshot(orc, stats=orc.weight_stats(), counts=counter.take(), astern=(pos, neg))
            orc.normalize(snap.stats[0], snap.stats[1])
            if round_to is not None:
                orc.logw = orc.logw.astype(NP_DTYPE[round_to]).astype(np.float64)
            snap.sums = orc.mean_pose_sums()
            snap.logw_norm = orc.logw.copy()
            out.append(snap)
    return out


def _round_state(orc, dtype):
    t = NP_DTYPE[dtype]
    orc.pose = orc.pose.astype(t).astype(np.float64)
    orc.lm = orc.lm.astype(t).astype(np.float64)
    orc.logw = orc.logw.astype(t).astype(np.float64)


def hardness(run, n):
    """Per step of an oracle run: the share of particles whose heading the wrap changed, the share of (observation, own
    landmark) innovations it changed, the signs of the astern landmark's atan2."""
    rows = []
    for s in run:
        c = s.counts
        cross = c["predict.heading"][2] + c["proposal.heading"][2]
        # (a proposal step evaluates a matched pair twice: in the proposal from the mean pose, in the update from the sampled one)
        v1_el = c["known.v1"][1] + c["proposal.v1"][1]
        v1_ch = c["known.v1"][2] + c["proposal.v1"][2]
        rows.append(dict(cross=float(cross / n), v1=float(v1_ch / v1_el if v1_el else 0.0), v1_changed=int(v1_ch), v1_elements=int(v1_el),
                         astern=s.astern))
    return rows


def assert_hard(rows, what):
    """The scene's conditions (see the header).  Returns the index of the step with the population astride the seam."""
    shares = [r["cross"] for r in rows]
    astride = [t for t, c in enumerate(shares) if 0.10 <= c <= 0.90]
    assert astride, f"{what}: no step with 10-90 % of the particles crossing the seam: {shares}"
    for t, r in enumerate(rows):
        if t >= 1:
            assert r["v1_elements"] > 0 and r["v1"] >= 0.25, f"{what}: step {t}: only {r['v1']:.3f} of the matched innovations wrap"
    n = max(sum(r["astern"]) for r in rows)
    assert any(min(r["astern"]) >= 0.03 * n > 0 for r in rows), f"{what}: the astern landmark's atan2 never takes both signs: {[r['astern'] for r in rows]}"
    return astride[0]


ORACLE_STEPS = 6


@functools.lru_cache(maxsize=None)
def known_scene(sign, proposal):
    """The 6-step known-id scene of the tests against the oracle (computed once, never changed): steps, the oracle's run, its
    hardness rows and the step with the population astride the seam."""
    steps = known_steps(sign, ORACLE_STEPS)
    run = run_known(sign, steps, proposal=proposal)
    rows = hardness(run, N_ORACLE)
    astride = assert_hard(rows, f"known-id scene, sign {sign:+d}, proposal {proposal}")
    ids_all = np.concatenate([s[3] for s in steps])
    assert any(len(np.unique(s[3])) < len(s[3]) for s in steps), "a step with a repeated landmark"
    assert set(range(RING_KNOWN + 1, RING_N + 1)) <= set(ids_all.tolist()), "first sightings of 13..16"
    return types.SimpleNamespace(sign=sign, steps=steps, run=run, rows=rows, astride=astride, n=N_ORACLE, seed=KNOWN_PF_SEED)


def driver_force(nsteps, batch):
    """The resampling rules of the runs that go through the drivers.  Step by step: Neff rule / never mixed, one forced
    resampling at step CROSS_AT + 2, after the seam has been crossed.  Batch: the rule of tests/test_gpu_pf_batch.py (runs of at
    least four steps that cannot resample go as one persistent launch), its forced resampling at step 13."""
    if batch:
        return [None if t % 9 == 8 else (True if t % 27 == 13 else False) for t in range(nsteps)]
    return [True if t == CROSS_AT + 2 else (None if t % 3 == 2 else False) for t in range(nsteps)]


@functools.lru_cache(maxsize=None)
def driver_scene(sign, nsteps, batch, repeat_at):
    """A known-id run for the bit-for-bit comparisons between the forms of the step: distinct ids in every step but
    `repeat_at` (None: in every step), first sightings, the resampling rules of `driver_force`.  The hardness is asserted on
    the oracle's first N_ORACLE particles WITHOUT resampling for both the FastSLAM-1.0 and the 2.0 step (the seam is crossed
    at step CROSS_AT - 1, before the first step that may resample)."""
    force = driver_force(nsteps, batch)
    steps = known_steps(sign, nsteps, force=force, repeat_at=repeat_at)
    first_may_resample = min(t for t, f in enumerate(force) if f is not False)
    for proposal in (False, True):
        rows = hardness(run_known(sign, steps, proposal=proposal, full_q=False), N_ORACLE)
        astride = assert_hard(rows, f"driver scene, sign {sign:+d}, {nsteps} steps, proposal {proposal}")
        assert astride <= first_may_resample, "the seam is crossed while the filter is still the oracle's"
    forced = [t for t, f in enumerate(force) if f is True]
    assert forced and min(forced) > astride, "a forced resampling after the seam has been crossed"
    return steps


# ---- unknown-correspondence runs -----------------------------------------------------------------------------------------
UNKNOWN_SLOTS = 18
# 0-based landmark indices per step.  PLAN16: what the legacy call takes (m <= 16); PLAN40: the fused step's wider calls --
# two sightings of every ring landmark (m = 32: two LDS groups of 16), interleaved the other way round, and (fp64 only) m = 40.
PLAN16 = (tuple(range(12)), tuple(range(16)), tuple(range(16)), (8, 9, 10, 11, 12, 13, 1, 2, 3, 8), tuple(range(16)),
          tuple(range(12, 16)) + tuple(range(8)))
PLAN40 = (tuple(range(16)), tuple(range(16)) * 2, tuple(range(15, -1, -1)) + tuple(range(16)),
          tuple(range(16)) * 2 + tuple(range(4, 12)))
# the seeds of the observation noise, chosen so that the astern landmark (whose position every particle sets for itself at the first
# sighting) is seen with both signs of atan2 in one step; the margins of the decisions are asserted, not searched for
UNKNOWN_SEED = {("m16", +1): 23, ("m16", -1): 26, ("m40", +1): 23, ("m40", -1): 23}
UNKNOWN_PF_SEED = 23


def unknown_steps(sign, plan, seed):
    V, dt = SMALL_MOTION["V"], SMALL_MOTION["dt"]
    lm = ring()
    rng = np.random.default_rng(seed + (0 if sign > 0 else 1000))
    pose = start_pose(sign, V, dt)
    steps = []
    for idx in plan:
        pose = advance(pose, V, sign * STEER, dt)
        steps.append(observe_wrapped(lm, pose, np.array(idx) + 1, rng, noise=1.0 / 3.0))
    return steps


def fresh_unknown(f, sign):
    f.set_pose(start_pose(sign, **SMALL_MOTION))
    f.clear_landmarks()


def run_unknown(sign, steps, scores=None, n=N_ORACLE, seed=UNKNOWN_PF_SEED, wrap_fn=None, round_to=None, astern_slot=8):
    """The oracle over an unknown-correspondence run from an empty map (predict + update_unknown per step): per step a snapshot
    (pose, logw, lm, assoc, stats), the wrap counts and -- when `scores` (tests/test_gpu_pf_unknown_step.py::_scores) is
    given -- the smallest relative distance of any (observation, used slot) NIS from a gate and the smallest gap between the best
    and the second-best candidate of a matched observation."""
    orc = F.OraclePF(n, UNKNOWN_SLOTS, seed)
    fresh_unknown(orc, sign)
    counter = WrapCounter(wrap_fn)
    out = []
    with replaced_wrap(counter):
        for z in steps:
            orc.predict(SMALL_MOTION["V"], sign * STEER, WHEELBASE, Q, SMALL_MOTION["dt"])
            gate_margin = nd_gap = math.inf
            if scores is not None:
                nis, nd, used = scores(orc, z)
                u = np.broadcast_to(used[None], nis.shape)
                if u.any():
                    gate_margin = min(float(np.min(np.abs(nis[u] - g) / g)) for g in (GATE1, GATE2))
                cand = np.where(u & (nis < GATE1), nd, np.inf)
                two = np.sort(cand, axis=1)[:, :2, :]
                matched = np.isfinite(two[:, 0, :])
                if matched.any():
                    nd_gap = float(np.min(two[:, 1, :][matched] - two[:, 0, :][matched]))
            used_before = orc.lm[astern_slot, 2] >= 0
            astern = _astern_signs(orc, astern_slot) if used_before.all() else (0, 0)
            assoc = orc.update_unknown(z, R, GATE1, GATE2)
            if round_to is not None:
                _round_state(orc, round_to)
            out.append(_snapshot(orc, assoc=assoc.copy(), stats=orc.weight_stats(), counts=counter.take(), astern=astern,
                                 gate_margin=gate_margin, nd_gap=nd_gap, z=z))
    return out


@functools.lru_cache(maxsize=None)
def unknown_scene(sign, which):
    """`which`: "m16" (PLAN16) or "m40" (PLAN40).  Computed once; the margins of the decisions and the hardness are asserted
    here, from the oracle alone."""
    from test_gpu_pf_unknown_step import _scores
    plan = PLAN16 if which == "m16" else PLAN40
    seed = UNKNOWN_SEED[(which, sign)]
    steps = unknown_steps(sign, plan, seed)
    run = run_unknown(sign, steps, scores=_scores)
    what = f"unknown-correspondence scene {which}, sign {sign:+d}"
    for t, s in enumerate(run):
        assert s.gate_margin > 1e-3, f"{what}: step {t}: a NIS sits at a gate ({s.gate_margin:.2e})"
        assert s.nd_gap > 1e-3, f"{what}: step {t}: two candidates tie ({s.nd_gap:.2e})"
    rows = hardness(run, N_ORACLE)
    astride = assert_hard(rows, what)
    assert np.all(run[0].assoc == -1), "an empty map: every observation of the first step is new"
    for t, s in enumerate(run[1:], 1):
        assert np.all(s.assoc != -2), f"{what}: step {t}: a dropped observation"
    assert np.all(run[-1].assoc >= 0) and np.all((run[-1].lm[:, 2, :] >= 0).sum(axis=0) == RING_N)
    return types.SimpleNamespace(sign=sign, steps=steps, run=run, rows=rows, astride=astride, n=N_ORACLE, seed=UNKNOWN_PF_SEED)


# ---- the comparison ----------------------------------------------------------------------------------------------------------
def compare_with_oracle(state, oracle, dtype, assoc=None):
    """`state` = (pose [3, n], logw [n], lm [nl, 5, n]) as downloaded, `oracle` anything with .pose, .logw, .lm in float64,
    against the tolerances of tests/test_gpu_pf.py.  Known ids (assoc None): test_predict_update_weights_against_oracle's
    bounds on ALL particles.  Unknown correspondences (assoc = (decisions [m, n] of the state, of the oracle)):
    test_unknown_correspondences_against_oracle's rule -- fp64 identical decisions; the state is compared on the particles
    whose decisions agree, slot usage included.  Raises AssertionError; returns {quantity: error / bound, "compared": count,
    "agree": .., "total": ..} for the record."""
    pose, logw, lm = (np.asarray(a, dtype=np.float64) for a in state)
    o_pose, o_logw, o_lm = oracle.pose, oracle.logw, oracle.lm
    assert pose.shape == o_pose.shape and logw.shape == o_logw.shape and lm.shape == o_lm.shape, "the whole filter, in the oracle's shape"
    assert np.all(np.isfinite(pose)) and np.all(np.isfinite(logw))
    n = pose.shape[1]
    tol = TOL[dtype]
    out = {}
    if assoc is None:
        same = np.ones(n, dtype=bool)
        pose_scale = max(float(np.max(np.abs(o_pose))), 1e-30)                 # (close(p, orc.pose, tol): the scale is the largest entry)
    else:
        a, ao = (np.asarray(v) for v in assoc)
        assert a.shape == ao.shape and a.shape[1] == n
        out["agree"], out["total"] = int(np.sum(a == ao)), int(a.size)
        if dtype == "f64":
            assert np.array_equal(a, ao), "fp64: the decisions must be identical"
        same = np.all(a == ao, axis=0)
        pose_scale = 20.0
    out["compared"] = int(same.sum())
    if assoc is None or dtype == "f64":
        assert out["compared"] == n, "no particle may be left out"
    ok, out["xy"] = close(pose[0:2, same], o_pose[0:2, same], tol, scale=pose_scale)
    assert ok, f"position: {out['xy']:.3g} x the bound"
    bound = tol * pose_scale
    out["heading range"] = max(0.0, float(np.max(np.abs(pose[2, same]))) - math.pi) / bound if same.any() else 0.0
    assert out["heading range"] <= 1.0, f"a stored heading outside [-pi, pi]: max |phi| - pi = {out['heading range'] * bound:.3g}"
    dphi = np.abs(wrap(pose[2, same] - o_pose[2, same]))                       # (+pi against -pi: 2 pi apart before the wrap, 0 after)
    out["heading"] = float(np.max(dphi)) / bound if same.any() else 0.0
    assert out["heading"] <= 1.0, f"heading: {out['heading']:.3g} x the bound"
    if assoc is None:
        ok, out["landmark means"] = close(lm[:, 0:2], o_lm[:, 0:2], tol)
        assert ok, f"landmark means: {out['landmark means']:.3g} x the bound"
        ok, out["landmark cov"] = close(lm[:, 2:5], o_lm[:, 2:5], tol * 10, scale=float(np.max(np.abs(o_lm[:, 2:5]))))
        assert ok, f"landmark covariances: {out['landmark cov']:.3g} x the bound"
    else:
        used_o = o_lm[:, 2, :] >= 0
        assert np.array_equal((lm[:, 2, :] >= 0)[:, same], used_o[:, same]), "slot usage differs"
        mask = np.broadcast_to(used_o[:, None, :] & same[None, None, :], o_lm.shape)
        ok, out["landmarks"] = close(np.where(mask, lm, 0.0), np.where(mask, o_lm, 0.0), 10 * tol, scale=20.0)
        assert ok, f"landmarks: {out['landmarks']:.3g} x the bound"
    ok, out["logw"] = close(logw[same], o_logw[same], tol * 10, scale=max(1.0, float(np.max(np.abs(o_logw)))))
    assert ok, f"log-weights: {out['logw']:.3g} x the bound"
    return out


def worst(records):
    """The largest error / bound per quantity over a list of compare_with_oracle results."""
    out = {}
    for r in records:
        for k, v in r.items():
            if k not in ("agree", "total", "compared"):
                out[k] = max(out.get(k, 0.0), v)
    return out
