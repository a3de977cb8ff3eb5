"""NumPy restatement of the landmark-evidence rule of include/slamhip_evidence.h (slam_pf_evidence_update): one existence
counter per (slot, particle) of an unknown-correspondence particle filter, raised by a match, lowered when the landmark
lies inside the sensor's field of view and was not observed, the record discarded when the counter falls below zero
(Probabilistic Robotics, Table 13.1).

Geometry in float64 from the values handed in (for a GPU test: the downloaded state, i.e. exactly the stored values),
integer counters.  Besides the result the function returns every in-use pair's distance to the two field-of-view
boundaries, so that a test can assert that no pair of its scene sits where fp32 rounding of sqrt / atan2 could decide."""
import math

import numpy as np

EMPTY = -128
EMPTY_RECORD = (0.0, 0.0, -1.0, 0.0, 0.0)        # what pf_clear_lm_kernel writes


def _wrap(a):
    return np.where(a > math.pi, a - 2 * math.pi, np.where(a < -math.pi, a + 2 * math.pi, a))


def geometry(pose, lm):
    """(d, b) [nl, n] of every record from its particle's pose: range and wrapped bearing, float64."""
    pose = np.asarray(pose, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    with np.errstate(all="ignore"):
        dx, dy = lm[:, 0, :] - pose[0][None], lm[:, 1, :] - pose[1][None]
        d = np.sqrt(dx * dx + dy * dy)
        b = _wrap(np.arctan2(dy, dx) - pose[2][None])
    return d, b


def evidence_update(c, lm, pose, assoc, r_max, half_fov, inc=1, dec=1, init=1, cap=5):
    """One pass of the rule.

    c      [nl, n] integer counters (EMPTY = -128: no landmark here)
    lm     [nl, 5, n] records (x, y, Pxx, Pxy, Pyy); Pxx < 0 marks a free slot
    pose   [3, n]
    assoc  [m, n] decisions of the step just made (slot >= 0 matched, negative: not matched), or None / m = 0

    Returns (c_new int8 [nl, n], lm_new (same dtype as lm), counts, margins):
      counts   [in use after the call, created, decremented, pruned]; "decremented" counts every application of case 4,
               the pruned ones included
      margins  dict(range=[nl, n], bearing=[nl, n]): |d - r_max| / r_max and ||b| - half_fov| (radians) of every pair in
               use before the call, +inf elsewhere; pruned=[nl, n] bool; in_view=[nl, n] bool (False where not in use)
    """
    assert r_max > 0 and math.isfinite(r_max) and 0 < half_fov <= math.pi
    assert inc >= 1 and dec >= 1 and 0 <= init <= cap <= 127
    c = np.asarray(c).astype(np.int64)
    lm_in = np.asarray(lm)
    nl, _, n = lm_in.shape
    assert c.shape == (nl, n)
    used = ~(lm_in[:, 2, :] < 0)
    matched = np.zeros((nl, n), dtype=bool)
    if assoc is not None:
        a = np.asarray(assoc).reshape(-1, n)
        pidx = np.arange(n)
        for i in range(a.shape[0]):
            ok = (a[i] >= 0) & (a[i] < nl)
            matched[a[i][ok], pidx[ok]] = True
    d, b = geometry(pose, lm_in)
    in_view = used & (d <= r_max) & (np.abs(b) <= half_fov)

    case1 = ~used
    case2 = used & (c == EMPTY)
    case3 = used & ~case2 & matched
    case4 = used & ~case2 & ~matched & in_view
    out = c.copy()
    out[case1] = EMPTY
    out[case2] = init
    out[case3] = np.minimum(c[case3] + inc, cap)
    out[case4] = c[case4] - dec
    pruned = case4 & (out < 0)
    out[pruned] = EMPTY
    lm_new = lm_in.copy()
    for k, v in enumerate(EMPTY_RECORD):
        lm_new[:, k, :][pruned] = v
    counts = [int((used & ~pruned).sum()), int(case2.sum()), int(case4.sum()), int(pruned.sum())]
    with np.errstate(all="ignore"):
        margins = dict(range=np.where(used, np.abs(d - r_max) / r_max, np.inf),
                       bearing=np.where(used, np.abs(np.abs(b) - half_fov), np.inf),
                       pruned=pruned, in_view=in_view)
    assert out.min() >= EMPTY and out.max() <= 127
    return out.astype(np.int8), lm_new, counts, margins


def gap_midpoint(values, lo, hi, min_gap):
    """The midpoint of the widest gap between consecutive sorted `values` inside (lo, hi), the two ends counting as values;
    the gap must exceed `min_gap`.  How a test picks r_max / half_fov so that no pair of its scene sits at the boundary."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    v = np.concatenate([[lo], v[(v > lo) & (v < hi)], [hi]])
    gaps = np.diff(v)
    k = int(np.argmax(gaps))
    assert gaps[k] > min_gap, f"the widest gap {gaps[k]:.3e} is too narrow"
    return 0.5 * (v[k] + v[k + 1])


def pick_fov(pose, lm, min_used=8):
    """(r_max, half_fov, slot) for a state: half_fov is the midpoint of the widest gap between the sorted |bearings| of all
    pairs in use inside (0.9, 2.2) rad; r_max is the midpoint of a gap between the sorted ranges of ALL pairs in use that lies
    between the 10th and the 90th percentile of ONE slot's ranges -- the slot, every one of whose bearings is inside half_fov,
    is then in view for some of its particles and out of view for the others.  Of all such slots the one with the widest gap
    relative to the range is taken.  Asserted: every pair in use is more than 2e-5 r_max / 2e-5 rad away from the boundaries
    (twice what the GPU test needs)."""
    lm = np.asarray(lm, dtype=np.float64)
    d, b = geometry(pose, lm)
    used = ~(lm[:, 2, :] < 0)
    half_fov = gap_midpoint(np.abs(b)[used], 0.9, 2.2, 4e-5)
    all_d = np.sort(d[used])
    best = None
    for l in range(lm.shape[0]):
        u = used[l]
        if u.sum() < min_used or not np.all(np.abs(b[l][u]) < half_fov):
            continue
        lo, hi = np.percentile(d[l][u], [10, 90])
        v = all_d[(all_d >= lo) & (all_d <= hi)]
        if v.size < 2:
            continue
        gaps = np.diff(v)
        k = int(np.argmax(gaps))
        score = gaps[k] / v[k + 1]
        if best is None or score > best[0]:
            best = (score, 0.5 * (v[k] + v[k + 1]), l)
    assert best is not None, "no slot of the scene can straddle r_max"
    assert best[0] > 4e-5, f"the widest gap is {best[0]:.2e} of the range"
    r_max, slot = best[1], best[2]
    inside = d[slot][used[slot]] <= r_max
    assert inside.any() and (~inside).any()
    return float(r_max), float(half_fov), slot


# ---- the scene of the GPU rule test: a few near landmarks ahead of the vehicle, the rest on a grid beyond 24 m ------------------
RULE = dict(pose=(0.0, 0.0, 0.2), V=1.0, G=0.02, wheelbase=4.0, dt=0.5, gate1=4.0, gate2=25.0, inc=2, dec=1, init=1, cap=3)
RULE_NEAR = [(8.0, 0.15), (11.0, -0.35), (14.0, 0.5), (17.0, -0.1), (9.0, 2.9)]       # (range, bearing from the heading)


def rule_landmarks(count):
    """`count` landmarks: the five near ones (four ahead, one behind), then jittered cells of a 10 m grid outside 24 m."""
    x0, y0, phi0 = RULE["pose"]
    lm = [[x0 + r * math.cos(phi0 + b), y0 + r * math.sin(phi0 + b)] for r, b in RULE_NEAR]
    g = np.random.default_rng(71)
    xs, ys = np.meshgrid(-75.0 + 10.0 * np.arange(16), -55.0 + 10.0 * np.arange(12), indexing="ij")
    cells = np.stack([xs.ravel(), ys.ravel()], axis=1) + g.uniform(-1.0, 1.0, (192, 2))
    cells = cells[np.hypot(cells[:, 0], cells[:, 1]) > 24.0]
    cells = cells[g.permutation(len(cells))]
    assert len(lm) + len(cells) >= count
    return np.array(lm + cells[:count - len(lm)].tolist())


def rule_plan(nl):
    """(landmarks, the z [2, m] of the three filling steps, the z of the step between the updates).  All but one (nl = 6) or
    five (larger maps) slots get a landmark: the first step sees up to 64 new ones (the near ones among them), the second the
    rest, the third revisits two -- so the near landmarks' ranges spread with the motion noise of two steps.  The step
    between the updates sees one landmark nobody holds and a revisit."""
    K = nl - 1 if nl <= 6 else nl - 5
    lm = rule_landmarks(K + 1)
    rng = np.random.default_rng(72)
    sig = np.array([[0.1], [math.pi / 180]])
    pose = np.array(RULE["pose"])
    chunks = [np.arange(min(K, 64)), np.arange(64, K) if K > 64 else np.array([3, 4]), np.array([3, 4]), np.array([K, 4])]
    zs = []
    for ids in chunks:
        pose = np.array([pose[0] + RULE["V"] * RULE["dt"] * math.cos(RULE["G"] + pose[2]),
                         pose[1] + RULE["V"] * RULE["dt"] * math.sin(RULE["G"] + pose[2]),
                         pose[2] + RULE["V"] * RULE["dt"] * math.sin(RULE["G"]) / RULE["wheelbase"]])
        dx, dy = lm[ids, 0] - pose[0], lm[ids, 1] - pose[1]
        zs.append(np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + 0.3 * rng.normal(0, sig, (2, len(ids))))
    return lm, zs[:3], zs[3]


def hand_decisions(u, m, n, nl):
    """A hand-made decision array [m, n] for update `u`: observation i names slot s_i (slots of every group of 64, the last
    slot of the map) for about one particle in seven, and otherwise -1, -2, a slot index past the map, 2^30, -5 or the most
    negative int32; observations 0 and 1 name the same slot for every particle (a slot matched twice in one call)."""
    slots = [s for s in (0, 1, 5, 63, 64, 100, 127, 128, nl - 1) if 0 <= s < nl]
    rng = np.random.default_rng(100 + u)
    a = np.empty((m, n), dtype=np.int32)
    for i in range(m):
        s = slots[(i + u) % len(slots)]
        pool = np.array([s, -1, -2, nl + 3, 2 ** 30, -5, -2 ** 31], dtype=np.int64)
        a[i] = pool[rng.integers(0, len(pool), n)].astype(np.int32)
    if m >= 2:
        a[0] = a[1] = slots[-1]
    return a


# ---- the scenario of the issue: clutter fills the map, the sixth landmark is lost; with pruning it is kept ------------
SCN = dict(n=300, slots=8, seed=11, pose=(0.0, 0.0, 0.1), V=3.0, G=0.0, wheelbase=4.0, dt=0.1, gate1=4.0, gate2=25.0,
           r_max=30.0, half_fov=math.pi / 2, inc=1, dec=1, init=1, cap=5, steps=14, clutter_steps=10, sixth_from=12)
SCN_LM = np.array([[12.0, 3.0], [9.0, -6.0], [15.0, -2.0], [7.0, 8.0], [18.0, 5.0]])
SCN_SIXTH = np.array([14.0, 9.0])
SCN_R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
SCN_Q = 0.01 * np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])


def scenario_observations(pad_step=None, pad_to=0):
    """The observation list z [2, m] of every step: the five landmarks with 0.3 sigma of noise from the noise-free
    trajectory, one false detection (range 5 + 1.7 t, bearing -1.2 + 0.24 t) in steps 0 .. 9, the sixth landmark from
    step 12 on.  `pad_step`: that step's list is padded to `pad_to` observations with second looks at the five landmarks
    (fresh 0.3 sigma noise), which every particle matches to the slots it already holds."""
    rng = np.random.default_rng(SCN["seed"])
    pose = np.array(SCN["pose"])
    sig = np.array([[0.1], [math.pi / 180]])
    out = []
    for t in range(SCN["steps"]):
        pose = np.array([pose[0] + SCN["V"] * SCN["dt"] * math.cos(SCN["G"] + pose[2]),
                         pose[1] + SCN["V"] * SCN["dt"] * math.sin(SCN["G"] + pose[2]),
                         pose[2] + SCN["V"] * SCN["dt"] * math.sin(SCN["G"]) / SCN["wheelbase"]])
        lms = SCN_LM if t < SCN["sixth_from"] else np.vstack([SCN_LM, SCN_SIXTH])
        dx, dy = lms[:, 0] - pose[0], lms[:, 1] - pose[1]
        true = np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]])
        z = true + 0.3 * rng.normal(0, sig, true.shape)
        if t < SCN["clutter_steps"]:
            z = np.hstack([z, [[5.0 + 1.7 * t], [-1.2 + 0.24 * t]]])
        if t == pad_step and z.shape[1] < pad_to:
            k = pad_to - z.shape[1]
            idx = np.arange(k) % 5
            z = np.hstack([z, true[:, idx] + 0.3 * rng.normal(0, sig, (2, k))])
        out.append(z)
    return out


RULE_Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])      # the motion noise of the rule scene
