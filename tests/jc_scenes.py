"""Seeded scenes for the joint-compatibility search (include/slamhip_jc.h), shared by tests/test_jc_ref_cpu.py and
tests/test_gpu_ekf_jc.py.  NumPy, the oracle and tests/jc_ref.py only.

A scene is a dict: x, P (already rounded as a device of `dtype` holds them, tests/assoc_scenes.round_state), z (2 x nz, fp64), N,
`ref` (the literal reference's record for the scene's gates and thresholds) and per-kind fields.  Observations are drawn the way
a filter meets them: a true state is sampled from N(x, P), the landmarks are observed from it with noise R.

CONDITIONS (verify, with the reference alone; DELTA and TOL are the project's constants):
  * every individual nis is DELTA (relative) away from gate1 and from gate2;
  * the candidates of one observation are DELTA apart in nis;
  * every joint test the reference evaluates is DELTA away from its threshold and has all pivots positive;
  * 2k * 2^-53 * cond2(S_H) <= 1e-10 at every evaluated test: ten times under TOL, so a device that computes in double can neither
    flip a decision nor miss the value bar;
  * `truncated` is set only in the scene built for it.
A scene that misses a condition, or the property its kind is built for, is drawn again with the next seed."""
import functools
import math

import numpy as np

from oracle import ekf_ref as O
from tests import assoc_scenes as AS
from tests import jc_ref as JR

R = AS.R
GATE1, GATE2, DELTA = AS.GATE1, AS.GATE2, AS.DELTA
TOL = 1e-9
CONFIDENCE = 0.95
COND_BAR = 1e-10
MAX_NODES = 20000
CHI2 = JR.chi2_table(JR.MAXOBS, CONFIDENCE)


def observe(xt, ids, rng, noise=1.0):
    """Range and bearing (wrapped into (-pi, pi], as a sensor reports it) of the landmarks ids (1-based) of the state xt."""
    ids = np.asarray(ids, dtype=np.int64)
    f = 3 + 2 * (ids - 1)
    dx, dy = xt[f] - xt[0], xt[f + 1] - xt[1]
    b = np.arctan2(dy, dx) - xt[2]
    b = np.arctan2(np.sin(b), np.cos(b))
    z = np.stack([np.hypot(dx, dy), b])
    return z + noise * np.sqrt(np.diag(R))[:, None] * rng.standard_normal(z.shape)


def true_state(x, P, rng, spread=1.0):
    return x + spread * (np.linalg.cholesky(P) @ rng.standard_normal(len(x)))


def ring_state(rng, N, dtype, d_xy=0.1, d_phi=0.02, heading=None):
    """N landmarks 15 .. 80 m around the pose, one per sector of 2 pi / N (so no two share a direction and a range), pose sigma
    0.5 d_xy metres and 0.5 d_phi radians, landmark sigmas 5 .. 10 cm, everything correlated (assoc_scenes.scaled_cov)."""
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3) if heading is None else heading])
    th = 2 * math.pi * (rng.permutation(N) + rng.uniform(0.2, 0.8, N)) / max(N, 1)
    r = rng.uniform(15, 80, N)
    pts = pose[:2] + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    x = np.concatenate([pose, pts.reshape(-1)])
    return AS.round_state(x, AS.scaled_cov(rng, N, d_xy, d_phi, 0.1, 0.2), dtype)


def nn_vector(x, P, z):
    nis, nd = O.association_table_sparse(x, P, z, R)
    return O.assoc_vector(nis, nd, GATE1, GATE2)


def verify(scene, max_nodes=MAX_NODES):
    """The conditions of the module docstring, or None where the scene misses one (the builder then takes the next seed)."""
    x, P, z = scene["x"], scene["P"], scene["z"]
    assert np.array_equal(P, P.T)
    ref = JR.associate_joint(x, P, z, R, GATE1, GATE2, CHI2, max_nodes, form="literal")
    nis = ref["nis"]
    fin = nis[~np.isnan(nis)]
    for g in (GATE1, GATE2):
        if fin.size and np.any(np.abs(fin / g - 1.0) < DELTA):
            return None
    for lst in ref["cand"]:
        n = np.array([c[0] for c in lst])
        if len(n) >= 2 and np.any(np.diff(n) < DELTA * np.abs(n[1:])):
            return None
    worst_margin, worst_cond = math.inf, 0.0
    for pairs, d2, thr, ok, cond in ref["trace"]:
        if not ok:
            return None
        bar = 2 * len(pairs) * 2.0 ** -53 * cond
        worst_margin, worst_cond = min(worst_margin, abs(d2 / thr - 1.0)), max(worst_cond, bar)
        if abs(d2 / thr - 1.0) < DELTA or bar > COND_BAR:
            return None
    if bool(ref["truncated"]) != bool(scene.get("truncated_ok", False)):
        return None
    if ref["exhausted"]:
        return None
    scene.update(ref=ref, N=(len(x) - 3) // 2, worst_margin=worst_margin, worst_cond_bar=worst_cond, nn=nn_vector(x, P, z))
    return scene


def _reused(assoc):
    a = np.asarray(assoc)
    a = a[a > 0]
    return len(a) != len(set(a.tolist()))


# ---- the builders: one draw each; None = take the next seed ------------------------------------------------------------------------
def _pairs(seed, dtype):
    """40 landmarks in pairs 1.2 m apart, pose sigma 0.5 m / 0.15 rad, 10 true and 2 spurious observations.  Kept when the nearest
    neighbour uses a landmark twice and the joint search does not."""
    rng = np.random.default_rng(seed)
    NP_ = 20
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3)])
    th, r = rng.uniform(0, 2 * math.pi, NP_), rng.uniform(8, 30, NP_)
    a = pose[:2] + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    ph = rng.uniform(0, 2 * math.pi, NP_)
    b = a + 1.2 * np.stack([np.cos(ph), np.sin(ph)], axis=1)
    pts = np.stack([a, b], axis=1).reshape(-1, 2)[rng.permutation(2 * NP_)]
    x, P = AS.round_state(np.concatenate([pose, pts.reshape(-1)]), AS.scaled_cov(rng, 2 * NP_, 1.0, 0.3, 0.2, 0.4), dtype)
    xt = true_state(x, P, rng)
    ids = rng.choice(np.arange(1, 2 * NP_ + 1), 12, replace=False)
    z = observe(xt, ids[:10], rng)
    ghost = xt.copy()                                    # two things that are not in the map, 0.7 m beside a landmark each
    for j in ids[10:]:
        f = 3 + 2 * (j - 1)
        ang = rng.uniform(0, 2 * math.pi)
        ghost[f:f + 2] += 0.7 * np.array([math.cos(ang), math.sin(ang)])
    z = np.hstack([z, observe(ghost, ids[10:], rng)])[:, rng.permutation(12)]
    sc = verify(dict(x=x, P=P, z=z))
    if sc is None or not _reused(sc["nn"]) or _reused(sc["ref"]["assoc"]):
        return None
    return sc


def _sizes(seed, dtype, nz, N=None):
    """nz true observations of distinct landmarks of a ring map (N = max(nz + 16, 24) landmarks), drawn at half the spread the
    state claims, so that every prefix passes its joint test: all paired, depth nz."""
    rng = np.random.default_rng(seed)
    N = max(nz + 16, 24) if N is None else N
    x, P = ring_state(rng, N, dtype)
    xt = true_state(x, P, rng, 0.5)
    ids = rng.choice(np.arange(1, N + 1), nz, replace=False)
    sc = verify(dict(x=x, P=P, z=observe(xt, ids, rng, 0.5), ids=ids))
    if sc is None or sc["ref"]["pairings"] != nz or sc["ref"]["deepest"] != nz or not np.array_equal(sc["ref"]["assoc"], ids):
        return None
    return sc


def _empty(seed, dtype, _arg=None):
    rng = np.random.default_rng(seed)
    x, P = AS.round_state(np.array([50.0, 50.0, 0.3]), 0.01 * np.eye(3), dtype)
    return verify(dict(x=x, P=P, z=np.stack([rng.uniform(5, 30, 3), rng.uniform(-3, 3, 3)])))


def _outer(seed, dtype, _arg=None):
    """Four true observations and two with no candidate: nis 20 (dropped) and nis 30 (new) against their nearest landmark."""
    rng = np.random.default_rng(seed)
    x, P = ring_state(rng, 30, dtype)
    ids = rng.choice(np.arange(1, 31), 6, replace=False)
    z = np.hstack([observe(true_state(x, P, rng, 0.5), ids[:4], rng, 0.5), AS.edge_obs(x, P, ids[4:], [20.0, 30.0], rng, alone=True)])
    sc = verify(dict(x=x, P=P, z=z, ids=ids))
    if sc is None or sc["ref"]["assoc"].tolist() != ids[:4].tolist() + [0, -1]:
        return None
    return sc


def _trunc(seed, dtype, _arg=None):
    """Twelve landmarks within 30 cm of each other under a pose sigma of half a metre: the observation of one of them has twelve
    candidates, eight are kept."""
    rng = np.random.default_rng(seed)
    N = 24
    x, P = ring_state(rng, N, dtype, d_xy=1.0, d_phi=0.05)
    c = x[3:5].copy()
    for j in range(12):
        x[3 + 2 * j:5 + 2 * j] = c + rng.uniform(-0.15, 0.15, 2)
    x, P = AS.round_state(x, P, dtype)
    ids = np.array([5, 14, 17, 20])
    sc = verify(dict(x=x, P=P, z=observe(true_state(x, P, rng, 0.5), ids, rng, 0.5), truncated_ok=True, ids=ids))
    if sc is None or int(np.sum(sc["ref"]["nis"][0] < GATE1)) <= JR.MAXCAND or len(sc["ref"]["cand"][0]) != JR.MAXCAND:
        return None
    return sc


def _wrap(seed, dtype, _arg=None):
    """Two landmarks straight behind the vehicle, one on each side of the cut: the predicted bearing (not wrapped) and the reported
    one (wrapped) differ by about 2 pi; four ordinary observations beside them."""
    rng = np.random.default_rng(seed)
    N = 20
    x, P = ring_state(rng, N, dtype, heading=0.5)
    for j, off in ((3, -0.004), (11, 0.004)):
        x[3 + 2 * j:5 + 2 * j] = x[:2] + 30.0 * (1 + 0.3 * j) / 4 * np.array([math.cos(0.5 + math.pi + off), math.sin(0.5 + math.pi + off)])
    x, P = AS.round_state(x, P, dtype)
    ids = np.array([4, 12, 2, 7, 9, 16])
    z = observe(true_state(x, P, rng, 0.5), ids, rng, 0.5)
    zp, _ = O._landmark_S(x, P, R, ids[:2])
    sc = verify(dict(x=x, P=P, z=z, ids=ids))
    if sc is None or not np.all(np.abs(z[1, :2] - zp[:, 1]) > math.pi) or not np.array_equal(sc["ref"]["assoc"], ids):
        return None
    return sc


BUILDERS = {"pairs": _pairs, "sizes": _sizes, "empty": _empty, "outer": _outer, "trunc": _trunc, "wrap": _wrap}
SCENES = [("pairs", 0), ("pairs", 1), ("sizes", 1), ("sizes", 2), ("sizes", 63), ("sizes", 64), ("empty", 0), ("outer", 0),
          ("trunc", 0), ("wrap", 0)]
DTYPES = ("f64", "f32")


@functools.lru_cache(maxsize=None)
def build(kind, arg, dtype):
    """The scene (kind, arg): the first seed from 9000 + 100 * (index of the scene) on that meets every condition."""
    base = 9000 + 100 * SCENES.index((kind, arg)) + (50 if dtype == "f32" else 0)
    for seed in range(base, base + 50):
        sc = BUILDERS[kind](seed, dtype) if kind in ("pairs",) else BUILDERS[kind](seed, dtype, arg)
        if sc is not None:
            sc.update(name=f"{kind}{arg}-{dtype}", seed=seed, dtype=dtype)
            return sc
    raise AssertionError(f"no admissible seed for {kind} {arg} {dtype}")


# ---- designed hypotheses for joint_nis --------------------------------------------------------------------------------------------
NIS_N = (1, 31, 32, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def nis_state(N, dtype):
    rng = np.random.default_rng(9900 + N)
    x, P = ring_state(rng, N, dtype)
    xt = true_state(x, P, rng)
    return x, P, xt


def nis_cases(N, dtype):
    """[(name, ids)] for a map of N landmarks: single pairs, a pair on each side of a tile edge and the landmark that straddles it
    (1-based 63 for fp32, 31 for fp64: its two coordinates are the last row of one tile and the first of the next), ids ascending
    and descending, m = 64."""
    s = 63 if dtype == "f32" else 31
    cases = [("first", [1]), ("last", [N])]
    if N >= 2:
        cases += [("asc2", [1, N]), ("desc2", [N, 1])]
    if N > s:
        cases += [("straddler", [s]), ("across", [s - 1, s + 1]), ("across_desc", [s + 1, s - 1]), ("with_straddler", [s + 1, s, s - 1, 1]),
                  ("straddler_first", [s, N, 2])]
    if N >= 8:
        asc = list(range(N - 7, N + 1))
        cases += [("asc8", asc), ("desc8", asc[::-1])]
    if N >= 64:
        rng = np.random.default_rng(N)
        cases += [("m64", rng.permutation(np.arange(1, N + 1))[:64].tolist()), ("m64_asc", list(range(N - 63, N + 1)))]
    return cases
