"""Seeded data-association scenes that are HARD for the gating (csrc/ekf_gate.hip), shared by tests/test_assoc_scenes.py
(CPU: each scene is as hard as it claims, by the oracle alone) and tests/test_gpu_ekf_association.py (the three forms of
the device gating against the oracle on exactly these numbers).  NumPy and the oracle only.

Every builder takes `dtype` ("f64" / "f32") and returns a state ALREADY ROUNDED as the device will hold it; observations are
built from that rounded state and are always fp64 (the ABI takes them as doubles).  A scene is a dict:
    x, P        the state (float64 arrays holding dtype-representable values, P exactly symmetric)
    z           2 x nz observations (rows range, bearing)
    want        the oracle's decision vector for (x, P, z): j >= 1 matched, 0 dropped, -1 new
    pairs       [(observation, landmark 1-based, target nis)] for the observations placed at a prescribed nis
    group       per landmark the lowest 0-based index of its exact copies (itself when it has none)
    + per-builder fields (cases, dec_ids, tie_obs, intended, selective, ...)

MARGIN.  DELTA = 1e-7: every (observation, landmark) pair of every scene is DELTA, less the placement error, away (relative)
from gate1 and gate2 in the oracle's table: the pairs placed AT gate * (1 -+ DELTA) sit there to PLACED = 1e-10 relative (see
`verify`), so what `row_margin_ok` asserts on every pair is DELTA * (1 - 1e-3).  The best and the second-best candidate of an observation differ in nd by 1e-9 * max(1, |nd|) unless they are exact copies
of each other.  DELTA is 100 x the fp64 value tolerance the device is held to (1e-9, tests/test_gpu_ekf.py: TOL), so a
device that meets that tolerance cannot flip a decision, and 1e8 x the 5e-16 by which the oracle's formula and the device's
qa, qb, qc form of nis differ in fp64.  An observation whose drawn direction puts ANOTHER landmark nearer than that to a
gate, or two candidates nearer than that to each other, is drawn again.
"""
import functools
import math

import numpy as np

from oracle import ekf_ref as O

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
GATE1, GATE2 = 4.0, 25.0
DELTA = 1e-7
PLACED = 1e-10                    # a placed pair's nis against its target (relative): rounding of zp + t u, measured 1e-13
ND_GAP = 1e-9
EDGE_TARGETS = (GATE1 * (1 - DELTA), GATE1 * (1 + DELTA), GATE2 * (1 - DELTA), GATE2 * (1 + DELTA), 1.0, 9.0, 30.0)
NP_DTYPE = {"f64": np.float64, "f32": np.float32}

PARTITION_N = (1, 63, 64, 65, 127, 128, 129, 513)
PARTITION_NZ = (1, 7, 8, 9, 127, 128, 129, 257)


# ---- state helpers -----------------------------------------------------------------------------------------------------
def round_state(x, P, dtype):
    """(x, P) as a device of `dtype` holds them, back in float64; P exactly symmetric."""
    t = NP_DTYPE[dtype]
    P = (np.asarray(P, dtype=np.float64) + np.asarray(P, dtype=np.float64).T) / 2
    P = np.tril(P) + np.tril(P, -1).T
    return np.asarray(x, dtype=np.float64).astype(t).astype(np.float64), P.astype(t).astype(np.float64)


def scaled_cov(rng, N, d_xy, d_phi, d_lo, d_hi, rank=6):
    """P = D (A A' + 0.01 I) D: positive definite, strongly correlated (rank-6 factor), per-landmark scale D log-uniform
    in [d_lo, d_hi] (the same for a landmark's two coordinates)."""
    n = 3 + 2 * N
    A = rng.normal(0, 0.2, (n, rank))
    M = A @ A.T + 0.01 * np.eye(n)
    d_lm = np.exp(rng.uniform(math.log(d_lo), math.log(d_hi), N))
    D = np.concatenate([[d_xy, d_xy, d_phi], np.repeat(d_lm, 2)])
    return D[:, None] * M * D[None, :]


def copy_landmarks(x, P, src):
    """Landmark j (0-based) becomes an exact copy of landmark src[j]: same mean, same rows and columns of P (P -> E P E':
    positive semi-definite).  Such a state is for association only, never for an update."""
    src = np.asarray(src)
    idx = np.concatenate([[0, 1, 2], np.stack([3 + 2 * src, 4 + 2 * src], axis=1).reshape(-1)])
    return x[idx].copy(), P[np.ix_(idx, idx)].copy()


# ---- margins -----------------------------------------------------------------------------------------------------------
def row_margin_ok(nis, nd, group):
    """One observation's row of the oracle's table: every pair DELTA away from both gates, the best candidate ND_GAP away
    from every candidate that is not an exact copy of it (exact copies must tie bit for bit)."""
    fin = nis[~np.isnan(nis)]
    tol = DELTA * (1 - 1e-3)              # a pair placed at gate (1 -+ DELTA) sits there to PLACED = 1e-3 DELTA
    for g in (GATE1, GATE2):
        if np.any(np.abs(fin / g - 1.0) < tol):
            return False
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero((nis < GATE1) & (nd < math.inf))
    if len(cand) >= 2:
        b = cand[np.argmin(nd[cand])]
        for j in cand:
            if j == b:
                continue
            if group[j] == group[b]:
                if nd[j] != nd[b]:
                    return False
            elif nd[j] - nd[b] < ND_GAP * max(1.0, abs(nd[b])):
                return False
    return True


def edge_obs(x, P, ids, targets, rng, group=None, dirs=None, alone=False, strict=True):
    """One observation per landmark of `ids` (1-based) at a prescribed nis:  z = zp + t u,  t = sqrt(target / (u' inv(S) u)),
    u a random direction in (range, bearing) space -- or dirs[i] where that is not None.  The direction is drawn again when
    the row misses the margin (module docstring) or, with alone=True, when ANOTHER landmark that is no copy of the target
    comes within gate2 (1 + DELTA) of the observation.  Returns z (2 x len(ids)); with strict=False an observation whose FIXED
    direction misses the margin is returned as NaN (the caller leaves it out) instead of failing."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    N = (len(x) - 3) // 2
    group = np.arange(N) if group is None else group
    zp, S = O._landmark_S(x, P, R, ids)
    Si = np.linalg.inv(S)
    z = np.zeros((2, len(ids)))
    for i, (j, target) in enumerate(zip(ids, targets)):
        for _try in range(400):
            if dirs is not None and dirs[i] is not None:
                u = np.asarray(dirs[i], dtype=np.float64)
            else:
                a = rng.uniform(0, 2 * math.pi)
                # (bearing innovations are ~100 x smaller than range ones: scale u so both components matter)
                u = np.array([math.cos(a) * math.sqrt(S[i, 0, 0]), math.sin(a) * math.sqrt(S[i, 1, 1])])
            t = math.sqrt(target / float(u @ Si[i] @ u))
            zi = zp[i] + t * u
            nis, nd = O.association_table_sparse(x, P, zi.reshape(2, 1), R)
            ok = row_margin_ok(nis[0], nd[0], group) and (target == 0.0 or abs(nis[0, j - 1] / target - 1.0) <= PLACED)
            if ok and alone:
                others = group != group[j - 1]
                with np.errstate(invalid="ignore"):
                    ok = not np.any(nis[0, others] <= GATE2 * (1 + DELTA))
            if ok:
                break
            if dirs is not None and dirs[i] is not None:
                assert not strict, f"observation {i} of landmark {j}: the fixed direction misses the margin"
                zi = np.array([math.nan, math.nan])
                break
        else:
            raise AssertionError(f"no admissible direction for observation {i} of landmark {j}")
        z[:, i] = zi
    return z


def verify(scene):
    """The builder's closing assertion on the oracle's whole table; fills `want`."""
    x, P, z = scene["x"], scene["P"], scene["z"]
    N = (len(x) - 3) // 2
    scene.setdefault("group", np.arange(N))
    scene.setdefault("pairs", [])
    assert np.array_equal(P, P.T)
    nis, nd = O.association_table_sparse(x, P, z, R)
    for i in range(z.shape[1]):
        assert row_margin_ok(nis[i], nd[i], scene["group"]), f"{scene['name']}: observation {i} misses the margin"
    for i, j, target in scene["pairs"]:
        assert abs(nis[i, j - 1] / target - 1.0) <= PLACED, (scene["name"], i, j, target, nis[i, j - 1])
    scene["want"] = O.assoc_vector(nis, nd, GATE1, GATE2)
    scene["N"] = N
    return scene


def _scene(name, dtype, x, P, **kw):
    return dict(name=f"{name}-{dtype}", dtype=dtype, x=x, P=P, **kw)


# ---- the cluster scene -------------------------------------------------------------------------------------------------
N_CLUSTERS, PER_CLUSTER, N_ISOLATED, CLUSTER_NZ = 40, 16, 16, 96
ISOLATED_TARGETS = (GATE2 * (1 + DELTA), GATE2 * (1 - DELTA), 30.0, GATE1 * (1 + DELTA))


def cluster_state(seed, dtype):
    """656 landmarks: 40 clusters of 16 (sigma 1.5 m) within 100 m of the pose plus 16 isolated ones on a ring at 220 m
    (55 m apart, a bearing sigma of 1 degree is 4 m there: nothing else within gate2), the landmark order shuffled;
    landmark sigmas 0.15 .. 1.2 m (a 60 x range of variances), comparable with the spacing inside a cluster.
    Returns x, P, isolated (1-based ids) and the generator, for the scene's draw of observations."""
    rng = np.random.default_rng(seed)
    N = N_CLUSTERS * PER_CLUSTER + N_ISOLATED
    pose = np.array([50.0, 50.0, rng.uniform(-3, 3)])
    centres = pose[:2] + rng.uniform(-100, 100, (N_CLUSTERS, 2))
    pts = (centres[:, None, :] + rng.normal(0, 1.5, (N_CLUSTERS, PER_CLUSTER, 2))).reshape(-1, 2)
    ang = rng.uniform(0, 2 * math.pi) + 0.25 * np.arange(N_ISOLATED)
    iso = pose[:2] + 220.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    order = rng.permutation(N)
    allp = np.vstack([pts, iso])[order]
    isolated = np.flatnonzero(order >= N_CLUSTERS * PER_CLUSTER) + 1
    x = np.concatenate([pose, allp.reshape(-1)])
    d_lo = 0.3
    P = scaled_cov(rng, N, 0.2, 0.01, d_lo, d_lo * math.sqrt(60.0))
    x, P = round_state(x, P, dtype)
    return x, P, isolated, rng


def cluster_draw(x, P, isolated, rng, nz=CLUSTER_NZ, twice=False):
    """96 edge observations: 80 of clustered landmarks, the targets cycling through EDGE_TARGETS, and 16 of the isolated
    ones cycling through ISOLATED_TARGETS (the outer gate decides those: new / dropped); order shuffled."""
    N = (len(x) - 3) // 2
    clustered = np.setdiff1d(np.arange(1, N + 1), isolated)
    n_iso = min(len(isolated), N_ISOLATED)
    n_cl = nz - n_iso
    n_rep = 16 if twice else 0              # twice: 16 landmarks observed twice each, inside the inner gate (duplicate ids)
    pick = rng.choice(clustered, n_cl - n_rep, replace=False)
    ids = np.concatenate([np.repeat(pick[:n_rep], 2), pick[n_rep:], isolated[:n_iso]])
    inner = (1.0, GATE1 * (1 - DELTA), 3.0, 0.5)
    targets = [inner[i % 4] for i in range(2 * n_rep)] + [EDGE_TARGETS[i % len(EDGE_TARGETS)] for i in range(n_cl - 2 * n_rep)] + \
              [ISOLATED_TARGETS[i % len(ISOLATED_TARGETS)] for i in range(n_iso)]
    perm = rng.permutation(nz)
    ids, targets = ids[perm], [targets[p] for p in perm]
    z = edge_obs(x, P, ids, targets, rng)
    return z, [(i, int(j), t) for i, (j, t) in enumerate(zip(ids, targets))]


@functools.lru_cache(maxsize=None)
def cluster_scene(seed, dtype, twice=False):
    """twice=True: 16 of the clustered landmarks are observed twice each, inside the inner gate, and 48 once at the edge
    targets (observe() then updates with many duplicate ids)."""
    x, P, isolated, rng = cluster_state(seed, dtype)
    z, pairs = cluster_draw(x, P, isolated, rng, twice=twice)
    return verify(_scene(f"cluster{seed}{'x2' if twice else ''}", dtype, x, P, z=z, pairs=pairs, isolated=isolated, selective=False))


# ---- exact copies and near-ties ----------------------------------------------------------------------------------------
def _sparse_state(rng, N, spread, scale=0.01):
    """Landmarks `spread` metres across with sigma ~0.05 m: far apart compared with every gate."""
    n = 3 + 2 * N
    x = np.concatenate([[50.0, 50.0, rng.uniform(-3, 3)], rng.uniform(50 - spread / 2, 50 + spread / 2, 2 * N)])
    A = rng.normal(0, 0.2, (n, 6))
    return x, scale * (A @ A.T + 0.01 * np.eye(n))


# (lower, higher) 0-based landmark indices; N = 327 = 5 workgroups of 64 + a ragged one of 7
COPY_N = 327
COPY_PAIRS = ((3, 4),          # one wave, neighbours
              (64, 127),       # one wave, lanes 0 and 63
              (10, 74),        # neighbouring workgroups, the same lane
              (20, 212),       # three workgroups apart
              (130, 258),      # two workgroups apart
              (30, 322),       # into the ragged last workgroup
              (321, 325),      # both inside the ragged last workgroup
              (191, 320))      # last lane of a full workgroup and first lane of the ragged one


@functools.lru_cache(maxsize=None)
def copies_scene(kind, dtype):
    """kind "placed": COPY_PAIRS, each pair observed three times (nis 0.5, 3 and gate1 (1 - DELTA) of both copies): exact
    ties in nd that the lower landmark wins, plus a dropped and a new observation per pair.
    kind "all" / "all_small": N = 64 k + 1 identical landmarks (k = 6 / 2): every workgroup appends one equal entry to
    every matched observation's list; the fold has to pick landmark 1.
    kind "near": the lower landmark of each pair has its 2 x 2 block inflated by 1e-6, so the pair differs in log det S
    alone at v = 0 and the HIGHER landmark wins."""
    rng = np.random.default_rng({"placed": 301, "all": 302, "all_small": 303, "near": 304}[kind])
    if kind in ("all", "all_small"):
        N = 64 * (6 if kind == "all" else 2) + 1
        x, P = _sparse_state(rng, 1, 60.0)
        x, P = copy_landmarks(x, P, np.zeros(N, dtype=np.int64))
        x, P = round_state(x, P, dtype)
        group = np.zeros(N, dtype=np.int64)
        ids = [1 + (i * 64) % N for i in range(10)]                    # the target's index must not matter
        targets = [0.5, 1.0, 3.0, GATE1 * (1 - DELTA), GATE1 * (1 + DELTA), 9.0, GATE2 * (1 - DELTA), GATE2 * (1 + DELTA), 30.0, 2.0]
        z = edge_obs(x, P, ids, targets, rng, group=group)
        return verify(_scene(f"copies_{kind}", dtype, x, P, z=z, group=group, selective=False,
                             pairs=[(i, j, t) for i, (j, t) in enumerate(zip(ids, targets))], tie_obs=[0, 1, 2, 3, 9]))
    N = COPY_N
    x, P = _sparse_state(rng, N, 600.0)
    src = np.arange(N)
    for lo, hi in COPY_PAIRS:
        src[hi] = lo
    x, P = copy_landmarks(x, P, src)
    group = src.copy()
    if kind == "near":
        for lo, hi in COPY_PAIRS:
            f = 3 + 2 * lo
            P[f:f + 2, f:f + 2] *= 1.0 + 1e-6                       # P + a positive semi-definite block
        group = np.arange(N)
    x, P = round_state(x, P, dtype)
    ids, targets, dirs = [], [], []
    for lo, hi in COPY_PAIRS:
        if kind == "near":
            ids += [hi + 1, lo + 1]; targets += [0.0, 0.5]; dirs += [(1.0, 0.0), None]      # v = 0, and nis = 0.5
        else:
            ids += [hi + 1, lo + 1, hi + 1, lo + 1, hi + 1]
            targets += [0.5, 3.0, GATE1 * (1 - DELTA), 9.0, 30.0]
            dirs += [None] * 5
    z = edge_obs(x, P, ids, targets, rng, group=group, dirs=dirs)
    pairs = [(i, j, t) for i, (j, t) in enumerate(zip(ids, targets)) if t > 0.0]
    return verify(_scene(f"copies_{kind}", dtype, x, P, z=z, group=group, pairs=pairs, selective=False, obs_ids=ids))


# ---- the grid's reach --------------------------------------------------------------------------------------------------
def grid_geometry(xb):
    """Host mirror of grid_prepare_kernel (ekf_gate.hip): G, origin and cell edges from the means at build time."""
    N = (len(xb) - 3) // 2
    lx, ly = xb[3::2], xb[4::2]
    G = min(128, max(4, int(math.sqrt(N / 4.0))))
    scale = max(abs(lx.min()), abs(lx.max()), abs(ly.min()), abs(ly.max()))
    tiny = max(1e-9, 1e-12 * scale)
    cw = [(lx.max() - lx.min()) / G, (ly.max() - ly.min()) / G]
    cw = [c if c > tiny else max(1.0, tiny) for c in cw]
    return dict(G=G, x0=lx.min(), y0=ly.min(), cwx=cw[0], cwy=cw[1])


def _arc_has(a, b, t):
    return t + 2 * math.pi * math.ceil((a - t) / (2 * math.pi)) <= b


def _cell(p, p0, cw, G):
    t = math.floor((p - p0) * (1.0 / cw))
    return G - 1 if t >= G - 1 else (int(t) if t > 0 else 0)


def grid_reach(x, P, z, geo, drift=0.0, beta_scale=1.0, arcs=(True, True, True, True), use_drift=True):
    """Host mirror of the reach of ONE observation in gate_grid_kernel, from the header's formulas: rho, beta, th, the arc
    [a, b], the box in cells and the annulus [d_lo, d_hi] on build-time distances.  It restates the block of
    csrc/ekf_gate.hip that begins "the reach of this observation" (lines 589-628, with arc_has at 524-528 and grid_coord at
    398-402; grid_geometry restates grid_prepare_kernel, 441-473): a change to either side has to be made on the other.  beta_scale, arcs (whether arc_has is
    consulted for 0, pi, pi/2, -pi/2) and use_drift (the drift term of d_hi) restate what a WRONG kernel would do, so that
    the CPU tests can show that a scene tells the difference."""
    G = geo["G"]
    pvv = P[0:3, 0:3]
    pmax = max(float(np.max(np.diag(P)[3:])), 0.0) if len(x) > 3 else 0.0
    A0 = math.sqrt(max(pvv[0, 0], 0) + max(pvv[1, 1], 0)) + math.sqrt(2 * pmax)
    sp = math.sqrt(max(pvv[2, 2], 0))
    rho = math.sqrt(GATE2 * (A0 * A0 + R[0, 0])) * (1 + 1e-6) + 1e-9
    dmax, dmin = z[0] + rho, max(z[0] - rho, 0.0)
    out = dict(rho=rho, beta=math.inf, th=z[1] + x[2], a=-math.inf, b=math.inf, empty=False, whole_annulus=True)
    if dmax < 0:
        out.update(empty=True, box=(1, 0, 0, G - 1), d_lo=math.inf, d_hi=-math.inf)
        return out
    cmin, cmax, smin, smax = -1.0, 1.0, -1.0, 1.0
    if dmin > 0:
        beta = (math.sqrt(GATE2 * ((A0 / dmin + sp) ** 2 + R[1, 1])) * (1 + 1e-6) + 1e-9) * beta_scale
        out["beta"] = beta
        if beta < math.pi:
            a, b = out["th"] - beta, out["th"] + beta
            out.update(a=a, b=b, whole_annulus=False)
            ca, cb, sa, sb = math.cos(a), math.cos(b), math.sin(a), math.sin(b)
            cmax = 1.0 if arcs[0] and _arc_has(a, b, 0.0) else max(ca, cb)
            cmin = -1.0 if arcs[1] and _arc_has(a, b, math.pi) else min(ca, cb)
            smax = 1.0 if arcs[2] and _arc_has(a, b, 0.5 * math.pi) else max(sa, sb)
            smin = -1.0 if arcs[3] and _arc_has(a, b, -0.5 * math.pi) else min(sa, sb)
    eps = 1e-9 * (dmax + abs(x[0]) + abs(x[1]) + 1.0)
    pad = drift + eps
    xlo, xhi = min(cmin * dmax, cmin * dmin), max(cmax * dmax, cmax * dmin)
    ylo, yhi = min(smin * dmax, smin * dmin), max(smax * dmax, smax * dmin)
    out["box"] = (_cell(x[0] + xlo - pad, geo["x0"], geo["cwx"], G), _cell(x[0] + xhi + pad, geo["x0"], geo["cwx"], G),
                  _cell(x[1] + ylo - pad, geo["y0"], geo["cwy"], G), _cell(x[1] + yhi + pad, geo["y0"], geo["cwy"], G))
    out["d_lo"] = dmin - math.sqrt(2) * drift - eps
    out["d_hi"] = dmax + (math.sqrt(2) * drift if use_drift else 0.0) + eps
    return out


def reach_sees(reach, pose_now, xb, j, geo):
    """Would the grid query with this reach evaluate landmark j (1-based), whose mean at build time is in xb?"""
    if reach["empty"]:
        return False
    bx, by = xb[3 + 2 * (j - 1)], xb[4 + 2 * (j - 1)]
    cx, cy = _cell(bx, geo["x0"], geo["cwx"], geo["G"]), _cell(by, geo["y0"], geo["cwy"], geo["G"])
    cx0, cx1, cy0, cy1 = reach["box"]
    db = math.hypot(bx - pose_now[0], by - pose_now[1])
    return cx0 <= cx <= cx1 and cy0 <= cy <= cy1 and reach["d_lo"] <= db <= reach["d_hi"]


REACH_N = 1000
# global direction of the deciding landmarks seen from the pose: the four axes, both sides of the +-pi cut, two diagonals
REACH_ANGLES = (0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi - 0.04, -math.pi + 0.04, math.pi / 4, -3 * math.pi / 4)


def _rim_cases(k):
    """(tag, target nis, direction, alone) for deciding landmark k: the rim of the sector on both sides, the rim of the
    annulus on both sides, just outside the outer gate, the inner gate, a plain match."""
    s = 1.0 if k % 2 == 0 else -1.0
    return (("sector_rim", GATE2 * (1 - DELTA), (0.0, s), True), ("sector_rim", GATE2 * (1 - DELTA), (0.0, -s), True),
            ("annulus_rim", GATE2 * (1 - DELTA), (s, 0.0), True), ("annulus_rim", GATE2 * (1 - DELTA), (-s, 0.0), True),
            ("outside", GATE2 * (1 + DELTA), (0.0, s), True), ("inner_edge", GATE1 * (1 - DELTA), None, False),
            ("match", 1.0, None, False))


@functools.lru_cache(maxsize=None)
def reach_scene(kind, dtype):
    """kind "inside": the pose in the middle of 1000 landmarks over 800 m, heading sigma 0.06 rad, position and landmark
    sigmas of centimetres (the grid is selective).  Eight deciding landmarks 200-300 m out in the directions REACH_ANGLES,
    each observed at nis = gate2 (1 - DELTA) along the bearing (it then lies ~0.3 rad = 60-90 m sideways of the
    observation's ray, on the rim of the sector) and along the range (the rim of the annulus); one landmark 0.25 m from the
    pose for r <= rho and for a negative range; ranges beyond every landmark; a bearing given as b + 2 pi.
    kind "outside": the pose 300 m west of the landmarks' bounding box.   kind "huge": "inside" with one landmark of
    sigma ~25 m -- the variance bound is useless and the grid may visit everything (decisions only)."""
    rng = np.random.default_rng({"inside": 401, "outside": 402, "huge": 403}[kind])
    N = REACH_N
    outside = kind == "outside"
    pose = np.array([50.0, 50.0, 2.5])
    angles = (0.0, 0.8, -0.8, 0.4, -0.4) if outside else REACH_ANGLES      # outside: all towards the map
    K = len(angles)
    near = 0 if outside else 1
    radii = 200.0 + (rng.permutation(K) + rng.uniform(0.2, 0.8, K)) * (100.0 / K)      # 200-300 m, no two alike
    dec = pose[:2] + radii[:, None] * np.stack([np.cos(angles), np.sin(angles)], axis=1)
    lo = np.array([350.0, -350.0]) if outside else np.array([-350.0, -350.0])
    bg = pose[:2] + lo + rng.uniform(0, 700, (N - K - near, 2))
    if not outside:
        # The four landmarks ON the axes sit 4 m beyond a cell boundary of the grid (the cells follow from the bounding box
        # of the background): the box of an observation that looks straight at one reaches its cell only because the arc
        # th +- beta CONTAINS the axis (cos or sin = +-1 there, ~0.95 at the arc's ends: 10-14 m less at this range).
        geo = grid_geometry(np.concatenate([pose, bg.reshape(-1)]))
        for k, (ax, sgn) in enumerate(((0, 1.0), (1, 1.0), (1, -1.0), (0, -1.0))):
            along = math.cos(angles[k]) if ax == 0 else math.sin(angles[k])
            assert along == sgn, "REACH_ANGLES[0..3] are the four axes"
            p0, cw = (geo["x0"], geo["cwx"]) if ax == 0 else (geo["y0"], geo["cwy"])
            want = pose[ax] + sgn * radii[k]
            m = math.ceil((want - p0) / cw) if sgn > 0 else math.floor((want - p0) / cw)
            dec[k, ax] = p0 + m * cw + sgn * 4.0
            dec[k, 1 - ax] = pose[1 - ax]
    pts = np.vstack([dec, pose[:2] + np.array([[0.25 * math.cos(1.0), 0.25 * math.sin(1.0)]])[:near], bg])
    P = scaled_cov(rng, N, 0.1, 0.12, 0.04, 0.08)
    # a landmark exactly at the pose (d = 0) has no finite innovation covariance in the oracle (0 / 0 in the Jacobian):
    # such a landmark is left out of every scene
    with np.errstate(all="ignore"):
        x0 = np.concatenate([pose, pose[:2]])
        _, S0 = O._landmark_S(x0, P[:5, :5], R, [1])
    d0_finite = bool(np.all(np.isfinite(S0)))
    # shuffle the landmark order; ids of the deciding landmarks and of the one next to the pose
    order = rng.permutation(N)
    pts_s = pts[order]
    inv = np.empty(N, dtype=np.int64)
    inv[order] = np.arange(N)
    dec_ids, near_id = inv[:K] + 1, (int(inv[K]) + 1 if near else None)
    if kind == "huge":                      # the last background landmark, in the far corner of the map: sigma ~25 m
        pts_s[inv[N - 1]] = pose[:2] + 345.0
        f = 3 + 2 * int(inv[N - 1])
        P[f:f + 2, :] *= 800.0
        P[:, f:f + 2] *= 800.0
    for _round in range(50):
        x = np.concatenate([pose, pts_s.reshape(-1)])
        xr, Pr = round_state(x, P, dtype)
        ids, targets, dirs, alone, cases = [], [], [], [], []
        for k in range(K):
            for tag, t, u, al in _rim_cases(k):
                ids.append(int(dec_ids[k])); targets.append(t); dirs.append(u); alone.append(al); cases.append(f"{tag}:{k}")
        # the rim observations are fixed by their landmark alone: move every background landmark that comes near one
        zp, S = O._landmark_S(xr, Pr, R, ids)
        Si = np.linalg.inv(S)
        zfix = np.zeros((2, len(ids)))
        for i, u in enumerate(dirs):
            u = np.array(u if u is not None else (0.0, 0.0))
            if dirs[i] is not None:
                zfix[:, i] = zp[i] + math.sqrt(targets[i] / float(u @ Si[i] @ u)) * u
            else:
                zfix[:, i] = zp[i]
        nis, _ = O.association_table_sparse(xr, Pr, zfix, R)
        with np.errstate(invalid="ignore"):
            close = nis <= GATE2 * 1.5
        close[np.arange(len(ids)), np.asarray(ids) - 1] = False
        bad = np.unique(np.nonzero(close)[1])
        if len(bad) == 0:
            break
        assert not set(bad + 1) & set(int(d) for d in dec_ids), "two deciding landmarks within reach of each other"
        pts_s[bad] = pose[:2] + lo + rng.uniform(0, 700, (len(bad), 2))
    else:
        raise AssertionError("the background keeps crowding the deciding landmarks")
    x, P = xr, Pr
    z = edge_obs(x, P, ids, targets, rng, dirs=dirs)
    for i, al in enumerate(alone):                                   # "alone": the deciding landmark is the only one within gate2
        if al:
            row, _ = O.association_table_sparse(x, P, z[:, i:i + 1], R)
            row[0, ids[i] - 1] = math.inf
            assert not np.any(row[0] <= GATE2 * (1 + DELTA)), cases[i]
    pairs = [(i, j, t) for i, (j, t) in enumerate(zip(ids, targets))]
    extra, extra_cases = [], []
    i_un = cases.index("match:0")
    extra.append(z[:, i_un] + [0.0, 2 * math.pi]); extra_cases.append("unwrapped")
    extra.append(z[:, cases.index("sector_rim:3" if not outside else "sector_rim:1")] - [0.0, 2 * math.pi]); extra_cases.append("unwrapped_rim")
    for r, b in ((5000.0, 0.3), (1200.0, -2.0), (1e5, 3.0)):
        extra.append(np.array([r, b])); extra_cases.append("beyond")
    extra.append(np.array([-5.0, 0.3])); extra_cases.append("negative_far")
    if near:
        zn = edge_obs(x, P, [near_id, near_id], [1.0, 16.0], rng, dirs=[None, (-1.0, 0.0)])
        assert zn[0, 1] < 0.0, zn
        pairs += [(len(ids) + len(extra), near_id, 1.0), (len(ids) + len(extra) + 1, near_id, 16.0)]
        extra += [zn[:, 0], zn[:, 1]]; extra_cases += ["r_le_rho", "negative_near"]
    z = np.hstack([z, np.array(extra).T])
    return verify(_scene(f"reach_{kind}", dtype, x, P, z=z, pairs=pairs, cases=cases + extra_cases, dec_ids=dec_ids,
                         near_id=near_id, selective=kind != "huge", d0_finite=d0_finite, obs_ids=ids))


def reach_update_inputs(scene):
    """An update of 16 known landmarks for the "inside" reach scene that MOVES means by decimetres (an update is not gated):
    every deciding landmark is seen 8 m nearer than predicted, eight background ones at their prediction.  (z, ids)."""
    rng = np.random.default_rng(411)
    others = np.setdiff1d(np.arange(1, scene["N"] + 1), list(scene["dec_ids"]) + [scene["near_id"]])
    ids = np.concatenate([scene["dec_ids"], rng.choice(others, 16 - len(scene["dec_ids"]), replace=False)])
    zp, _ = O._landmark_S(scene["x"], scene["P"], R, ids)
    z = zp.T.copy()
    z[0, :len(scene["dec_ids"])] -= 8.0
    return z, ids


def reach_rim_after(x, P, dec_ids, seed=412):
    """From a LATER state: every deciding landmark on the outer and on the inner rim of the annulus (nis = gate2 (1 - DELTA)
    along the range), alone within gate2.  (z, ids); an observation that misses the margin in this state is left out."""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.asarray(dec_ids), 2)
    dirs = [(-1.0, 0.0), (1.0, 0.0)] * len(dec_ids)
    z = edge_obs(x, P, ids, [GATE2 * (1 - DELTA)] * len(ids), rng, dirs=dirs, alone=True, strict=False)
    keep = ~np.isnan(z[0])
    return z[:, keep], ids[keep]


# ---- the sweep's partition ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def partition_state(N, dtype):
    rng = np.random.default_rng(500 + N)
    spread = 40.0 * math.sqrt(N) + 40.0
    x, P = _sparse_state(rng, N, spread)
    for _round in range(100):                      # no landmark within nis 150 of another one's predicted observation
        xr, Pr = round_state(x, P, dtype)
        zp, _ = O._landmark_S(xr, Pr, R, np.arange(1, N + 1))
        nis, _ = O.association_table_sparse(xr, Pr, zp.T, R)
        np.fill_diagonal(nis, math.inf)
        crowd = np.unique(np.nonzero(nis <= 150.0)[1])
        if len(crowd) == 0:
            return xr, Pr
        for j in crowd:
            x[3 + 2 * j:5 + 2 * j] = rng.uniform(50 - spread / 2, 50 + spread / 2, 2)
    raise AssertionError("the partition map stays crowded")


@functools.lru_cache(maxsize=None)
def partition_cells(N, nz, dtype):
    """nz observations over N well-separated landmarks: the first and the last landmark (the last is alone in a ragged
    last workgroup when N = 64 k + 1) are matched first, then random landmarks, with nis 1 (matched), 10 (dropped) and
    30 (new) in turn; no other landmark within gate2, so `intended` is known without the oracle."""
    x, P = partition_state(N, dtype)
    rng = np.random.default_rng(1000 * N + nz)
    ids = np.concatenate([[1, N], rng.integers(1, N + 1, max(nz - 2, 0))])[:nz]
    targets = np.array([1.0, 1.0] + [(1.0, 10.0, 30.0, 3.0)[i % 4] for i in range(max(nz - 2, 0))])[:nz]
    perm = rng.permutation(nz)
    ids, targets = ids[perm], targets[perm]
    z = edge_obs(x, P, ids, targets, rng, alone=True)
    intended = np.where(targets < GATE1, ids, np.where(targets < GATE2, 0, -1)).astype(np.int32)
    return verify(_scene(f"partition{N}x{nz}", dtype, x, P, z=z, intended=intended, selective=False,
                         pairs=[(i, int(j), float(t)) for i, (j, t) in enumerate(zip(ids, targets))]))


# ---- what the GPU test walks through -----------------------------------------------------------------------------------
CLUSTER_SEEDS = (11, 12, 13)
SCENES = [("cluster", s) for s in CLUSTER_SEEDS] + [("copies", k) for k in ("placed", "all", "all_small", "near")] + \
         [("reach", k) for k in ("inside", "outside", "huge")]


def build(which, arg, dtype):
    return {"cluster": cluster_scene, "copies": copies_scene, "reach": reach_scene}[which](arg, dtype)
