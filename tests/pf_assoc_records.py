"""Designed per-particle maps for the association with unknown correspondences of the FastSLAM path (pf_update_unknown_kernel in
csrc/pf_legacy.hip, the fused pf_step_unknown_kernel in csrc/pf_unknown.hip), with a longdouble restatement of the rule, per-pair
rounding scales, admissible decision sets, a replay of the updates and planted defects.  NumPy and the oracle only; shared by
tests/test_pf_assoc_records_cpu.py (CPU: the table is what it claims, the margins follow their rule, the comparison rejects the
planted defects) and tests/test_gpu_pf_assoc_records.py (the kernels on exactly these numbers).

WHY.  The scenes of tests/test_gpu_pf_unknown_step.py, tests/test_gpu_pf.py and tests/test_gpu_pf_wrap.py keep every NIS 1e-3
(relative) away from a gate and every pair of candidates 1e-3 apart, start from clear_landmarks with a tight cloud (every particle
the same slots in the same order, no holes), and allow fp32 0.1 % of disagreement.  Here every (particle, observation) pair is a
designed SITUATION at a designed distance from a gate or a rival, measured in units of that pair's OWN rounding bound, in maps
that differ from particle to particle; a pair whose decision the bounds leave open is allowed exactly the decisions the bounds
can reach, every other pair must equal the truth.  There is no agreement quota.

TABLE.  `table(dtype, which)`: N = 3019 particles (47 waves and 11 lanes, 11 workgroups and 203 lanes; the last particle is a
`full` one), each with its own pose (|x|, |y| <= 5 m, any heading) and its own map of NL = 71 slots (ragged for 2, 3 and 4
groups), every number rounded to the storage dtype first: device and reference share inputs bit for bit.  The M = 64 observations
are filter-wide.  They sit at 48 LOCATIONS on eight rings of six (ranges 10.3-49.8 m, the rings 5.64 m apart and staggered by
half a bearing step: at least 8 m between any two); 16 observations (DUP_OF) repeat an earlier one bit for bit.  (48, not 64: with the
suite's R one degree of bearing is 0.87 m at 50 m, and no more locations fit between 10 and 50 m if every foreign landmark is to
stay beyond 100 x gate2 -- which `case` asserts from the truth for every non-designed (observation, used slot) pair.)  A slot is
used iff Pxx >= 0.  Slots are dealt per particle from a random permutation, so used and unused slots interleave; most unused slots
hold the zeros of clear_landmarks, a `stale` one holds coordinates exactly on an observation with a stale positive Pyy.

  situation   slots   placed                                                        decision of the truth
  new         0       nothing near                                                  -1
  gate1_in    1       NIS = gate1 - k bound                                         the slot
  gate1_out   1       NIS = gate1 + k bound                                         -2
  gate2_in    1       NIS = gate2 - k bound                                         -2
  gate2_out   1       NIS = gate2 + k bound                                         -1
  rival       2       both well inside gate1, nd_A = nd_B - k (bound_A + bound_B);  A
                      A has the larger NIS and the smaller log det
  twin        2       two bit-identical records inside gate1                        the lower slot, exactly
  stale       1       an unused slot exactly on the observation                     -1
 and as attributes of a pair: `dup` (the observation repeats an earlier one and both match the same landmark), `wrapped`
 (z_b - zp1 beyond +-pi before the wrap: a matter of the particle's heading), `full` (a particle with fewer unused slots than
 observations that want one: the association still says -1, the late ones change no slot; FULL particles have 0-3 unused slots,
 the others filled with far landmarks).  EMPTY particles hold no landmark at all.

BANDS of k (per pair, by BANDS): `near` 1.5-3, `far` 10-30 (the two DECIDED classes, in units of the pair's bound in the
table's own dtype), `edge` below 0.25 of the pair's fp32 bound (in both tables: undecided for fp32, decided for fp64).
Placed coarsely through the landmark's coordinates (the innovation is chosen, the landmark follows), finely through ONE
covariance entry (Pxx or Pyy, whichever moves the score more) by a root search over the dtype's representable values: one
fp32 ulp of it moves NIS by about 1e-7, one ulp of a coordinate by 1e-5..1e-4.

TRUTH.  `truth(t, obs)` restates OraclePF.associate_unknown in np.longdouble: nis, nd per (observation, slot, particle) and the
used mask.  MODEL: `decide(T, ...)` is the same rule in the arithmetic of T with the library sqrt / atan2 / log, as the kernels
have it here (not m_atan2) -- the model of a correctly rounding device, not the truth.  The CPU test pins the float64 model to
OraclePF.associate_unknown itself (identical decisions, nis to 1e-12).

SCALES (`scales`), first order, from the truth's own intermediates; eps = the dtype's unit roundoff:
  dv0   = eps (|r| + 3 d + |x| + |lx| + |y| + |ly|),   dv1 = eps (|b| + 2 pi + |phi| + (|x| + |lx| + |y| + |ly|) / d)
  prod  = |qa v0 v0| + |qb v0 v1| + |qc v1 v1|,   cdet = (|s00 s11| + |s01 s10|) / |det|   (the inverse is explicit and S is not
          symmetrised: the cancellation in det = s00 s11 - s01 s10 reaches all three of qa, qb, qc)
  nis   : |2 qa v0 + qb v1| dv0 + |qb v0 + 2 qc v1| dv1 + eps (8 + 4 cdet) prod
  nd    : nis's + eps (|logdet| + |nd|) + 4 eps cdet
BOUNDS.  bound = margin x scale, MARGINS[dtype][class][quantity] = max(4, 4 x worst model error / scale) over the class's designed
pairs and both noise matrices (classes: gate1, gate2, rival, twin); committed, re-derived by the CPU test (`derive_margins`).
Nothing here comes from a device's output.

ADMISSIBLE SETS (`admissible`): the decisions reachable when each NIS moves by at most its bound and each nd by at most its bound.
Slot l MAY be a candidate if nis - b < gate1, MUST be one if nis + b < gate1; l is admissible if it may be a candidate and
nd_l - b_l <= min over must-candidates of (nd + b), never if a lower slot holds the same record bit for bit; -2 if there is no
must-candidate and some slot may satisfy nis <= gate2; -1 if there is no must-candidate and no slot must satisfy nis <= gate2.
A pair is DECIDED when the set is a singleton.

REPLAY (`replay`): given decisions, applied in observation order in longdouble with lm_records.reference (matched: the update of
that slot; -1: the first sighting in the particle's lowest unused slot at its turn, or nowhere), bounds per touched record from
lm_records.scales with REPLAY_MARGINS (lm_records' rule re-derived on these records), the log-weight increment with the
sum of its touches' bounds plus eps |log-weight| per addition.  A record touched twice (`dup`) has a rounded prior at its second
touch: the GPU test holds those at the suite's TOL.
"""
import functools
import math
import types

import numpy as np

import lm_records as L

LD = np.longdouble
NP_DTYPE, EPS, NOISES = L.NP_DTYPE, L.EPS, L.NOISES
GATE1, GATE2 = 4.0, 25.0                                    # exact in both dtypes
NL, N, M = 71, 3019, 64
assert N % 64 and N % 256 and all(NL % g for g in (2, 3, 4))
SEED = 20241019
FOREIGN_MIN = 100.0 * GATE2
RING0, RING_STEP, RINGS, PER_RING = 10.3, 5.64, 8, 6
# observation -> the earlier observation it repeats bit for bit
DUP_OF = {4: 1, 11: 7, 16: 15, 21: 3, 26: 18, 29: 20, 35: 34, 40: 9, 44: 32, 47: 46, 51: 0, 55: 30, 58: 48, 60: 22, 62: 49, 63: 12}
NLOC = M - len(DUP_OF)
assert NLOC == RINGS * PER_RING and all(s < d and s not in DUP_OF for d, s in DUP_OF.items())
BOUNDARY_OBS = (15, 16, 31, 32, 47, 48, 63)

SITS = ("new", "gate1_in", "gate1_out", "gate2_in", "gate2_out", "rival", "twin", "stale", "exact")
NEW, G1IN, G1OUT, G2IN, G2OUT, RIVAL, TWIN, STALE, EXACT = range(9)
CYCLE = (NEW, G1IN, G1OUT, G2IN, G2OUT, RIVAL, TWIN, STALE, G1IN, G2IN, G1OUT, G1IN)
BANDS = ("near", "far", "edge")
BAND_RANGE = {"near": (1.5, 3.0), "far": (10.0, 30.0), "edge": (0.0, 0.25)}
BAND_DRAW = {"near": (1.8, 2.7), "far": (12.0, 25.0), "edge": (0.03, 0.2)}
NORMAL, FULL, EMPTY, EXACTP = 0, 1, 2, 3
EXACT_V0 = {GATE2: 0.625, GATE1: 0.25}                      # range innovations whose NIS is the gate itself with S00 = 2^-6
CLASSES = ("gate1", "gate2", "rival", "twin")
CLASS_OF_SIT = {G1IN: 0, G1OUT: 0, G2IN: 1, G2OUT: 1, RIVAL: 2, TWIN: 3, EXACT: 1}
QUANT = ("nis", "nd")

# margin = max(4, 4 x worst model error / scale) (derive_margins; the CPU test checks it)
MARGINS = {
    "f32": {c: {"nis": 4.0, "nd": 4.0} for c in CLASSES},
    "f64": {c: {"nis": 4.0, "nd": 4.0} for c in CLASSES},
}
REPLAY_MARGINS = {
    "f32": {"mean": 8.0, "cov": 5.5, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
    "f64": {"mean": 8.5, "cov": 5.5, "inc": 4.0, "init_mean": 7.5, "init_cov": 10.0},
}


def _pi(T):
    return 4 * np.arctan(LD(1)) if T is LD else T(math.pi)


def noise(which, dtype):
    return L.noise(which, dtype)


# ---- the rule, in the arithmetic of T ------------------------------------------------------------------------------------------
def slot_quantities(T, x, y, phi, lx, ly, pxx, pxy, pyy, R):
    """What a slot contributes to every observation's score (OraclePF.associate_unknown, term for term), every operation in T."""
    c = lambda a: np.asarray(a, dtype=T)                                                       # noqa: E731
    x, y, phi, lx, ly, pxx, pxy, pyy = (c(a) for a in (x, y, phi, lx, ly, pxx, pxy, pyy))
    R00, R01, R10, R11 = T(R[0, 0]), T(R[0, 1]), T(R[1, 0]), T(R[1, 1])
    q = types.SimpleNamespace()
    with np.errstate(all="ignore"):
        dx, dy = lx - x, ly - y
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2)
        q.d, q.zp1 = d, np.arctan2(dy, dx) - phi
        h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
        t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
        t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
        q.s00 = h00 * t00 + h01 * t10 + R00
        q.s01 = h00 * t01 + h01 * t11 + R01
        q.s10 = h10 * t00 + h11 * t10 + R10
        q.s11 = h10 * t01 + h11 * t11 + R11
        q.det = q.s00 * q.s11 - q.s01 * q.s10
        rdet = T(1) / q.det
        q.qa, q.qb, q.qc = q.s11 * rdet, -(q.s01 + q.s10) * rdet, q.s00 * rdet
        q.logdet = np.log(q.det)
    return q


def score(T, q, zr, zb, wrapped=True):
    """nis, nd of observations (zr, zb) against the slot quantities q (broadcast against each other)."""
    pi = _pi(T)
    two_pi = T(2) * pi if T is LD else T(2.0 * math.pi)
    s = types.SimpleNamespace()
    with np.errstate(all="ignore"):
        s.v0 = np.asarray(zr, dtype=T) - q.d
        s.raw = np.asarray(zb, dtype=T) - q.zp1
        s.v1 = np.where(s.raw > pi, s.raw - two_pi, np.where(s.raw < -pi, s.raw + two_pi, s.raw)) if wrapped else s.raw
        s.nis = q.qa * s.v0 * s.v0 + q.qb * s.v0 * s.v1 + q.qc * s.v1 * s.v1
        s.nd = s.nis + q.logdet
    return s


def scales(dtype, x, y, phi, lx, ly, zr, zb, q, s):
    """The first-order rounding scales of nis and nd (see the header) from the truth's intermediates, float64."""
    eps = EPS[dtype]
    f = lambda a: np.abs(np.asarray(a, dtype=np.float64))                                      # noqa: E731
    with np.errstate(all="ignore"):
        d, v0, v1 = f(q.d), np.asarray(s.v0, dtype=np.float64), np.asarray(s.v1, dtype=np.float64)
        qa, qb, qc = (np.asarray(a, dtype=np.float64) for a in (q.qa, q.qb, q.qc))
        geo = f(x) + f(lx) + f(y) + f(ly)
        dv0 = eps * (f(zr) + 3 * d + geo)
        dv1 = eps * (f(zb) + 2 * math.pi + f(phi) + geo / d)
        prod = np.abs(qa * v0 * v0) + np.abs(qb * v0 * v1) + np.abs(qc * v1 * v1)
        cdet = (f(q.s00) * f(q.s11) + f(q.s01) * f(q.s10)) / f(q.det)
        s_nis = np.abs(2 * qa * v0 + qb * v1) * dv0 + np.abs(qb * v0 + 2 * qc * v1) * dv1 + eps * (8 + 4 * cdet) * prod
        s_nd = s_nis + eps * (f(q.logdet) + f(s.nd)) + 4 * eps * cdet
    return s_nis, s_nd


DEFECTS = ("nd_gated", "le_in_minimum", "strict_gate2", "nearest_by_nis", "no_wrap", "unused_ignored", "first_16_slots",
           "ragged_round_dropped", "sequential_map", "new_to_slot0_when_full", "near_first_chunk_only")
DECISION_DEFECTS = tuple(d for d in DEFECTS if d not in ("sequential_map", "new_to_slot0_when_full"))


def decide(T, pose, lm, z, R, gate1, gate2, defect=None, want_nis=False):
    """The association of z [2, m] against the maps lm [nl, 5, n] from the poses pose [3, n] in the arithmetic of T, slot after
    slot with a running minimum as the kernels keep it: decisions [m, n] (slot, -1 new, -2 dropped).  `defect`: a planted variant
    (DECISION_DEFECTS).  `want_nis`: also nis [m, nl, n]."""
    assert defect is None or defect in DECISION_DEFECTS
    nl, n = lm.shape[0], lm.shape[2]
    m = z.shape[1]
    g1, g2 = T(gate1), T(gate2)
    best = np.full((m, n), np.inf, dtype=T)
    best_l = np.full((m, n), -1, dtype=np.int64)
    near = np.zeros((m, n), dtype=bool)
    zr, zb = z[0][:, None], z[1][:, None]
    upto = 16 if defect == "first_16_slots" else nl - nl % 4 if defect == "ragged_round_dropped" else nl
    all_nis = np.full((m, nl, n), np.nan) if want_nis else None
    for l in range(upto):
        ok = np.ones(n, dtype=bool) if defect == "unused_ignored" else lm[l, 2] >= 0
        q = slot_quantities(T, pose[0], pose[1], pose[2], lm[l, 0], lm[l, 1], lm[l, 2], lm[l, 3], lm[l, 4], R)
        s = score(T, q, zr, zb, wrapped=defect != "no_wrap")
        gated = s.nd if defect == "nd_gated" else s.nis
        key = s.nis if defect == "nearest_by_nis" else s.nd
        with np.errstate(invalid="ignore"):
            better = ok & (gated < g1) & ((key <= best) if defect == "le_in_minimum" else (key < best))
            nr = ok & ((s.nis < g2) if defect == "strict_gate2" else (s.nis <= g2))
        if defect == "near_first_chunk_only":
            nr = nr & (np.arange(m) < 16)[:, None]
        best = np.where(better, key, best)
        best_l = np.where(better, l, best_l)
        near |= nr
        if want_nis:
            all_nis[:, l, :] = s.nis
    dec = np.where(best_l >= 0, best_l, np.where(near, -2, -1))
    return (dec, all_nis) if want_nis else dec


# ---- the designed table ---------------------------------------------------------------------------------------------------------
def _locations(rng):
    j, k = np.divmod(np.arange(NLOC), PER_RING)
    r = RING0 + RING_STEP * j + rng.uniform(-0.03, 0.03, NLOC)
    b = -math.pi + (k + 0.5 * (j % 2)) * (2 * math.pi / PER_RING) + rng.uniform(0.0, 0.02, NLOC)
    order = rng.permutation(NLOC)
    return r[order], b[order]


def _obs_loc():
    loc = np.full(M, -1, dtype=np.int64)
    loc[[i for i in range(M) if i not in DUP_OF]] = np.arange(NLOC)
    for d, s in DUP_OF.items():
        loc[d] = loc[s]
    return loc


OBS_LOC = _obs_loc()


def _eval(pose, land, zr, zb, R):
    """Truth's slot quantities and score for flat arrays of pairs: pose (x, y, phi), land (lx, ly, pxx, pxy, pyy)."""
    q = slot_quantities(LD, *pose, *land, R)
    return q, score(LD, q, zr, zb)


def _place(pose, cov, zr, zb, R, target, ang):
    """Landmark coordinates (longdouble) at which the truth's NIS of (zr, zb) is `target`, the whitened innovation along `ang`."""
    x, y, phi = (np.asarray(a, dtype=LD) for a in pose)
    zr, zb, target = np.asarray(zr, dtype=LD), np.asarray(zb, dtype=LD), np.asarray(target, dtype=LD)
    v0, v1 = np.zeros_like(x), np.zeros_like(x)
    for _ in range(5):
        d, th = zr - v0, phi + zb - v1
        lx, ly = x + d * np.cos(th), y + d * np.sin(th)
        q, s = _eval((x, y, phi), (lx, ly) + tuple(cov), zr, zb, R)
        sm = (q.s01 + q.s10) / 2
        c00 = np.sqrt(q.s00)
        c10 = sm / c00
        c11 = np.sqrt(q.s11 - c10 * c10)
        u0, u1 = np.cos(ang), np.sin(ang)
        w0, w1 = c00 * u0, c10 * u0 + c11 * u1                     # v = chol(S) u sqrt(target), rescaled to the non-symmetric form
        form = q.qa * w0 * w0 + q.qb * w0 * w1 + q.qc * w1 * w1
        k = np.sqrt(target / form)
        v0, v1 = k * w0, k * w1
    d, th = zr - v0, phi + zb - v1
    return x + d * np.cos(th), y + d * np.sin(th)


def _root(f, lo, hi, target, T):
    """Per element the value of the dtype T between lo and hi at which the monotone f comes closest to `target` (a secant search in
    longdouble, then the neighbouring representable values)."""
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)                # noqa: E731
    a, b = np.asarray(lo, dtype=LD), np.asarray(hi, dtype=LD)
    fa, fb = f(a) - target, f(b) - target
    assert np.all(fa * fb <= 0), f"{int(np.sum(fa * fb > 0))} targets outside the bracket"
    for _ in range(12):
        with np.errstate(all="ignore"):
            c = b - fb * (b - a) / (fb - fa)
        c = np.where(np.isfinite(c), c, b)
        fc = f(c) - target
        left = fa * fc <= 0                                            # keep the bracket (regula falsi with the secant's point)
        b, fb, a, fa = np.where(left, c, b), np.where(left, fc, fb), np.where(left, a, c), np.where(left, fa, fc)
    x = np.where(np.abs(fa) < np.abs(fb), a, b)
    c0 = rd(x)
    cands = [c0, rd(np.nextafter(c0.astype(T), T(np.inf))), rd(np.nextafter(c0.astype(T), T(-np.inf)))]
    errs = [np.abs(f(np.asarray(c, dtype=LD)) - target) for c in cands]
    pick = np.argmin(np.stack(errs), axis=0)
    return np.choose(pick, cands)


def _bound_pairs(dtype, pose, land, zr, zb, R, cls):
    """(bound of nis, bound of nd, q, s) of flat pairs at the truth; `cls` the class index per pair."""
    q, s = _eval(pose, land, zr, zb, R)
    s_nis, s_nd = scales(dtype, *pose, land[0], land[1], zr, zb, q, s)
    m_nis = np.array([MARGINS[dtype][c]["nis"] for c in CLASSES])[cls]
    m_nd = np.array([MARGINS[dtype][c]["nd"] for c in CLASSES])[cls]
    return m_nis * s_nis, m_nd * s_nd, q, s


def table(dtype, which="diag"):
    return _table(dtype, which)


@functools.lru_cache(maxsize=None)
def _table(dtype, which):
    """The designed table for storage dtype `dtype` and noise `which`, float64 arrays that hold only values of that dtype:
    .pose [3, n], .lm [NL, 5, n], .records [3 + 5 NL, n], .z [2, M], .R, .gate1, .gate2; per (location, particle): .sit, .band,
    .slot_a, .slot_b (-1: none), .k_draw; per particle: .kind (NORMAL / FULL / EMPTY).  Computed once, never changed."""
    T = NP_DTYPE[dtype]
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)                # noqa: E731
    rng = np.random.default_rng(SEED)
    R = noise(which, dtype)
    n = N
    lr, lb = _locations(rng)
    lr, lb = rd(lr), np.clip(rd(lb), -rd(math.pi), rd(math.pi))
    z = np.stack([lr[OBS_LOC], lb[OBS_LOC]])
    p = np.arange(n)
    kind = np.where(p % 7 == 3, FULL, NORMAL)
    kind[p % 190 == 7] = EMPTY
    kind[p % 47 == 5] = EXACTP
    kind[n - 1] = FULL
    x, y, phi = rd(rng.uniform(-5, 5, n)), rd(rng.uniform(-5, 5, n)), rd(rng.uniform(-3.14, 3.14, n))
    k = np.arange(NLOC)[:, None]
    sit = np.asarray(CYCLE)[(k + p[None, :]) % len(CYCLE)]
    sit = np.where((kind == FULL)[None, :] & (sit == STALE), NEW, sit)
    sit = np.where(np.isin(kind, (EMPTY, EXACTP))[None, :], NEW, sit)
    # exact particles (diagonal R only; with the full R they stay empty): one observation each, its NIS the gate itself
    exact_gate = np.zeros(n)
    if which == "diag":
        # (the innermost and the outermost ring, the landmark on the side away from the other rings: P is larger here)
        ok_obs = [i for i in range(M) if i not in DUP_OF and abs(z[1, i]) < 3.1 and not RING0 + 1 < z[0, i] < RING0 + (RINGS - 1) * RING_STEP - 1]
        for e, j in enumerate(np.nonzero(kind == EXACTP)[0]):
            i = ok_obs[e % len(ok_obs)]
            sit[OBS_LOC[i], j] = EXACT
            exact_gate[j] = GATE1 if e % 3 == 0 else GATE2
            x[j], y[j], phi[j] = 0.0, 0.0, -z[1, i]
    band = (k + p[None, :] // len(CYCLE)) % 3
    # slots: dealt per particle from a random permutation, in location order
    perm = np.argsort(rng.random((n, NL)), axis=1).T                                            # [NL, n]
    need = np.where(np.isin(sit, (RIVAL, TWIN)), 2, np.where(sit == NEW, 0, 1))
    start = np.cumsum(need, axis=0) - need
    assert (start[-1] + need[-1]).max() <= NL
    take = lambda pos: perm[np.minimum(pos, NL - 1), p[None, :]]                                # noqa: E731
    s1, s2 = take(start), take(start + 1)
    slot_a = np.where(need >= 1, s1, -1)
    slot_b = np.where(need == 2, s2, -1)
    tw = sit == TWIN
    slot_a, slot_b = np.where(tw, np.minimum(s1, s2), slot_a), np.where(tw, np.maximum(s1, s2), slot_b)
    lm = np.zeros((NL, 5, n))
    lm[:, 2, :] = -1.0
    # flat list of designed landmarks A: every situation with a slot but `stale`
    P, K = np.broadcast_to(p[None, :], sit.shape), np.broadcast_to(k, sit.shape)
    pose_of = lambda sel: (x[P[sel]], y[P[sel]], phi[P[sel]])                                   # noqa: E731
    obs_of = lambda sel: (lr[K[sel]], lb[K[sel]])                                               # noqa: E731

    def covs(cnt, lo, hi):
        pxx, pyy = L._loguniform(rng, lo, hi, cnt), L._loguniform(rng, lo, hi, cnt)
        return rd(pxx), rd(rng.uniform(-0.5, 0.5, cnt) * np.sqrt(pxx * pyy)), rd(pyy)

    def angles(cnt):
        return np.radians(rng.uniform(-60, 60, cnt)) + math.pi * rng.integers(0, 2, cnt)

    k_draw = np.zeros(sit.shape)
    for bi, name in enumerate(BANDS):
        sel = band == bi
        k_draw[sel] = rng.uniform(*BAND_DRAW[name], int(sel.sum()))

    def tune(sel, pose, land, zr, zb, cls, fn, target_fn):
        """Round the coordinates, then move Pxx or Pyy (the one with the larger response) over the dtype's values until fn(q, s)
        meets target_fn(bound_nis, bound_nd).  Returns the rounded (lx, ly, pxx, pxy, pyy)."""
        land = [rd(a) for a in land]
        b_nis, b_nd, _q, _s = _bound_pairs(dtype, pose, land, zr, zb, R, cls)
        if band_units is not None:                                                              # the edge band: fp32 units
            e_nis, e_nd, _q, _s = _bound_pairs("f32", pose, land, zr, zb, R, cls)
            edge = band[sel] == BANDS.index("edge")
            b_nis, b_nd = np.where(edge, e_nis, b_nis), np.where(edge, e_nd, b_nd)
        target = target_fn(b_nis, b_nd)

        def f_of(entry):
            def f(v):
                l2 = list(land)
                l2[entry] = v
                q, s = _eval(pose, l2, zr, zb, R)
                return fn(q, s)
            return f
        resp = [np.abs(f_of(e)(land[e] * 1.1) - f_of(e)(land[e] * 0.9)) for e in (2, 4)]
        use_xx = resp[0] >= resp[1]
        out = list(land)
        for e, pick in ((2, use_xx), (4, ~use_xx)):
            if not pick.any():
                continue
            sub = lambda a: a[pick] if isinstance(a, np.ndarray) and a.shape == pick.shape else a   # noqa: E731
            pose_s, land_s, zr_s, zb_s = [sub(a) for a in pose], [sub(a) for a in land], sub(zr), sub(zb)
            tgt = target[pick]

            def f(v, e=e, pose_s=pose_s, land_s=land_s, zr_s=zr_s, zb_s=zb_s):
                l2 = list(land_s)
                l2[e] = v
                q, s = _eval(pose_s, l2, zr_s, zb_s, R)
                return fn(q, s)
            val = _root(f, rd(land_s[e] * 0.75), rd(land_s[e] * 1.25), tgt, T)
            out[e] = out[e].copy()
            out[e][pick] = val
        return out

    band_units = "f32"
    # gates: one landmark at NIS = gate -+ k bound
    gsel = np.isin(sit, (G1IN, G1OUT, G2IN, G2OUT))
    cnt = int(gsel.sum())
    pose, (zr, zb) = pose_of(gsel), obs_of(gsel)
    gate = np.where(np.isin(sit[gsel], (G1IN, G1OUT)), GATE1, GATE2)
    sign = np.where(np.isin(sit[gsel], (G1IN, G2IN)), -1.0, 1.0)
    cls = np.where(gate == GATE1, 0, 1)
    cv = covs(cnt, 2.5e-4, 1e-3)
    ang = angles(cnt)
    lx, ly = _place(pose, cv, zr, zb, R, gate, ang)
    b0 = _bound_pairs(dtype, pose, (lx, ly) + cv, zr, zb, R, cls)[0]
    e0 = _bound_pairs("f32", pose, (lx, ly) + cv, zr, zb, R, cls)[0]
    b0 = np.where(band[gsel] == BANDS.index("edge"), e0, b0)
    lx, ly = _place(pose, cv, zr, zb, R, gate + sign * k_draw[gsel] * b0, ang)      # (the bounds hardly move with the placement)
    land = tune(gsel, pose, (lx, ly) + cv, zr, zb, cls, lambda q, s: s.nis, lambda bn, bd: LD(1) * gate + sign * k_draw[gsel] * bn)
    lm[slot_a[gsel], :, P[gsel]] = np.stack(land, axis=1)
    # twins: one record inside gate1, stored twice
    tsel = sit == TWIN
    cnt = int(tsel.sum())
    pose, (zr, zb) = pose_of(tsel), obs_of(tsel)
    cv = covs(cnt, 2.5e-4, 1e-3)
    lx, ly = _place(pose, cv, zr, zb, R, rng.uniform(0.5, 3.0, cnt), angles(cnt))
    rec = np.stack([rd(lx), rd(ly)] + list(cv), axis=1)
    lm[slot_a[tsel], :, P[tsel]] = rec
    lm[slot_b[tsel], :, P[tsel]] = rec
    # rivals: B with the smaller NIS and the larger covariance, A tuned to nd_A = nd_B - k (bound_A + bound_B)
    rsel = sit == RIVAL
    cnt = int(rsel.sum())
    pose, (zr, zb) = pose_of(rsel), obs_of(rsel)
    cls = np.full(cnt, 2)
    cvb = covs(cnt, 2e-3, 4e-3)
    lxb, lyb = _place(pose, cvb, zr, zb, R, rng.uniform(0.05, 0.3, cnt), angles(cnt))
    landb = [rd(lxb), rd(lyb)] + list(cvb)
    bb_nis, bb_nd, qb_, sb_ = _bound_pairs(dtype, pose, landb, zr, zb, R, cls)
    eb_nis, eb_nd, _q, _s = _bound_pairs("f32", pose, landb, zr, zb, R, cls)
    bb_nd = np.where(band[rsel] == BANDS.index("edge"), eb_nd, bb_nd)
    cva = covs(cnt, 2.5e-4, 5e-4)
    anga = angles(cnt)
    nis_a = np.asarray(sb_.nis, dtype=np.float64) + 0.15
    for _ in range(3):
        lxa, lya = _place(pose, cva, zr, zb, R, nis_a, anga)
        _bn, ba_nd, qa_, _sa = _bound_pairs(dtype, pose, (lxa, lya) + cva, zr, zb, R, cls)
        ea_nd = _bound_pairs("f32", pose, (lxa, lya) + cva, zr, zb, R, cls)[1]
        ba_nd = np.where(band[rsel] == BANDS.index("edge"), ea_nd, ba_nd)
        nis_a = np.asarray(sb_.nd - k_draw[rsel] * (ba_nd + bb_nd) - qa_.logdet, dtype=np.float64)
    landa = tune(rsel, pose, (lxa, lya) + cva, zr, zb, cls, lambda q, s: s.nd, lambda bn, bd: sb_.nd - k_draw[rsel] * (bd + bb_nd))
    lm[slot_a[rsel], :, P[rsel]] = np.stack(landa, axis=1)
    lm[slot_b[rsel], :, P[rsel]] = np.stack(landb, axis=1)
    # stale: an unused slot exactly on the observation, with a stale positive Pyy
    ssel = sit == STALE
    (sx, sy, sphi), (zr, zb) = pose_of(ssel), obs_of(ssel)
    lm[slot_a[ssel], 0, P[ssel]] = rd(sx + zr * np.cos(sphi + zb))
    lm[slot_a[ssel], 1, P[ssel]] = rd(sy + zr * np.sin(sphi + zb))
    lm[slot_a[ssel], 4, P[ssel]] = rd(0.01)
    # exact: pose (0, 0, -b), the landmark on the particle's x axis at r - v0, P = diag(2^-6 - R00, 0): S = diag(2^-6, R11), v1 = 0,
    # NIS = 64 v0^2 -- every operation of the rule is exact in fp32 and fp64, fused or not (1 / (2^-6 R11) R11 = 64 is checked)
    esel = sit == EXACT
    _ex_p, (zr, _zb) = P[esel], obs_of(esel)
    v0 = np.array([EXACT_V0[g] for g in exact_gate[_ex_p]]) * np.where(zr < RING0 + 1, 1.0, -1.0)
    assert np.all(rd(zr - v0) == zr - v0) and T(R[1, 1]) * (T(1) / T(R[1, 1])) == 1 and T(T(2.0 ** -6) - T(R[0, 0])) + T(R[0, 0]) == T(2.0 ** -6)
    lm[slot_a[esel], :, _ex_p] = np.stack([zr - v0, 0 * v0, np.full(len(v0), float(T(T(2.0 ** -6) - T(R[0, 0])))), 0 * v0, 0 * v0], axis=1)
    # full particles: all but 0-3 of the remaining slots hold landmarks far beyond every observation
    used_cnt = (start[-1] + need[-1])
    for pi_ in np.nonzero(kind == FULL)[0]:
        rest = perm[used_cnt[pi_]:, pi_]
        fill = rest[: len(rest) - (pi_ // 7) % 4]
        if pi_ == n - 1:
            fill = rest[: len(rest) - 2]
        a, d = rng.uniform(-math.pi, math.pi, len(fill)), rng.uniform(70, 90, len(fill))
        lm[fill, 0, pi_], lm[fill, 1, pi_] = rd(x[pi_] + d * np.cos(a)), rd(y[pi_] + d * np.sin(a))
        lm[fill, 2, pi_], lm[fill, 3, pi_], lm[fill, 4, pi_] = rd(1e-3), 0.0, rd(2e-3)
    t = types.SimpleNamespace(dtype=dtype, which=which, n=n, R=R, gate1=float(T(GATE1)), gate2=float(T(GATE2)), z=z,
                              pose=np.stack([x, y, phi]), lm=lm, sit=sit, band=band, slot_a=slot_a, slot_b=slot_b, kind=kind,
                              k_draw=k_draw, exact_gate=exact_gate)
    t.records = np.vstack([t.pose, lm.reshape(NL * 5, n)])
    assert np.array_equal(t.records, rd(t.records)), "only values of the storage dtype"
    u = lm[:, 2, :] >= 0
    u = u & ~(np.zeros((NL, n), dtype=bool) | (kind == EXACTP)[None, :])
    assert np.all(lm[:, 4, :][u] > 0) and np.all((lm[:, 2, :] * lm[:, 4, :])[u] > (lm[:, 3, :] ** 2)[u]), "used records positive definite"
    for a in vars(t).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


# ---- the truth, the bounds, the admissible sets ------------------------------------------------------------------------------------
def truth(t, obs):
    """OraclePF.associate_unknown's scores in longdouble for the observations `obs` (indices) of table t: (q, s, used) with
    s.nis, s.nd [len(obs), NL, n] and used [NL, n]."""
    lm = t.lm
    q = slot_quantities(LD, t.pose[0][None], t.pose[1][None], t.pose[2][None], lm[:, 0], lm[:, 1], lm[:, 2], lm[:, 3], lm[:, 4], t.R)
    for key, val in vars(q).items():
        setattr(q, key, val[None])
    obs = np.atleast_1d(obs)
    s = score(LD, q, t.z[0][obs][:, None, None], t.z[1][obs][:, None, None])
    return q, s, lm[:, 2, :] >= 0


def twin_lower(t):
    """[NL, n]: a lower slot holds the same record bit for bit."""
    out = np.zeros((NL, t.n), dtype=bool)
    for l in range(1, NL):
        same = np.all(t.lm[:l] == t.lm[l][None], axis=1) & (t.lm[:l, 2, :] >= 0)
        out[l] = same.any(axis=0) & (t.lm[l, 2, :] >= 0)
    return out


def admissible(nis, nd, b_nis, b_nd, used, lower_twin, gate1, gate2):
    """The admissible decisions (see the header) of observations against the map: (slots [.., NL, n] bool, minus2 [.., n],
    minus1 [.., n]).  nis, nd: the truth's (longdouble); b_*: the bounds."""
    with np.errstate(invalid="ignore"):
        may = used & (nis - b_nis < gate1)
        must = used & (nis + b_nis < gate1)
        thr = np.min(np.where(must, nd + b_nd, np.inf), axis=-2, keepdims=True)
        slots = may & (nd - b_nd <= thr) & ~lower_twin
        none_must = ~must.any(axis=-2)
        minus2 = none_must & (used & (nis - b_nis <= gate2)).any(axis=-2)
        minus1 = none_must & ~(used & (nis + b_nis <= gate2)).any(axis=-2)
    return slots, minus2, minus1


def designed_mask(t, i):
    """[NL, n]: the slots designed for observation i's location."""
    k = OBS_LOC[i]
    out = np.zeros((NL, t.n), dtype=bool)
    p = np.arange(t.n)
    for s in (t.slot_a[k], t.slot_b[k]):
        out[np.maximum(s, 0), p] |= s >= 0
    return out


def case(dtype, which="diag", units=None):
    return _case(dtype, which, units or dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, which, units):
    """Everything a comparison on table(dtype, which) needs, computed once: the truth's decisions .dec [M, n], the admissible sets
    .adm_slot [M, NL, n] / .adm_m2 / .adm_m1 [M, n], .decided [M, n], the truth's scores and bounds of the designed slots (.nis_a,
    .nd_a, .b_nis_a, .b_nd_a, .nis_b, ... [M, n], nan where there is none), .raw_a (the bearing innovation before the wrap),
    .foreign_min (the smallest NIS of a non-designed (observation, used slot) pair, in float64: the CPU test asserts it beyond
    FOREIGN_MIN = 100 x gate2, so no rounding bound brings a foreign slot into a set and only the designed slots are scored in
    longdouble).  `units`: the dtype whose eps and margins make the bounds (default: the table's) -- "f32" on the f64 table gives
    the edge band's units there."""
    t = table(dtype, which)
    units = units or dtype
    n = t.n
    c = types.SimpleNamespace(t=t, dtype=dtype, which=which, units=units)
    p = np.arange(n)
    # foreign pairs, float64
    q64 = slot_quantities(np.float64, t.pose[0][None], t.pose[1][None], t.pose[2][None], *(t.lm[:, j] for j in range(5)), t.R)
    used = t.lm[:, 2, :] >= 0
    c.foreign_min = np.inf
    for i in range(M):
        foreign = used & ~designed_mask(t, i)
        nis = score(np.float64, q64, t.z[0, i], t.z[1, i]).nis
        c.foreign_min = min(c.foreign_min, float(nis[foreign].min()))
    # designed pairs, longdouble
    c.sit = t.sit[OBS_LOC]                                                                      # per (observation, particle)
    c.band = t.band[OBS_LOC]
    cls = np.array([CLASS_OF_SIT.get(v, 0) for v in range(len(SITS))])[c.sit]
    P = np.broadcast_to(p[None, :], (M, n))
    pose = tuple(np.broadcast_to(a[None, :], (M, n)) for a in t.pose)
    zr, zb = (np.broadcast_to(a[:, None], (M, n)) for a in t.z)
    cols = {}
    for tag, slot in (("a", t.slot_a[OBS_LOC]), ("b", t.slot_b[OBS_LOC])):
        has = (slot >= 0) & (c.sit != STALE)
        sl = np.maximum(slot, 0)
        land = tuple(t.lm[sl, j, P] for j in range(5))
        b_nis, b_nd, q, s = _bound_pairs(units, pose, land, zr, zb, t.R, cls)
        if tag == "a":                                                                           # exact pairs: no operation rounds
            ex = c.sit == EXACT
            want = np.broadcast_to(t.exact_gate[None, :], (M, n))
            assert np.all(np.abs(np.asarray(s.nis - want, dtype=np.float64))[ex] < 1e-15)
            s.nis = np.where(ex, LD(1) * want, s.nis)
            b_nis, b_nd = np.where(ex, 0.0, b_nis), np.where(ex, 0.0, b_nd)
        cols[tag] = (has, sl, s.nis, s.nd, b_nis, b_nd)
        for name, arr in (("nis", s.nis), ("nd", s.nd), ("b_nis", b_nis), ("b_nd", b_nd), ("raw", np.asarray(s.raw, dtype=np.float64))):
            setattr(c, f"{name}_{tag}", np.where(has, arr, np.nan))
    stack = lambda k: np.stack([cols["a"][k], cols["b"][k]], axis=1)                            # noqa: E731  [M, 2, n]
    has2, sl2, nis2, nd2 = stack(0), stack(1), stack(2), stack(3)
    lower = np.stack([np.zeros((M, n), dtype=bool), (c.sit == TWIN) & cols["b"][0]], axis=1)   # B of a twin: the same record, higher up
    assert np.all(sl2[:, 0][c.sit == TWIN] < sl2[:, 1][c.sit == TWIN])
    slots2, c.adm_m2, c.adm_m1 = admissible(nis2, nd2, stack(4), stack(5), has2, lower, LD(t.gate1), LD(t.gate2))
    c.adm_slot = np.zeros((M, NL, n), dtype=bool)
    I = np.broadcast_to(np.arange(M)[:, None], (M, n))
    for j in (0, 1):
        on = slots2[:, j]
        c.adm_slot[I[on], sl2[:, j][on], P[on]] = True
    with np.errstate(invalid="ignore"):                                                          # the oracle's rule on the truth's numbers
        cand = has2 & (nis2 < LD(t.gate1))
        best = np.argmin(np.where(cand, nd2, np.inf), axis=1)                                   # (a tie: A, the lower slot of a twin)
        nearby = (has2 & (nis2 <= LD(t.gate2))).any(axis=1)
    c.dec = np.where(cand.any(axis=1), np.take_along_axis(sl2, best[:, None, :], axis=1)[:, 0], np.where(nearby, -2, -1))
    c.count = c.adm_slot.sum(axis=1) + c.adm_m2 + c.adm_m1
    c.decided = c.count == 1
    c.has_band = np.isin(c.sit, (G1IN, G1OUT, G2IN, G2OUT, RIVAL))
    c.dup = np.zeros((M, n), dtype=bool)
    for d_, s_ in DUP_OF.items():
        c.dup[d_] = (c.dec[d_] >= 0) & (c.dec[d_] == c.dec[s_])
    c.wrapped = np.abs(c.raw_a) > math.pi
    return c


def truth_in_sets(c):
    """The truth's decision is in its own admissible set, everywhere."""
    p = np.arange(c.t.n)[None, :]
    i = np.arange(M)[:, None]
    d = c.dec
    return np.where(d >= 0, c.adm_slot[i, np.maximum(d, 0), p], np.where(d == -2, c.adm_m2, c.adm_m1))


def check_decisions(c, got, m):
    """`got` [m, n]: every decision in its admissible set, every decided pair equal to the truth.  Returns (outside [m, n] bool,
    wrong [m, n] bool): both must be empty."""
    got = np.asarray(got)
    p = np.arange(c.t.n)[None, :]
    i = np.arange(m)[:, None]
    ok = np.where(got >= 0, c.adm_slot[i, np.clip(got, 0, NL - 1), p] & (got < NL),
                  np.where(got == -2, c.adm_m2[:m], np.where(got == -1, c.adm_m1[:m], False)))
    wrong = c.decided[:m] & (got != c.dec[:m])
    return ~ok, wrong


def derive_margins(dtype):
    """{class: {quantity: max(4, 4 x worst |model - truth| / scale)}} over the class's designed pairs and both noise matrices."""
    T = NP_DTYPE[dtype]
    worst = {cl: {qn: 0.0 for qn in QUANT} for cl in CLASSES}
    for which in NOISES:
        t = table(dtype, which)
        p = np.arange(t.n)
        for k in range(NLOC):
            i = int(np.nonzero(OBS_LOC == k)[0][0])
            for slot in (t.slot_a[k], t.slot_b[k]):
                has = (slot >= 0) & (t.sit[k] != STALE)
                sl = slot[has]
                pose = tuple(a[has] for a in t.pose)
                land = tuple(t.lm[sl, j, p[has]] for j in range(5))
                q, s = _eval(pose, land, t.z[0, i], t.z[1, i], t.R)
                qm = slot_quantities(T, *pose, *land, t.R)
                sm = score(T, qm, t.z[0, i], t.z[1, i])
                s_nis, s_nd = scales(dtype, *pose, land[0], land[1], t.z[0, i], t.z[1, i], q, s)
                cls = np.array([CLASS_OF_SIT.get(v, 0) for v in range(len(SITS))])[t.sit[k][has]]
                for qn, sc in (("nis", s_nis), ("nd", s_nd)):
                    ratio = np.abs(np.asarray(getattr(sm, qn).astype(LD) - getattr(s, qn), dtype=np.float64)) / sc
                    for ci, cl in enumerate(CLASSES):
                        if (cls == ci).any():
                            worst[cl][qn] = max(worst[cl][qn], float(ratio[cls == ci].max()))
    return {cl: {qn: max(4.0, 4.0 * worst[cl][qn]) for qn in QUANT} for cl in CLASSES}


# ---- the replay of the updates ----------------------------------------------------------------------------------------------------
class Replay:
    """The state of table t under decisions applied in observation order, in the arithmetic of T (np.longdouble: the truth, with
    bounds in the units of `t.dtype`; float32 / float64: the model).  .lm [NL, 5, n], .inc [n] (log-weight increment), .touch [NL, n]
    (how often a record was written), .b_lm [NL, 5, n], .b_inc [n], .dropped [n] (-1 decisions that found no slot)."""

    def __init__(self, t, T=LD, defect=None, margins=None):
        assert defect in (None, "new_to_slot0_when_full")
        self.t, self.T, self.defect = t, T, defect
        self.margins = REPLAY_MARGINS[t.dtype] if margins is None else margins
        n = t.n
        self.pose = [np.asarray(a, dtype=T) for a in t.pose]
        self.lm = np.asarray(t.lm, dtype=T).copy()
        self.inc = np.zeros(n, dtype=T)
        self.lw0 = NP_DTYPE[t.dtype](-math.log(n))
        self.touch = np.zeros((NL, n), dtype=np.int64)
        self.b_lm, self.b_inc = np.zeros((NL, 5, n)), np.zeros(n)
        self.dropped = np.zeros(n, dtype=np.int64)
        self.ratio = {q: [] for q in L.QUANTITIES}                      # (filled by derive_replay_margins)

    def step(self, zr, zb, dec):
        t, T, n = self.t, self.T, self.t.n
        p = np.arange(n)
        dec = np.asarray(dec)
        matched, new = dec >= 0, dec == -1
        free = self.lm[:, 2, :] < 0
        first = np.argmax(free, axis=0)
        has = free[first, p]
        if self.defect == "new_to_slot0_when_full":
            first, has = np.where(has, first, 0), np.ones(n, dtype=bool)
        init = new & has
        self.dropped += new & ~has
        slot = np.where(matched, np.clip(dec, 0, NL - 1), first)
        rec = self.lm[slot, :, p]                                                                 # [n, 5]
        x, y, phi = self.pose
        ps = types.SimpleNamespace(n=n, x=x, y=y, phi=phi, lx=np.where(matched, rec[:, 0], x + 10), ly=np.where(matched, rec[:, 1], y),
                                   pxx=np.where(matched, rec[:, 2], 0.01), pxy=np.where(matched, rec[:, 3], 0.0),
                                   pyy=np.where(matched, rec[:, 4], 0.01), r=np.full(n, zr), b=np.full(n, zb), r3=np.full(n, zr),
                                   b3=np.full(n, zb))
        ref = L.reference(T, ps, t.R)
        mean = np.where(matched, ref.mean, ref.init_mean)
        cov = np.where(matched, ref.cov, ref.init_cov)
        act = matched | init
        self.lm[slot[act], 0:2, p[act]] = mean[:, act].T
        self.lm[slot[act], 2:5, p[act]] = cov[:, act].T
        self.inc = np.where(matched, self.inc + ref.inc, self.inc)
        self.touch[slot[act], p[act]] += 1
        if T is LD:
            sc = L.scales(ps, t.R, ref, t.dtype)
            mg = self.margins
            bm = np.where(matched, mg["mean"] * sc["mean"], mg["init_mean"] * sc["init_mean"])
            bc = np.where(matched, mg["cov"] * sc["cov"], mg["init_cov"] * sc["init_cov"])
            self.b_lm[slot[act], 0:2, p[act]] = bm[:, act].T
            self.b_lm[slot[act], 2:5, p[act]] = bc[:, act].T
            lw = np.abs(np.asarray(self.lw0 + self.inc, dtype=np.float64))
            self.b_inc += np.where(matched, mg["inc"] * sc["inc"] + EPS[t.dtype] * lw, 0.0)
        return ref, ps, matched, init


def replay(t, decisions, m, T=LD, defect=None, margins=None):
    rp = Replay(t, T, defect, margins)
    for i in range(m):
        rp.step(t.z[0, i], t.z[1, i], decisions[i])
    return rp


def derive_replay_margins(dtype):
    """lm_records' rule on these records: max(4, 4 x worst |model - truth| / scale) per quantity, over every record the truth's
    decisions touch FIRST in the call of 64 observations (a second touch has a rounded prior), both noise matrices."""
    T = NP_DTYPE[dtype]
    worst = {q: 0.0 for q in L.QUANTITIES}
    one = {q: 1.0 for q in L.QUANTITIES}
    for which in NOISES:
        c = case(dtype, which)
        rp = Replay(c.t, LD, margins=one)
        for i in range(M):
            before = rp.touch.copy()
            ref, ps, matched, init = rp.step(c.t.z[0, i], c.t.z[1, i], c.dec[i])
            slot = np.where(matched, np.clip(c.dec[i], 0, NL - 1), 0)
            fresh = matched & (before[slot, np.arange(c.t.n)] == 0)
            mod = L.reference(T, types.SimpleNamespace(**{k: np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v
                                                          for k, v in vars(ps).items()}), c.t.R)
            sc = L.scales(ps, c.t.R, ref, dtype)
            for q, sel in (("mean", fresh), ("cov", fresh), ("inc", fresh), ("init_mean", init), ("init_cov", init)):
                if sel.any():
                    err = np.abs(np.asarray(np.asarray(getattr(mod, q)).astype(LD) - getattr(ref, q), dtype=np.float64)) / sc[q]
                    worst[q] = max(worst[q], float(err[..., sel].max()))
    return {q: max(4.0, 4.0 * worst[q]) for q in L.QUANTITIES}


def check_state(t, rp, lm, inc):
    """The state after a call (lm [NL, 5, n], inc [n] the log-weight increments; float64 views of the device's or a model's numbers)
    against the replay rp of the SAME decisions: the set of used slots exact, untouched records bit for bit, records touched once
    and the increments of particles without a twice-touched record within the replay's bounds.  Returns a dict: `used_wrong`,
    `untouched_changed`, `out_of_bound` (counts: all must be 0), `worst_lm`, `worst_inc` (error / bound), `twice` [NL, n] and
    `twice_p` [n] (what the caller holds at the suite's tolerance)."""
    lm, inc = np.asarray(lm, dtype=np.float64), np.asarray(inc, dtype=np.float64)
    want = np.asarray(rp.lm, dtype=np.float64)
    out = {}
    out["used_wrong"] = int(np.sum((lm[:, 2, :] >= 0) != (want[:, 2, :] >= 0)))
    un = rp.touch == 0
    same = np.all((lm == t.lm) & (np.signbit(lm) == np.signbit(t.lm)), axis=1)
    out["untouched_changed"] = int(np.sum(un & ~same))
    once = rp.touch == 1
    err = np.abs(lm - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(once[:, None, :], err / rp.b_lm, 0.0)
    ratio = np.where(np.isfinite(ratio), ratio, np.where(once[:, None, :], np.inf, 0.0))
    twice = rp.touch >= 2
    twice_p = twice.any(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_inc = np.where(twice_p | (rp.b_inc == 0), 0.0, np.abs(inc - np.asarray(rp.inc, dtype=np.float64)) / rp.b_inc)
    exact_inc = (rp.b_inc == 0) & (inc != 0)                                                       # no matched observation: untouched
    out["worst_lm"], out["worst_inc"] = float(ratio.max()), float(np.nanmax(r_inc))
    out["out_of_bound"] = int(np.sum(ratio > 1.0) + np.sum(~(r_inc <= 1.0)) + np.sum(exact_inc))
    out["twice"], out["twice_p"] = twice, twice_p
    return out


def model_call(T, t, m, defect=None):
    """The whole call in the arithmetic of T: (decisions [m, n], Replay).  `defect`: any of DEFECTS."""
    if defect == "sequential_map":                                         # every observation against the map as it is at its turn
        rp = Replay(t, T)
        dec = np.zeros((m, t.n), dtype=np.int64)
        for i in range(m):
            dec[i] = decide(T, t.pose, np.asarray(rp.lm, dtype=np.float64), t.z[:, i:i + 1], t.R, t.gate1, t.gate2)[0]
            rp.step(t.z[0, i], t.z[1, i], dec[i])
        return dec, rp
    dec = decide(T, t.pose, t.lm, t.z[:, :m], t.R, t.gate1, t.gate2, defect if defect in DECISION_DEFECTS else None)
    return dec, replay(t, dec, m, T, defect if defect == "new_to_slot0_when_full" else None)
