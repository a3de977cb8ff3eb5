"""Designed landmark records for the per-particle 2 x 2 EKF of the FastSLAM path (csrc/pf_device.h: lm_update, lm_init), with a
re-anchored high-precision reference, per-record rounding scales and planted defects.  NumPy and the oracle only; shared by
tests/test_lm_records_cpu.py (CPU: the records are as hard as they claim, the margins follow their rule, the comparison rejects
the planted defects) and tests/test_gpu_pf_records.py (the kernels on exactly these numbers).

WHY.  The scenes of tests/test_gpu_pf.py compare covariances against the LARGEST covariance entry of the whole filter, means
against the largest coordinate and log-weights against the largest log-weight; a converged landmark may be wrong by 100 % there.
Here every record is judged against a bound built from ITS OWN numbers, after ONE call, from inputs that device and reference
share bit for bit (everything is rounded to the storage dtype first): nothing accumulates, nothing is relative to a global scale.

RECORDS.  `table(dtype)`: N particles in seven classes (CLASSES), N_PER_CLASS each, N no multiple of 64.  A particle holds
landmark 1 (the designed record, updated), landmark 2 (benign, never observed) and the empty slot 3 (first sighted).

  class       range            prior variance      rho                          innovation
  benign      10-50 m          1e-2                |rho| <= 0.9                 ~1 sigma
  near        0.05-1 m         1e-4..1e-2          |rho| <= 0.9                 ~1 sigma
  far         200-2000 m       1e-2..1             |rho| <= 0.9                 ~1 sigma
  bigP        10-50 m          1e2..1e4            |rho| <= 0.9                 ~1 sigma      (P / R up to 1e6)
  tinyP       10-50 m          1e-8..1e-6          |rho| <= 0.9                 ~1 sigma
  correlated  10-50 m          1e-2                1 - |rho| in 1e-6..1e-2      ~1 sigma      (both signs, PD after rounding)
  outlier     10-50 m          1e-2                |rho| <= 0.9                 up to 60 sigma in range AND in bearing

AN OBSERVATION IS FILTER-WIDE: slam_pf_update_known takes one (range, bearing) per landmark for all particles, so a particle
whose innovation is to be one sigma at 0.05 m cannot share a call with one at 2000 m.  The particles of a class are therefore
split into GROUPS (8 per class, two for the outlier class); a group shares one observation of landmark 1 and one first sighting
of landmark 3, and every particle of the group is designed around them: pose anywhere within +-5 m with any heading in (-pi, pi),
the landmark at range r - v0 in the direction phi + b - v1 with the innovation v drawn from chol(S)' e.  A test runs ONE call per
group on the freshly injected table and keeps the group's particles; the other particles of that call see an observation that
was not made for them and are not compared in it (every particle is compared in its own group's call: compare_records asserts
that nothing is left out).  "60 sigma" is 60 sqrt(S) in each component, so the outlier class's increments reach
about -0.5 (60^2 + 60^2) = -3.6e3 (more is not reachable inside 10-50 m: 200 sigma of range are 28 m).
Eight particles per group sit exactly on the axes and the diagonals as seen from the particle (dy = 0, dx = 0, |dy| = |dx|,
exact in fp32: poses and offsets on a 2^-10 grid) -- the branches and ties of the fp32 atan2; the others cover the quadrants.
Bearings are reported in [-pi, pi]; the share of particles whose bearing innovation lies beyond pi before the wrap is asserted
by the CPU test (WRAP_SHARE_MIN).  Two noise matrices: the suite's diagonal R and a full NON-symmetric one (R_FULL), for which
the symmetrisation s01 = (s01a + s10a) / 2 matters.

REFERENCE.  `reference(T, tab, R)` restates OraclePF.update_known's two branches (seen / first sighting) for one observation per
particle in the arithmetic of T.  T = np.longdouble (64-bit mantissa, asserted below) is the TRUTH; T = np.float32 / np.float64
are the MODEL of a device that rounds every operation correctly -- not the truth.  The CPU test pins the float64 instance against
OraclePF.update_known itself to 1e-12.

SCALES (`scales`), first order, from the truth's own intermediates; eps = the dtype's unit roundoff (2^-24, 2^-53):
  dv0   = eps (|r| + 3 d + |x| + |lx| + |y| + |ly|)                                       error of the range innovation
  dv1   = eps (|b| + 2 pi + |phi| + (|x| + |lx| + |y| + |ly|) / d) + a_atan               ... of the bearing innovation
  mean  : eps |l| + |K| (dv0, dv1)' + 8 eps |K| |v| + eps cond(S) |K| |v|,   K = P H' S^-1
  cov   : eps max(pxx, pyy) of the PRIOR, for all three entries
  inc   : |S^-1 v| . (dv0, dv1) + 8 eps (nis + |inc| + 10)
  first sighting, with da = eps (|phi| + |b| + |phi + b|) + a_sc the ABSOLUTE error of sin and cos of the rounded angle:
    mean: eps (|x| + r) + r da
    cov : eps x (the entry's sum of absolute terms) + sum over its terms g_a g_b R_ab of (dg_a |g_b| + |g_a| dg_b) |R_ab|,
          dg = da for cos / sin, r da for -r sin / r cos
  a_atan = 8.3e-8 (the degree-15 polynomial) and a_sc = 1e-6 (v_sin_f32 / v_cos_f32) as csrc/pf_device.h states them; 0 in fp64.
Two terms are additions to the first draft of these scales, both read off the formula.  (1) eps cond(S) |K| |v|: the gain is
formed through chol(S), whose rounding is amplified by cond(S) = s_max / s_min of S (with P >> R up to 5e5 here); without the
term the correctly rounded model is 8 x over the scale on the bigP class's means, with it 0.6 x.  (The increment needs no
such term: nis = |C' v|^2 is computed from the factor directly.)  (2) the first sighting's covariance is a product of sines and
cosines whose error is ABSOLUTE (a_sc, and eps times the angle): relative to |cos sin| alone the scale would vanish on the axes.

BOUNDS.  bound = margin x scale with MARGINS[dtype][class][quantity] = max(4, 4 x the worst error / scale of the MODEL of that
dtype against the truth on the class's records, over both noise matrices): the factor 4 is for 1-ulp rsq / rcp / log in place
of correctly rounded operations and for another contraction.  The table below is committed; the CPU test re-derives it
(`derive_margins`) and fails if a committed value is below the rule.  Nothing here comes from a device's output.

EXCLUSION.  A record is left out only if the truth's own posterior, rounded to the dtype, is not strictly positive definite;
at most 0.1 % of a class (EXCLUDE_CAP); fp64 leaves out none.  POSITIVE DEFINITENESS: wherever the model's posterior has
Pxx > 0, Pyy > 0, Pxx Pyy > Pxy^2 the device's must, too (a negative Pxx reads as "slot unused" in the unknown-correspondence
path).

KNOWN LIMIT (documented in DESIGN.md): the covariance bound is relative to the PRIOR.  With P / R = 1e6 the posterior is 1e-6 of
the prior and P - W1 W1' cancels: fp32 keeps about 8 eps max(pxx, pyy), which is up to tens of per cent of the posterior.
"""
import functools
import math
import types

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "the truth needs a longdouble with a 64-bit mantissa"

NP_DTYPE = {"f64": np.float64, "f32": np.float32}
EPS = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
A_ATAN = {"f64": 0.0, "f32": 8.3e-8}
A_SC = {"f64": 0.0, "f32": 1e-6}

R_DIAG = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])            # tests/test_gpu_pf.py::R
R_FULL = np.array([[0.1 ** 2, 4e-4], [1e-4, (math.pi / 180) ** 2]])          # not symmetric: (R01 + R10) / 2 = 2.5e-4
NOISES = {"diag": R_DIAG, "full": R_FULL}

CLASSES = ("benign", "near", "far", "bigP", "tinyP", "correlated", "outlier")
N_PER_CLASS = 1001
N = N_PER_CLASS * len(CLASSES)                                               # 7007 = 109 * 64 + 31: a ragged last wave
assert N % 64 != 0
NL = 3                                                                       # landmark slots: updated, untouched, first sighted
SEED = 20240611
QUANTITIES = ("mean", "cov", "inc", "init_mean", "init_cov")
EXCLUDE_CAP = 1e-3
WRAP_SHARE_MIN = 0.15
OUTLIER_SIGMAS = 60.0

# range, prior variance (log-uniform), groups, largest |e| of the innovation v = chol(S)' e
SPEC = {
    "benign": dict(rng=(10.0, 50.0), var=(1e-2, 1e-2), groups=8, emax=2.5),
    "near": dict(rng=(0.05, 1.0), var=(1e-4, 1e-2), groups=8, emax=1.5),
    "far": dict(rng=(200.0, 2000.0), var=(1e-2, 1.0), groups=8, emax=2.5),
    "bigP": dict(rng=(10.0, 50.0), var=(1e2, 1e4), groups=8, emax=2.5),
    "tinyP": dict(rng=(10.0, 50.0), var=(1e-8, 1e-6), groups=8, emax=2.5),
    "correlated": dict(rng=(10.0, 50.0), var=(1e-2, 1e-2), groups=8, emax=2.5),
    "outlier": dict(rng=(10.0, 50.0), var=(1e-2, 1e-2), groups=2, emax=OUTLIER_SIGMAS),
}
# world directions of the landmark as seen from the particle, exact: both axes and |dy| = |dx| in every quadrant
SPECIAL = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
GRID = 1024.0

# margin = max(4, 4 x worst model error / scale), rounded up with about 10 % to spare (derive_margins; the CPU test checks it)
MARGINS = {
    "f32": {
        "benign": {"mean": 4.0, "cov": 16.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "near": {"mean": 6.0, "cov": 26.5, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "far": {"mean": 6.5, "cov": 23.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "bigP": {"mean": 4.0, "cov": 30.5, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "tinyP": {"mean": 8.0, "cov": 4.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "correlated": {"mean": 6.5, "cov": 19.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "outlier": {"mean": 4.0, "cov": 16.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
    },
    "f64": {
        "benign": {"mean": 6.0, "cov": 17.5, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "near": {"mean": 7.5, "cov": 32.0, "inc": 4.0, "init_mean": 7.0, "init_cov": 4.0},
        "far": {"mean": 8.5, "cov": 25.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "bigP": {"mean": 4.0, "cov": 26.5, "inc": 5.0, "init_mean": 4.0, "init_cov": 4.0},
        "tinyP": {"mean": 9.0, "cov": 4.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "correlated": {"mean": 7.0, "cov": 17.5, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
        "outlier": {"mean": 4.0, "cov": 21.0, "inc": 4.0, "init_mean": 4.0, "init_cov": 4.0},
    },
}


def wrap(a):
    return np.where(a > math.pi, a - 2 * math.pi, np.where(a < -math.pi, a + 2 * math.pi, a))


# ---- the designed records ----------------------------------------------------------------------------------------------------
def _loguniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), size))


def _design():
    """The records in float64, before rounding to a storage dtype.  Seeded; the same numbers on every call."""
    rng = np.random.default_rng(SEED)
    cols = {k: np.zeros(N) for k in ("x", "y", "phi", "lx", "ly", "pxx", "pxy", "pyy", "r", "b", "r3", "b3", "l2x", "l2y")}
    cls = np.repeat(np.arange(len(CLASSES)), N_PER_CLASS)
    group = np.zeros(N, dtype=np.int64)
    special = np.full(N, -1, dtype=np.int64)
    obs = []                                                        # per group: (class, r, b, r3, b3)
    for ci, name in enumerate(CLASSES):
        sp = SPEC[name]
        lo, hi = sp["rng"]
        G = sp["groups"]
        idx = np.nonzero(cls == ci)[0]
        # observed ranges: the ends of the class's interval and log-spaced values in between; bearings over [-pi, pi], the ends included
        # (the outlier class: the middle of the interval, 60 sigma of range are 8 m either way; a bearing on either side)
        rs = np.exp(np.linspace(math.log(lo * 1.05), math.log(hi / 1.05), G)) if G > 2 else np.full(G, math.sqrt(lo * hi * 1.8))
        bs = rng.permutation(np.linspace(-math.pi, math.pi, G)) if G > 2 else np.array([2.6, -2.6])
        for g in range(G):
            gi = len(obs)
            members = idx[g::G]
            group[members] = gi
            r, b = float(rs[g]), float(bs[g])
            obs.append((ci, r, b, float(_loguniform(rng, lo, hi)), float(rng.uniform(-math.pi, math.pi))))
            m = len(members)
            x, y = rng.uniform(-5, 5, m), rng.uniform(-5, 5, m)
            phi = rng.uniform(-3.14, 3.14, m)
            pxx, pyy = _loguniform(rng, *sp["var"], m), _loguniform(rng, *sp["var"], m)
            if name == "correlated":
                rho = (1.0 - _loguniform(rng, 1e-6, 1e-2, m)) * rng.choice([-1.0, 1.0], m)
            else:
                rho = rng.uniform(-0.9, 0.9, m)
            pxy = rho * np.sqrt(pxx * pyy)
            # the innovation v = chol(S)' e; S depends on where the landmark ends up (1 / d in H: strongly at short range), so the
            # geometry is iterated a few times from the nominal one (landmark where the observation says)
            if name == "outlier":
                e = rng.uniform(-sp["emax"], sp["emax"], (2, m))
                e[:, :4] = sp["emax"] * np.array([[1, 1, -1, -1], [1, -1, 1, -1]])                # the corners themselves
            else:
                e = np.clip(rng.normal(0, 1, (2, m)), -sp["emax"], sp["emax"])
            d, th = np.full(m, r), phi + b
            P = np.array([[pxx, pxy], [pxy, pyy]])
            for _ in range(6):
                h = np.array([[np.cos(th), np.sin(th)], [-np.sin(th) / d, np.cos(th) / d]])       # [2, 2, m]
                S = np.einsum("ijm,jkm,lkm->ilm", h, P, h) + R_DIAG[:, :, None]
                u00 = np.sqrt(S[0, 0])
                u01 = S[0, 1] / u00
                u11 = np.sqrt(S[1, 1] - u01 * u01)
                v0 = u00 * e[0]
                v1 = np.clip(u01 * e[0] + u11 * e[1], -3.0, 3.0)
                d = 0.5 * (d + np.clip(r - v0, lo, hi))                                             # (damped: it need not converge, only settle)
                th = phi + b - v1
            v0 = r - d
            lx, ly = x + d * np.cos(th), y + d * np.sin(th)
            # the first eight: exactly on an axis or a diagonal (grid values: every sum below is exact in fp32), the heading chosen so
            # that the bearing innovation is still v1
            k = min(len(SPECIAL), m)
            for j in range(k):
                sx, sy = SPECIAL[j]
                x[j], y[j] = np.round(x[j] * GRID) / GRID, np.round(y[j] * GRID) / GRID
                a = max(np.round(d[j] / math.hypot(sx, sy) * GRID), 1.0) / GRID
                lx[j], ly[j] = x[j] + sx * a, y[j] + sy * a
                phi[j] = float(wrap(math.atan2(sy, sx) - b + v1[j]))
                phi[j] = min(max(phi[j], -3.14), 3.14)
                special[members[j]] = j
            for key, val in (("x", x), ("y", y), ("phi", phi), ("lx", lx), ("ly", ly), ("pxx", pxx), ("pxy", pxy), ("pyy", pyy)):
                cols[key][members] = val
            cols["r"][members], cols["b"][members] = r, b
            cols["r3"][members], cols["b3"][members] = obs[-1][3], obs[-1][4]
    cols["l2x"], cols["l2y"] = rng.uniform(-40, 40, N), rng.uniform(-40, 40, N)
    return cols, cls, group, special, obs


@functools.lru_cache(maxsize=None)
def table(dtype):
    """The designed records rounded to `dtype` ("f32" / "f64"), as float64 arrays that hold only values of that dtype:
    .x .y .phi (pose), .lx .ly .pxx .pxy .pyy (landmark 1), .r .b (its observation, per particle: constant within a group),
    .r3 .b3 (the first sighting of landmark 3), .cls .group .special, .obs (per group: class, r, b, r3, b3, rounded),
    .records ([3 + 5 NL, N] as slam_pf_resample_apply takes them).  Computed once, never changed."""
    cols, cls, group, special, obs = _design()
    T = NP_DTYPE[dtype]
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)                   # noqa: E731
    t = types.SimpleNamespace(dtype=dtype, cls=cls, group=group, special=special, n=N)
    for k, v in cols.items():
        setattr(t, k, rd(v))
    t.obs = [(c,) + tuple(float(rd(v)) for v in rest) for c, *rest in obs]
    assert np.all(t.pxx > 0) and np.all(t.pyy > 0) and np.all(t.pxx * t.pyy > t.pxy * t.pxy), "priors strictly positive definite after rounding"
    assert np.all(np.abs(t.phi) < math.pi) and np.all(np.abs(t.b) <= math.pi + 1e-6) and np.all(np.abs(t.b3) <= math.pi + 1e-6)
    rec = np.zeros((3 + 5 * NL, N))
    rec[0:3] = t.x, t.y, t.phi
    rec[3:8] = t.lx, t.ly, t.pxx, t.pxy, t.pyy
    rec[8:13] = t.l2x, t.l2y, rd(np.full(N, 0.01)), np.zeros(N), rd(np.full(N, 0.01))
    rec[13:18] = 0.0
    t.records = rec
    for a in vars(t).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def noise(which, dtype):
    """The noise matrix `which` ("diag" / "full") rounded to the dtype."""
    return NOISES[which].astype(NP_DTYPE[dtype]).astype(np.float64)


def group_call(t, g):
    """(z [2, 2], ids) of group g's call: landmark 1 with the group's observation, landmark 3 first sighted."""
    _c, r, b, r3, b3 = t.obs[g]
    return np.array([[r, r3], [b, b3]]), np.array([1, 3], dtype=np.int32)


# ---- the reference -----------------------------------------------------------------------------------------------------------
DEFECTS = ("no_symmetrisation", "pxy_cross_sign", "cov_1e-4", "log2pi_1.84", "atan2_no_swap_branch", "no_wrap", "h_over_d")


def _poly_atan2_f32(y, x, swap_branch=True):
    """The fp32 atan2 of csrc/pf_device.h (degree-15 odd polynomial on [0, 1], then the three reflections), float32 in and out.
    `swap_branch=False`: without `ay > ax ? pi/2 - a : a`."""
    f = np.float32
    ax, ay = np.abs(x), np.abs(y)
    t = (np.minimum(ax, ay) * (f(1) / np.maximum(ax, ay))).astype(f)
    q = t * t
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f)   # noqa: E731
    p = np.full(t.shape, 0.002622197614982724, dtype=f)
    for c in (-0.015132341533899307, 0.041121527552604675, -0.0736667662858963, 0.10573917627334595, -0.14185971021652222,
              0.1999039649963379, -0.33332985639572144):
        p = fma(p, q, f(c))
    a = (((t * q).astype(np.float64) * p.astype(np.float64)) + t.astype(np.float64)).astype(f)
    if swap_branch:
        a = np.where(ay > ax, f(1.57079633) - a, a).astype(f)
    a = np.where(x < 0, f(3.14159265) - a, a).astype(f)
    return np.copysign(a, y).astype(f)


def reference(T, t, R, defect=None):
    """OraclePF.update_known's two branches for one observation per particle, every operation in the arithmetic of T:
    landmark 1 of table `t` updated with (t.r, t.b), landmark 3 first sighted with (t.r3, t.b3), noise R ([2, 2]).
    Returns a namespace: mean [2, n], cov [3, n], inc [n] (the log-weight increment), init_mean [2, n], init_cov [3, n] and the
    intermediates the scales are built from.  `defect`: one of DEFECTS, a planted variant of the model."""
    assert defect is None or defect in DEFECTS
    c = lambda a: np.asarray(a, dtype=T)                                                       # noqa: E731
    if T is np.longdouble:
        pi = 4 * np.arctan(np.longdouble(1))
    else:
        pi = T(math.pi)
    two_pi = T(2) * pi
    log2pi = np.log(T(2) * pi) if defect != "log2pi_1.84" else T(1.84)
    half = T(0.5)
    x, y, phi = c(t.x), c(t.y), c(t.phi)
    lx, ly, pxx, pxy, pyy = c(t.lx), c(t.ly), c(t.pxx), c(t.pxy), c(t.pyy)
    r, b, r3, b3 = c(t.r), c(t.b), c(t.r3), c(t.b3)
    R00, R01, R10, R11 = (T(R[0, 0]), T(R[0, 1]), T(R[1, 0]), T(R[1, 1]))
    o = types.SimpleNamespace()
    # first sighting (src/ekf.jl:94-103,112 without the pose term)
    ang = phi + b3
    s, cs = np.sin(ang), np.cos(ang)
    g00, g01, g10, g11 = cs, -r3 * s, s, r3 * cs
    a00 = g00 * R00 + g01 * R10
    a01 = g00 * R01 + g01 * R11
    a10 = g10 * R00 + g11 * R10
    a11 = g10 * R01 + g11 * R11
    o.init_mean = np.stack([x + r3 * cs, y + r3 * s])
    o.init_cov = np.stack([a00 * g00 + a01 * g01, a00 * g10 + a01 * g11, a10 * g10 + a11 * g11])
    o.g = (g00, g01, g10, g11)
    # seen landmark
    dx, dy = lx - x, ly - y
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2)
    v0 = r - d
    if defect == "atan2_no_swap_branch":
        at = c(_poly_atan2_f32(dy.astype(np.float32), dx.astype(np.float32), swap_branch=False))
    else:
        at = np.arctan2(dy, dx)
    raw = b - (at - phi)
    o.raw_v1 = raw
    v1 = raw if defect == "no_wrap" else np.where(raw > pi, raw - two_pi, np.where(raw < -pi, raw + two_pi, raw))
    h00, h01 = dx / d, dy / d
    h10, h11 = (-dy / d, dx / d) if defect == "h_over_d" else (-dy / d2, dx / d2)
    t00 = pxx * h00 + pxy * h01
    t01 = pxx * h10 + pxy * h11
    t10 = pxy * h00 + pyy * h01
    t11 = pxy * h10 + pyy * h11
    s00 = h00 * t00 + h01 * t10 + R00
    s01 = h00 * t01 + h01 * t11 + R01
    s10 = h10 * t00 + h11 * t10 + R10
    s11 = h10 * t01 + h11 * t11 + R11
    if defect != "no_symmetrisation":
        s01 = half * (s01 + s10)
    with np.errstate(invalid="ignore", divide="ignore"):
        u00 = np.sqrt(s00)
        u01 = s01 / u00
        u11 = np.sqrt(s11 - u01 * u01)
        c00, c01, c11 = T(1) / u00, -u01 / (u00 * u11), T(1) / u11
        w00 = t00 * c00
        w01 = t00 * c01 + t01 * c11
        w10 = t10 * c00
        w11 = t10 * c01 + t11 * c11
        y0 = c00 * v0
        y1 = c01 * v0 + c11 * v1
        o.mean = np.stack([lx + w00 * y0 + w01 * y1, ly + w10 * y0 + w11 * y1])
        cross = (w00 * w10 - w01 * w11) if defect == "pxy_cross_sign" else (w00 * w10 + w01 * w11)
        o.cov = np.stack([pxx - (w00 * w00 + w01 * w01), pxy - cross, pyy - (w10 * w10 + w11 * w11)])
        if defect == "cov_1e-4":
            o.cov = o.cov * T(1.0001)
        nis = y0 * y0 + y1 * y1
        o.inc = -half * nis - np.log(u00 * u11) - log2pi
    # intermediates (the scales use the truth's)
    o.d, o.v, o.nis, o.at = d, (v0, v1), nis, at
    o.K = ((w00 * c00 + w01 * c01, w01 * c11), (w10 * c00 + w11 * c01, w11 * c11))                 # P H' S^-1 = W1 C'
    o.Sinv_v = (c00 * y0 + c01 * y1, c11 * y1)                                                      # S^-1 v = C y
    tr, det = s00 + s11, s00 * s11 - s01 * s01
    big = tr / 2 + np.sqrt(np.maximum(tr * tr / 4 - det, 0))                                       # the larger eigenvalue of S
    o.cond = big * big / det                                                                        # (the smaller one is det / big)
    return o


def as_f64(o):
    """The five compared quantities of a reference / device result as float64 arrays."""
    return {q: np.asarray(getattr(o, q) if not isinstance(o, dict) else o[q], dtype=np.float64) for q in QUANTITIES}


def scales(t, R, truth, dtype):
    """The per-record first-order rounding scales (see the header), float64 arrays shaped like the quantities."""
    eps, a_atan, a_sc = EPS[dtype], A_ATAN[dtype], A_SC[dtype]
    f = lambda a: np.abs(np.asarray(a, dtype=np.float64))                                      # noqa: E731
    d = f(truth.d)
    v0, v1 = f(truth.v[0]), f(truth.v[1])
    geo = f(t.x) + f(t.lx) + f(t.y) + f(t.ly)
    dv0 = eps * (f(t.r) + 3 * d + geo)
    dv1 = eps * (f(t.b) + 2 * math.pi + f(t.phi) + geo / d) + a_atan
    K = [[f(k) for k in row] for row in truth.K]
    cond, nis, inc = f(truth.cond), f(truth.nis), f(truth.inc)
    out = {}
    out["mean"] = np.stack([eps * f(l) + (K[i][0] * dv0 + K[i][1] * dv1) + (8 + cond) * eps * (K[i][0] * v0 + K[i][1] * v1)
                            for i, l in enumerate((t.lx, t.ly))])
    out["cov"] = np.broadcast_to(eps * np.maximum(t.pxx, t.pyy), (3, t.n)).copy()
    siv = [f(s) for s in truth.Sinv_v]
    out["inc"] = siv[0] * dv0 + siv[1] * dv1 + 8 * eps * (nis + inc + 10)
    # first sighting
    r3 = f(t.r3)
    da = eps * (f(t.phi) + f(t.b3) + f(t.phi + t.b3)) + a_sc
    out["init_mean"] = np.stack([eps * (f(t.x) + r3) + r3 * da, eps * (f(t.y) + r3) + r3 * da])
    g = [f(v) for v in truth.g]                                                                 # |g00|, |g01|, |g10|, |g11|
    dg = [da, r3 * da + eps * g[1], da, r3 * da + eps * g[3]]
    Ra = np.abs(R)
    rows = []
    for (i, j) in ((0, 0), (0, 1), (1, 1)):                                                     # entry (i, j) = sum_ab G[i, a] R[a, b] G[j, b]
        total = np.zeros(t.n)
        for a in (0, 1):
            for b_ in (0, 1):
                ga, gb = g[2 * i + a], g[2 * j + b_]
                total += (eps * ga * gb + dg[2 * i + a] * gb + ga * dg[2 * j + b_]) * Ra[a, b_]
        rows.append(total)
    out["init_cov"] = np.stack(rows)
    return out


def pos_def(cov):
    cov = np.asarray(cov, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (cov[0] > 0) & (cov[2] > 0) & (cov[0] * cov[2] > cov[1] * cov[1])


@functools.lru_cache(maxsize=None)
def case(dtype, which):
    """Everything a comparison on table(dtype) with noise `which` needs, computed once: the truth (longdouble, as float64 arrays
    for the five quantities plus the longdouble increment), the model of the dtype, the scales, the excluded records and the
    records on which the model's posterior is positive definite."""
    t = table(dtype)
    R = noise(which, dtype)
    truth = reference(np.longdouble, t, R)
    model = reference(NP_DTYPE[dtype], t, R)
    T = NP_DTYPE[dtype]
    posterior_rounded = np.asarray(truth.cov).astype(T).astype(np.float64)
    excluded = ~pos_def(posterior_rounded)
    return types.SimpleNamespace(t=t, R=R, truth=as_f64(truth), truth_ld=truth, model=as_f64(model), scales=scales(t, R, truth, dtype),
                                 excluded=excluded, model_pd=pos_def(as_f64(model)["cov"]), dtype=dtype, which=which)


def ratios(got, cs):
    """error / scale per quantity and particle ([n], the largest over the quantity's components)."""
    out = {}
    for q in QUANTITIES:
        g, w, s = np.asarray(got[q], dtype=np.float64), cs.truth[q], cs.scales[q]
        with np.errstate(invalid="ignore"):
            e = np.abs(g - w) / s
        out[q] = e if e.ndim == 1 else e.max(axis=0)
    return out


def derive_margins(dtype):
    """{class: {quantity: 4 x the worst model error / scale over both noise matrices, at least 4}} -- the rule of the header."""
    out = {}
    for ci, name in enumerate(CLASSES):
        out[name] = {}
        for q in QUANTITIES:
            worst = 0.0
            for which in NOISES:
                cs = case(dtype, which)
                sel = (cs.t.cls == ci) & ~cs.excluded
                worst = max(worst, float(np.max(ratios(cs.model, cs)[q][sel])))
            out[name][q] = max(4.0, 4.0 * worst)
    return out


def compare_records(got, truth, scales_, margins, cls, excluded=None, model_pd=None, compared=None, enforce=True):
    """`got`, `truth`, `scales_`: {quantity: array [k, n] or [n]} over ALL particles of the table; `margins`: {class: {quantity: m}};
    `cls` [n] the class index.  Every particle of every class must be compared (`compared` [n] bool says which columns of `got`
    were filled in -- all of them unless the caller ran only some groups, which this function refuses), except the `excluded`
    ones (capped at EXCLUDE_CAP per class).  Everything must be finite, every error within margin x scale, and the posterior
    positive definite wherever `model_pd` says the model's is.  Returns {(class, quantity): worst error / bound}.
    `enforce=False` (the CPU test's survey of planted defects): the bounds and the definiteness are reported, not asserted --
    a non-finite value counts as infinitely far off, (class, "pd") is the number of posteriors that lost definiteness."""
    n = len(cls)
    excluded = np.zeros(n, dtype=bool) if excluded is None else np.asarray(excluded, dtype=bool)
    compared = np.ones(n, dtype=bool) if compared is None else np.asarray(compared, dtype=bool)
    assert compared.shape == (n,) and compared.all(), f"{int((~compared).sum())} particles were never run"
    out = {}
    for ci, name in enumerate(CLASSES):
        sel = cls == ci
        assert sel.sum() >= 1000, f"class {name}: {int(sel.sum())} particles"
        assert excluded[sel].sum() <= EXCLUDE_CAP * sel.sum() + 1e-9, f"class {name}: {int(excluded[sel].sum())} records left out"
        keep = sel & ~excluded
        for q in QUANTITIES:
            g = np.asarray(got[q], dtype=np.float64)
            w, s = np.asarray(truth[q], dtype=np.float64), np.asarray(scales_[q], dtype=np.float64)
            assert g.shape == w.shape == s.shape and g.shape[-1] == n, f"{q}: the whole table, in the truth's shape"
            assert not enforce or np.all(np.isfinite(g[..., sel])), f"class {name}: {q} not finite"
            with np.errstate(invalid="ignore"):
                ratio = np.abs(g[..., keep] - w[..., keep]) / (margins[name][q] * s[..., keep])
            out[(name, q)] = float(np.where(np.isfinite(ratio), ratio, np.inf).max())
            assert ratio.shape[-1] == keep.sum() == sel.sum() - excluded[sel].sum()
    lost = (np.asarray(model_pd, dtype=bool) & ~pos_def(got["cov"])) if model_pd is not None else np.zeros(n, dtype=bool)
    if not enforce:
        for ci, name in enumerate(CLASSES):
            out[(name, "pd")] = int(lost[cls == ci].sum())
        return out
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, "beyond margin x scale (error / bound): " + ", ".join(f"{c}.{q} {v:.3g}" for (c, q), v in bad.items())
    assert not lost.any(), f"{int(lost.sum())} posteriors lost positive definiteness where the model keeps it (first: particle {int(np.argmax(lost))})"
    return out


def compare_case(got, cs, margins=None, compared=None, enforce=True):
    """compare_records for a `case`."""
    return compare_records(got, cs.truth, cs.scales, MARGINS[cs.dtype] if margins is None else margins, cs.t.cls, excluded=cs.excluded,
                           model_pd=cs.model_pd, compared=compared, enforce=enforce)


def planted(name, dtype="f32", which="diag"):
    """The five quantities of the dtype's model with the planted defect `name` (DEFECTS), on table(dtype) and noise `which`."""
    return as_f64(reference(NP_DTYPE[dtype], table(dtype), noise(which, dtype), defect=name))


# ---- the suite's own bounds on the same records ------------------------------------------------------------------------------
OLD_TOL = {"f64": 1e-9, "f32": 2e-4}                                         # tests/test_gpu_pf.py::TOL


def old_bounds_accept(got, cs, sel, n_global=2 * N):
    """tests/test_gpu_pf.py::test_predict_update_weights_against_oracle's assertions (close with TOL, 10 x on covariances and
    log-weights, its scales) on the particles `sel` as if they were the filter: landmark 1 after the update, landmark 2 untouched,
    landmark 3 after its first sighting."""
    tol = OLD_TOL[cs.dtype]
    t = cs.t

    def state(q):
        means = np.stack([q["mean"][:, sel], np.stack([t.l2x[sel], t.l2y[sel]]), q["init_mean"][:, sel]])
        covs = np.stack([q["cov"][:, sel], np.stack([t.records[10, sel], t.records[11, sel], t.records[12, sel]]), q["init_cov"][:, sel]])
        return means, covs, -math.log(n_global) + q["inc"][sel]
    (gm, gc, gw), (wm, wc, ww) = state(got), state(cs.truth)
    ok_mean = np.max(np.abs(gm - wm)) <= tol * np.max(np.abs(wm))
    ok_cov = np.max(np.abs(gc - wc)) <= 10 * tol * np.max(np.abs(wc))
    ok_w = np.max(np.abs(gw - ww)) <= 10 * tol * max(1.0, float(np.max(np.abs(ww))))
    return bool(ok_mean and ok_cov and ok_w)
