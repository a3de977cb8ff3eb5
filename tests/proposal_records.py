"""Designed records for the motion model and the FastSLAM-2.0 proposal (csrc/pf_device.h: normals2, motion_pose, step_core's
written-out copy, proposal_core), with a high-precision reference per particle, first-order rounding scales built from each
record's own numbers, and planted defects.  NumPy and the oracle only.  Shared by tests/test_proposal_records_cpu.py (the records
are as hard as they claim, the reference is the oracle, the margins follow their rule, the comparison rejects the planted defects
that the scene-wide tolerances of tests/test_gpu_pf.py::test_proposal_step_against_oracle let through) and
tests/test_gpu_pf_proposal_records.py (the kernels on exactly these numbers).  The pattern, the helpers, the landmark reference,
its scales and its margins are those of tests/lm_records.py (L below); nothing of it is restated here.

RECORDS.  `table(dtype)`: N = 11 x 1001 particles (N % 64 = 3) in the ten bound classes below and `beyond`.  A particle holds NL = 66
landmark slots: 1 .. 64 seen before the call (the designed ones first, benign ones behind them), 65 and 66 empty (first sighted by
the `mixed` class).  Observations, controls, Q, dt and R are filter-wide, so a class is split into GROUPS that share one call
(`t.calls[g]`); every particle of a group is designed around that call: from its pose, the call's control gives the MEAN pose
(xm, ym, pm); the k-th designed landmark lies at range r_k - v0 in the direction pm + b_k - v1 from (xm, ym), with the innovation
v = B w* + chol(Sf) e: w* ~ N(0, I) is the particle's own control noise (clipped to 2.5; 1 .. 3 prior sigma in `informative`), e the
measurement noise -- a consistent filter -- or, in `outlier`, v = chol(B B' + Sf) e with |e| up to 60 in both components.  B and Sf depend
on where the landmark ends up, so the geometry is iterated a few times (it need not converge, only settle).  A test runs ONE call per
group from the freshly injected table, group g as the shard's g-th stepping call (the Philox step word is the call's index), and
keeps the group's particles; `compare` asserts that every particle was run and nothing else is skipped.

  class        call                                                           what it exercises
  motion       no observation; V 0 .. 30, G in +-0.6, dt 0.025 .. 1            normals2 and the motion model alone; headings over all of
                                                                              (-pi, pi], a share within 1e-3 of +-pi (the single wrap)
  weak         1 observation, suite settings (dt 0.1, R, variance 1e-2)        Sig in 0.5 .. 1 (0.8 .. 1 on these records): the suite's regime
  near         1 - 2 observations at 0.5 - 2 m                                 h10, h11 = O(1 / d): the bearing rows of B, - gl20 / - gl21
  far          200 - 2000 m                                                    d = d2 rsq(d2), cancellation in r - d
  informative  8 observations, dt 1 s, variance 1e-4                           Sig 1e-2 .. 1e-3, |mu| of 1 - 3 prior sigma
  many         M_MAX = 64 observations, dt 1 s, variance 1e-4                  64 subtractive down-dates in a row, 16 rounds of the ring
  collapsed    64 observations, dt 1 s, R x 0.01, variance 1e-6, Q x 16        Sig about 3e-7: the hardest regime in which the fp32 MODEL
                                                                              keeps every particle positive definite
  fullQR       8 observations, non-diagonal non-symmetric Q (lq10 of both      lq10 in gl.. and in Gn; both symmetrisations (f01, s01)
               signs), R_FULL only
  mixed        ids [1, 65, 2, 1, 65, 66, 3]: a repeat of an informative         pass 1 reads the PRIOR record for both copies; NEW / FRESH
               landmark, a first sighting re-observed in the call, another     observations stay out of the proposal; pass 2 in order
  outlier      1 observation, innovation up to 60 sigma of S, both components  increments of thousands in logw, mu far outside the prior
  beyond       64 observations, dt 1 s, R x 1e-4, variance 1e-8, Q x 16        NOT a bound class: the fp32 model itself loses Sig's positive
                                                                              definiteness here; finiteness rule and DESIGN.md only
M_MAX is what slam_pf_step_auto and the batch entry take (PF_AUTO_MAXOBS; pf_check_obs of the legacy entry points stops at the staging
buffer's 1024): every class goes through both forms, so the smaller maximum is the one a record can be designed for.

EXACT DIRECTIONS.  In every group with an observation eight particles see a designed landmark exactly on an axis or a diagonal FROM
THE MEAN POSE: their heading is -G (G + phi = 0: sin = 0 and cos = 1 exactly, also in the fp32 sine unit) and y = 0, so ym = 0 and
xm = fl(x + fl(V dt)) are the same bits in every arithmetic, and the landmark is placed in the arithmetic of the dtype: ly = 0,
lx = xm, or ly = +-fl(lx - xm).  Designed observation k is made for direction (k + off) mod 8 (off differs from group to group): its
bearing is set so that this particle's innovation is small; with fewer than eight observations the other exact particles are
bearing outliers (their direction is fixed, the bearing is filter-wide): harder, not easier.  Bearings are reported in [-pi, pi];
the CPU test asserts the share of bearing innovations beyond pi before the wrap (L.WRAP_SHARE_MIN).

INPUTS.  Everything is rounded to the storage dtype first: records, observations, controls, dt, Q, R.  Lq = chol(Q) is formed by the
host in double and handed to the kernel in the storage dtype: it is an input like the others, the reference takes the same values.
So are the two uniforms: u01<T> IS the dtype's rounding of (k + 0.5) 2^-24 (in fp32 the half step rounds to even from k = 2^23 on);
the Philox words and oracle/pf_ref.py::_u01 are exact, the reference rounds them to the dtype and evaluates Box-Muller in T.

REFERENCE.  `step(T, ...)` restates OraclePF.step_proposal (and with no observation OraclePF.predict) per particle in the arithmetic
of T: np.longdouble is the TRUTH, np.float64 / np.float32 the MODEL of a device that rounds every operation correctly.  Its second
pass is L.reference per observation.  The CPU test pins the float64 instance to the oracle at 1e-12.

COMPARED, each against a bound from the record's own numbers: (1) pose after the call; (2) inc, the log-weight increment (motion:
the log-weight unchanged bit for bit); (3) every updated or first-sighted landmark against L.reference(np.longdouble) evaluated from
the prior record and the DEVICE'S OWN downloaded pose (which is the pose its second pass used), with L.scales and L.MARGINS' near
(d < 5 m) / far (d > 100 m) / benign rows as they are; a second update of a slot inside the call (the repeat, the re-observed first
sighting) starts from the truth of the first and its bound carries the first one's (the prior's error passes through I - K H);
unobserved landmarks bit for bit; (4) wherever the model's pose is finite the device's must be (every class, `beyond` included, under both
noise matrices), and the landmark rule of L (model positive definite => device positive definite).

SCALES (`step(..., err=dtype)`, from the truth's intermediates; eps, a_atan, a_sc as in L).  With da(t) = eps |t| + a_sc,
dpos = eps (|x| + |V dt|) + |V dt| da(G + phi) the error of xm and ym, dpm = eps (|phi| + |V dt sG / wb|) + |V dt / wb| da(G) of pm:
  gl..  : the sines and cosines enter with da: dgl(column j) = da(G + phi) GS_j, GS = (dt lq00 + |V dt lq10|, |V dt| lq11); row 2 with da(G) / wb
  B     : dB_0j = (8 eps + 2 dpos / d) Babs_0j + (|h00| + |h01|) dgl_j;  dB_1j = (8 eps + 4 dpos / d) Babs_1j + (|h10| + |h11|) dgl_j + dgl2_j
          (Babs: the sum of the absolute terms of the entry)
  v     : L's dv0 / dv1 from the mean pose, + 2 dpos (2 dpos / d + dpm for the bearing), + the B mu term |B| dmu + dB |mu| + 4 eps |B| |mu|
  S     : dS = (8 eps + 4 dpos / d) Sfabs + dB |Sig| |B|' + |B| dSig |B|' + |B| |Sig| dB' + 8 eps |B| |Sig| |B|'
  mu    : L's mean rule with the control-space gain K = Sig B' S^-1: eps |mu| + |K| dv + (8 + cond S) eps |K| |v|, and the gain's own error
          dSig |B' S^-1 v| + |Sig| dB' |S^-1 v| + |K| dS |S^-1 v|
  Sig   : eps max(g00, g11) of the value BEFORE the down-date (the known limit of the subtractive form, as for the landmark covariance)
          + |K| dB |Sig| + its transpose + |K| dS |K|'
  inc   : L's increment rule |S^-1 v| . dv + 8 eps (nis + |inc_k| + |logw so far| + 10), + (|S^-1| : dS + |S^-1 v|' dS |S^-1 v|) / 2
all accumulated over the observations.  The a_sc terms are not decoration: B carries sines and cosines of 1e-6 absolute error, 16 eps.
The draw: de = a_norm + 4 eps |e|; chol(Sig) by the chain rule (dl00 = dg00 / 2 l00 + eps l00, ...); dw = dmu + dl |e| + |l| de;
dVn = eps (|V| + |lq00 w0|) + lq00 dw0, dGn likewise; then the motion model: dx = eps (|x| + 4 |Vn dt|) + |Vn dt| (da(Gn + phi) + dGn)
+ dt dVn, and for the heading eps (|phi| + |phi'| + 4 |Vn dt sin Gn / wb|) + (dt / wb) dVn + |Vn dt / wb| (dGn + da(Gn)).
a_norm = sqrt(-2 ln 2^-25) a_sc = 5.9e-6: csrc/pf_device.h states 1 ulp for the log and square-root units (the 4 eps |e|) and about
1e-6 ABSOLUTE for sin / cos (a_sc), and normals2 multiplies that by rad = sqrt(-2 ln u1) <= sqrt(-2 ln 2^-25) = 5.89; 0 in fp64.

BOUNDS.  bound = margin x scale, MARGINS[dtype][class][pose | inc] = max(4, 4 x the worst error / scale of the MODEL of that dtype
against the truth, over both noise matrices), rounded up with about 10 %: L's rule and L's factor 4.  Committed below; the CPU test
re-derives it.  Nothing here comes from a device's output.

EXCLUSION.  A particle is left out only if the truth's own Sig after the last down-date, or a landmark posterior of the truth, rounded to
the dtype, is not strictly positive definite; at most L.EXCLUDE_CAP of a class; fp64 leaves out none.
"""
import functools
import math
import types

import numpy as np

import lm_records as L
from oracle import pf_ref as F

NP_DTYPE, EPS, A_ATAN, A_SC = L.NP_DTYPE, L.EPS, L.A_ATAN, L.A_SC
RAD_MAX = math.sqrt(2 * 25 * math.log(2.0))                                  # sqrt(-2 ln 2^-25): the largest Box-Muller radius
A_NORM = {"f64": 0.0, "f32": RAD_MAX * A_SC["f32"]}

BOUND_CLASSES = ("motion", "weak", "near", "far", "informative", "many", "collapsed", "fullQR", "mixed", "outlier")
CLASSES = BOUND_CLASSES + ("beyond",)
N_PER_CLASS = 1001
N = N_PER_CLASS * len(CLASSES)                                               # 11011 = 172 * 64 + 3
assert N % 64 != 0
M_MAX = 64                                                                   # PF_AUTO_MAXOBS
NSEEN, NL = 64, 66
SEED = 20241019
SHARD_SEED = 5
WHEELBASE = 4.0
Q_SUITE = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])       # tests/test_gpu_pf.py::Q
QUANTITIES = ("pose", "inc")
LM_QUANTITIES = ("lm_mean", "lm_cov")
NCROSS = 8
NEAR_BELOW, FAR_ABOVE = 5.0, 100.0                                           # which row of L.MARGINS a landmark update takes

# groups, observations, dt, landmark variance, range, R scale, Q scale
SPEC = {
    "motion": dict(groups=8, m=0),
    "weak": dict(groups=4, m=1, dt=0.1, var=1e-2, rng=(10.0, 50.0)),
    "near": dict(groups=4, m=(1, 2, 1, 2), dt=0.1, var=1e-3, rng=(0.5, 2.0)),
    "far": dict(groups=4, m=1, dt=0.1, var=1e-2, rng=(200.0, 2000.0)),
    "informative": dict(groups=4, m=8, dt=1.0, var=1e-4, rng=(10.0, 50.0), wstar=(1.0, 3.0)),
    "many": dict(groups=4, m=M_MAX, dt=1.0, var=1e-4, rng=(10.0, 50.0)),
    "collapsed": dict(groups=4, m=M_MAX, dt=1.0, var=1e-6, rng=(10.0, 50.0), rs=1e-2, qs=16.0),
    "fullQR": dict(groups=4, m=8, dt=0.5, var=1e-2, rng=(10.0, 50.0), rho_q=(0.6, -0.6, 0.3, -0.9)),
    "mixed": dict(groups=4, m=3, dt=0.5, var=1e-3, rng=(10.0, 50.0)),
    "outlier": dict(groups=2, m=1, dt=0.1, var=1e-2, rng=(25.0, 35.0), emax=L.OUTLIER_SIGMAS),
    "beyond": dict(groups=4, m=M_MAX, dt=1.0, var=1e-8, rng=(10.0, 50.0), rs=1e-4, qs=16.0),
}
MIXED_IDS = (1, 65, 2, 1, 65, 66, 3)                                         # designed: positions 0, 2, 6
MOTION_CALLS = ((0.0, 0.0, 0.025), (0.5, -0.59375, 1.0), (3.0, 0.59375, 0.1), (6.0, 0.03125, 0.1), (12.0, -0.25, 0.5), (20.0, 0.125, 0.25),
                (30.0, 0.59375, 1.0), (30.0, -0.59375, 0.025))               # (V, G, dt)
GS_CALL = (0.0625, -0.125, 0.03125, -0.046875)                               # steering of the other groups (exact in fp32), V = 6

# margin = max(4, 4 x worst model error / scale), rounded up with about 10 % to spare (derive_margins; the CPU test checks it)
MARGINS = {
    "f32": {
        "motion": {"pose": 4.0, "inc": 4.0},
        "weak": {"pose": 4.0, "inc": 4.0},
        "near": {"pose": 4.0, "inc": 4.0},
        "far": {"pose": 4.0, "inc": 4.0},
        "informative": {"pose": 4.0, "inc": 4.0},
        "many": {"pose": 4.0, "inc": 4.0},
        "collapsed": {"pose": 4.0, "inc": 4.0},
        "fullQR": {"pose": 4.0, "inc": 4.0},
        "mixed": {"pose": 4.0, "inc": 4.0},
        "outlier": {"pose": 4.0, "inc": 4.0},
    },
    "f64": {
        "motion": {"pose": 5.3, "inc": 4.0},
        "weak": {"pose": 4.0, "inc": 4.0},
        "near": {"pose": 4.0, "inc": 4.0},
        "far": {"pose": 4.0, "inc": 4.0},
        "informative": {"pose": 4.0, "inc": 4.0},
        "many": {"pose": 4.0, "inc": 4.0},
        "collapsed": {"pose": 4.0, "inc": 4.0},
        "fullQR": {"pose": 4.0, "inc": 4.0},
        "mixed": {"pose": 4.0, "inc": 4.0},
        "outlier": {"pose": 4.0, "inc": 4.0},
    },
}


def classes_of(which):
    """The bound classes a run with noise matrix `which` compares: fullQR has only the non-symmetric R."""
    return tuple(c for c in BOUND_CLASSES if which == "full" or c != "fullQR")


def noise(which, dtype, rs=1.0):
    """The noise matrix `which` ("diag" / "full") times rs, rounded to the dtype."""
    return (L.NOISES[which] * rs).astype(NP_DTYPE[dtype]).astype(np.float64)


# ---- the designed records ----------------------------------------------------------------------------------------------------
def _mean_motion(x, y, phi, V, G, dt, lq):
    lq00, lq10, lq11 = lq
    s, c = np.sin(G + phi), np.cos(G + phi)
    vts, vtc = V * dt * s, V * dt * c
    gu20, gu21 = dt * math.sin(G) / WHEELBASE, V * dt * math.cos(G) / WHEELBASE
    gl = (dt * c * lq00 - vts * lq10, -vts * lq11, dt * s * lq00 + vtc * lq10, vtc * lq11, gu20 * lq00 + gu21 * lq10, gu21 * lq11)
    return x + vtc, y + vts, L.wrap(phi + V * dt * math.sin(G) / WHEELBASE), gl


def _chol_q(Q):
    lq00 = math.sqrt(Q[0, 0])
    lq10 = 0.5 * (Q[0, 1] + Q[1, 0]) / lq00
    return lq00, lq10, math.sqrt(Q[1, 1] - lq10 * lq10)


def _place(pm, gl, r, b, P, R, wstar, e, outlier, lo, hi, th_fixed):
    """Range and world direction of a landmark whose innovation under the observation (r, b) is the designed one."""
    pxx, pxy, pyy = P
    d, th = np.full(pm.shape, r), pm + b
    fixed = ~np.isnan(th_fixed)
    th = np.where(fixed, th_fixed, th)
    for _ in range(5):
        cs, sn = np.cos(th), np.sin(th)
        h00, h01, h10, h11 = cs, sn, -sn / d, cs / d
        b00, b01 = -(h00 * gl[0] + h01 * gl[2]), -(h00 * gl[1] + h01 * gl[3])
        b10, b11 = -(h10 * gl[0] + h11 * gl[2]) - gl[4], -(h10 * gl[1] + h11 * gl[3]) - gl[5]
        t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
        t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
        f00, f01, f11 = h00 * t00 + h01 * t10 + R[0, 0], h00 * t01 + h01 * t11 + 0.5 * (R[0, 1] + R[1, 0]), h10 * t01 + h11 * t11 + R[1, 1]
        if outlier:
            f00, f01, f11 = f00 + b00 * b00 + b01 * b01, f01 + b00 * b10 + b01 * b11, f11 + b10 * b10 + b11 * b11
        c00 = np.sqrt(f00)
        c10 = f01 / c00
        c11 = np.sqrt(f11 - c10 * c10)
        v0, v1 = c00 * e[0], c10 * e[0] + c11 * e[1]
        if not outlier:
            v0, v1 = v0 + b00 * wstar[0] + b01 * wstar[1], v1 + b10 * wstar[0] + b11 * wstar[1]
        d = 0.5 * (d + np.clip(r - v0, lo, hi))
        th = np.where(fixed, th_fixed, pm + b - np.clip(v1, -3.0, 3.0))
    return d, th


def _design():
    """The records in float64, before rounding to a storage dtype.  Seeded; the same numbers on every call."""
    rng = np.random.default_rng(SEED)
    rec = np.zeros((3 + 5 * NL, N))
    for l in range(NSEEN):                                                    # every seen slot benign unless designed below
        rec[3 + 5 * l], rec[4 + 5 * l] = rng.uniform(-40, 40, N), rng.uniform(-40, 40, N)
        rec[5 + 5 * l], rec[7 + 5 * l] = 0.01, 0.01
    cls = np.repeat(np.arange(len(CLASSES)), N_PER_CLASS)
    group = np.zeros(N, dtype=np.int64)
    special = np.full(N, -1, dtype=np.int64)                                  # direction index (L.SPECIAL), or -1
    special_slot = np.full(N, -1, dtype=np.int64)                             # 0-based landmark slot of the exact landmark
    calls = []
    for ci, name in enumerate(CLASSES):
        sp = SPEC[name]
        idx = np.nonzero(cls == ci)[0]
        for g in range(sp["groups"]):
            members = idx[g::sp["groups"]]
            group[members] = len(calls)
            k = len(members)
            x, y = rng.uniform(-5, 5, k), rng.uniform(-5, 5, k)
            phi = rng.uniform(-3.14, 3.14, k)
            if name == "motion":
                V, G, dt = MOTION_CALLS[g]
                edge = slice(0, k, 4)                                         # a quarter of the headings within 1e-3 of +-pi
                phi[edge] = rng.choice([-1.0, 1.0], len(phi[edge])) * (math.pi - rng.uniform(1e-6, 1e-3, len(phi[edge])))
                calls.append(types.SimpleNamespace(cls=ci, V=V, G=G, dt=dt, Q=Q_SUITE.copy(), rs=1.0, z=np.zeros((2, 0)), ids=np.zeros(0, dtype=np.int32)))
                rec[0, members], rec[1, members], rec[2, members] = x, y, phi
                continue
            V, G, dt = 6.0, GS_CALL[g], sp["dt"]
            Q = Q_SUITE * sp.get("qs", 1.0)
            if "rho_q" in sp:
                q01 = sp["rho_q"][g] * math.sqrt(Q[0, 0] * Q[1, 1])
                Q = np.array([[Q[0, 0], 1.2 * q01], [0.8 * q01, Q[1, 1]]])    # not symmetric: (Q01 + Q10) / 2 = q01
            rs = sp.get("rs", 1.0)
            R = L.R_DIAG * rs
            lq = _chol_q(Q)
            m = sp["m"][g] if isinstance(sp["m"], tuple) else sp["m"]
            lo, hi = sp["rng"]
            # the exact eight: heading -G, y = 0, x on the grid
            ns = min(len(L.SPECIAL), k)
            phi[:ns], y[:ns] = -G, 0.0
            x[:ns] = np.round(x[:ns] * L.GRID) / L.GRID
            special[members[:ns]] = np.arange(ns)
            # the next eight: a heading so close to +-pi that the MEAN heading crosses it (pm is wrapped before it is used)
            shift = V * dt * math.sin(G) / WHEELBASE
            phi[ns:ns + NCROSS] = math.copysign(1.0, shift) * (math.pi - rng.uniform(0.1, 0.9, len(phi[ns:ns + NCROSS])) * abs(shift))
            xm, ym, pm, gl = _mean_motion(x, y, phi, V, G, dt, lq)
            c0 = float(L.wrap(-G + V * dt * math.sin(G) / WHEELBASE))        # pm of the exact eight
            rs_obs = np.exp(rng.uniform(math.log(lo * 1.05), math.log(hi / 1.05), m))
            rs_obs[0], rs_obs[-1] = (lo * 1.05, hi / 1.05) if g % 2 == 0 else (hi / 1.05, lo * 1.05)
            bs_obs = rng.uniform(-math.pi, math.pi, m)
            if m > len(L.SPECIAL):
                bs_obs[-1], bs_obs[-2] = math.pi, -math.pi
            off = (3, 5, 2, 6)[g % 4]                                         # which exact direction observation 0 is made for
            for kk in range(min(ns, m)):                                      # the bearing that makes an exact particle's innovation small
                sx, sy = L.SPECIAL[(kk + off) % len(L.SPECIAL)]
                bs_obs[kk] = float(L.wrap(math.atan2(sy, sx) - c0 + rng.normal(0, math.sqrt(R[1, 1]))))
            if "wstar" in sp:
                rad, ang = rng.uniform(*sp["wstar"], k), rng.uniform(-math.pi, math.pi, k)
                wstar = np.stack([rad * np.cos(ang), rad * np.sin(ang)])
            else:
                wstar = np.clip(rng.normal(0, 1, (2, k)), -2.5, 2.5)
            slots = (0, 1, 2) if name == "mixed" else tuple(range(m))
            for kk, slot in enumerate(slots):
                var = sp["var"] * np.exp(rng.uniform(math.log(0.5), math.log(2.0), (2, k)))
                rho = rng.uniform(-0.9, 0.9, k)
                P = (var[0], rho * np.sqrt(var[0] * var[1]), var[1])
                outlier = name == "outlier"
                if outlier:
                    e = rng.uniform(-sp["emax"], sp["emax"], (2, k))
                    e[:, ns + NCROSS:ns + NCROSS + 4] = sp["emax"] * np.array([[1, 1, -1, -1], [1, -1, 1, -1]])       # the corners themselves
                else:
                    e = np.clip(rng.normal(0, 1, (2, k)), -2.5, 2.5)
                th_fixed = np.full(k, np.nan)
                for j in range(ns):
                    if ((j - off) % len(L.SPECIAL) if (j - off) % len(L.SPECIAL) < len(slots) else j % len(slots)) == kk:
                        th_fixed[j] = math.atan2(L.SPECIAL[j][1], L.SPECIAL[j][0])
                        special_slot[members[j]] = slot
                if name == "many" and kk == (m - 1 if shift > 0 else m - 2):
                    # two of the crossing particles see this observation (bearing +-pi) from the far side of the seam: the only place where
                    # the wrap of pm shows (b - atan2 + pm stays within ONE wrap of the innovation for bearings in [-pi, pi] unless the
                    # innovation itself lies within |V dt sin G / wb| of +-pi)
                    for j in (ns, ns + 1):
                        uj = (math.pi - abs(phi[j])) / abs(shift)
                        th_fixed[j] = -math.copysign(1.0, shift) * (math.pi - 0.5 * (1.0 - uj) * abs(shift))
                d, th = _place(pm, gl, rs_obs[kk], bs_obs[kk], P, R, wstar, e, outlier, 0.8 * lo, 1.25 * hi, th_fixed)
                base = 3 + 5 * slot
                rec[base, members], rec[base + 1, members] = xm + d * np.cos(th), ym + d * np.sin(th)
                rec[base + 2, members], rec[base + 3, members], rec[base + 4, members] = P
            if name == "mixed":
                z1 = np.array([rs_obs[0] * 1.001, bs_obs[0] + 0.002])                              # the repeat of landmark 1
                f65 = np.array([rng.uniform(lo, hi), rng.uniform(-3.0, 3.0)])
                f66 = np.array([rng.uniform(lo, hi), rng.uniform(-3.0, 3.0)])
                z = np.stack([[rs_obs[0], bs_obs[0]], f65, [rs_obs[1], bs_obs[1]], z1, f65 * np.array([1.0005, 1.0]) + np.array([0.0, 0.001]), f66,
                              [rs_obs[2], bs_obs[2]]], axis=1)
                ids = np.array(MIXED_IDS, dtype=np.int32)
            else:
                z, ids = np.stack([rs_obs, bs_obs]), np.arange(1, m + 1, dtype=np.int32)
            calls.append(types.SimpleNamespace(cls=ci, V=V, G=G, dt=dt, Q=Q, rs=rs, z=z, ids=ids))
            rec[0, members], rec[1, members], rec[2, members] = x, y, phi
    return rec, cls, group, special, special_slot, calls


@functools.lru_cache(maxsize=None)
def table(dtype):
    """The designed records rounded to `dtype`, as float64 arrays that hold only values of that dtype: .records ([3 + 5 NL, N] as
    slam_pf_resample_apply takes them), .cls .group .special .special_slot, .calls (per group: V, G, dt, Q, rs, z [2, m], ids, all
    rounded; group g is the shard's g-th stepping call).  Computed once, never changed."""
    rec, cls, group, special, special_slot, calls = _design()
    T = NP_DTYPE[dtype]
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)                   # noqa: E731
    rec = rd(rec)
    calls = [types.SimpleNamespace(cls=c.cls, V=float(rd(c.V)), G=float(rd(c.G)), dt=float(rd(c.dt)), Q=rd(c.Q), rs=c.rs, z=rd(c.z), ids=c.ids)
             for c in calls]
    # the exact eight, placed in the arithmetic of the dtype (see the header)
    for p in np.nonzero(special_slot >= 0)[0]:
        c = calls[group[p]]
        sx, sy = L.SPECIAL[special[p]]
        base = 3 + 5 * special_slot[p]
        assert rec[1, p] == 0.0 and rec[2, p] == -c.G
        xm = T(rec[0, p]) + T(c.V) * T(c.dt)
        a = T(max(np.round(math.hypot(rec[base, p] - float(xm), rec[base + 1, p]) / math.hypot(sx, sy) * L.GRID), 1.0) / L.GRID)
        if sx == 0:
            lx, ly = xm, T(sy) * a
        elif sy == 0:
            lx, ly = xm + T(sx) * a, T(0)
        else:
            lx = xm + T(sx) * a
            ly = T(sy) * abs(lx - xm)
        rec[base, p], rec[base + 1, p] = float(lx), float(ly)
    t = types.SimpleNamespace(dtype=dtype, cls=cls, group=group, special=special, special_slot=special_slot, n=N, records=rec, calls=calls)
    lm = rec[3:3 + 5 * NSEEN].reshape(NSEEN, 5, N)
    assert np.all(lm[:, 2] > 0) and np.all(lm[:, 4] > 0) and np.all(lm[:, 2] * lm[:, 4] > lm[:, 3] ** 2), "priors strictly positive definite after rounding"
    assert np.all(np.abs(rec[2]) < math.pi) and np.all(rec[3 + 5 * NSEEN:] == 0)
    for a in (rec, cls, group, special, special_slot):
        a.setflags(write=False)
    return t


# ---- the reference -----------------------------------------------------------------------------------------------------------
DEFECTS = ("b10_without_gl20", "no_B_mu", "q01_q10_exchanged", "lq10_ignored", "weight_from_Sf", "w1_without_l10_e1", "fresh_enters",
           "repeat_reads_updated", "pm_unwrapped", "v1_unwrapped", "gain_1_percent", "R_not_symmetrised", "second_pass_from_mean")


def normals(T, gids, stepno, seed, dtype):
    """The two normals of oracle/pf_ref.py::normals2 (same Philox words, same _u01, exact), the uniforms rounded to the storage
    dtype as u01<T> has them, Box-Muller in T."""
    gids = np.asarray(gids, dtype=np.uint64)
    r = F.philox4x32((gids & F.MASK32).astype(np.uint32), (gids >> np.uint64(32)).astype(np.uint32), np.full(gids.shape, stepno, dtype=np.uint32),
                     np.full(gids.shape, F.STREAM_PREDICT, dtype=np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1, u2 = (F._u01(w).astype(NP_DTYPE[dtype]).astype(T) for w in (r[0], r[1]))
    two_pi = 8 * np.arctan(np.longdouble(1)) if T is np.longdouble else T(2 * math.pi)
    rad = np.sqrt(T(-2) * np.log(u1))
    return rad * np.cos(two_pi * u2), rad * np.sin(two_pi * u2)


def _lm_ns(pose, rec, r, b, first):
    """One observation per particle as L.reference / L.scales take it: an update of `rec` (5 arrays), or a first sighting."""
    x, y, phi = pose
    n = len(x)
    one = np.ones(n, dtype=x.dtype)
    if first:
        return types.SimpleNamespace(x=x, y=y, phi=phi, lx=x + 10 * one, ly=y, pxx=0.01 * one, pxy=0 * one, pyy=0.01 * one, r=10 * one, b=0 * one,
                                     r3=r * one, b3=b * one, n=n)
    return types.SimpleNamespace(x=x, y=y, phi=phi, lx=rec[0], ly=rec[1], pxx=rec[2], pxy=rec[3], pyy=rec[4], r=r * one, b=b * one, r3=one, b3=0 * one, n=n)


def second_pass(T, pose, lm, seen, call, R, dtype=None):
    """OraclePF.update_known from `pose` ([3, n]) on the records `lm` ([NL, 5, n]) in the arithmetic of T, observation by observation
    through L.reference; a slot touched twice starts from its first result.  Returns (lm after the call in T, touched [NL] bool,
    bound [NL, 5, n] or None): with `dtype`, bound = L.MARGINS row x L.scales per entry, carried across a second touch."""
    c = lambda a: np.asarray(a, dtype=T)                                                          # noqa: E731
    pose, lm = c(pose), c(lm).copy()
    seen = np.array(seen, dtype=bool)
    touched = np.zeros(lm.shape[0], dtype=bool)
    bound = np.zeros(lm.shape) if dtype else None
    for i, l1 in enumerate(call.ids):
        l = int(l1) - 1
        first = not seen[l]
        ns = _lm_ns(pose, lm[l], T(call.z[0, i]), T(call.z[1, i]), first)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            o = L.reference(T, ns, R)
            if dtype:
                sc = L.scales(ns, R, o, dtype)
                if first:
                    mg = L.MARGINS[dtype]["benign"]
                    now = np.concatenate([mg["init_mean"] * sc["init_mean"], mg["init_cov"] * sc["init_cov"]])
                else:
                    d = np.asarray(o.d, dtype=np.float64)
                    pick = lambda q: np.where(d < NEAR_BELOW, L.MARGINS[dtype]["near"][q], np.where(d > FAR_ABOVE, L.MARGINS[dtype]["far"][q],   # noqa: E731
                                                                                                    L.MARGINS[dtype]["benign"][q]))
                    now = np.concatenate([pick("mean") * sc["mean"], pick("cov") * sc["cov"]])
                bound[l] = np.asarray(now, dtype=np.float64) + (bound[l] if touched[l] else 0.0)
        lm[l, 0:2], lm[l, 2:5] = (o.init_mean, o.init_cov) if first else (o.mean, o.cov)
        seen[l] = True
        touched[l] = True
    return lm, touched, bound


def step(T, pose, lm, seen, gids, stepno, seed, call, R, dtype, defect=None, err=False, logw0=0.0):
    """OraclePF.step_proposal for the particles (pose [3, n], lm [NL, 5, n], global ids gids) in the arithmetic of T, inputs as the storage
    dtype `dtype` holds them.  Returns a namespace: pose [3, n], inc [n], lm [NL, 5, n] after the call (T), sig [3, n] (Sig after the last
    down-date), mean_pose, and, with `err` (scales: meant for the truth), scale_pose [3, n], scale_inc [n] in float64 and the
    per-observation intermediates `obs` the CPU test reads.  `defect`: one of DEFECTS, a planted variant."""
    assert defect is None or defect in DEFECTS
    c = lambda a: np.asarray(a, dtype=T)                                                          # noqa: E731
    a64 = lambda q: np.abs(np.asarray(q, dtype=np.float64))                                       # noqa: E731
    pi = 4 * np.arctan(np.longdouble(1)) if T is np.longdouble else T(math.pi)
    two_pi, half = T(2) * pi, T(0.5)
    log2pi = np.log(two_pi)
    wrap = lambda a: np.where(a > pi, a - two_pi, np.where(a < -pi, a + two_pi, a))               # noqa: E731
    eps, a_atan, a_sc, a_norm = EPS[dtype], A_ATAN[dtype], A_SC[dtype], A_NORM[dtype]
    x, y, phi = c(pose)
    lm = c(lm)
    n = len(x)
    seen0 = np.array(seen, dtype=bool)
    V, G, dt, wb = T(call.V), T(call.G), T(call.dt), T(WHEELBASE)
    lq00, lq10, lq11 = (T(NP_DTYPE[dtype](v)) for v in _chol_q(np.asarray(call.Q, dtype=np.float64)))
    if defect == "lq10_ignored":
        lq10 = T(0)
    R00, R01, R10, R11 = T(R[0, 0]), T(R[0, 1]), T(R[1, 0]), T(R[1, 1])
    s, cs = np.sin(G + phi), np.cos(G + phi)
    sG, cG = np.sin(G), np.cos(G)
    vts, vtc = V * dt * s, V * dt * cs
    xm, ym = x + vtc, y + vts
    pm = phi + V * dt * sG / wb
    if defect != "pm_unwrapped":
        pm = wrap(pm)
    gu20, gu21 = dt * sG / wb, V * dt * cG / wb
    gl00, gl01 = dt * cs * lq00 + (-vts) * lq10, (-vts) * lq11
    gl10, gl11 = dt * s * lq00 + vtc * lq10, vtc * lq11
    gl20, gl21 = gu20 * lq00 + gu21 * lq10, gu21 * lq11
    mu0, mu1 = np.zeros(n, dtype=T), np.zeros(n, dtype=T)
    g00, g01, g11 = np.ones(n, dtype=T), np.zeros(n, dtype=T), np.ones(n, dtype=T)
    inc = np.zeros(n, dtype=T)
    out = types.SimpleNamespace(obs=[])
    if err:
        Vdt = abs(float(call.V) * float(call.dt))
        da0, daG = eps * a64(G + phi) + a_sc, eps * abs(float(G)) + a_sc
        dpos = eps * (np.maximum(a64(x), a64(y)) + Vdt) + Vdt * da0
        dpm = eps * (a64(phi) + a64(V * dt * sG / wb)) + Vdt / WHEELBASE * daG
        GS = (float(call.dt) * float(lq00) + Vdt * abs(float(lq10)), Vdt * float(lq11))
        dgl = [da0 * GS[0], da0 * GS[1]]
        dgl2 = [daG * GS[0] / WHEELBASE, daG * GS[1] / WHEELBASE]
        gla = [[a64(gl00), a64(gl01)], [a64(gl10), a64(gl11)], [a64(gl20), a64(gl21)]]
        dmu = [np.zeros(n), np.zeros(n)]
        dg = [[np.zeros(n), np.zeros(n)], [np.zeros(n), np.zeros(n)]]
        dinc = np.zeros(n)
        lw_run = np.full(n, abs(float(logw0)))
    first_in_call = {}
    mean_updated = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i, l1 in enumerate(call.ids):
            l = int(l1) - 1
            repeat = l in first_in_call
            first_in_call.setdefault(l, i)
            if not seen0[l] and not (defect == "fresh_enters" and repeat):
                continue
            r, b = T(call.z[0, i]), T(call.z[1, i])
            rec = lm[l]
            if not seen0[l]:                                   # (fresh_enters) a kernel that forgot FRESH_FLAG reads the record just initialised
                k0 = first_in_call[l]
                o = L.reference(T, _lm_ns(np.stack([xm, ym, pm]), rec, T(call.z[0, k0]), T(call.z[1, k0]), True), R)
                rec = np.concatenate([o.init_mean, o.init_cov])
            if defect == "repeat_reads_updated":
                if repeat:
                    rec = mean_updated[l]
                o = L.reference(T, _lm_ns(np.stack([xm, ym, pm]), rec, r, b, False), R)
                mean_updated[l] = np.concatenate([o.mean, o.cov])
            lx, ly, pxx, pxy, pyy = rec
            dx, dy = lx - xm, ly - ym
            d2 = dx * dx + dy * dy
            d = np.sqrt(d2)
            h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
            b00 = -(h00 * gl00 + h01 * gl10)
            b01 = -(h00 * gl01 + h01 * gl11)
            b10 = -(h10 * gl00 + h11 * gl10) - (T(0) if defect == "b10_without_gl20" else gl20)
            b11 = -(h10 * gl01 + h11 * gl11) - gl21
            raw = b - (np.arctan2(dy, dx) - pm)
            bm0, bm1 = (T(0), T(0)) if defect == "no_B_mu" else (b00 * mu0 + b01 * mu1, b10 * mu0 + b11 * mu1)
            v0 = (r - d) - bm0
            v1 = (raw if defect == "v1_unwrapped" else wrap(raw)) - bm1
            t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
            t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
            f00 = h00 * t00 + h01 * t10 + R00
            if defect == "R_not_symmetrised":
                f01 = h00 * t01 + h01 * t11 + R01
            else:
                f01 = half * ((h00 * t01 + h01 * t11 + R01) + (h10 * t00 + h11 * t10 + R10))
            f11 = h10 * t01 + h11 * t11 + R11
            q00, q01 = g00 * b00 + g01 * b01, g00 * b10 + g01 * b11
            q10, q11 = g01 * b00 + g11 * b01, g01 * b10 + g11 * b11
            if defect == "q01_q10_exchanged":
                q01, q10 = q10, q01
            s00 = b00 * q00 + b01 * q10 + f00
            s01 = half * ((b00 * q01 + b01 * q11 + f01) + (b10 * q00 + b11 * q10 + f01))
            s11 = b10 * q01 + b11 * q11 + f11
            u00 = np.sqrt(s00)
            u01 = s01 / u00
            u11 = np.sqrt(s11 - u01 * u01)
            c00, c01, c11 = T(1) / u00, -u01 / (u00 * u11), T(1) / u11
            w00, w01 = q00 * c00, q00 * c01 + q01 * c11
            w10, w11 = q10 * c00, q10 * c01 + q11 * c11
            if defect == "gain_1_percent":
                w00, w01, w10, w11 = (w * T(1.01) for w in (w00, w01, w10, w11))
            y0, y1 = c00 * v0, c01 * v0 + c11 * v1
            if defect == "weight_from_Sf":
                k00 = np.sqrt(f00)
                k01 = f01 / k00
                k11 = np.sqrt(f11 - k01 * k01)
                z0 = v0 / k00
                z1 = (v1 - k01 * z0) / k11
                inc_k = -half * (z0 * z0 + z1 * z1) - np.log(k00 * k11) - log2pi
            else:
                inc_k = -half * (y0 * y0 + y1 * y1) - np.log(u00 * u11) - log2pi
            if err:
                d_ = a64(d)
                geo = a64(xm) + a64(lx) + a64(ym) + a64(ly)
                ha = [[a64(h00), a64(h01)], [a64(h10), a64(h11)]]
                Ba = [[a64(b00), a64(b01)], [a64(b10), a64(b11)]]
                Sg = [[a64(g00), a64(g01)], [a64(g01), a64(g11)]]
                mua = [a64(mu0), a64(mu1)]
                Babs = [[ha[0][0] * gla[0][j] + ha[0][1] * gla[1][j] for j in (0, 1)],
                        [ha[1][0] * gla[0][j] + ha[1][1] * gla[1][j] + gla[2][j] for j in (0, 1)]]
                dB = [[(8 * eps + 2 * dpos / d_) * Babs[0][j] + (ha[0][0] + ha[0][1]) * dgl[j] for j in (0, 1)],
                      [(8 * eps + 4 * dpos / d_) * Babs[1][j] + (ha[1][0] + ha[1][1]) * dgl[j] + dgl2[j] for j in (0, 1)]]
                dBmu = [sum(dB[i][j] * mua[j] + 4 * eps * Ba[i][j] * mua[j] for j in (0, 1)) for i in (0, 1)]      # (without |B| dmu: see A below)
                dv = [eps * (abs(float(r)) + 3 * d_ + geo) + 2 * dpos + dBmu[0],
                      eps * (abs(float(b)) + 2 * math.pi + a64(pm) + geo / d_) + a_atan + 2 * dpos / d_ + dpm + dBmu[1]]
                dvf = [dv[i] + Ba[i][0] * dmu[0] + Ba[i][1] * dmu[1] for i in (0, 1)]
                va = [a64(v0), a64(v1)]
                Ks = [[w00 * c00 + w01 * c01, w01 * c11], [w10 * c00 + w11 * c01, w11 * c11]]
                K = [[a64(k) for k in row] for row in Ks]
                Bs = [[b00, b01], [b10, b11]]
                # the errors already made pass through A = I - K B (= Sig_new Sig_old^-1, a contraction in Sig's norm), entry by entry
                A = [[a64((1 if i == j else 0) - (Ks[i][0] * Bs[0][j] + Ks[i][1] * Bs[1][j])) for j in (0, 1)] for i in (0, 1)]
                u = [a64(c00 * y0 + c01 * y1), a64(c11 * y1)]                                      # |S^-1 v|
                Si = [[a64(c00 * c00 + c01 * c01), a64(c01 * c11)], [a64(c01 * c11), a64(c11 * c11)]]
                tr, det = s00 + s11, s00 * s11 - s01 * s01
                big = tr / 2 + np.sqrt(np.maximum(tr * tr / 4 - det, 0))
                cond = a64(big * big / det)
                fa = [[a64(f00), np.sqrt(a64(f00) * a64(f11))], [np.sqrt(a64(f00) * a64(f11)), a64(f11)]]
                mm = lambda A_, B_: [[A_[i][0] * B_[0][j] + A_[i][1] * B_[1][j] for j in (0, 1)] for i in (0, 1)]  # noqa: E731
                tp = lambda A_: [[A_[0][0], A_[1][0]], [A_[0][1], A_[1][1]]]                                        # noqa: E731
                BSB = [mm(mm(dB, Sg), tp(Ba)), mm(mm(Ba, Sg), tp(dB)), mm(mm(Ba, Sg), tp(Ba)), mm(mm(Ba, dg), tp(Ba))]
                dS = [[(8 * eps + 4 * dpos / d_) * fa[i][j] + BSB[0][i][j] + BSB[1][i][j] + 8 * eps * BSB[2][i][j] for j in (0, 1)] for i in (0, 1)]
                dSf = [[dS[i][j] + BSB[3][i][j] for j in (0, 1)] for i in (0, 1)]
                Btu = [Ba[0][j] * u[0] + Ba[1][j] * u[1] for j in (0, 1)]
                dBtu = [dB[0][j] * u[0] + dB[1][j] * u[1] for j in (0, 1)]
                dSu = [dS[j][0] * u[0] + dS[j][1] * u[1] for j in (0, 1)]
                Adg = mm(A, dg)
                gmax = np.maximum(a64(g00), a64(g11))
                mu_new = [a64(mu0 + (w00 * y0 + w01 * y1)), a64(mu1 + (w10 * y0 + w11 * y1))]
                dmu = [A[i][0] * dmu[0] + A[i][1] * dmu[1] + eps * mu_new[i] + K[i][0] * dv[0] + K[i][1] * dv[1]
                       + (8 + cond) * eps * (K[i][0] * va[0] + K[i][1] * va[1])
                       + Adg[i][0] * Btu[0] + Adg[i][1] * Btu[1] + Sg[i][0] * dBtu[0] + Sg[i][1] * dBtu[1] + K[i][0] * dSu[0] + K[i][1] * dSu[1]
                       for i in (0, 1)]
                M = mm(mm(K, dB), Sg)
                KSK = mm(mm(K, dS), tp(K))
                AdA = mm(Adg, tp(A))
                dg = [[AdA[i][j] + eps * gmax + M[i][j] + M[j][i] + KSK[i][j] for j in (0, 1)] for i in (0, 1)]
                nis = a64(y0 * y0 + y1 * y1)
                lw_run = lw_run + a64(inc_k)
                dinc = (dinc + u[0] * dvf[0] + u[1] * dvf[1] + 8 * eps * (nis + a64(inc_k) + lw_run + 10)
                        + 0.5 * sum(Si[i][j] * dSf[i][j] + u[i] * dSf[i][j] * u[j] for i in (0, 1) for j in (0, 1)))
                out.obs.append(types.SimpleNamespace(i=i, slot=l, d=np.asarray(d, dtype=np.float64), raw_v1=np.asarray(raw, dtype=np.float64), nis=nis,
                                                     dx=np.asarray(dx, dtype=np.float64), dy=np.asarray(dy, dtype=np.float64),
                                                     g00_before=np.asarray(g00, dtype=np.float64), h1=np.maximum(ha[1][0], ha[1][1])))
            mu0 = mu0 + (w00 * y0 + w01 * y1)
            mu1 = mu1 + (w10 * y0 + w11 * y1)
            g00 = g00 - (w00 * w00 + w01 * w01)
            g01 = g01 - (w00 * w10 + w01 * w11)
            g11 = g11 - (w10 * w10 + w11 * w11)
            inc = inc + inc_k
        e1, e2 = normals(T, gids, stepno, seed, dtype)
        l00 = np.sqrt(g00)
        l10 = g01 / l00
        l11 = np.sqrt(g11 - l10 * l10)
        w0 = mu0 + l00 * e1
        w1 = mu1 + (T(0) if defect == "w1_without_l10_e1" else l10 * e1) + l11 * e2
        Vn = V + lq00 * w0
        Gn = G + (lq10 * w0 + lq11 * w1)
        sgn = Vn * dt * np.sin(Gn) / wb
        out.pose = np.stack([x + Vn * dt * np.cos(Gn + phi), y + Vn * dt * np.sin(Gn + phi), wrap(phi + sgn)])
        if err:
            rad = np.hypot(a64(e1), a64(e2))
            de = [a_norm + 4 * eps * a64(e1) + 4 * math.pi * eps * rad, a_norm + 4 * eps * a64(e2) + 4 * math.pi * eps * rad]
            L00, L10, L11 = a64(l00), a64(l10), a64(l11)
            dl00 = dg[0][0] / (2 * L00) + eps * L00
            dl10 = dg[0][1] / L00 + L10 * dl00 / L00 + eps * L10
            dl11 = (dg[1][1] + 2 * L10 * dl10 + eps * (a64(g11) + L10 * L10)) / (2 * L11) + eps * L11
            dw0 = dmu[0] + dl00 * a64(e1) + L00 * de[0] + 2 * eps * (a64(mu0) + a64(l00 * e1))
            dw1 = dmu[1] + dl10 * a64(e1) + dl11 * a64(e2) + L10 * de[0] + L11 * de[1] + 3 * eps * (a64(mu1) + a64(l10 * e1) + a64(l11 * e2))
            q00_, q10_, q11_ = abs(float(lq00)), abs(float(lq10)), abs(float(lq11))
            dVn = eps * (abs(float(V)) + a64(lq00 * w0)) + q00_ * dw0
            dGn = eps * (abs(float(G)) + 2 * a64(lq10 * w0) + 2 * a64(lq11 * w1)) + q10_ * dw0 + q11_ * dw1
            vd, dtf = a64(Vn * dt), float(call.dt)
            daP, daN = eps * a64(Gn + phi) + a_sc, eps * a64(Gn) + a_sc
            sx = lambda p: eps * (a64(p) + 4 * vd) + vd * (daP + dGn) + dtf * dVn                  # noqa: E731
            out.scale_pose = np.stack([sx(x), sx(y), eps * (a64(phi) + a64(out.pose[2]) + 4 * a64(sgn)) + dtf / WHEELBASE * dVn + vd / WHEELBASE * (dGn + daN)])
            out.scale_inc = dinc + 8 * eps * lw_run * (len(out.obs) == 0)
    out.inc, out.sig, out.mu, out.mean_pose = inc, np.stack([g00, g01, g11]), np.stack([mu0, mu1]), np.stack([xm, ym, pm])
    from_pose = out.mean_pose if defect == "second_pass_from_mean" else out.pose
    out.lm = second_pass(T, from_pose, lm, seen0, call, R)[0] if len(call.ids) else lm
    return out


def run(T, t, which, defect=None, err=False, groups=None):
    """`step` for every group of table `t` (or `groups`) on the group's own particles, with the group's call and noise matrix `which`.
    Returns pose [3, N], inc [N], lm [NL, 5, N], sig [3, N] as float64 (NaN where no group ran) and, with `err`, scale_pose, scale_inc and
    obs (per group: the list of per-observation intermediates)."""
    res = types.SimpleNamespace(pose=np.full((3, t.n), np.nan), inc=np.full(t.n, np.nan), lm=np.full((NL, 5, t.n), np.nan), sig=np.full((3, t.n), np.nan),
                                mu=np.full((2, t.n), np.nan), scale_pose=np.full((3, t.n), np.nan), scale_inc=np.full(t.n, np.nan), obs={})
    seen = np.arange(NL) < NSEEN
    for g, call in enumerate(t.calls):
        if (groups is not None and g not in groups) or CLASSES[call.cls] not in classes_of(which) + ("beyond",):
            continue
        m = np.nonzero(t.group == g)[0]
        o = step(T, t.records[0:3, m], t.records[3:].reshape(NL, 5, t.n)[:, :, m], seen, m, g, SHARD_SEED, call, noise(which, t.dtype, call.rs), t.dtype,
                 defect=defect, err=err, logw0=-math.log(t.n))
        res.pose[:, m], res.inc[m], res.lm[:, :, m], res.sig[:, m], res.mu[:, m] = o.pose, o.inc, o.lm, o.sig, o.mu
        if err:
            res.scale_pose[:, m], res.scale_inc[m], res.obs[g] = o.scale_pose, o.scale_inc, o.obs
    return res


@functools.lru_cache(maxsize=None)
def case(dtype, which):
    """Everything a comparison on table(dtype) with noise `which` needs, computed once: truth (longdouble) and model (the dtype) as
    float64 arrays, the scales, the excluded particles (truth's Sig or a landmark posterior of the truth not positive definite in the
    dtype), the particles on which the model's pose is finite."""
    t = table(dtype)
    T = NP_DTYPE[dtype]
    truth = run(np.longdouble, t, which, err=True)
    model = run(T, t, which)
    rd = lambda a: np.asarray(a).astype(T).astype(np.float64)                                     # noqa: E731
    ran = np.isin(t.cls, [CLASSES.index(c) for c in classes_of(which) + ("beyond",)])
    touched = np.zeros((NL, t.n), dtype=bool)
    for g, call in enumerate(t.calls):
        touched[np.asarray(call.ids, dtype=np.int64)[:, None] - 1, np.nonzero(t.group == g)[0][None, :]] = True
    bad_lm = (touched & ~L.pos_def(rd(truth.lm[:, 2:5]).transpose(1, 0, 2))).any(axis=0)
    excluded = ran & (~L.pos_def(rd(truth.sig)) | bad_lm)
    return types.SimpleNamespace(t=t, dtype=dtype, which=which, truth=truth, model=model, excluded=excluded, ran=ran,
                                 model_finite=np.isfinite(model.pose).all(axis=0))


def ratios(got, cs):
    """error / scale for pose and inc per particle ([N]; the largest over the pose's coordinates; the heading's error modulo 2 pi)."""
    with np.errstate(invalid="ignore"):
        ep = np.abs(np.asarray(got["pose"], dtype=np.float64) - cs.truth.pose)
        ep[2] = np.minimum(ep[2], np.abs(ep[2] - 2 * math.pi))
        return {"pose": (ep / cs.truth.scale_pose).max(axis=0), "inc": np.abs(np.asarray(got["inc"], dtype=np.float64) - cs.truth.inc) / cs.truth.scale_inc}


def derive_margins(dtype):
    """{class: {quantity: 4 x the worst model error / scale over the noise matrices, at least 4}} -- the rule of the header."""
    out = {}
    for name in BOUND_CLASSES:
        out[name] = {}
        for q in QUANTITIES:
            worst = 0.0
            for which in L.NOISES:
                if name not in classes_of(which):
                    continue
                cs = case(dtype, which)
                sel = (cs.t.cls == CLASSES.index(name)) & ~cs.excluded
                worst = max(worst, float(np.max(ratios({"pose": cs.model.pose, "inc": cs.model.inc}, cs)[q][sel])))
            out[name][q] = max(4.0, 4.0 * worst)
    return out


def landmark_ratios(got, cs, groups=None):
    """The landmarks re-anchored: per group, L.reference(np.longdouble) from the prior records and got's OWN pose, against got's records.
    Returns (mean error / bound [N], cov error / bound [N], lost [N]: positive definiteness lost where the dtype's model from the
    same pose keeps it, untouched_equal: every unobserved landmark of every compared particle bit for bit the prior)."""
    t = cs.t
    T = NP_DTYPE[cs.dtype]
    rm, rc, lost = np.zeros(t.n), np.zeros(t.n), np.zeros(t.n, dtype=bool)
    untouched_equal = True
    seen = np.arange(NL) < NSEEN
    prior = t.records[3:].reshape(NL, 5, t.n)
    glm = np.asarray(got["lm"], dtype=np.float64)
    for g, call in enumerate(t.calls):
        m = np.nonzero((t.group == g) & cs.ran)[0]
        if not len(m) or CLASSES[call.cls] == "beyond" or (groups is not None and g not in groups):
            continue
        if not len(call.ids):
            untouched_equal &= bool(np.array_equal(glm[:, :, m], prior[:, :, m]))
            continue
        R = noise(cs.which, cs.dtype, call.rs)
        pose = np.asarray(got["pose"], dtype=np.float64)[:, m]
        want, touched, bound = second_pass(np.longdouble, pose, prior[:, :, m], seen, call, R, dtype=cs.dtype)
        model = second_pass(T, pose, prior[:, :, m], seen, call, R)[0]
        untouched_equal &= bool(np.array_equal(glm[~touched][:, :, m], prior[~touched][:, :, m]))
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.abs(glm[touched][:, :, m] - np.asarray(want[touched], dtype=np.float64)) / bound[touched]
        e = np.where(np.isfinite(e), e, np.inf)
        rm[m], rc[m] = e[:, 0:2].max(axis=(0, 1)), e[:, 2:5].max(axis=(0, 1))
        mpd = L.pos_def(np.asarray(model[touched][:, 2:5], dtype=np.float64).transpose(1, 0, 2))
        gpd = L.pos_def(glm[touched][:, 2:5][:, :, m].transpose(1, 0, 2))
        lost[m] = (mpd & ~gpd).any(axis=0)
    return rm, rc, lost, untouched_equal


def compare(got, cs, margins=None, compared=None, enforce=True, groups=None):
    """`got`: {"pose" [3, N], "inc" [N], "lm" [NL, 5, N]} over ALL particles of the table, each from its own group's call (`compared` [N]
    says which were run: all of the classes of cs.which, or this function refuses).  Every bound class: pose and inc within
    margin x scale, the landmarks within their re-anchored bounds, unobserved landmarks untouched, no positive definiteness lost, at
    most L.EXCLUDE_CAP excluded; every class, `beyond` included: a finite pose wherever the model's is finite.  Returns
    {(class, quantity): worst error / bound} plus (class, "pd") and (class, "nonfinite") counts.  `enforce=False`: reported only."""
    t = cs.t
    margins = MARGINS[cs.dtype] if margins is None else margins
    compared = np.ones(t.n, dtype=bool) if compared is None else np.asarray(compared, dtype=bool)
    assert groups is None or not enforce, "a survey of some groups asserts nothing"
    in_groups = np.ones(t.n, dtype=bool) if groups is None else np.isin(t.group, list(groups))
    assert compared[cs.ran & in_groups].all(), f"{int((~compared[cs.ran & in_groups]).sum())} particles were never run"
    r = ratios(got, cs)
    rm, rc, lost, untouched_equal = landmark_ratios(got, cs, groups)
    r["lm_mean"], r["lm_cov"] = rm, rc
    finite = np.isfinite(np.asarray(got["pose"], dtype=np.float64)).all(axis=0)
    out = {}
    for name in classes_of(cs.which) + ("beyond",):
        sel = t.cls == CLASSES.index(name)
        assert sel.sum() >= 1000
        sel = sel & in_groups
        out[(name, "nonfinite")] = int((cs.model_finite & ~finite)[sel].sum())
        if name == "beyond":
            continue
        assert cs.excluded[sel].sum() <= L.EXCLUDE_CAP * sel.sum() + 1e-9, f"class {name}: {int(cs.excluded[sel].sum())} particles left out"
        keep = sel & ~cs.excluded
        for q in QUANTITIES + LM_QUANTITIES:
            v = r[q][keep] / (margins[name][q] if q in QUANTITIES else 1.0)
            out[(name, q)] = float(np.where(np.isfinite(v), v, np.inf).max())
            assert len(v) == sel.sum() - cs.excluded[sel].sum()
        out[(name, "pd")] = int(lost[keep].sum())
    if not enforce:
        out["untouched"] = untouched_equal
        return out
    counts = ("pd", "nonfinite")
    bad = {k: v for k, v in out.items() if (k[1] in counts and v) or (k[1] not in counts and not v <= 1.0)}
    assert not bad, "beyond margin x scale (error / bound), or counts of lost definiteness / non-finite poses: " + ", ".join(
        f"{c}.{q} {v:.3g}" for (c, q), v in bad.items())
    assert untouched_equal, "an unobserved landmark changed"
    return out


def planted(name, dtype, which, groups=None):
    """The dtype's model with the planted defect `name` on table(dtype) (or on its groups `groups`), as `compare` takes it."""
    o = run(NP_DTYPE[dtype], table(dtype), which, defect=name, groups=groups)
    return {"pose": o.pose, "inc": o.inc, "lm": o.lm}


# ---- the suite's own bounds, on the suite's own scene -------------------------------------------------------------------------
def scene_accepts(defect, dtype="f32"):
    """tests/test_gpu_pf.py::test_proposal_step_against_oracle with the dtype's MODEL (planted defect `defect`, or None) in the device's
    place: the same scene, steps, tolerances and assertions (the three returned statistics from the model's log-weights).  True if
    every assertion of that test holds."""
    import test_gpu_pf as G
    T = NP_DTYPE[dtype]
    n, nl, seed = 3000 + 11, 10, 91
    lmxy = G.scene(nl, 21)
    Qf = np.array([[0.3, 0.004], [0.004, 0.003]])
    orc = F.OraclePF(n, nl, seed)
    orc.set_pose([1.0, -2.0, 0.4])
    orc.init_landmarks(lmxy[:6], 0.01, 0.1)
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)                   # noqa: E731
    pose, lm, seen, logw = orc.pose.astype(T), orc.lm.astype(T), orc.seen.copy(), orc.logw.astype(T)
    rng = np.random.default_rng(22)
    true = np.array([1.0, -2.0, 0.4])
    tol = G.TOL[dtype]
    for k in range(6):
        g = 0.04 * k - 0.1
        true = np.array([true[0] + 0.6 * math.cos(g + true[2]), true[1] + 0.6 * math.sin(g + true[2]), true[2] + 0.6 * math.sin(g) / 4.0])
        ids = np.array([1 + k % 6, 1 + (k + 3) % 6, 7 + k % 4, 1 + k % 6, 7 + k % 4])
        z = G.observe(lmxy, true, ids, rng)
        Qk = Qf if k % 2 else G.Q
        call = types.SimpleNamespace(V=6.0, G=float(rd(g)), dt=float(rd(0.1)), Q=rd(Qk), z=rd(z), ids=ids)
        o = step(T, pose, lm, seen, np.arange(n), k, seed, call, rd(G.R), dtype, defect=defect)
        orc.step_proposal(6.0, g, 4.0, Qk, 0.1, z, ids, G.R)
        pose, lm, logw = o.pose.astype(T), o.lm.astype(T), (logw + o.inc).astype(T)
        seen[ids - 1] = True
        lw = logw.astype(np.float64)
        if not np.all(np.isfinite(lw)):
            return False
        gm = float(lw.max())
        s1 = float(np.exp(lw - gm).sum())
        om, o1, _ = orc.weight_stats()
        ok = (G.close(pose, orc.pose, tol) and G.close(lm[:, 0:2], orc.lm[:, 0:2], tol)
              and G.close(lm[:, 2:5], orc.lm[:, 2:5], tol * 10, scale=float(np.max(np.abs(orc.lm[:, 2:5]))))
              and G.close(logw, orc.logw, tol * 10, scale=max(1.0, float(np.max(np.abs(orc.logw)))))
              and abs(gm - om) <= tol * 50 and abs(s1 - o1) <= tol * 200 * abs(o1))
        if not ok:
            return False
        logw = (logw - T(gm + math.log(s1))).astype(T)
        orc.normalize(om, o1)
    return True
