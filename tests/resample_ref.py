"""Exact reference, device-order model and hard scenes of the systematic resampling (csrc/pf_device.h block_scan1024,
csrc/pf_legacy.hip pf_scan1/2 + pf_ancestor_kernel, csrc/pf_auto.hip pf_auto_scan1 + pf_auto_resample_kernel).
Host-only NumPy / Python integers; nothing here needs a GPU.

The exact reference
    w = exp(float64(logw) - gmax) with NumPy (the subtraction is the device's: one IEEE rounding, the same on both
    sides).  Every double is an integer multiple of 2^-1074, so the cdf is accumulated EXACTLY in index order on Python
    integers.  Slot p of an n-particle filter has the exact target (p + u0) / n * W (W = the exact total, u0 a double, hence a
    dyadic rational) and the exact ancestor is the first j with cdf[j] >= target.  Only particles of positive weight
    ("live") can be ancestors; the table is built from the exact number of slots at or below every live particle's cdf step.

Decided and undecided slots
    The device's cdf is a floating-point one and its `exp` is another library's.  A slot is DECIDED when its exact
    target is further than delta * W from every cdf step, and only there the device must return the exact ancestor; on an
    UNDECIDED slot it must return one of the live particles on either side of the step(s) within delta * W.  With
        delta(nb) = C_DELTA * 2^-53 * (TREE_DEPTH + nb),      nb = scan blocks of 1024 particles,
        TREE_DEPTH = 23: six Hillis-Steele levels inside a wave, fifteen wave totals, the wave offset, the block offset.
    What delta has to cover, in units of W: the device compares cdf_dev[j] >= fl(fl((p + u0) / n) * total_dev); against the
    exact comparison that is wrong by at most  err(cdf_dev[j]) + err(total_dev) + 2 * 2^-53  (the two roundings of the
    target), and each of the two cdf errors is the rounding of the block scan plus 2 * 2^-53 for two `exp`s of 1 ulp (the
    device's and NumPy's).  The rounding of the scan is MEASURED on the CPU with the device-order model below, over every
    builder scene at every size the GPU tests use (tests/test_resample_ref_cpu.py::test_delta_constant_is_twice_the_measured):
        largest (2 * max_j |cdf_model[j] - cdf_exact[j]| / W + 6 * 2^-53) / (2^-53 * (TREE_DEPTH + nb))   = 0.41  (C_MEASURED)
        C_DELTA = 2 * C_MEASURED, rounded up                                                             = 0.85
    Targets lie W / n apart, and delta * n < 1e-7 at every size used, so at most ONE slot per cdf step can be undecided.
    A test may leave out (treat as undecided) at most max(2, 1e-4 n) slots per scene (`undecided_cap`); the builders assert
    it for the three offsets U0S.

The device-order model (for the CPU tests only; the GPU tests compare with the exact reference)
    `model_cdf`: block_scan1024 with its order of additions (shuffle levels 1, 2, 4, ..., 32 inside each 64-lane wave, the
    wave totals added serially from 0.0), the serial block offsets (pf_scan2_kernel = thread 0 of pf_auto_resample_kernel
    = the last workgroup of pf_auto_scan1_kernel: one order).  `legacy_search`: pf_ancestor_kernel's binary search over
    cdf[j] + boff[j / 1024].  `auto_search`: the block out of the offsets, then three rounds of probes (strides 128, 16,
    1).  `mutant=` switches ONE defect on in the model: the CPU tests assert that the scenes catch each.

Scenes (seeded; log-weights in the filter's dtype; dead particles have logw - gmax < -800, live ones > -600, so "zero weight"
means the same on the device and on the host whatever either `exp` does near the denormal range)
    depleted        1-3 % survivors at random places
    one_survivor    one live particle at index 0, 63, 64, 1023, 1024 or n - 1
    dead_blocks     whole 1024-particle blocks of dead particles between live ones, the first and the last block dead
    edge_survivors  live particles only at indices = 0, 15, 16, 127, 128 or 1023 mod 1024: the probe rounds' boundaries
    uniform         equal weights: the identity table
    two_level       a third of the weights 1, a third 1e-300, a third in between.  (1e-300 is logw = -690.8: still a NORMAL
                    double -- the smallest is e^-708.4 -- so both `exp`s are accurate and nonzero; this scene's live bound is
                    -700 instead of -600, and it has no dead particles.)
"""
import functools
import math
from fractions import Fraction
from itertools import accumulate

import numpy as np

SCAN_BLOCK = 1024
WAVE = 64
PF_BOFF_MIN_NB = 192
AUTO_NB_MAX = 2048
TREE_DEPTH = 23
EPS53 = Fraction(1, 2 ** 53)
C_MEASURED = 0.41
C_DELTA = Fraction(17, 20)
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
U0S = (2.0 ** -25, 0.37, 1.0 - 2.0 ** -25)           # the extremes resample_offset can produce, and one in between
DEAD_LOGW = -1000.0
SCENES = ("depleted", "one_survivor@0", "one_survivor@63", "one_survivor@64", "one_survivor@1023", "one_survivor@1024",
          "one_survivor@last", "dead_blocks", "edge_survivors", "uniform", "two_level")


def nblocks(n):
    return (int(n) + SCAN_BLOCK - 1) // SCAN_BLOCK


def delta(n):
    """The decidedness bound of an n-particle filter, as a Fraction (in units of W)."""
    return C_DELTA * EPS53 * (TREE_DEPTH + nblocks(n))


def undecided_cap(n):
    return max(2, int(1e-4 * n))


def weights(logw, gmax):
    """The weights as the cdf kernels form them: exp((double)logw - gmax)."""
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(logw).astype(np.float64) - float(gmax))


def _as_ints(w):
    """Positive doubles as Python integers in units of 2^-1074 (exact)."""
    m, e = np.frexp(np.asarray(w, dtype=np.float64))
    mi = (m * 2.0 ** 53).astype(np.int64).tolist()
    sh = (e.astype(np.int64) - 53 + 1074).tolist()
    return [a << s if s >= 0 else a >> -s for a, s in zip(mi, sh)]


class Exact:
    """The exact ancestor table of one resampling and what a floating-point implementation may do differently.

    anc[p]        exact ancestor of global slot p
    undecided[p]  the target of slot p lies within delta * W of a cdf step
    lo[p], hi[p]  the live particles an implementation may return for slot p (lo == hi == anc on a decided slot)
    """

    def __init__(self, logw, gmax, u0, dlt=None, w=None):
        self.w = weights(logw, gmax) if w is None else np.asarray(w, dtype=np.float64)
        n = self.n = self.w.shape[0]
        self.live = np.flatnonzero(self.w > 0)
        assert self.live.size, "no particle has weight"
        self.ints = _as_ints(self.w[self.live])
        self.cdf = list(accumulate(self.ints))             # exact, at the live particles
        W = self.W = self.cdf[-1]
        u = Fraction(float(u0))
        a, den = u.numerator, u.denominator
        assert 0 <= u < 1
        # slots q with (q + u0) / n * W <= C_k, i.e. q <= (C_k n den - a W) / (den W): floor + 1 of them
        D = den * W
        nden, aW = n * den, a * W
        self.delta = dlt = Fraction(dlt) if dlt is not None else delta(n)
        assert dlt * n < Fraction(1, 4)
        tol = dlt.numerator * n * D                        # |q D - x_k| <= delta n D, times delta's denominator
        thr = tol // dlt.denominator + 1
        cnt, near = [], []
        for k, c in enumerate(self.cdf):
            q0, r = divmod(c * nden - aW, D)               # the step's place on the slot axis: q0 + r / D
            cnt.append(min(max(q0 + 1, 0), n))
            if dlt > 0 and (r <= thr or D - r <= thr):     # (delta = 0: exact arithmetic, a tie is decided)
                near.append((k, q0, r))
        assert cnt[-1] == n
        self.copies = np.diff(np.array([0] + cnt, dtype=np.int64))
        self.anc = np.repeat(self.live, self.copies).astype(np.int64)
        self.undecided = np.zeros(n, dtype=bool)
        self.lo, self.hi = self.anc.copy(), self.anc.copy()
        for k, q0, r in near:                              # the slot below or above step k (the last step, W itself, is no boundary)
            if k == len(self.cdf) - 1:
                continue
            for q, dist in ((q0, r), (q0 + 1, D - r)):
                if 0 <= q < n and dist * dlt.denominator <= tol:
                    self.undecided[q] = True
                    self.lo[q] = min(self.lo[q], self.live[k])
                    self.hi[q] = max(self.hi[q], self.live[k + 1])

    @property
    def n_undecided(self):
        return int(self.undecided.sum())

    def check(self, anc, first=0, counts=True, what=""):
        """Assert that `anc` (the table of global slots [first, first + len)) is an admissible table; returns the number
        of undecided slots on which it differs from the exact one."""
        anc = np.asarray(anc).astype(np.int64)
        sl = slice(first, first + anc.shape[0])
        assert anc.shape[0] and first + anc.shape[0] <= self.n
        assert anc.min() >= 0 and anc.max() < self.n, f"{what}: ancestor out of range"
        dec = ~self.undecided[sl]
        bad = np.flatnonzero(dec & (anc != self.anc[sl]))
        assert bad.size == 0, (f"{what}: {bad.size} decided slots differ from the exact table, first at slot {first + bad[0]}: "
                               f"got {anc[bad[0]]}, exact {self.anc[sl][bad[0]]}")
        assert np.all((anc >= self.lo[sl]) & (anc <= self.hi[sl])), f"{what}: an undecided slot left its neighbouring candidates"
        assert np.all(np.diff(anc) >= 0), f"{what}: the table decreases"
        assert np.all(self.w[anc] > 0), f"{what}: a dead particle is an ancestor"
        if counts and anc.shape[0] == self.n:
            self.check_counts(anc, what)
        return int(np.sum(anc != self.anc[sl]))

    def check_counts(self, anc, what=""):
        """Copies of particle j within [floor(n w_j / W - eps), ceil(n w_j / W + eps)], eps = 2 delta n (either end of
        its cdf interval may move by delta W, that is delta n slots); none of a dead particle."""
        got = np.bincount(anc, minlength=self.n)
        assert got[self.w == 0].sum() == 0, f"{what}: copies of a dead particle"
        eps = 2 * self.delta * self.n
        en, ed = eps.numerator, eps.denominator
        Wd, eW = self.W * ed, en * self.W
        for j, wi, c in zip(self.live.tolist(), self.ints, got[self.live].tolist()):
            x = self.n * wi * ed
            lo, hi = (x - eW) // Wd, -((-(x + eW)) // Wd)
            assert lo <= c <= hi, f"{what}: particle {j} has {c} copies, n w / W = {float(Fraction(self.n * wi, self.W)):.6f}"


# ---- the device-order model ---------------------------------------------------------------------------------------------
def block_scan1024(v, mutant=None):
    """Inclusive scan inside every 1024-particle block ([nb, 1024] doubles) in the order of csrc/pf_device.h."""
    x = np.array(v, dtype=np.float64).reshape(-1, SCAN_BLOCK // WAVE, WAVE)
    off = 1
    while off < WAVE:                                      # Hillis-Steele over the 64 lanes: lane >= off adds lane - off
        x[..., off:] = x[..., off:] + x[..., :-off]
        off <<= 1
    tot = x[..., WAVE - 1]
    offs = np.zeros_like(tot)
    for wv in range(1, tot.shape[1]):                      # offs = 0.0 + sh16[0] + sh16[1] + ... in wave order
        offs[:, wv] = offs[:, wv - 1] + tot[:, wv - 1]
    if mutant == "wave_offset_dropped":                    # the loop stops one wave short
        offs[:, 1:] = offs[:, :-1].copy()
    return (offs[..., None] + x).reshape(-1, SCAN_BLOCK)


def model_cdf(w, mutant=None):
    """(cdf [n] inside the blocks, boff [nb + 1]): what the cdf kernels leave in memory; boff[nb] is the total."""
    n = w.shape[0]
    nb = nblocks(n)
    pad = np.zeros(nb * SCAN_BLOCK)
    pad[:n] = w
    c = block_scan1024(pad, mutant)
    bsum = c[:, SCAN_BLOCK - 1]
    boff = np.zeros(nb + 1)
    run = 0.0
    for b in range(nb):                                    # the serial order of pf_scan2_kernel
        boff[b] = run
        run = run + bsum[b]
    boff[nb] = run
    if mutant == "block_offsets_shifted":                  # block b gets the offset of block b + 1
        boff[:nb - 1] = boff[1:nb].copy()
    return c.reshape(-1)[:n].copy(), boff


def _targets(n_global, first, n, u0, total, targets):
    if targets is not None:
        return np.asarray(targets, dtype=np.float64)
    return (np.arange(first, first + n, dtype=np.float64) + float(u0)) / float(n_global) * total


def legacy_search(cdf, boff, u0, first=0, n=None, targets=None, mutant=None):
    """pf_ancestor_kernel: binary search for the first j with cdf[j] + boff[j / 1024] >= target."""
    ng = cdf.shape[0]
    t = _targets(ng, first, ng if n is None else n, u0, boff[-1], targets)
    lo = np.zeros(t.shape[0], dtype=np.int64)
    hi = np.full(t.shape[0], ng - 1, dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        c = cdf[mid] + boff[mid // SCAN_BLOCK]
        ge = (c > t) if mutant == "gt_for_ge" else (c >= t)
        hi = np.where(act & ge, mid, hi)
        lo = np.where(act & ~ge, mid + 1, lo)


def auto_search(cdf, boff, u0, first=0, n=None, targets=None, mutant=None):
    """pf_auto_resample_kernel: the block out of the offsets, then probes at strides 128, 16 and 1."""
    ng = cdf.shape[0]
    nb = boff.shape[0] - 1
    t = _targets(ng, first, ng if n is None else n, u0, boff[-1], targets)
    reach = (lambda c: c > t) if mutant == "gt_for_ge" else (lambda c: c >= t)
    bl = np.zeros(t.shape[0], dtype=np.int64)
    bh = np.full(t.shape[0], nb - 1, dtype=np.int64)
    while True:
        act = bl < bh
        if not act.any():
            break
        bm = (bl + bh) >> 1
        ge = reach(boff[bm + 1])
        bh = np.where(act & ge, bm, bh)
        bl = np.where(act & ~ge, bm + 1, bl)
    lo = bl * SCAN_BLOCK
    last = np.minimum(lo + SCAN_BLOCK - 1, ng - 1)
    bo = boff[bl]
    for stride, nprobe in ((128, 7), (16, 7), (1, 15)):
        sel = np.full(t.shape[0], nprobe, dtype=np.int64)
        for u in range(nprobe - 1, -1, -1):
            j = lo + stride * (u + 1) - 1
            c = np.where(j <= last, cdf[np.minimum(j, ng - 1)], 0.0)
            sel = np.where((j >= last) | reach(c + bo), u, sel)
        if mutant == "wrong_group_of_16" and stride == 16:  # no probe reached the target: the LAST group, not the one before
            sel = np.where(sel == nprobe, nprobe - 1, sel)
        lo = np.minimum(lo + stride * sel, last)
    return lo


MUTANTS = ("wave_offset_dropped", "block_offsets_shifted", "gt_for_ge", "wrong_group_of_16")


def model_tables(logw, gmax, u0, first=0, n=None, mutant=None):
    """(legacy table, auto table) of the device-order model."""
    c, boff = model_cdf(weights(logw, gmax), mutant)
    return legacy_search(c, boff, u0, first, n, mutant=mutant), auto_search(c, boff, u0, first, n, mutant=mutant)


def descents(cdf, boff):
    """Indices j with value[j + 1] < value[j], value = cdf + block offset: where the stored cdf is not monotone."""
    v = cdf + boff[np.arange(cdf.shape[0]) // SCAN_BLOCK]
    return np.flatnonzero(v[1:] < v[:-1]), v


def half_dead(n=5000, seed=0, floor=None):
    """The set of the non-monotonicity finding: half of the weights in U(0.5, 1), half dead (or `floor`), float64."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.0, n)
    dead = rng.permutation(n)[: n // 2]
    lw = np.log(w)
    lw[dead] = DEAD_LOGW if floor is None else math.log(floor)
    return lw


# ---- scenes -------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, n, dtype, logw, live_bound=-600.0):
        self.name, self.n, self.dtype = name, n, dtype
        self.logw = np.ascontiguousarray(logw, dtype=NP_DTYPE[dtype])
        self.gmax = float(self.logw.max())
        rel = self.logw.astype(np.float64) - self.gmax
        self.live = rel > live_bound
        assert np.all(self.live | (rel < -800.0)), f"{name}: a weight between dead and live"
        w = weights(self.logw, self.gmax)
        assert np.array_equal(w > 0, self.live)
        self.n_live = int(self.live.sum())

    @functools.lru_cache(maxsize=None)
    def exact(self, u0):
        return Exact(self.logw, self.gmax, u0)

    def assert_cap(self):
        worst = max(self.exact(u0).n_undecided for u0 in U0S)
        assert worst <= undecided_cap(self.n), f"{self.name} n={self.n}: {worst} undecided slots"
        return worst


def fits(name, n):
    """Has the scene a meaning at n particles?"""
    if name == "depleted":
        k = round(0.02 * n)
        return k >= 1 and 0.01 * n <= k <= 0.03 * n
    if name.startswith("one_survivor@"):
        at = name.split("@")[1]
        return at == "last" or int(at) < n - 1
    if name == "dead_blocks":
        return nblocks(n) >= 3
    if name == "edge_survivors":
        return n >= 16
    if name == "two_level":
        return n >= 3
    return name == "uniform"


EDGE_RESIDUES = (0, 15, 16, 127, 128, 1023)


@functools.lru_cache(maxsize=None)
def scene(name, n, dtype, seed=0):
    """The scene `name` at n particles in the filter's dtype; asserts its own hardness and the undecided cap."""
    assert fits(name, n), (name, n)
    rng = np.random.default_rng([seed, n, SCENES.index(name)])
    lw = np.full(n, DEAD_LOGW)
    idx = np.arange(n)
    bound = -600.0
    if name == "depleted":
        k = round(0.02 * n)
        live = np.sort(rng.permutation(n)[:k])
        lw[live] = rng.normal(0.0, 2.0, k)
    elif name.startswith("one_survivor@"):
        at = name.split("@")[1]
        live = np.array([n - 1 if at == "last" else int(at)])
        lw[live] = -3.25
    elif name == "dead_blocks":
        nb = nblocks(n)
        blk = idx // SCAN_BLOCK
        live = np.flatnonzero((blk % 2 == 1) & (blk < nb - 1))
        lw[live] = np.log(rng.uniform(0.5, 1.0, live.size))
    elif name == "edge_survivors":
        live = np.flatnonzero(np.isin(idx % SCAN_BLOCK, EDGE_RESIDUES))
        lw[live] = np.log(rng.uniform(0.5, 1.0, live.size))
    elif name == "uniform":
        live = idx
        lw[:] = -math.log(n)
    else:                                                  # two_level
        live = idx
        kind = rng.permutation(n) % 3
        lw[:] = np.where(kind == 0, 0.0, np.where(kind == 1, math.log(1e-300), -rng.uniform(0.0, 690.0, n)))
        bound = -700.0
    sc = Scene(name, n, dtype, lw, bound)
    assert np.array_equal(np.flatnonzero(sc.live), live), f"{name}: survivors are not where they were put"
    if name == "depleted":
        assert 0.01 * n <= sc.n_live <= 0.03 * n
    elif name.startswith("one_survivor@"):
        assert sc.n_live == 1
    elif name == "dead_blocks":
        per_block = np.bincount(idx[sc.live] // SCAN_BLOCK, minlength=nblocks(n))
        assert per_block[0] == 0 and per_block[-1] == 0 and np.all((per_block == 0) | (per_block == SCAN_BLOCK))
        assert per_block.max() == SCAN_BLOCK
    elif name == "edge_survivors":
        assert sc.n_live >= 2 and set((idx[sc.live] % SCAN_BLOCK).tolist()) <= set(EDGE_RESIDUES)
    elif name == "two_level":
        w = weights(sc.logw, sc.gmax)
        assert sc.n_live == n and w.max() == 1.0 and 0 < w.min() < 1e-299
    sc.worst_undecided = sc.assert_cap()
    return sc


GPU_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 5000, 16 * 1024 + 1)


def gpu_cells():
    """(scene name, n) of every cell of tests/test_gpu_pf_resample.py's table test: every scene that fits every size."""
    return [(name, n) for n in GPU_SIZES for name in SCENES if fits(name, n)]


# ---- depleted weights through the real API (tests/test_gpu_pf_resample.py, part c) --------------------------------------
# One pose, landmarks with per-particle jitter, ONE step (predict with Q: every pose distinct; one known-id observation with a
# tight R).  The R values were found with the float64 oracle (oracle/pf_ref.py; tests/test_resample_ref_cpu.py repeats it):
#   "few"   R = diag(rho^2, (rho / 20)^2), rho = sqrt(6 / (165 n)): the oracle's Neff is 4.5 .. 8.1 at every API_SIZES entry
#           (Neff grows as 165 n rho^2 in this scene), about 2000 particles keep a positive weight
#   "one"   rho = 2e-5 and the range reading 1 m off: the second-best particle is > 1e7 below the best, Neff = 1 exactly
API_SEED = 11
API_LM = np.array([[20.0, 5.0], [-8.0, 15.0]])
API_Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
API_CTL = (5.0, 0.02, 4.0, 0.1)                            # V, G, wheelbase, dt
API_JITTER = 0.05
API_SIZES = (3000 + 37, 65536 + 77, 191 * 1024, 192 * 1024, 192 * 1024 + 1, 1024 * 1024 + 1025, 2048 * 1024, 2048 * 1024 + 1)
NEFF_FEW = (2.0, 32.0)                                     # "a few particles": the oracle's 4.5 .. 8.1 with a factor of 4 for
                                                           # the fp32 rounding of the innovations (2 % of sigma at 2 M particles)


def api_cell(kind, n, step=0):
    """(initial landmark variance, z [2, 1], ids, R) of the depleted step `step` (0, 1, 2: landmarks 1, 2, 2)."""
    lid = 1 if step == 0 else 2
    px = 0.5 * (step + 1)                                  # where the nominal vehicle is after step + 1 moves of V dt
    dx, dy = API_LM[lid - 1, 0] - px, API_LM[lid - 1, 1]
    z = np.array([[math.hypot(dx, dy)], [math.atan2(dy, dx)]])
    if kind == "few":
        rho, var = math.sqrt(6.0 / (165.0 * n)), 1e-10
    else:
        rho, var = 2e-5, 1e-12
        z[0, 0] += 1.0
    return var, z, np.array([lid]), np.diag([rho ** 2, (rho / 20.0) ** 2])


def api_oracle_logw(kind, n):
    """The float64 oracle's normalised log-weights after the one step of `api_cell(kind, n)`, and its Neff."""
    from oracle import pf_ref as F
    var, z, ids, R = api_cell(kind, n)
    o = F.OraclePF(n, 2, API_SEED)
    o.set_pose([0.0, 0.0, 0.0])
    o.init_landmarks(API_LM, var, API_JITTER)
    V, G, wb, dt = API_CTL
    o.predict(V, G, wb, API_Q, dt)
    o.update_known(z, ids, R)
    gm, s1, s2 = o.weight_stats()
    o.normalize(gm, s1)
    return o.logw, s1 * s1 / s2
