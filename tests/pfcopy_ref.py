"""Literal NumPy / Python-integer models of include/slamhip_pfcopy.h (csrc/pf_copy.hip): select / copy, resize, the exact
ancestor table of n particles resampled into m slots, the pose histogram and the KLD count.  Host only; nothing here needs a GPU.

LazySource
    A particle set as the library holds it under lazy resampling: landmark l's record of particle p lies in buffer lbuf[l] at slot
    tab[ltab[l]][p] (ltab = -1: slot p).  `plain()` is what slam_pf_download returns.  `scatter()` builds one with both buffers
    full of designed values that are distinct everywhere and a random buffer and table per landmark -- so a gather that
    ignores a table or reads the wrong buffer cannot pass by accident.

select(src, ids, nl_dst, fill) / resize(src, anc, nl_dst, fill)
    The rules of the header, one NumPy statement each: dst(k, q) = src(ids[k - 1], anc[q]) read through (lbuf, ltab), the fill
    records, the log-weight rule (the downloaded values / (T)(-log m)), the RNG state and the resample count.  `mutant=`
    switches ONE defect on; tests/test_pfcopy_ref_cpu.py asserts that the designed sets catch each.

ExactInto
    tests/resample_ref.py::Exact with the target formed with m: slot q of m has the exact target (q + u0) / m * W and the exact
    ancestor is the first j with cdf[j] >= target.  Same method (Python integers in units of 2^-1074, decided and undecided
    slots), and the SAME delta: the cdf is the source's -- block_scan1024 over nb = ceil(n / 1024) blocks, so the measured
    constant of resample_ref carries over unchanged -- while the targets lie W / m apart, so the slot axis is scaled by m:
    a slot is undecided when its target is within delta(n) W of a cdf step, that is within delta(n) m slots.  delta(n) m < 1/4
    is asserted: at most one slot per side of a step.  At m == n it is Exact.  A test may treat at most max(2, 1e-4 m) slots per
    scene as undecided (`undecided_cap(m)`).

model_table
    The device-order model of the table: resample_ref.model_cdf (block_scan1024's order, serial block offsets) and the binary
    search of pc_ancestor_kernel with t_q = fl(fl(fl(q + u0) / m) * total).
"""
from fractions import Fraction
from itertools import accumulate
import math

import numpy as np

from tests import resample_ref as RR

NP_DTYPE = RR.NP_DTYPE
FILL_RECORD = {0: (0.0, 0.0, 0.0, 0.0, 0.0), 1: (0.0, 0.0, -1.0, 0.0, 0.0)}
MUTANTS = ("target_with_n", "gt_for_ge", "table_ignored", "buffer_cur_only", "fill_swapped")
# resize: the (n, m) cells of tests/test_gpu_pfcopy.py
RESIZE_NS = (65, 1025, 5013)


def resize_ms(n):
    return tuple(dict.fromkeys(m for m in (1, 64, 65, 1023, n - 1, n + 1, 2 * n + 1) if m >= 1))


def undecided_cap(m):
    return max(2, int(1e-4 * m))


# ---- designed values ---------------------------------------------------------------------------------------------------------
def designed(shape, dtype, seed):
    """Distinct bit patterns per element (a counter scrambled by the seed), negative zeros, denormals and a large value placed in;
    no NaN (array_equal) and nothing the filter would interpret: these arrays are only moved."""
    T = NP_DTYPE[dtype]
    U = np.uint32 if T == np.float32 else np.uint64
    cnt = int(np.prod(shape))
    idx = np.arange(cnt, dtype=np.uint64)
    if T == np.float32:
        bits = (np.uint64(0x3F000000) + ((idx * np.uint64(2654435761) + np.uint64(seed * 7919)) % np.uint64(0x00FFFFFF))).astype(U)
    else:
        bits = (np.uint64(0x3FE0000000000000) + ((idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed * 7919)) % np.uint64(0x000FFFFFFFFFFFFF))).astype(U)
    bits[idx % np.uint64(3) == 1] |= U(1) << U(8 * bits.itemsize - 1)          # a third negative
    a = bits.view(T).copy()
    flat = a.reshape(-1)
    tiny = np.finfo(T).tiny
    special = [T(-0.0), T(tiny / 4), T(-tiny / 8), T(np.finfo(T).max / 2), T(np.finfo(T).smallest_subnormal)]
    for i, v in enumerate(special):
        flat[(i * 37 + seed) % cnt] = v
    return a.reshape(shape)


def bits_equal(a, b):
    """Bit-for-bit equality (negative zero is not zero)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    U = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(U), b.view(U)))


# ---- a particle set as the library holds it ---------------------------------------------------------------------------------
class LazySource:
    def __init__(self, pose, logw, buf, lbuf, ltab, tabs, seen, cur=0, pend=None, seed=0, step=0, resamples=0):
        self.pose, self.logw, self.buf = pose, logw, buf                   # [3, n], [n], [2][nl, 5, n]
        self.lbuf, self.ltab, self.tabs = np.asarray(lbuf), np.asarray(ltab), tabs
        self.seen = np.asarray(seen, dtype=np.uint8)
        self.cur, self.pend, self.seed, self.step, self.resamples = cur, pend, seed, step, resamples
        self.nl, self.n = buf[0].shape[0], buf[0].shape[2]
        self.T = pose.dtype.type

    @classmethod
    def from_plain(cls, pose, logw, lm, seen, **kw):
        """Plain maps: every record in buffer 0 at its particle's slot."""
        nl, _, n = lm.shape
        return cls(pose, logw, [lm, lm], np.zeros(nl, dtype=np.int64), np.full(nl, -1), np.zeros((0, n), dtype=np.int64), seen, **kw)

    def record(self, l, mutant=None):
        """[5, n]: landmark l (0-based) of every particle, read where it lies."""
        b = self.cur if mutant == "buffer_cur_only" else int(self.lbuf[l])
        t = -1 if mutant == "table_ignored" else int(self.ltab[l])
        slot = np.arange(self.n) if t < 0 else self.tabs[t]
        return self.buf[b][l][:, slot]

    def plain(self):
        return np.stack([self.record(l) for l in range(self.nl)]) if self.nl else np.zeros((0, 5, self.n), self.T)

    def downloaded_logw(self):
        """(T)(logw - (T) pend) when a shift is pending, the stored values otherwise."""
        return self.logw if self.pend is None else (self.logw - self.T(self.pend)).astype(self.T)


def scatter(pose, logw, nl, seen, rng, ntab=3, **kw):
    """A LazySource of nl landmarks over the particles of `pose` whose records lie scattered as lazy resampling leaves them: two
    buffers of designed values, distinct everywhere, per landmark a random buffer and a random table (or none).  Table 0 is a
    real ancestor table (sorted, with repeats), the others are permutations.  plain() is the truth a copy must reproduce."""
    n = pose.shape[1]
    dtype = "f32" if pose.dtype == np.float32 else "f64"
    buf = [designed((nl, 5, n), dtype, 1000 + b) for b in range(2)]
    tabs = np.stack([rng.permutation(n) for _ in range(ntab)]) if ntab else np.zeros((0, n), dtype=np.int64)
    if ntab and n > 1:
        tabs[0] = np.sort(rng.integers(0, n, n))
    lbuf = rng.integers(0, 2, nl)
    ltab = rng.integers(-1, ntab, nl) if ntab else np.full(nl, -1)
    return LazySource(pose, logw, buf, lbuf, ltab, tabs, seen, **kw)


# ---- the rules -----------------------------------------------------------------------------------------------------------------
def _fill(nl, n, T, fill, mutant):
    if mutant == "fill_swapped":
        fill = 1 - fill
    out = np.zeros((nl, 5, n), dtype=T)
    out[:] = np.array(FILL_RECORD[fill], dtype=T)[None, :, None]
    return out


def select(src, ids, nl_dst, fill, mutant=None):
    """slam_pf_select: ids 1-based (None: 1 .. src.nl).  Returns {"pose", "logw", "lm", "seen", "seed", "step", "resamples"}."""
    ids = list(range(1, src.nl + 1)) if ids is None else [int(i) for i in ids]
    assert len(set(ids)) == len(ids) and all(1 <= i <= src.nl for i in ids) and len(ids) <= nl_dst and fill in (0, 1)
    lm = _fill(nl_dst, src.n, src.T, fill, mutant)
    seen = np.zeros(nl_dst, dtype=np.uint8)
    for k, i in enumerate(ids):
        lm[k] = src.record(i - 1, mutant)
        seen[k] = src.seen[i - 1]
    return dict(pose=src.pose.copy(), logw=src.downloaded_logw().copy(), lm=lm, seen=seen, seed=src.seed, step=src.step,
                resamples=src.resamples)


def resize(src, anc, nl_dst, fill, mutant=None):
    """slam_pf_resize given its ancestor table: dst particle q = src particle anc[q]."""
    anc = np.asarray(anc).astype(np.int64)
    m = anc.shape[0]
    assert nl_dst >= src.nl and anc.min() >= 0 and anc.max() < src.n
    lm = _fill(nl_dst, m, src.T, fill, mutant)
    seen = np.zeros(nl_dst, dtype=np.uint8)
    for l in range(src.nl):
        lm[l] = src.record(l, mutant)[:, anc]
        seen[l] = src.seen[l]
    logw = np.full(m, src.T(-math.log(m)), dtype=src.T)
    return dict(pose=src.pose[:, anc].copy(), logw=logw, lm=lm, seen=seen, seed=src.seed, step=src.step, resamples=src.resamples + 1)


def resize_weights(src, gmax):
    """exp((double)(T)(logw - (T) pend) - gmax)"""
    return RR.weights(src.downloaded_logw(), gmax)


def model_table(w, u0, m, mutant=None):
    """The device-order table of n weights into m slots (pc_scan1 / pc_scan2 / pc_ancestor_kernel)."""
    n = w.shape[0]
    cdf, boff = RR.model_cdf(np.asarray(w, dtype=np.float64))
    q = np.arange(m, dtype=np.float64)
    t = (q + float(u0)) / float(n if mutant == "target_with_n" else m) * boff[-1]
    return RR.legacy_search(cdf, boff, u0, targets=t, mutant="gt_for_ge" if mutant == "gt_for_ge" else None)


class ExactInto:
    """The exact ancestor table of n particles resampled into m slots, and what a floating-point implementation may do
    differently (see the module docstring).  Fields as resample_ref.Exact: anc, undecided, lo, hi [m]."""

    def __init__(self, logw, gmax, u0, m, w=None):
        self.w = RR.weights(logw, gmax) if w is None else np.asarray(w, dtype=np.float64)
        n = self.n = self.w.shape[0]
        m = self.m = int(m)
        self.live = np.flatnonzero(self.w > 0)
        assert self.live.size, "no particle has weight"
        self.ints = RR._as_ints(self.w[self.live])
        self.cdf = list(accumulate(self.ints))
        W = self.W = self.cdf[-1]
        u = Fraction(float(u0))
        a, den = u.numerator, u.denominator
        assert 0 <= u < 1
        # slots q with (q + u0) / m * W <= C_k, i.e. q <= (C_k m den - a W) / (den W): floor + 1 of them
        D = den * W
        mden, aW = m * den, a * W
        self.delta = dlt = RR.delta(n)                       # nb = the scan blocks of the SOURCE
        assert dlt * m < Fraction(1, 4)
        tol = dlt.numerator * m * D
        thr = tol // dlt.denominator + 1
        cnt, near = [], []
        for k, c in enumerate(self.cdf):
            q0, r = divmod(c * mden - aW, D)
            cnt.append(min(max(q0 + 1, 0), m))
            if r <= thr or D - r <= thr:
                near.append((k, q0, r))
        assert cnt[-1] == m
        self.copies = np.diff(np.array([0] + cnt, dtype=np.int64))
        self.anc = np.repeat(self.live, self.copies).astype(np.int64)
        self.undecided = np.zeros(m, dtype=bool)
        self.lo, self.hi = self.anc.copy(), self.anc.copy()
        for k, q0, r in near:
            if k == len(self.cdf) - 1:
                continue
            for q, dist in ((q0, r), (q0 + 1, D - r)):
                if 0 <= q < m and dist * dlt.denominator <= tol:
                    self.undecided[q] = True
                    self.lo[q] = min(self.lo[q], self.live[k])
                    self.hi[q] = max(self.hi[q], self.live[k + 1])

    @property
    def n_undecided(self):
        return int(self.undecided.sum())

    def check(self, anc, what=""):
        """Assert that `anc` ([m]) is an admissible table; returns the number of undecided slots on which it differs."""
        anc = np.asarray(anc).astype(np.int64)
        assert anc.shape == (self.m,), f"{what}: {anc.shape} entries for {self.m} slots"
        assert anc.min() >= 0 and anc.max() < self.n, f"{what}: ancestor out of range"
        bad = np.flatnonzero(~self.undecided & (anc != self.anc))
        assert bad.size == 0, (f"{what}: {bad.size} decided slots differ from the exact table, first at slot {bad[0]}: "
                               f"got {anc[bad[0]]}, exact {self.anc[bad[0]]}")
        assert np.all((anc >= self.lo) & (anc <= self.hi)), f"{what}: an undecided slot left its neighbouring candidates"
        assert np.all(np.diff(anc) >= 0), f"{what}: the table decreases"
        assert np.all(self.w[anc] > 0), f"{what}: a dead particle is an ancestor"
        return int(np.sum(anc != self.anc))


# ---- the pose histogram and the KLD count ------------------------------------------------------------------------------------------
PI = 3.14159265358979323846


def pose_keys(pose, cell_xy, cell_phi):
    """[n, 3] int64 cells (ix, iy, ip) of the header's rule; ValueError where the library answers SLAM_E_BADARG."""
    p = np.asarray(pose).astype(np.float64)
    if not (cell_xy > 0 and cell_phi > 0 and math.isfinite(cell_xy) and math.isfinite(cell_phi)):
        raise ValueError("cell")
    if not np.all(np.isfinite(p)):
        raise ValueError("pose not finite")
    ix, iy = np.floor(p[0] / cell_xy), np.floor(p[1] / cell_xy)
    if np.any(np.abs(ix) >= 2.0 ** 20) or np.any(np.abs(iy) >= 2.0 ** 20):
        raise ValueError("pose out of range")
    ip = np.clip(np.floor((p[2] + PI) / cell_phi), 0, math.ceil(2.0 * PI / cell_phi) - 1)
    return np.stack([ix, iy, ip], axis=1).astype(np.int64)


def pose_bins(pose, cell_xy, cell_phi):
    return int(np.unique(pose_keys(pose, cell_xy, cell_phi), axis=0).shape[0])


def kld_count(k, eps=0.05, z=2.326, n_min=64, n_max=1 << 22):
    """ceil((k - 1) / (2 eps) (1 - 2 / (9 (k - 1)) + sqrt(2 / (9 (k - 1))) z)^3), clamped; n_min for k < 2."""
    if k < 2:
        return n_min
    a = 2.0 / (9.0 * (k - 1))
    return min(max(math.ceil((k - 1) / (2.0 * eps) * (1.0 - a + math.sqrt(a) * z) ** 3), n_min), n_max)
