"""The per-particle trajectory history of include/slamhip_path.h, run literally in NumPy: a list of (poses, ancestors | None)
records, the pending map of the resamplings since the last record, and the read-outs from them.  Host only.

    record(poses)     append (poses, pending map or None); keep the last `cap`; nothing is pending afterwards
    resample(anc)     pending'[p] = pending[anc[p]], or anc[p] when nothing was pending (an ancestor outside 0 .. n - 1 counts as p)
    indices()         [L, n]: where every CURRENT particle's ancestor sits at each held record, oldest first
    trace / best / mean / survivors   read off that table

`mean` also returns what a bound on a floating-point implementation needs: the sums are formed with math.fsum (correctly
rounded: the reference adds no summation error of its own), the weights are NumPy's exp (1 ulp)."""
import math

import numpy as np

EPS52 = 2.0 ** -52


class PathRef:
    def __init__(self, n, cap):
        assert n >= 1 and cap >= 1
        self.n, self.cap = int(n), int(cap)
        self.held = []                 # (poses [3, n] float64, ancestors [n] int64 or None), oldest first
        self.pending = None
        self.records = 0
        self.resamples = 0

    # -- the rule -------------------------------------------------------------------------------------------------------------
    def record(self, poses):
        poses = np.array(poses, dtype=np.float64).reshape(3, self.n)
        self.held.append((poses, None if self.pending is None else self.pending.copy()))
        if len(self.held) > self.cap:
            del self.held[0]
        self.pending = None
        self.records += 1

    def resample(self, anc):
        a = np.array(anc, dtype=np.int64).reshape(self.n)
        own = np.arange(self.n)
        a = np.where((a < 0) | (a >= self.n), own, a)
        self.pending = a if self.pending is None else self.pending[a]
        self.resamples += 1

    @property
    def L(self):
        return len(self.held)

    def info(self):
        return dict(L=self.L, records=self.records, cap=self.cap, resamples=self.resamples)

    def get(self, k):
        """The record k back: (poses, ancestors -- the identity where none were stored --, stored?)."""
        poses, anc = self.held[self.L - 1 - k]
        return poses, (np.arange(self.n) if anc is None else anc), anc is not None

    # -- the read-outs --------------------------------------------------------------------------------------------------------
    def indices(self):
        assert self.L > 0
        out = np.empty((self.L, self.n), dtype=np.int64)
        idx = np.arange(self.n) if self.pending is None else self.pending.copy()
        for t in range(self.L - 1, -1, -1):
            out[t] = idx
            anc = self.held[t][1]
            if t > 0 and anc is not None:
                idx = anc[idx]
        return out

    def trace(self, ids):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        idx = self.indices()[:, ids]                                                   # [L, cnt]
        return np.stack([self.held[t][0][:, idx[t]].T for t in range(self.L)], axis=1)  # [cnt, L, 3]

    @staticmethod
    def best_index(logw):
        """The largest log-weight, the lowest index on a tie, a NaN never wins (all NaN: 0)."""
        lw = np.asarray(logw, dtype=np.float64)
        ok = ~np.isnan(lw)
        if not ok.any():
            return 0
        return int(np.flatnonzero(ok & (lw == lw[ok].max()))[0])

    def best(self, logw):
        b = self.best_index(logw)
        return b, self.trace([b])[0]

    def survivors(self):
        return np.array([np.unique(row).size for row in self.indices()], dtype=np.int64)

    def mean(self, logw):
        """(out [L, 4] = {x, y, phi, R}, detail): detail[t] = dict(S, C, abs = sum w |v| / sum w for v in x, y, sin, cos)."""
        lw = np.asarray(logw).astype(np.float64)
        w = np.exp(lw - lw[self.best_index(lw)])
        W = math.fsum(w)
        idx = self.indices()
        out = np.empty((self.L, 4))
        detail = []
        for t in range(self.L):
            p = self.held[t][0][:, idx[t]]
            cols = (p[0], p[1], np.sin(p[2]), np.cos(p[2]))
            sums = [math.fsum(w * v) for v in cols]
            S, Cc = sums[2] / W, sums[3] / W
            out[t] = (sums[0] / W, sums[1] / W, math.atan2(sums[2], sums[3]), math.hypot(S, Cc))
            detail.append(dict(S=S, C=Cc, abs=[math.fsum(w * np.abs(v)) / W for v in cols]))
        return out, detail


def mean_bounds(n, detail):
    """Per record the bounds on a device mean formed in double in ANY order of additions: (n + 16) 2^-52 sum w |v| / sum w for
    x, y, S = sum w sin / sum w and C = sum w cos / sum w -- n - 1 roundings of the additions in the worst order, the rest for
    4 ulp on each weight (two `exp`s of 1 ulp, the device's and NumPy's, on numerator and denominator), the products, sin / cos
    and the division -- and from them (err_S + err_C) / R for the heading.  R itself is not returned as S and C but as
    hypot(S, C), which moves by at most err_S + err_C when its arguments move by that much (1-Lipschitz in each)."""
    out = []
    for d in detail:
        e = [(n + 16) * EPS52 * a for a in d["abs"]]
        R = math.hypot(d["S"], d["C"])
        out.append(dict(x=e[0], y=e[1], S=e[2], C=e[3], phi=(e[2] + e[3]) / R, R=e[2] + e[3]))
    return out


def recover_ancestors(pre, post):
    """The ancestors of a resampling from the poses before and after it: post[:, p] is bit for bit pre[:, anc[p]].  The triples
    of `pre` must be pairwise distinct (asserted: otherwise the ancestors cannot be told apart)."""
    pre, post = np.ascontiguousarray(pre), np.ascontiguousarray(post)
    n = pre.shape[1]
    where = {}
    for p in range(n):
        where[pre[:, p].tobytes()] = p
    assert len(where) == n, f"{n - len(where)} particles share a pose before the resampling: choose another seed"
    return np.array([where[post[:, p].tobytes()] for p in range(n)], dtype=np.int64)
