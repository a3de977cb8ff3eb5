"""The joint-compatibility rule of include/slamhip_jc.h in fp64 NumPy on top of oracle.ekf_ref, run LITERALLY: the candidates, the
depth-first search with its count of evaluated tests, the decisions.  Two forms of the joint test:

* literal      dense H from predict_observation for every pairing of the hypothesis, S_H = H P H' + blockdiag(R) rebuilt and solved
               with numpy.linalg.solve at EVERY test (the pivots: numpy.linalg.cholesky succeeds and the result is finite);
* incremental  the twin of csrc/ekf_jc.hip: one cross matrix over the distinct candidate landmarks from the 5 non-zero Jacobian
               columns, the Cholesky factor grown two rows per pairing.

Both return the same record, so tests compare them field by field.  Every evaluated test is recorded in `trace` with its threshold
and the condition number of its S_H: tests/jc_scenes.verify reads the margins from there."""
import math

import numpy as np

from oracle import ekf_ref as O

MAXOBS, MAXCAND = 64, 8


def chi2_table(m, confidence=0.95):
    """The closed form for even degrees of freedom, by bisection (restated here so that the CPU tests hold the package's helper
    against an independent one)."""
    out = np.empty(m)
    for k in range(1, m + 1):
        def cdf(x):
            return 1.0 - math.exp(-x / 2) * sum((x / 2) ** i / math.factorial(i) for i in range(k))
        lo, hi = 0.0, 10.0 * k + 40.0
        for _ in range(120):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if cdf(mid) < confidence else (lo, mid)
        out[k - 1] = (lo + hi) / 2
    return out


def candidates(x, P, z, R, gate1):
    """Step 1 of the rule.  Returns cand (list of [(nis, j 1-based)] per observation, sorted, at most MAXCAND), min_i, rem,
    truncated, the table of distinct candidate landmarks in order of first appearance, and the full nis table."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    nz = z.shape[1]
    nis, _nd = O.association_table_sparse(x, P, z, R)
    cand, mins, truncated = [], [], False
    for i in range(nz):
        row = nis[i]
        with np.errstate(invalid="ignore"):
            js = np.flatnonzero(row < gate1)
        lst = sorted((float(row[j]), int(j) + 1) for j in js)
        if len(lst) > MAXCAND:
            truncated = True
            lst = lst[:MAXCAND]
        cand.append(lst)
        fin = row[~np.isnan(row)]
        mins.append(float(fin.min()) if fin.size else math.inf)
    rem = [sum(1 for t in range(i + 1, nz) if cand[t]) for i in range(nz)]
    table = []
    for lst in cand:
        for _n, j in lst:
            if j not in table:
                table.append(j)
    return cand, mins, rem, truncated, table, nis


def innovation(x, z_i, j):
    zp, _H = O.predict_observation(x, j)
    v = np.asarray(z_i, dtype=np.float64) - zp
    v[1] = O.mpi_to_pi(v[1])
    return v


def joint_literal(x, P, z, R, pairs):
    """d2, S_H and pivots-ok of the hypothesis `pairs` = [(observation, landmark 1-based)] in that order: dense H, solve."""
    m = len(pairs)
    H = np.zeros((2 * m, len(x)))
    v = np.zeros(2 * m)
    for t, (i, j) in enumerate(pairs):
        _zp, Hj = O.predict_observation(x, j)
        H[2 * t:2 * t + 2] = Hj
        v[2 * t:2 * t + 2] = innovation(x, z[:, i], j)
    S = H @ P @ H.T + np.kron(np.eye(m), R)
    try:
        Lc = np.linalg.cholesky((S + S.T) / 2)
        ok = bool(np.all(np.isfinite(Lc)))
    except np.linalg.LinAlgError:
        ok = False
    with np.errstate(all="ignore"):
        d2 = float(v @ np.linalg.solve(S, v)) if ok else math.nan
    return d2, S, ok


def cross_matrix(x, P, R, table):
    """The symmetric matrix over the distinct candidate landmarks whose 2 x 2 blocks are the blocks of every S_H, and their zp."""
    ids = np.asarray(table, dtype=np.int64)
    U = len(ids)
    if U == 0:
        return np.zeros((0, 0)), np.zeros((0, 2))
    zp, Hv, Hf = O.obs_blocks(x, ids)
    f = 3 + 2 * (ids - 1)
    Pvv = P[0:3, 0:3]
    M = np.zeros((2 * U, 2 * U))
    for a in range(U):
        Pav = P[f[a]:f[a] + 2, 0:3]
        for b in range(U):
            Pvb = P[0:3, f[b]:f[b] + 2]
            Pab = P[f[a]:f[a] + 2, f[b]:f[b] + 2]
            B = Hv[a] @ Pvv @ Hv[b].T + Hv[a] @ Pvb @ Hf[b].T + Hf[a] @ Pav @ Hv[b].T + Hf[a] @ Pab @ Hf[b].T
            M[2 * a:2 * a + 2, 2 * b:2 * b + 2] = B + (R if a == b else 0.0)
    return M, zp


class _Incremental:
    """The factor of the current S_H, two rows per pairing; test() does not change it, push() appends what test() computed."""

    def __init__(self, x, P, z, R, table):
        self.M, self.zp = cross_matrix(x, P, R, table)
        self.index = {j: u for u, j in enumerate(table)}
        self.z = z
        self.L = np.zeros((2 * MAXOBS, 2 * MAXOBS))
        self.y = np.zeros(2 * MAXOBS)
        self.d = [0.0]
        self.rows = []

    def test(self, i, j):
        u, n = self.index[j], 2 * len(self.rows)
        cols = [2 * t + q for t in self.rows for q in (0, 1)]
        b = self.M[2 * u:2 * u + 2, cols].T.copy()                 # n x 2
        for c in range(n):                                          # column-oriented forward substitution
            b[c] /= self.L[c, c]
            b[c + 1:n] -= np.outer(self.L[c + 1:n, c], b[c])
        A = self.M[2 * u:2 * u + 2, 2 * u:2 * u + 2] - b.T @ b
        with np.errstate(all="ignore"):
            p0 = A[0, 0]
            l00 = math.sqrt(p0) if p0 > 0 else math.nan
            l10 = A[1, 0] / l00
            p1 = A[1, 1] - l10 * l10
            l11 = math.sqrt(p1) if p1 > 0 else math.nan
            ok = bool(p0 > 0 and p1 > 0 and math.isfinite(p0) and math.isfinite(p1))
            v = self.z[:, i] - self.zp[u]
            v[1] = O.mpi_to_pi(v[1])
            y0 = (v[0] - b[:, 0] @ self.y[:n]) / l00
            y1 = (v[1] - b[:, 1] @ self.y[:n] - l10 * y0) / l11
            d2 = self.d[-1] + y0 * y0 + y1 * y1
        self._new = (u, b, l00, l10, l11, y0, y1, d2)
        return float(d2), ok

    def push(self):
        u, b, l00, l10, l11, y0, y1, d2 = self._new
        n = 2 * len(self.rows)
        self.L[n, :n], self.L[n + 1, :n] = b[:, 0], b[:, 1]
        self.L[n, n], self.L[n + 1, n], self.L[n + 1, n + 1] = l00, l10, l11
        self.y[n], self.y[n + 1] = y0, y1
        self.d.append(d2)
        self.rows.append(u)

    def pop(self):
        self.rows.pop()
        self.d.pop()


class _Stop(Exception):
    pass


def associate_joint(x, P, z, R, gate1, gate2, chi2, max_nodes, form="literal", want_cond=True):
    """The whole rule.  Returns a dict: assoc (int32), pairings, d2, tests, exhausted, truncated, candidates (distinct candidate
    landmarks), deepest, and trace = [(pairs tested, d2, threshold, ok, cond2(S_H) or None)] for every evaluated test, cand, mins."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    nz = z.shape[1]
    assert nz <= MAXOBS
    cand, mins, rem, truncated, table, nis = candidates(x, P, z, R, gate1)
    inc = _Incremental(x, P, z, R, table) if form == "incremental" else None
    st = dict(tests=0, exhausted=False, deepest=0, best=[], bestd=0.0, trace=[])
    H, dstack = [], [0.0]

    def walk(i):
        k = len(H)
        if i == nz:
            if k > len(st["best"]):
                st["best"], st["bestd"] = list(H), dstack[-1]
            return
        for _n, j in cand[i]:
            if any(j == jj for _i, jj in H):
                continue
            if st["tests"] == max_nodes:
                st["exhausted"] = True
                raise _Stop
            st["tests"] += 1
            st["deepest"] = max(st["deepest"], k + 1)
            if inc is not None:
                d2, ok = inc.test(i, j)
                cond = None
            else:
                d2, S, ok = joint_literal(x, P, z, R, H + [(i, j)])
                cond = float(np.linalg.cond(S)) if want_cond else None
            st["trace"].append((tuple(H + [(i, j)]), d2, float(chi2[k]), ok, cond))
            if ok and d2 < chi2[k]:
                H.append((i, j))
                dstack.append(d2)
                if inc is not None:
                    inc.push()
                walk(i + 1)
                H.pop()
                dstack.pop()
                if inc is not None:
                    inc.pop()
        if k + rem[i] > len(st["best"]):
            walk(i + 1)

    try:
        walk(0)
    except _Stop:
        pass
    assoc = np.zeros(nz, dtype=np.int32)
    paired = dict(st["best"])
    for i in range(nz):
        assoc[i] = paired[i] if i in paired else (-1 if mins[i] > gate2 else 0)
    return dict(assoc=assoc, pairings=len(st["best"]), d2=st["bestd"], tests=st["tests"], exhausted=int(st["exhausted"]),
                truncated=int(truncated), candidates=len(table), deepest=st["deepest"], trace=st["trace"], cand=cand, mins=mins,
                nis=nis, best=list(st["best"]))


def joint_nis(x, P, z, R, idf):
    """The literal d2 of the hypothesis observation i <-> landmark idf[i]."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    d2, _S, ok = joint_literal(np.asarray(x, float), np.asarray(P, float), z, R, [(i, int(j)) for i, j in enumerate(np.asarray(idf).reshape(-1))])
    assert ok
    return d2


def exhaustive_best_count(x, P, z, R, gate1, chi2):
    """The largest number of pairings over ALL hypotheses (each observation unpaired or one of its candidates, no landmark twice)
    every prefix of which passes its joint test -- the set the depth-first search walks, without its pruning."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    nz = z.shape[1]
    cand = candidates(x, P, z, R, gate1)[0]
    best = 0

    def walk(i, H):
        nonlocal best
        if i == nz:
            best = max(best, len(H))
            return
        for _n, j in cand[i]:
            if any(j == jj for _i, jj in H):
                continue
            d2, _S, ok = joint_literal(x, P, z, R, H + [(i, j)])
            if ok and d2 < chi2[len(H)]:
                walk(i + 1, H + [(i, j)])
        walk(i + 1, H)

    walk(0, [])
    return best
