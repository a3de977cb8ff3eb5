"""Dense restatement of map joining (slam_ekf_join, include/slamhip_join.h) with DERIVED per-entry bounds, and a literal NumPy run
of the kernels' ownership rule on small tile-major buffers (csrc/ekf_join.hip).

    x' = (g(p_vB), mpi_to_pi(phi + phi_B), a's landmarks, g(b_1), g(b_2), ...),      P' = F P_a F' + G P_b G'

c and s are the doubles nearest to cos / sin of a's stored heading (`cs_of`: 60-digit decimal arithmetic, rounded once -- the
library forms the same two doubles in double-double arithmetic, csrc/dd_trig.h).  F and G are built from those doubles and the
stored values in np.longdouble where that has 64 significant bits (tests/strip_ref.EXTENDED; the fallback to float64 doubles
the slack as there), and so is the product.

The bound.  Every entry of P' is, as the kernels evaluate it, a sum of at most six products of stored values with entries of F and
G.  The roundings on the longest path, in units of 2^-53:
    j = -(s px + c py) as a carried dot product (dot2_rn)      1
    j * P_a[2, l], added to P_a[i, l]                             2      (GP = J_gr Pvv)
    GP[i, 2] * j_c, added to GP[i, j]                             2  (+1: j_c's own rounding)
    the rotated part R B R': two nested (c b - s b')              2 x 3 = 6 on ITS path, which is the shorter one
    the sum of both parts                                         1
that is 7 on the rank-3 path and 7 on the rotation path; nothing else is rounded before the single rounding to the dtype (the
u of the bound).  K = 16 is that count with room for the second-order terms, for FMA contraction that re-associates a product
with its sum, and for dot2_rn's residual.  K is a condition, not a knob, and stays below 64.
    |P'_got - P'_ref| <= (u + K 2^-53) (|F| |P_a| |F|' + |G| |P_b| |G|'),       u = 2^-24 (fp32) / 2^-53 (fp64)
Means: (u + K 2^-53) (|x| + |c| |px| + |s| |py|); the heading: |phi| + |phi_B| + 2 pi (one addition, the single wrap)."""
import math
from decimal import Decimal, getcontext

import numpy as np

from tests import strip_ref as SR

K = 16.0
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
LD = SR.LD
SLACK = K * SR.C_FACTOR * 2.0 ** -53
_PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803")


def _series(x, first, start):
    """sum of the alternating Taylor series with first term `first` (x or 1) and index `start` (1 or 0), decimal recipe."""
    i, last, s, fact, num, sign = start, 0, first, 1, first, 1
    for _ in range(200):
        if s == last:
            break
        last = s
        i += 2
        fact *= i * (i - 1)
        num *= x * x
        sign = -sign
        s += num / fact * sign
    return s


def cs_of(phi):
    """(c, s): the float64 nearest to cos(phi), sin(phi) of the float64 phi."""
    getcontext().prec = 70
    x = Decimal(float(phi))
    x = x - (x / (2 * _PI)).to_integral_value() * 2 * _PI           # |x| <= pi: the series loses no more than two digits
    return float(_series(x, Decimal(1), 0)), float(_series(x, x, 1))


def mpi_to_pi(phi):
    if phi > math.pi:
        return phi - 2.0 * math.pi
    if phi < -math.pi:
        return phi + 2.0 * math.pi
    return phi


def f(j):
    return 3 + 2 * (j - 1)


def g_point(pose, c, s, p):
    return np.array([pose[0] + c * p[0] - s * p[1], pose[1] + s * p[0] + c * p[1]], dtype=LD)


def J_point(c, s, p):
    one, zero = LD(1), LD(0)
    return np.array([[one, zero, -(s * p[0] + c * p[1])], [zero, one, c * p[0] - s * p[1]]], dtype=LD)


def FG(xA, xB):
    """F (n' x n_A), G (n' x n_B) in LD, and (c, s)."""
    xA, xB = np.asarray(xA, dtype=np.float64), np.asarray(xB, dtype=np.float64)
    nA, nB = xA.shape[0], xB.shape[0]
    NB = (nB - 3) // 2
    n2 = nA + 2 * NB
    c, s = (LD(v) for v in cs_of(xA[2]))
    R = np.array([[c, -s], [s, c]], dtype=LD)
    xb = xB.astype(LD)
    F = np.zeros((n2, nA), dtype=LD)
    G = np.zeros((n2, nB), dtype=LD)
    F[0:2, 0:3] = J_point(c, s, xb[0:2])
    F[2, 2] = 1
    F[3:nA, 3:nA] = np.eye(nA - 3, dtype=LD)
    G[0:2, 0:2] = R
    G[2, 2] = 1
    for j in range(1, NB + 1):
        d, b = nA + 2 * (j - 1), f(j)
        F[d:d + 2, 0:3] = J_point(c, s, xb[b:b + 2])
        G[d:d + 2, b:b + 2] = R
    return F, G, (c, s)


def state_map(xA, xB):
    """x' in LD (used for the central differences as well: any float64 inputs)."""
    xA, xB = np.asarray(xA, dtype=np.float64), np.asarray(xB, dtype=np.float64)
    c, s = (LD(v) for v in cs_of(xA[2]))
    a, b = xA.astype(LD), xB.astype(LD)
    NB = (xB.shape[0] - 3) // 2
    out = np.concatenate([a, np.zeros(2 * NB, dtype=LD)])
    out[0:2] = g_point(a, c, s, b[0:2])
    out[2] = LD(mpi_to_pi(float(xA[2]) + float(xB[2])))
    for j in range(1, NB + 1):
        out[len(a) + 2 * (j - 1):len(a) + 2 * j] = g_point(a, c, s, b[f(j):f(j) + 2])
    return out


def join(xA, PA, xB, PB):
    """(x', P') in LD from float64 copies of what the two handles hold; P' symmetrised."""
    F, G, _cs = FG(xA, xB)
    P = F @ np.asarray(PA, dtype=LD) @ F.T + G @ np.asarray(PB, dtype=LD) @ G.T
    return state_map(xA, xB), (P + P.T) / 2


def bound_P(xA, PA, xB, PB, dtype):
    F, G, _cs = FG(xA, xB)
    F, G = np.abs(F).astype(np.float64), np.abs(G).astype(np.float64)
    return (U[dtype] + SLACK) * (F @ np.abs(np.asarray(PA, dtype=np.float64)) @ F.T + G @ np.abs(np.asarray(PB, dtype=np.float64)) @ G.T)


def bound_x(xA, xB, dtype):
    c, s = (abs(v) for v in cs_of(np.asarray(xA, dtype=np.float64)[2]))
    xA, xB = np.abs(np.asarray(xA, dtype=np.float64)), np.abs(np.asarray(xB, dtype=np.float64))
    NB = (xB.shape[0] - 3) // 2
    b = np.concatenate([np.zeros_like(xA), np.zeros(2 * NB)])         # a's landmark means: bit for bit, bound 0
    pts = [(0, 0)] + [(len(xA) + 2 * (j - 1), f(j)) for j in range(1, NB + 1)]
    for d, q in pts:
        b[d] = xA[0] + c * xB[q] + s * xB[q + 1]
        b[d + 1] = xA[1] + s * xB[q] + c * xB[q + 1]
    b[2] = xA[2] + xB[2] + 2.0 * math.pi
    return (U[dtype] + SLACK) * b


def worst_ratio(got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=LD) for a in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---- blockwise form: what one owner computes ---------------------------------------------------------------------------------
def grp_first(g):
    return 2 * g if g < 2 else 2 * g - 1


def grp_size(g):
    return 1 if g == 1 else 2


def _JR(g, c, s, xb):
    if g == 1:
        return np.array([[0, 0, 1]], dtype=LD), np.array([[1]], dtype=LD)
    q = grp_first(g)
    return J_point(c, s, xb[q:q + 2]), np.array([[c, -s], [s, c]], dtype=LD)


def block_new(Pvv, Bblk, gr, gc, c, s, xb):
    """P'[dest gr, dest gc] = J_gr Pvv J_gc' + R_gr B R_gc'."""
    Jr, Rr = _JR(gr, c, s, xb)
    Jc, Rc = _JR(gc, c, s, xb)
    return Jr @ Pvv @ Jc.T + Rr @ np.asarray(Bblk, dtype=LD).reshape(grp_size(gr), grp_size(gc)) @ Rc.T


def block_cross(col3, gr, c, s, xb):
    """P'[dest gr, col] = J_gr P_a[0:3, col]."""
    Jr, _ = _JR(gr, c, s, xb)
    return Jr @ np.asarray(col3, dtype=LD).reshape(3)


def dest_first(g, NA):
    return grp_first(g) if g < 2 else grp_first(g) + 2 * NA


# ---- the kernels' ownership rule, literally, on tile-major buffers ------------------------------------------------------------
class _Buf:
    def __init__(self, buf, ld, E, frozen=False):
        self.b, self.ld, self.E, self.L, self.frozen = buf, ld, E, E.bit_length() - 1, frozen
        self.writes = np.zeros(buf.shape[0], dtype=np.int64)

    def at(self, r, c):
        assert (r >> self.L) >= (c >> self.L)
        return float(self.b[int(SR.p_off(self.ld, self.L, r, c))])

    def store_sym(self, r, c, v):                       # p_store_sym
        assert not self.frozen
        L = self.L
        for rr, cc in ((r, c), (c, r)) if r != c else ((r, c),):
            if (rr >> L) >= (cc >> L):
                o = int(SR.p_off(self.ld, L, rr, cc))
                self.b[o] = v
                self.writes[o] += 1


SC, CG = 8, 4


def _threads(NA, NB):
    """Every thread of the three launches as (launch, closure).  Launch 1: strip threads (one per (landmark j of b, column)) and
    block threads (one per (gr, chunk of CG column groups)); launch 2: one per old column; launch 3: the pose thread."""
    nA = 3 + 2 * NA
    th = []

    def strip(A, B, xa, xb, cs, j, col):
        c, s = cs
        px, py = xb[3 + 2 * j], xb[4 + 2 * j]
        j0, j1 = -(s * px + c * py), c * px - s * py
        p0, p1, p2 = A.at(col, 0), A.at(col, 1), A.at(col, 2)
        A.store_sym(nA + 2 * j, col, float(p0 + j0 * p2))
        A.store_sym(nA + 2 * j + 1, col, float(p1 + j1 * p2))

    def block(A, B, xa, xb, cs, gr, gc0):
        c, s = cs
        Pvv = np.array([[A.at(max(i, k), min(i, k)) for k in range(3)] for i in range(3)], dtype=LD)
        rB = grp_first(gr)
        for gc in range(gc0, min(gc0 + CG, gr + 1)):
            qB, nc = grp_first(gc), grp_size(gc)
            blk = [[B.at(rB + i, qB + k) if (gr != gc or i >= k) else B.at(rB + k, qB + i) for k in range(nc)] for i in range(2)]
            out = block_new(Pvv, blk, gr, gc, LD(c), LD(s), xb.astype(LD))
            rD, qD = dest_first(gr, NA), dest_first(gc, NA)
            for i in range(2):
                for k in range(nc):
                    if gr != gc or i >= k:
                        A.store_sym(rD + i, qD + k, float(out[i, k]))
            if gc == 0:
                xa.store(rD, float(xa.v[0] + c * xb[rB] - s * xb[rB + 1]))
                xa.store(rD + 1, float(xa.v[1] + s * xb[rB] + c * xb[rB + 1]))

    def vehicle(A, B, xa, xb, cs, col):
        c, s = cs
        j0, j1 = -(s * xb[0] + c * xb[1]), c * xb[0] - s * xb[1]
        p0, p1, p2 = A.at(col, 0), A.at(col, 1), A.at(col, 2)
        A.store_sym(col, 0, float(p0 + j0 * p2))
        A.store_sym(col, 1, float(p1 + j1 * p2))
        A.store_sym(col, 2, p2)

    def pose(A, B, xa, xb, cs):
        c, s = cs
        Pvv = np.array([[A.at(max(i, k), min(i, k)) for k in range(3)] for i in range(3)], dtype=LD)
        Bvv = np.array([[B.at(max(i, k), min(i, k)) for k in range(3)] for i in range(3)], dtype=LD)
        out = {}
        for gr in (0, 1):
            for gc in range(gr + 1):
                r, q = grp_first(gr), grp_first(gc)
                o = block_new(Pvv, Bvv[r:r + grp_size(gr), q:q + grp_size(gc)], gr, gc, LD(c), LD(s), xb.astype(LD))
                for i in range(grp_size(gr)):
                    for k in range(grp_size(gc)):
                        if gr != gc or i >= k:
                            out[(r + i, q + k)] = float(o[i, k])
        new = [float(xa.v[0] + c * xb[0] - s * xb[1]), float(xa.v[1] + s * xb[0] + c * xb[1]), mpi_to_pi(float(xa.v[2]) + float(xb[2]))]
        for (r, q), v in out.items():                        # every read lies above: now the writes
            A.store_sym(r, q, v)
        for i in range(3):
            xa.store(i, new[i])

    for j in range(NB):
        for col in range(3, nA):
            th.append((1, lambda *a, j=j, col=col: strip(*a, j, col)))
    for gr in range(2, NB + 2):
        for gc0 in range(0, gr + 1, CG):
            th.append((1, lambda *a, gr=gr, gc0=gc0: block(*a, gr, gc0)))
    for col in range(3, nA):
        th.append((2, lambda *a, col=col: vehicle(*a, col)))
    th.append((3, pose))
    return th


class _Vec:
    def __init__(self, v):
        self.v = v
        self.writes = np.zeros(v.shape[0], dtype=np.int64)

    def store(self, i, val):
        self.v[i] = val
        self.writes[i] += 1


def run_join(bufA, ldA, xa, NA, bufB, ldB, xb, NB, E, order=None):
    """The three launches on `bufA` / `xa` (float64, a's tile-major buffer and mean vector with capacity) IN PLACE; `bufB` is
    frozen.  Launches run one after the other, the threads of a launch in the given order (None: ascending).  Returns the
    write counts (P offsets, x indices)."""
    A, B, X = _Buf(bufA, ldA, E), _Buf(bufB, ldB, E, frozen=True), _Vec(xa)
    cs = cs_of(xa[2])
    th = _threads(NA, NB)
    for launch in (1, 2, 3):
        mine = [t for l, t in th if l == launch]
        idx = range(len(mine)) if order is None else order(len(mine))
        for i in idx:
            mine[i](A, B, X, np.asarray(xb, dtype=np.float64), cs)
    return A.writes, X.writes
