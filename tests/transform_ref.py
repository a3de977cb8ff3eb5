"""Dense fp64 restatement of the rigid frame change (slam_ekf_transform, slam_pf_transform) with DERIVED per-entry bounds,
and a literal NumPy run of the EKF kernels' ownership rule on a small tile-major buffer (csrc/ekf_transform.hip).

    positions  p <- R p + t,   heading  phi <- mpi_to_pi(phi + theta),   P <- T P T',   T = blockdiag(R, 1, R, R, ...)

theta is reduced as the library reduces it (C remainder(theta, 2 pi) = math.remainder).  The library evaluates every result
in double from the stored values (two nested multiply-adds per entry of P, i.e. four double multiply-adds) and rounds once
to the dtype; its c and s come from libm, NumPy's may differ by an ulp each.  With A = |T| |P| |T|' (elementwise absolute
values) that is within  (u + 16 * 2^-53) * A  per entry, u = 2^-24 (fp32) / 2^-53 (fp64): derived, not measured.
"""
import math

import numpy as np

from tests import strip_ref as SR

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
SLACK = 16.0 * 2.0 ** -53
TINY = {"f32": float(np.finfo(np.float32).tiny), "f64": float(np.finfo(np.float64).tiny)}
NP = {"f32": np.float32, "f64": np.float64}


def reduce_angle(theta):
    return math.remainder(theta, 2.0 * math.pi)


def cs_of(theta):
    t = reduce_angle(theta)
    return math.cos(t), math.sin(t)


def mpi_to_pi(phi):
    if phi > math.pi:
        return phi - 2.0 * math.pi
    if phi < -math.pi:
        return phi + 2.0 * math.pi
    return phi


def T_of(n, theta):
    c, s = cs_of(theta)
    T = np.zeros((n, n))
    T[2, 2] = 1.0
    for f in [0] + list(range(3, n, 2)):
        T[f:f + 2, f:f + 2] = [[c, -s], [s, c]]
    return T


def transform(x, P, tx, ty, theta):
    """(x', P') in float64; P' symmetrised."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    n = x.shape[0]
    T = T_of(n, theta)
    xo = T @ x
    for f in [0] + list(range(3, n, 2)):
        xo[f] += tx
        xo[f + 1] += ty
    xo[2] = mpi_to_pi(x[2] + reduce_angle(theta))
    Po = T @ P @ T.T
    return xo, (Po + Po.T) / 2


def bound_P(P, theta, dtype):
    T = np.abs(T_of(P.shape[0], theta))
    return (U[dtype] + SLACK) * (T @ np.abs(np.asarray(P, dtype=np.float64)) @ T.T)


def bound_x(x, tx, ty, theta, dtype):
    """Positions: |c| |px| + |s| |py| + |tx| (and the y row alike); the heading: one addition and the single wrap."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    c, s = (abs(v) for v in cs_of(theta))
    b = np.zeros_like(x)
    for f in [0] + list(range(3, x.shape[0], 2)):
        b[f] = c * x[f] + s * x[f + 1] + abs(tx)
        b[f + 1] = s * x[f] + c * x[f + 1] + abs(ty)
    b[2] = x[2] + abs(reduce_angle(theta)) + 2.0 * math.pi
    return (U[dtype] + SLACK) * b


def inverse(tx, ty, theta):
    """g^-1: theta' = -theta, t' = -R(-theta) t."""
    c, s = math.cos(-theta), math.sin(-theta)
    return -(c * tx - s * ty), -(s * tx + c * ty), -theta


def roundtrip_bounds(x, P, tx, ty, theta, dtype):
    """g, then g^-1: the first call's error e1 <= eps A (A = |T| |P| |T|', and |R| |p| + |t| for a position) is carried back through
    |T^-1|, and the second call's own error is eps |T^-1| |P1| |T^-1|' with |P1| <= A (1 + eps): TWICE the bound of one call,
    taken on A through |T^-1| (the factor 1 + 2^-20 covers the (1 + eps)).  Returns (bound for x, bound for P)."""
    eps = 2.0 * (1.0 + 2.0 ** -20) * (U[dtype] + SLACK)
    x = np.abs(np.asarray(x, dtype=np.float64))
    Ta = np.abs(T_of(x.shape[0], theta))
    A = Ta @ np.abs(np.asarray(P, dtype=np.float64)) @ Ta.T
    t = np.zeros_like(x)
    for f in [0] + list(range(3, x.shape[0], 2)):
        t[f], t[f + 1] = abs(tx), abs(ty)
    bx = Ta @ (Ta @ x + t)                            # (|T(-theta)| = |T(theta)|)
    bx[2] = x[2] + abs(reduce_angle(theta)) + 2.0 * math.pi + 0.5 * math.pi
    return eps * bx, eps * (Ta @ A @ Ta.T)


def compose_bounds(x, P, g, h, dtype):
    """g = (tx, ty, theta), then h, each call rounding once: against the float64 restatement of both (no rounding in between).
    The first call's error e1 <= eps A_g (A_g = |T_g| |P| |T_g|'; |T_g| |x| + |t_g| for positions) is carried through |T_h|, and the
    second call's own error is eps |T_h| |P1| |T_h|' with |P1| <= A_g (1 + eps): twice the bound of one call taken on A_g through
    |T_h| (positions: the second call's own |t_h| once).  The heading: two additions and two wraps.  roundtrip_bounds is the
    case h = g^-1.  Returns (bound for x, bound for P)."""
    eps = (1.0 + 2.0 ** -20) * (U[dtype] + SLACK)
    x = np.abs(np.asarray(x, dtype=np.float64))
    Tg, Th = np.abs(T_of(x.shape[0], g[2])), np.abs(T_of(x.shape[0], h[2]))
    A = Tg @ np.abs(np.asarray(P, dtype=np.float64)) @ Tg.T
    tg, th = np.zeros_like(x), np.zeros_like(x)
    for f in [0] + list(range(3, x.shape[0], 2)):
        tg[f], tg[f + 1], th[f], th[f + 1] = abs(g[0]), abs(g[1]), abs(h[0]), abs(h[1])
    bx = 2.0 * (Th @ (Tg @ x + tg)) + th
    bx[2] = 2.0 * (x[2] + abs(reduce_angle(g[2])) + 2.0 * math.pi) + abs(reduce_angle(h[2])) + 2.0 * math.pi
    return eps * bx, 2.0 * eps * (Th @ A @ Th.T)


def worst_ratio(got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---- blockwise form: what one owner computes ---------------------------------------------------------------------------------
def grp_first(g):
    return 2 * g if g < 2 else 2 * g - 1


def grp_size(g):
    return 1 if g == 1 else 2


def block_image(B, nr, nc, c, s):
    """R_r B R_c' for an nr x nc block (R_g = 1 for the heading's single row / column), as transform_block evaluates it."""
    B = np.asarray(B, dtype=np.float64).reshape(nr, nc)
    R = np.array([[c, -s], [s, c]])
    M = R @ B if nr == 2 else B
    return M @ R.T if nc == 2 else M


# ---- the kernels' ownership rule, literally, on a tile-major buffer -------------------------------------------------------
class _Buf:
    def __init__(self, buf, ld, E):
        self.b, self.ld, self.E = buf, ld, E
        self.L = E.bit_length() - 1
        self.writes = np.zeros(buf.shape[0], dtype=np.int64)

    def off(self, r, c):
        assert (r >> self.L) >= (c >> self.L)
        return int(SR.p_off(self.ld, self.L, r, c))

    def load(self, o):
        return float(self.b[o])

    def store(self, o, v):
        self.b[o] = v
        self.writes[o] += 1

    def store_sym(self, r, c, v):                       # p_store_sym
        L = self.L
        if (r >> L) >= (c >> L):
            self.store(self.off(r, c), v)
        if (c >> L) >= (r >> L) and r != c:
            self.store(self.off(c, r), v)


def _block_thread(B, gr, gc, c, s):
    """transform_block: every read, then every write."""
    r, q, nr, nc = grp_first(gr), grp_first(gc), grp_size(gr), grp_size(gc)
    if gr == gc:
        if nr == 1:
            return
        b00, b10, b11 = B.load(B.off(r, r)), B.load(B.off(r + 1, r)), B.load(B.off(r + 1, r + 1))
        out = block_image([[b00, b10], [b10, b11]], 2, 2, c, s)
        B.store_sym(r, r, out[0, 0])
        B.store_sym(r + 1, r, out[1, 0])
        B.store_sym(r + 1, r + 1, out[1, 1])
        return
    blk = [[B.load(B.off(r + i, q + j)) for j in range(nc)] for i in range(nr)]
    out = block_image(blk, nr, nc, c, s)
    for i in range(nr):
        for j in range(nc):
            B.store_sym(r + i, q + j, out[i, j])


def tri_off(J, Tu):
    return J * (Tu - 1) - J * (J - 1) // 2


def tri_tile(t, Tu):
    """ekf_transform.hip's tri_tile: stored tile number t below the diagonal (band after band) -> (I, J)."""
    w = 2.0 * Tu - 1.0
    j = int((w - math.sqrt(w * w - 8.0 * t)) * 0.5)
    j = min(max(j, 0), Tu - 2)
    while j > 0 and tri_off(j, Tu) > t:
        j -= 1
    while tri_off(j + 1, Tu) <= t:
        j += 1
    return j + 1 + (t - tri_off(j, Tu)), j


def _threads(n, E):
    """Every thread of the launch (its three owner sets: diagonal tiles, column pairs, tiles) as a closure over the buffer."""
    L = E.bit_length() - 1
    half = E // 2
    NG = (n - 3) // 2 + 2
    Tu = ((n - 1) >> L) + 1
    th = []
    for D in range(Tu):                                  # transform_diag (the split among workgroups changes no ownership)
        lo = 0 if D == 0 else D * half + 1
        hi = min((D + 1) * half, NG - 1)
        K = hi - lo + 1
        for i in range(max(K, 0) ** 2):
            a, b = divmod(i, K)
            if b >= a:
                th.append(lambda B, c, s, gr=lo + b, gc=lo + a: _block_thread(B, gr, gc, c, s))
    if Tu > 1:
        for y in range(Tu + 1):                          # transform_cols
            gc = y if y < 2 else (y - 1) * half
            D = 0 if y < 2 else y - 2
            for t in range(NG):
                gr = (D + 1) * half + 1 + t
                if gc >= NG or gr >= NG:
                    continue
                th.append(lambda B, c, s, gr=gr, gc=gc: _block_thread(B, gr, gc, c, s))
        LPC = E // 2
        for t in range(Tu * (Tu - 1) // 2):              # transform_tile: one closure per WAVE ITERATION (its lanes run in
            I, J = tri_tile(t, Tu)                       # lock step: all loads, the exchange, all stores)
            assert J < I < Tu and (I << L) < n
            cl0 = 3 if J == 0 else 1
            for k in range((E - 1 - cl0) // 2):
                th.append(lambda B, c, s, I=I, J=J, cl=cl0 + 2 * k: _tile_wave(B, n, I, J, cl, LPC, c, s))
    return th


def _tile_wave(B, n, I, J, cl, LPC, c, s):
    E, L = B.E, B.L
    col = int(SR.tile_base(I, J, B.ld >> L, L)) + (cl << L)
    a = [(B.load(col + 2 * q), B.load(col + 2 * q + 1)) for q in range(LPC)]
    b = [(B.load(col + E + 2 * q), B.load(col + E + 2 * q + 1)) for q in range(LPC)]
    own = [(I << L) + 2 * q + 2 < n for q in range(LPC)]
    up = [q > 0 and (I << L) + 2 * q < n for q in range(LPC)]
    o = []
    for q in range(LPC):
        if q == LPC - 1:
            na, nb = (B.load(col + E * E), B.load(col + E * E + E)) if own[q] else (0.0, 0.0)
        else:
            na, nb = a[q + 1][0], b[q + 1][0]
        o.append(block_image([[a[q][1], b[q][1]], [na, nb]], 2, 2, c, s))
    for q in range(LPC):
        if up[q]:
            B.store(col + 2 * q, o[q - 1][1, 0])
            B.store(col + E + 2 * q, o[q - 1][1, 1])
        if own[q]:
            B.store(col + 2 * q + 1, o[q][0, 0])
            B.store(col + E + 2 * q + 1, o[q][0, 1])
            if q == LPC - 1:
                B.store(col + E * E, o[q][1, 0])
                B.store(col + E * E + E, o[q][1, 1])


def run_in_place(buf, ld, E, n, theta, order=None):
    """transform_P_kernel on `buf` (float64, tile-major) IN PLACE, thread after thread in the given order (None: ascending;
    any permutation must give the same buffer: the workgroups of the launch run in no order).  Returns the per-offset write counts."""
    c, s = cs_of(theta)
    B = _Buf(buf, ld, E)
    th = _threads(n, E)
    idx = range(len(th)) if order is None else order(len(th))
    for i in idx:
        th[i](B, c, s)
    return B.writes


# ---- FastSLAM records ---------------------------------------------------------------------------------------------------------
def in_use(pxx, seen):
    """pf_map.hip's rule: Pxx > 0, or Pxx == 0 with the landmark's `seen` state set.  pxx [nl, n], seen [nl]."""
    return (pxx > 0) | ((pxx == 0) & np.asarray(seen, dtype=bool)[:, None])


def records(lm, seen, tx, ty, theta, dtype):
    """lm [nl, 5, n] in the filter's dtype -> (transformed records in that dtype, per-value bound, in-use mask).  Unused records are
    returned as they are; a record that had Pxx > 0 keeps a positive Pxx (the smallest normal number otherwise)."""
    c, s = cs_of(theta)
    v = np.asarray(lm, dtype=np.float64)
    mx, my, pxx, pxy, pyy = (v[:, k, :] for k in range(5))
    use = in_use(np.asarray(lm)[:, 2, :], seen)
    cc, ss, cs = c * c, s * s, c * s
    new = np.stack([c * mx - s * my + tx, s * mx + c * my + ty, cc * pxx - 2 * cs * pxy + ss * pyy,
                    cs * (pxx - pyy) + (cc - ss) * pxy, ss * pxx + 2 * cs * pxy + cc * pyy], axis=1)
    mag = np.stack([abs(c) * abs(mx) + abs(s) * abs(my) + abs(tx), abs(s) * abs(mx) + abs(c) * abs(my) + abs(ty),
                    cc * abs(pxx) + 2 * abs(cs) * abs(pxy) + ss * abs(pyy),
                    abs(cs) * (abs(pxx) + abs(pyy)) + (cc + ss) * abs(pxy), ss * abs(pxx) + 2 * abs(cs) * abs(pxy) + cc * abs(pyy)], axis=1)
    out = new.astype(NP[dtype])
    fix = (pxx > 0) & ~(out[:, 2, :] > 0)
    out[:, 2, :][fix] = NP[dtype](TINY[dtype])
    bound = (U[dtype] + SLACK) * mag
    bound[:, 2, :][fix] = np.maximum(bound[:, 2, :][fix], TINY[dtype])       # (the mark replaces a value that rounded to <= 0)
    keep = np.broadcast_to(~use[:, None, :], out.shape)
    out = np.where(keep, np.asarray(lm), out)
    return out, np.where(keep, 0.0, bound), use


def poses(pose, tx, ty, theta, dtype):
    """pose [3, n] -> (float64 image, bound)."""
    c, s = cs_of(theta)
    p = np.asarray(pose, dtype=np.float64)
    t = reduce_angle(theta)
    h = p[2] + t
    h = np.where(h > math.pi, h - 2 * math.pi, np.where(h < -math.pi, h + 2 * math.pi, h))
    out = np.stack([c * p[0] - s * p[1] + tx, s * p[0] + c * p[1] + ty, h])
    mag = np.stack([abs(c) * abs(p[0]) + abs(s) * abs(p[1]) + abs(tx), abs(s) * abs(p[0]) + abs(c) * abs(p[1]) + abs(ty),
                    abs(p[2]) + abs(t) + 2 * math.pi])
    # the heading is rounded to the dtype BEFORE wrap_pi<T>, whose 2 pi is the dtype's: three roundings
    return out, (3 * U[dtype] + SLACK) * mag
