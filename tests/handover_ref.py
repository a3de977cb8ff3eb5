"""The two rules of include/slamhip_handover.h (csrc/handover.hip) run literally in fp64 NumPy, with their per-entry error bounds.
Host-only.  No BLAS product forms a compared quantity: every sum below is an elementwise product followed by ndarray.sum, or
numpy.einsum without optimisation (its own loop).

PARTICLES -> EKF (`pf_to_ekf`).  From the particle set as slam_pf_download returns it (the rounded values the kernel reads):
    w_k = exp((T)(logw_k - (T) pend)), W = sum w, what = w / W, Neff = W^2 / sum w^2
    mu = (sum what x, sum what y, atan2(sum what sin phi, sum what cos phi), sum what m ...)
    d_k = z_k - mu, the heading through the single conditional wrap
    P = sum what_k d_k d_k' + blockdiag(0_3, sum what_k P_k,l)
`variant` builds the wrong rules the CPU tests hold the bound against.

THE BOUND of P (u = 2^-24 / 2^-53 the dtype's unit roundoff, u64 = 2^-53; the header's summation structure, step by step):
  1. sw_k = (T) sqrt(what_k): sw_k = sqrt(what_k) (1 + e1), |e1| <= u (+ the fp64 error of what_k, below).
  2. Y[k][a] = ((T) d_ka) * sw_k in T: Y = d_ka sqrt(what_k) (1 + e2)(1 + e3)(1 + e1), three factors (1 + e), |e| <= u.
     A product Y[k][a] Y[k][b] therefore carries six such factors: relative error <= 6 u + O(u^2) of what_k |d_ka| |d_kb|.
  3. One slab's partial is ONE chain of at most Lc = min(n, SLAB) fused multiply-adds in T, one rounding per term: the classical
     bound of recursive summation, |error| <= Lc u sum_k |Y_ka Y_kb| (Higham, Accuracy and Stability, (3.4) with the product exact
     inside the fma; gamma_Lc = Lc u / (1 - Lc u) is within the 2 u of slack below for Lc <= 8192).
  4. The slabs' partials (each a T value: exact in fp64) are added in fp64, the within-particle term is added, the result is rounded
     to T once: u |P_ab|, plus fp64 terms.
  so  |P_ab - exact| <= (Lc + 8) u A_ab + u |P_ab| + F_ab (+ the underflow term written out in the code: it matters only where
  one particle holds nearly all the mass and sqrt(what_k) of the others leaves the dtype's range),  A_ab = sum_k what_k |d_ka| |d_kb|
  F_ab, the fp64 tail (all of it far below u A_ab in fp32): the weights (one exp, one division by W whose own sum is a fixed-order
  chain of at most 64 additions), the slab sum (at most n / SLAB + 1 additions) and the within-particle sums of pass 1 (chains of at
  most 64): 128 u64 (A_ab + B_ab), B_ab = sum_k what_k |P_k,ab|; and the means: mu carries |dmu_a| <= 128 u64 sum_k what_k |z_ka|
  (the heading: 128 u64 / Rbar, Rbar the mean resultant length), which moves P_ab by at most
  |dmu_a| sum what |d_b| + |dmu_b| sum what |d_a| + |dmu_a dmu_b|.
The bound of x: u |mu_a| + |dmu_a|.
Nothing in the bound comes from a device's output.

EKF -> PARTICLES (`ekf_table`, `ekf_to_pf`).  The table in fp64 in the kernel's own operation order; the draw in the arithmetic of
T, operation by operation.  THE BOUND of a drawn value, from the few operations of the rule (eps = u, a_norm and the Box-Muller
radius as tests/proposal_records.py has them):
    dxi     = a_norm + 16 eps rad + 4 eps |xi|      (the transcendental units of the fp32 path: 1e-6 absolute on sin / cos times the
              radius; fp64: the argument 2 pi u2 and the cosine to a few ulps, times the radius; the log and square root 1 ulp each)
    ddelta_i = sum_j |L_ij| dxi_j + 4 eps sum_j |L_ij xi_j|                 (three products, two additions, the table rounded to T)
    dpose_i  = ddelta_i + 2 eps (|x_v,i| + |delta_i|)
    dm_a     = sum_c |B_ac| ddelta_c + 4 eps (|m_a| + sum_c |B_ac delta_c|)
plus the fp64 error of the table's L_v and B_j, 64 u64 cond(P_vv) of each product they enter (the factorisation and the two
triangular solves; m_j and x_v are copied)."""
import math

import numpy as np

from oracle.pf_ref import MASK32, _u01, philox4x32

NP_DTYPE = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
U64 = 2.0 ** -53
ETA = {"f64": 2.0 ** -1074, "f32": 2.0 ** -149}
TILE = {"f32": 128, "f64": 64}
SLAB = {"f32": 8192, "f64": 4096}            # SLAM_HANDOVER_SLAB_F32 / _F64
STREAM_HANDOVER = 3
A_SC = {"f64": 0.0, "f32": 1e-6}             # csrc/pf_device.h: sin / cos of the fp32 path, absolute
RAD_MAX = math.sqrt(2 * 25 * math.log(2.0))
A_NORM = {"f64": 0.0, "f32": RAD_MAX * 1e-6}
VARIANTS = ("no_wrap", "no_within", "unnormalised", "no_pending", "unweighted_mean", "missing_mirror")


def wrap(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(a > math.pi, a - 2 * math.pi, np.where(a < -math.pi, a + 2 * math.pi, a))


def weights(logw, pend, dtype):
    """w_k as slam_pf_get_weights returns them: the shift subtracted in the dtype, the exponential in fp64."""
    T = NP_DTYPE[dtype]
    return np.exp((np.asarray(logw, dtype=T) - T(pend)).astype(np.float64))


def in_use(pxx, seen):
    """The "in use" test of slam_pf_map_sums."""
    return (pxx > 0) | (seen & (pxx == 0))


def _gram(Y, Z):
    """sum_k Y[k, a] Z[k, b] without a BLAS product: einsum with optimize=False is NumPy's own sum-of-products loop (only the
    optimised paths hand a contraction to tensordot); it gives the bits of (Y[:, a:a + 1] * Z).sum(axis=0) row by row."""
    return np.einsum("ka,kb->ab", Y, Z, optimize=False)


def pf_to_ekf(pose, logw, lm, ids, dtype, pend=0.0, seen=None, variant=None):
    """-> dict(x, P, info = (W, Neff, n, N'), xbound, Pbound, counts).  `ids` 1-based; `lm` [nl, 5, n]; everything float64 arithmetic
    on the given (dtype-rounded) values."""
    assert variant is None or variant in VARIANTS
    pose = np.asarray(pose, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n, cnt = pose.shape[1], ids.size
    D = 3 + 2 * cnt
    w = weights(logw, 0.0 if variant == "no_pending" else pend, dtype)
    W = w.sum()
    what = w / W
    seen = np.ones(lm.shape[0], dtype=bool) if seen is None else np.asarray(seen, dtype=bool)
    counts = np.array([np.count_nonzero(in_use(lm[l - 1, 2], seen[l - 1])) for l in ids], dtype=np.int64)
    z = np.empty((n, D))
    z[:, 0], z[:, 1], z[:, 2] = pose
    for k, l in enumerate(ids):
        z[:, 3 + 2 * k], z[:, 4 + 2 * k] = lm[l - 1, 0], lm[l - 1, 1]
    wm = np.full(n, 1.0 / n) if variant == "unweighted_mean" else what
    mu = (wm[:, None] * z).sum(axis=0)
    sn, cs = (wm * np.sin(pose[2])).sum(), (wm * np.cos(pose[2])).sum()
    mu[2] = math.atan2(sn, cs)
    d = z - mu
    if variant != "no_wrap":
        d[:, 2] = wrap(d[:, 2])
    wq = w if variant == "unnormalised" else what
    P = _gram(wq[:, None] * d, d)
    P = np.tril(P) + np.tril(P, -1).T          # one owner (r >= c) writes an entry and its mirror
    A = _gram(what[:, None] * np.abs(d), np.abs(d))
    B = np.zeros((D, D))
    for k, l in enumerate(ids):
        f = 3 + 2 * k
        pxx, pxy, pyy = ((wq * lm[l - 1, c]).sum() for c in (2, 3, 4))
        if variant != "no_within":
            P[f, f] += pxx; P[f + 1, f] += pxy; P[f, f + 1] += pxy; P[f + 1, f + 1] += pyy
        axx, axy, ayy = ((what * np.abs(lm[l - 1, c])).sum() for c in (2, 3, 4))
        B[f, f], B[f + 1, f], B[f, f + 1], B[f + 1, f + 1] = axx, axy, axy, ayy
    if variant == "missing_mirror" and D >= 2:
        E = TILE[dtype]
        r = min(D, E) - 1                      # the last row of the first diagonal tile and its first column: the upper mirror
        P[0, r] = 0.0
    u = U[dtype]
    Lc = min(n, SLAB[dtype])
    dmu = 128 * U64 * (what[:, None] * np.abs(z)).sum(axis=0)
    dmu[2] = 128 * U64 / max(math.hypot(sn, cs), 1e-300)
    s1 = (what[:, None] * np.abs(d)).sum(axis=0)
    F = 128 * U64 * (A + B) + dmu[:, None] * s1[None, :] + s1[:, None] * dmu[None, :] + dmu[:, None] * dmu[None, :]
    # underflow (eta: the smallest subnormal of the dtype, the absolute error of a rounding that underflows): sw_k and Y_ka each
    # carry at most eta, a product Y_ka Y_kb therefore sqrt(what_k) eta (|d_ka| (|d_kb| + 1) + |d_kb| (|d_ka| + 1)), and each of
    # the n + 1 additions and roundings of the chain and the final store eta
    eta = ETA[dtype]
    G = _gram(np.sqrt(what)[:, None] * np.abs(d), np.abs(d) + 1.0)
    Pb = (Lc + 8) * u * A + u * np.abs(P) + F + eta * (G + G.T + n + 2)
    xb = u * np.abs(mu) + dmu + eta
    return dict(x=mu, P=P, info=(W, W * W / (w * w).sum(), n, cnt), xbound=xb, Pbound=Pb, counts=counts)


# ---- EKF -> particles -------------------------------------------------------------------------------------------------------
class NotPD(Exception):
    pass


def ekf_table(x, P, ids):
    """(xv [3], Lv [3, 3] lower, m [cnt, 2], B [cnt, 2, 3], C [cnt, 3] = (xx, xy, yy)) in fp64, in the operation order of
    ho_table_kernel; NotPD for a pivot <= 0, C_xx <= 0 or det C <= 0.  P: the state's symmetric matrix (the LOWER entries are read)."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    p00, p10, p11, p20, p21, p22 = P[0, 0], P[1, 0], P[1, 1], P[2, 0], P[2, 1], P[2, 2]
    if not p00 > 0:
        raise NotPD("pivot 0")
    l00 = math.sqrt(p00); l10 = p10 / l00; l20 = p20 / l00
    t = p11 - l10 * l10
    if not t > 0:
        raise NotPD("pivot 1")
    l11 = math.sqrt(t); l21 = (p21 - l20 * l10) / l11
    q = (p22 - l20 * l20) - l21 * l21
    if not q > 0:
        raise NotPD("pivot 2")
    l22 = math.sqrt(q)
    Lv = np.array([[l00, 0, 0], [l10, l11, 0], [l20, l21, l22]])
    m = np.zeros((ids.size, 2)); B = np.zeros((ids.size, 2, 3)); Cm = np.zeros((ids.size, 3))
    for j, lid in enumerate(ids):
        f = 3 + 2 * (int(lid) - 1)
        pv = np.array([[P[f + a, c] for c in range(3)] for a in range(2)])
        for a in range(2):
            y0 = pv[a, 0] / l00
            y1 = (pv[a, 1] - l10 * y0) / l11
            y2 = ((pv[a, 2] - l20 * y0) - l21 * y1) / l22
            b2 = y2 / l22
            b1 = (y1 - l21 * b2) / l11
            b0 = ((y0 - l10 * b1) - l20 * b2) / l00
            B[j, a] = (b0, b1, b2)
        cxx = P[f, f] - ((B[j, 0, 0] * pv[0, 0] + B[j, 0, 1] * pv[0, 1]) + B[j, 0, 2] * pv[0, 2])
        cxy = P[f + 1, f] - ((B[j, 1, 0] * pv[0, 0] + B[j, 1, 1] * pv[0, 1]) + B[j, 1, 2] * pv[0, 2])
        cyy = P[f + 1, f + 1] - ((B[j, 1, 0] * pv[1, 0] + B[j, 1, 1] * pv[1, 1]) + B[j, 1, 2] * pv[1, 2])
        if not cxx > 0 or not cxx * cyy - cxy * cxy > 0:
            raise NotPD(f"landmark {int(lid)}")
        m[j] = x[f], x[f + 1]
        Cm[j] = cxx, cxy, cyy
    return x[:3].copy(), Lv, m, B, Cm


def words(gids, step, seed, stream=STREAM_HANDOVER):
    """The four Philox4x32-10 words of counter (g lo, g hi, step, stream), key = the seed."""
    gids = np.asarray(gids, dtype=np.uint64)
    return philox4x32((gids & MASK32).astype(np.uint32), (gids >> np.uint64(32)).astype(np.uint32), np.full(gids.shape, step, dtype=np.uint32),
                      np.full(gids.shape, stream, dtype=np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def normals3(gids, step, seed, dtype):
    """(xi [3, n], rad [3, n]) in the arithmetic of the dtype: Box-Muller on words 0, 1 (both outputs) and the first output of
    words 2, 3; the uniforms rounded to the dtype as u01<T> has them."""
    T = NP_DTYPE[dtype]
    r = words(gids, step, seed)
    u = [_u01(w).astype(T) for w in r]
    two_pi = T(2 * math.pi)
    rad01 = np.sqrt(T(-2) * np.log(u[0]))
    rad2 = np.sqrt(T(-2) * np.log(u[2]))
    xi = np.stack([rad01 * np.cos(two_pi * u[1]), rad01 * np.sin(two_pi * u[1]), rad2 * np.cos(two_pi * u[3])]).astype(T)
    return xi, np.stack([rad01, rad01, rad2]).astype(np.float64)


def ekf_to_pf(x, P, ids, n, step, seed, dtype, first=0, n_global=None):
    """-> dict(pose [3, n], lm [cnt, 5, n], logw, pose_bound, lm_bound [cnt, 2, n]) : the particles with global ids first .. first + n
    of an n_global-particle filter (default n) drawn from the state, in the arithmetic of the dtype (float64 arrays of dtype-rounded values), and the per-value bounds."""
    T = NP_DTYPE[dtype]
    eps = U[dtype]
    xv, Lv, m, B, Cm = ekf_table(x, P, ids)
    kappa = float(np.linalg.cond(np.asarray(P, dtype=np.float64)[:3, :3]))
    tab_err = 64 * U64 * kappa
    xi, rad = normals3(np.arange(first, first + n, dtype=np.uint64), step, seed, dtype)
    L_ = Lv.astype(T); xv_ = xv.astype(T); m_ = m.astype(T); B_ = B.astype(T); C_ = Cm.astype(T)
    d0 = L_[0, 0] * xi[0]
    d1 = L_[1, 0] * xi[0] + L_[1, 1] * xi[1]
    d2 = (L_[2, 0] * xi[0] + L_[2, 1] * xi[1]) + L_[2, 2] * xi[2]
    delta = np.stack([d0, d1, d2])
    assert delta.dtype == T
    pose = np.stack([xv_[0] + d0, xv_[1] + d1, wrap(xv_[2] + d2).astype(T)])
    xi64, de64 = xi.astype(np.float64), delta.astype(np.float64)
    dxi = A_NORM[dtype] + 16 * eps * rad + 4 * eps * np.abs(xi64)
    aL = np.abs(Lv)
    dde = np.stack([sum(aL[i, j] * dxi[j] for j in range(3)) + (4 * eps + tab_err) * sum(aL[i, j] * np.abs(xi64[j]) for j in range(3))
                    for i in range(3)])
    pose_bound = dde + 2 * eps * (np.abs(xv)[:, None] + np.abs(de64))
    cnt = m.shape[0]
    lm = np.zeros((cnt, 5, n))
    lmb = np.zeros((cnt, 2, n))
    for j in range(cnt):
        for a in range(2):
            v = m_[j, a] + ((B_[j, a, 0] * d0 + B_[j, a, 1] * d1) + B_[j, a, 2] * d2)
            assert v.dtype == T
            lm[j, a] = v
            aB = np.abs(B[j, a])
            sBd = sum(aB[c] * np.abs(de64[c]) for c in range(3))
            lmb[j, a] = sum(aB[c] * dde[c] for c in range(3)) + 4 * eps * (abs(m[j, a]) + sBd) + tab_err * sBd
        lm[j, 2:5] = C_[j].astype(np.float64)[:, None]
    logw = np.full(n, T(-math.log(n_global if n_global else n)), dtype=np.float64)
    return dict(pose=pose.astype(np.float64), lm=lm, logw=logw, pose_bound=pose_bound, lm_bound=lmb, table=(xv, Lv, m, B, Cm))
