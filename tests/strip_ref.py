"""Entry-wise reference of predict and add_features with a DERIVED error bound, and the storage invariants of the
tile-major covariance (csrc/ekf_strip.hip, csrc/device_math.h).  Host-only NumPy; nothing here needs a GPU.

The reference
    For ONE call, from a given state (on the GPU side: the device's own state, downloaded, so every comparison is
    re-anchored) it returns for every entry the call owns the value `ref` in extended precision and a magnitude `mag`:
    the same expression with every term replaced by its absolute value (|sin|, |cos| <= 1 are dropped from the strip,
    cross and x magnitudes).  The heading enters as the kernels and the reference formula take it: sin / cos of the
    FLOAT64-rounded g + phi (predict, src/ekf.jl:17-18) respectively phi + b (add_features, src/ekf.jl:94-95).

    `ref` is np.longdouble where that has at least 64 significant bits (x87); otherwise float64, and then the fp64 slack
    is doubled (`C_FACTOR`) -- the fallback is visible in `EXTENDED`, not silent.

What a call owns
    predict        strip P[f, 0:3], f >= 3 (and its mirror P[0:3, f]); P[0:3, 0:3]; x[0:3]
    add_features   cross blocks new x old (and mirrors); new x new blocks b < a (and mirrors); the diagonal 2 x 2 blocks;
                   the new entries of x
    Everything else must come back bit for bit.

The bound (derived, not measured)
    |got - ref| <= u_T |ref| + c 2^-53 mag,     u_T = 2^-24 (fp32: ONE rounding of the fp64 value to the state type)
                                                    or 0 (fp64: the store is exact)
    c = 16  strip, cross and x entries: six fp64 roundings on the way (sin / cos, v*dt, two products, the sum, the
            argument) plus room for FMA contraction and a device libm that differs from NumPy's by a few ulp;
    c = 32  the 3 x 3 pose block and the new x new 2 x 2 blocks: sums of up to 13 nested products.
    c is a condition, not a knob: the CPU emulation in tests/test_strip_ref_cpu.py needs c = 2.1 for the fp64 strip, and
    an emulated kernel whose strip arithmetic is `float` leaves the bound on 39-49 % of the entries even with c = 64.

Storage (device_math.h:106-173)
    Tile-major, block lower: tiles of edge E (128 fp32, 64 fp64) on and below the diagonal, each one contiguous E x E
    column-major block, column band after column band.  `p_off` / `tile_base` are restated here on NumPy integers;
    `expected_storage` lays a dense matrix out that way; `check_storage` reads a live handle's raw buffer and asserts
    the invariants every other kernel relies on without checking.
"""
import math

import numpy as np

EXTENDED = np.finfo(np.longdouble).nmant >= 63
LD = np.longdouble if EXTENDED else np.float64
C_FACTOR = 1.0 if EXTENDED else 2.0          # float64 reference: its own rounding sits inside the slack, so double it
C_STRIP = 16.0                               # strip, cross, x
C_BLOCK = 32.0                               # P[0:3, 0:3], new x new blocks
C_LIMIT = 64.0                               # never raised past this
EPS53 = 2.0 ** -53
U_T = {"f32": 2.0 ** -24, "f64": 0.0}
TILE = {"f32": 128, "f64": 64}
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
PI = math.pi                                 # SLAM_PI_D: the float64 constant, as device_math.h and the reference use it


def _ld(a):
    return np.asarray(a, dtype=LD)


def _sincos(angle64):
    """sin, cos in extended precision of the FLOAT64-rounded angle."""
    a = LD(np.float64(angle64))
    return np.sin(a), np.cos(a)


# ---- predict --------------------------------------------------------------------------------------------------------------
def predict_ref(x3, col, v, g, w, Q, dt):
    """One predict (src/ekf.jl:8-43) from pose x3 = x[0:3] and the column strip col = P[:, 0:3] (n x 3, float64 values of the
    state's dtype).  Returns a dict of (ref, mag) pairs: 'strip' (n - 3, 3), 'vv' (3, 3), 'x' (3,), and 'wrapped'."""
    x3 = np.asarray(x3, dtype=np.float64)
    col = _ld(col)
    Q = _ld(Q)
    v, g, w, dt = (LD(np.float64(t)) for t in (v, g, w, dt))
    phi = LD(x3[2])
    s, c = _sincos(np.float64(g) + x3[2])
    vdt = v * dt
    vts, vtc = vdt * s, vdt * c
    p0, p1, p2 = col[3:, 0], col[3:, 1], col[3:, 2]
    strip = np.stack([p0 - vts * p2, p1 + vtc * p2, p2], axis=1)
    a2 = np.abs(p2)
    strip_mag = np.stack([np.abs(p0) + np.abs(vdt) * a2, np.abs(p1) + np.abs(vdt) * a2, a2], axis=1)
    one, zero = LD(1), LD(0)
    Gv = np.array([[one, zero, -vts], [zero, one, vtc], [zero, zero, one]], dtype=LD)
    sg, cg = np.sin(g), np.cos(g)
    Gu = np.array([[dt * c, -vts], [dt * s, vtc], [dt * sg / w, vdt * cg / w]], dtype=LD)
    Pvv = col[0:3, 0:3]
    vv = Gv @ Pvv @ Gv.T + Gu @ Q @ Gu.T
    vv_mag = np.abs(Gv) @ np.abs(Pvv) @ np.abs(Gv).T + np.abs(Gu) @ np.abs(Q) @ np.abs(Gu).T
    turn = vdt * sg / w
    t = phi + turn
    wrapped = 0
    if t > LD(PI):                               # ONE conditional wrap (src/common.jl:102-110)
        t, wrapped = t - 2 * LD(PI), 1
    elif t < -LD(PI):
        t, wrapped = t + 2 * LD(PI), -1
    xr = np.array([LD(x3[0]) + vtc, LD(x3[1]) + vts, t], dtype=LD)
    xm = np.array([abs(LD(x3[0])) + abs(vdt), abs(LD(x3[1])) + abs(vdt), abs(phi) + abs(turn) + (2 * LD(PI) if wrapped else 0)],
                  dtype=LD)
    return {"strip": (strip, strip_mag), "vv": (vv, vv_mag), "x": (xr, xm), "wrapped": wrapped}


# ---- add_features -----------------------------------------------------------------------------------------------------------
def add_features_ref(x3, col, zn, R):
    """One add_features (src/ekf.jl:84-122) of the nn observations zn (2 x nn) from pose x3 and the column strip
    col = P[0:n0, 0:3].  Returns (ref, mag) pairs: 'cross' (2 nn, n0): the new rows against every OLD column (the pose
    columns included); 'new' (2 nn, 2 nn): the new x new corner, diagonal blocks with Gz R Gz'; 'x' (2 nn,)."""
    x3 = np.asarray(x3, dtype=np.float64)
    col = _ld(col)
    R = _ld(R)
    zn = np.asarray(zn, dtype=np.float64).reshape(2, -1)
    nn = zn.shape[1]
    n0 = col.shape[0]
    Pvv = col[0:3, 0:3]
    G = np.zeros((nn, 2, 3), dtype=LD)
    Gz = np.zeros((nn, 2, 2), dtype=LD)
    xr = np.zeros(2 * nn, dtype=LD)
    xm = np.zeros(2 * nn, dtype=LD)
    for a in range(nn):
        r = LD(zn[0, a])
        s, c = _sincos(x3[2] + zn[1, a])
        G[a] = [[1, 0, -r * s], [0, 1, r * c]]
        Gz[a] = [[c, -r * s], [s, r * c]]
        xr[2 * a], xr[2 * a + 1] = LD(x3[0]) + r * c, LD(x3[1]) + r * s
        xm[2 * a], xm[2 * a + 1] = abs(LD(x3[0])) + abs(r), abs(LD(x3[1])) + abs(r)
    rr = np.abs(_ld(zn[0]))
    # cross: P[fa + k, c] = col[c, k] + G[a][k][2] col[c, 2]      (Gv P[0:3, c], P[0:3, c] read as P[c, 0:3])
    cross = np.empty((2 * nn, n0), dtype=LD)
    cross_mag = np.empty((2 * nn, n0), dtype=LD)
    for k in range(2):
        cross[k::2] = col[None, :, k] + G[:, k, 2][:, None] * col[None, :, 2]
        cross_mag[k::2] = np.abs(col[None, :, k]) + rr[:, None] * np.abs(col[None, :, 2])
    GP = G @ Pvv                                                  # (nn, 2, 3): Gv_b Pvv
    GPm = np.abs(G) @ np.abs(Pvv)
    blk = G[:, None] @ np.transpose(GP, (0, 2, 1))[None]          # [a, b] = Gv_a (Gv_b Pvv)'
    blk_mag = np.abs(G)[:, None] @ np.transpose(GPm, (0, 2, 1))[None]
    new = np.empty((2 * nn, 2 * nn), dtype=LD)
    new_mag = np.empty((2 * nn, 2 * nn), dtype=LD)
    for a in range(nn):
        for b in range(a):
            new[2 * a:2 * a + 2, 2 * b:2 * b + 2] = blk[a, b]
            new[2 * b:2 * b + 2, 2 * a:2 * a + 2] = blk[a, b].T
            new_mag[2 * a:2 * a + 2, 2 * b:2 * b + 2] = blk_mag[a, b]
            new_mag[2 * b:2 * b + 2, 2 * a:2 * a + 2] = blk_mag[a, b].T
        new[2 * a:2 * a + 2, 2 * a:2 * a + 2] = G[a] @ Pvv @ G[a].T + Gz[a] @ R @ Gz[a].T
        new_mag[2 * a:2 * a + 2, 2 * a:2 * a + 2] = np.abs(G[a]) @ np.abs(Pvv) @ np.abs(G[a]).T + \
            np.abs(Gz[a]) @ np.abs(R) @ np.abs(Gz[a]).T
    return {"cross": (cross, cross_mag), "new": (new, new_mag), "x": (xr, xm)}


# ---- the bound --------------------------------------------------------------------------------------------------------------
def ratio(got, ref, mag, dtype):
    """(|got - ref| - u_T |ref|) / (2^-53 mag) per entry: what `c` would have to be.  An entry with mag == 0 must be exact
    (ratio 0) and is +inf otherwise."""
    got, ref, mag = _ld(got), _ld(ref), _ld(mag)
    over = np.abs(got - ref) - LD(U_T[dtype]) * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mag > 0, over / (LD(EPS53) * np.where(mag > 0, mag, 1)), np.where(got == ref, 0.0, np.inf))
    return np.asarray(np.maximum(q, 0), dtype=np.float64)


def assert_within(got, pair, dtype, c, what, log=None):
    """Every entry of `got` within u_T |ref| + c 2^-53 mag of pair = (ref, mag).  Returns the largest ratio (and records it
    in `log[what-kind]` when a dict is passed)."""
    ref, mag = pair
    got = np.asarray(got)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    if got.size == 0:
        return 0.0
    q = ratio(got, ref, mag, dtype)
    worst = float(np.max(q))
    if log is not None:
        key = (what.split(":")[0], dtype)
        log[key] = max(log.get(key, 0.0), worst)
    if not worst <= c * C_FACTOR:
        i = np.unravel_index(int(np.argmax(q)), q.shape)
        bad = int(np.sum(q > c * C_FACTOR))
        raise AssertionError(f"{what}: {bad} of {q.size} entries outside the bound, worst at {i}: got {float(got[i])!r}, "
                             f"ref {float(ref[i])!r}, needs c = {worst:.3g} (committed c = {c})")
    return worst


# ---- storage ----------------------------------------------------------------------------------------------------------------
def tile_base(I, J, T, L):
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    return (J * T - J * (J - 1) // 2 + (I - J)) << (2 * L)


def p_off(ld, L, r, c):
    """device_math.h:136-139 on NumPy integers; requires (r >> L) >= (c >> L)."""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    m = (1 << L) - 1
    return tile_base(r >> L, c >> L, ld >> L, L) + ((c & m) << L) + (r & m)


def stored_offsets(ld, L, r, c):
    """Offsets of every stored copy of the symmetric entries (r, c): the position itself, its mirror, or both (inside a
    diagonal tile) -- what p_store_sym writes."""
    r, c = np.broadcast_arrays(np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64))
    r, c = r.reshape(-1), c.reshape(-1)
    lo = (r >> L) >= (c >> L)
    up = (c >> L) >= (r >> L)
    return np.unique(np.concatenate([p_off(ld, L, r[lo], c[lo]), p_off(ld, L, c[up], r[up])]))


def expected_storage(P, ld, E):
    """The tile-major buffer (1-D, P's dtype) that holds the symmetric n x n matrix P in an allocation of ld x ld: every
    tile on and below the diagonal, diagonal tiles complete, rows / columns >= n zero."""
    P = np.asarray(P)
    n = P.shape[0]
    L = E.bit_length() - 1
    assert 1 << L == E and ld % E == 0 and n <= ld
    T = ld // E
    full = np.zeros((ld, ld), dtype=P.dtype)
    full[:n, :n] = P
    out = np.zeros(T * (T + 1) // 2 * E * E, dtype=P.dtype)
    for J in range(T):
        for I in range(J, T):
            b = int(tile_base(I, J, T, L))
            out[b:b + E * E] = full[I * E:(I + 1) * E, J * E:(J + 1) * E].T.reshape(-1)     # column-major tile
    return out


def _bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def raw_view(st):
    """A torch view over the handle's tile-major buffer (slam_ekf_device_ptrs documents the layout), after st.sync()."""
    import torch
    _dx, d_P, ld, _stream = st.device_ptrs()
    f32 = st.np_dtype == np.float32
    E = 128 if f32 else 64
    T = ld // E
    count = T * (T + 1) // 2 * E * E

    class _Raw:
        __cuda_array_interface__ = {"shape": (count,), "typestr": "<f4" if f32 else "<f8", "data": (d_P, False), "version": 2}
    st.sync()
    view = torch.as_tensor(_Raw(), device="cuda")
    assert view.dtype == (torch.float32 if f32 else torch.float64)
    return view, ld, E


def snapshot(st):
    """A device copy of the raw buffer, for `changed_offsets` after a call."""
    view, _ld_, _E = raw_view(st)
    import torch
    snap = view.clone()
    torch.cuda.synchronize()
    return snap


def changed_offsets(st, snap, chunk=1 << 28):
    """Sorted offsets of the raw buffer whose BITS differ from the snapshot."""
    import torch
    view, _ld_, _E = raw_view(st)
    it = torch.int32 if view.dtype == torch.float32 else torch.int64
    out = []
    for o in range(0, view.numel(), chunk):
        d = torch.nonzero(view[o:o + chunk].view(it) != snap[o:o + chunk].view(it)).reshape(-1)
        if d.numel():
            out.append(d.cpu().numpy().astype(np.int64) + o)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def predict_owned_offsets(n, ld, L):
    f = np.arange(3, n)
    strip = stored_offsets(ld, L, np.repeat(f, 3), np.tile(np.arange(3), len(f))) if n > 3 else np.zeros(0, dtype=np.int64)
    vv = stored_offsets(ld, L, np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3))
    return np.union1d(strip, vv)


def add_owned_offsets(n0, nn, ld, L):
    rows = np.arange(n0, n0 + 2 * nn)
    cols = np.arange(0, n0 + 2 * nn)
    return stored_offsets(ld, L, np.repeat(rows, len(cols)), np.tile(cols, len(rows)))


FULL_BYTES = 4 << 30      # above this the raw buffer is checked on the first block column and the diagonal tiles only


def check_storage(st, pkg=None, Pg=None, what="", full=None):
    """The storage invariants of a live handle, from its raw buffer:
      * every stored element with r >= n or c >= n is +0.0 (all bits clear);
      * every diagonal tile equals its own transpose bit for bit;
      * the stored triangle equals slam_ekf_get_block of the same entries read from BOTH triangles (block_gather_kernel),
        and the download `Pg` when one is passed (unpack_kernel);
      * the packed 2 x 2 side array equals the matrix's entries.
    Works column band by column band (one band of tiles on the host at a time); above FULL_BYTES only the first band and
    the diagonal tiles (with the tile below each: the straddling landmarks) are read."""
    view, ld, E = raw_view(st)
    L = E.bit_length() - 1
    T = ld // E
    n = st.n
    esz = 4 if E == 128 else 8
    if full is None:
        full = view.numel() * esz <= FULL_BYTES
    if Pg is not None:
        assert Pg.shape == (n, n)
    for J in range(T):
        cnt = (T - J) if (full or J == 0) else min(2, T - J)
        b = int(tile_base(J, J, T, L))
        band = view[b:b + cnt * E * E].cpu().numpy().reshape(cnt, E, E)          # [tile, column, row]
        rows = (J * E + np.arange(cnt * E)).reshape(cnt, 1, E)
        cols = (J * E + np.arange(E)).reshape(1, E, 1)
        pad = (rows >= n) | (cols >= n)
        nz = _bits(band)[np.broadcast_to(pad, band.shape)]
        assert not nz.any(), f"{what}: {int(np.count_nonzero(nz))} padding entries of column band {J} are not +0.0"
        assert np.array_equal(_bits(band[0]), _bits(band[0]).T), f"{what}: diagonal tile {J} is not bit-symmetric"
        c0 = J * E
        if c0 >= n:
            continue
        nc = min(E, n - c0)
        nr = min(cnt * E, n - c0)
        stored = band.transpose(0, 2, 1).reshape(cnt * E, E)[:nr, :nc]          # [row - c0, column - c0]
        low = st.get_block(c0, c0, nr, nc)
        assert np.array_equal(_bits(np.ascontiguousarray(low)), _bits(np.ascontiguousarray(stored))), \
            f"{what}: get_block below the diagonal differs from the stored tiles of band {J}"
        up = st.get_block(c0, c0, nc, nr)
        assert np.array_equal(_bits(np.ascontiguousarray(up)), _bits(np.ascontiguousarray(stored.T))), \
            f"{what}: get_block above the diagonal differs from the stored tiles of band {J}"
        if Pg is not None:
            assert np.array_equal(_bits(np.ascontiguousarray(Pg[c0:c0 + nr, c0:c0 + nc])), _bits(np.ascontiguousarray(stored))) and \
                np.array_equal(_bits(np.ascontiguousarray(Pg[c0:c0 + nc, c0:c0 + nr])), _bits(np.ascontiguousarray(stored.T))), \
                f"{what}: the download differs from the stored tiles of band {J}"
    N = st.N
    if N:
        import torch
        f = 3 + 2 * np.arange(N)
        idx = np.concatenate([p_off(ld, L, f, f), p_off(ld, L, f + 1, f), p_off(ld, L, f + 1, f + 1)])
        ent = view[torch.as_tensor(idx, device="cuda")].cpu().numpy().reshape(3, N)
        blk = st.landmark_blocks()
        assert np.array_equal(_bits(ent), _bits(blk)), f"{what}: the packed 2 x 2 side array differs from the matrix"
        if Pg is not None:
            assert np.array_equal(blk[0], Pg[f, f]) and np.array_equal(blk[1], Pg[f + 1, f]) and np.array_equal(blk[2], Pg[f + 1, f + 1]), what
