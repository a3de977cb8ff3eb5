"""The rule of slam_ekf_copy / slam_ekf_select (include/slamhip_copy.h, csrc/ekf_copy.hip) run literally in NumPy.  Host-only.

    x'[i] = x[s(i)],  P'[i, j] = P[s(i), s(j)]       s = the identity (copy) or the index map of the chosen landmarks (select)

`index_map` is s; `expected_copy` / `expected_select` are the raw tile-major buffer dst must hold afterwards, built on
strip_ref.expected_storage; `walk_copy` / `walk_select` execute the kernels' OWNERSHIP rule -- work item (tile, slice), thread,
piece or entry -- on raw buffers, in any order of work items and threads, and count the writes per destination offset.  The
offsets are restated here from the header's formula (`tile_base`, `p_off`, `tile_of`) on int64 and held against strip_ref's in
tests/test_copy_ref_cpu.py."""
import numpy as np

from tests import strip_ref as SR

THREADS = 256
SLICE_COLS = 32          # columns of a slice: 32 E elements = 16 KiB in both dtypes
GRID_MAX = 2048


def log2_edge(E):
    L = int(E).bit_length() - 1
    assert 1 << L == E
    return L


def tile_base(I, J, T, L):
    """Block number J T - J (J - 1) / 2 + (I - J) of tile (I, J), I >= J, times E^2; int64."""
    I, J, T = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.int64(T)
    return (J * T - J * (J - 1) // 2 + (I - J)) << np.int64(2 * L)


def p_off(ld, L, r, c):
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    m = np.int64((1 << L) - 1)
    return tile_base(r >> L, c >> L, ld >> L, L) + ((c & m) << np.int64(L)) + (r & m)


def tile_of(q, Tw):
    """(I, J) of tile number q among the Tw (Tw + 1) / 2 tiles of the leading Tw tile rows, band after band: the band J with
    base(J) <= q < base(J + 1), base(J) = J Tw - J (J - 1) / 2.  The kernel's arithmetic: a float64 square root, then a fix-up."""
    q = np.asarray(q, dtype=np.int64)
    Tw = np.int64(Tw)
    base = lambda j: j * Tw - j * (j - 1) // 2
    b = 2.0 * float(Tw) + 1.0
    j = ((b - np.sqrt(b * b - 8.0 * q.astype(np.float64))) * 0.5).astype(np.int64)
    j = np.clip(j, 0, Tw - 1)
    while True:
        down = (j > 0) & (base(j) > q)
        if not down.any():
            break
        j = j - down
    while True:
        up = (j < Tw - 1) & (base(j + 1) <= q)
        if not up.any():
            break
        j = j + up
    return j + (q - base(j)), j


def index_map(N_src, ids=None):
    """s: the source state index of every destination index.  ids None: a copy (the identity over 3 + 2 N_src); else the 1-based
    landmark ids, distinct, in any order (ValueError otherwise, where the library answers SLAM_E_BADARG)."""
    if ids is None:
        return np.arange(3 + 2 * N_src, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 1 or ids.max() > N_src):
        raise ValueError("landmark id out of range")
    if np.unique(ids).size != ids.size:
        raise ValueError("duplicate landmark id")
    i = np.arange(3 + 2 * ids.size, dtype=np.int64)
    s = i.copy()
    k = i[3:] - 3
    s[3:] = 3 + 2 * (ids[k >> 1] - 1) + (k & 1)
    return s


def straddlers(N, E):
    """The 1-based landmarks whose two rows lie in two tile rows: 3 + 2 (j - 1) is the last row of a tile (0-based j = 62 + 64 k
    for E = 128, 30 + 32 k for E = 64)."""
    return [j for j in range(1, N + 1) if (3 + 2 * (j - 1) + 1) % E == 0]


def straddle_subsets(N_src, E):
    """Two selections aimed at the tile edges: `in`: src's first straddling landmark lands on slot 2 (inside a tile) while an
    ordinary landmark of src lands on dst's straddling slot; `out`: src's straddler is left out and an ordinary landmark lands
    on dst's straddling slot, the selection ending one landmark later."""
    st = straddlers(N_src, E)[0]
    ins = np.array([7, st] + [j for j in range(8, 8 + st + 1) if j != st][:st], dtype=np.int64)
    outs = np.array(list(range(1, st)) + [st + 5, 2 * st], dtype=np.int64)
    for ids in (ins, outs):
        assert ids.size > st and np.unique(ids).size == ids.size and ids.max() <= N_src
        assert ids[st - 1] not in straddlers(N_src, E)             # dst's straddling slot takes a pair that lay inside a tile
    assert ins[1] == st and st not in outs
    return {"straddler_in": ins, "straddler_out": outs}


def plan(n_old, n_new, ld_dst, E):
    """(Tw, Tn, items, grid): tile rows written, tile rows that hold values, work items, workgroups."""
    Td = ld_dst // E
    Tw = min(Td, (max(n_old, n_new) + E - 1) // E)
    Tn = (n_new + E - 1) // E
    items = Tw * (Tw + 1) // 2 * (E // SLICE_COLS)
    return Tw, Tn, items, min(items, GRID_MAX)


def expected_copy(P_src, ld_dst, E):
    """The raw buffer of dst after a copy of the dense symmetric matrix P_src (dst's padding zero beyond what is written)."""
    return SR.expected_storage(P_src, ld_dst, E)


def expected_select(P_src, s, ld_dst, E):
    P_src = np.asarray(P_src)
    s = np.asarray(s, dtype=np.int64)
    return SR.expected_storage(P_src[s][:, s], ld_dst, E)


def _orders(items, rng):
    if rng is None:
        return np.arange(items), np.arange(THREADS)
    return rng.permutation(items), rng.permutation(THREADS)


def walk_copy(dst, ld_dst, n_old, src, ld_src, n_new, E, rng=None):
    """move_tiles_kernel on raw buffers.  Returns (dst after, writes per destination offset)."""
    L = log2_edge(E)
    esz = dst.dtype.itemsize
    Tw, Tn, items, _grid = plan(n_old, n_new, ld_dst, E)
    S = E // SLICE_COLS
    pieces = SLICE_COLS * esz * E // 16
    per = pieces // THREADS
    epp = 16 // esz                                    # elements of a 16-byte piece
    out = dst.copy()
    cnt = np.zeros(dst.size, dtype=np.int32)
    w_order, t_order = _orders(items, rng)
    lane = np.arange(epp, dtype=np.int64)
    for w in w_order:
        q, u = divmod(int(w), S)
        I, J = (int(v) for v in tile_of(q, Tw))
        piece = u * pieces + (np.arange(per, dtype=np.int64)[None, :] * THREADS + t_order.astype(np.int64)[:, None])
        within = (piece[..., None] * epp + lane).reshape(-1)
        d = int(tile_base(I, J, ld_dst // E, L)) + within
        if I < Tn:
            out[d] = src[int(tile_base(I, J, ld_src // E, L)) + within]
        else:
            out[d] = 0
        np.add.at(cnt, d, 1)
    return out, cnt


def _read_src(src, ld_src, L, a, b):
    """Source entry (a, b) from where it is stored; inside one source tile row the LOWER entry."""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    same = (a >> L) == (b >> L)
    rr = np.where(same, hi, np.where((a >> L) > (b >> L), a, b))
    cc = np.where(same, lo, np.where((a >> L) > (b >> L), b, a))
    return src[p_off(ld_src, L, rr, cc)]


def walk_select(dst, ld_dst, n_old, src, ld_src, s, E, rng=None):
    """gather_tiles_kernel on raw buffers; s = index_map(N_src, ids).  Returns (dst after, writes per destination offset)."""
    L = log2_edge(E)
    s = np.asarray(s, dtype=np.int64)
    nn = s.size
    Tw, _Tn, items, _grid = plan(n_old, nn, ld_dst, E)
    S = E // SLICE_COLS
    cstep = THREADS >> L
    out = dst.copy()
    cnt = np.zeros(dst.size, dtype=np.int32)
    w_order, t_order = _orders(items, rng)
    t = t_order.astype(np.int64)
    rl, c_sub = t & (E - 1), t >> L
    ks = np.arange(SLICE_COLS // cstep, dtype=np.int64)
    for w in w_order:
        q, u = divmod(int(w), S)
        I, J = (int(v) for v in tile_of(q, Tw))
        r = np.broadcast_to((I * E + rl)[:, None], (THREADS, ks.size)).reshape(-1)
        c = ((J * E + u * SLICE_COLS + c_sub)[:, None] + ks[None, :] * cstep).reshape(-1)
        if I == J:
            own = r >= c                               # the thread with r' < c' writes nothing
            r, c = r[own], c[own]
        live = (r < nn) & (c < nn)
        v = np.zeros(r.size, dtype=dst.dtype)
        if live.any():
            v[live] = _read_src(src, ld_src, L, s[r[live]], s[c[live]])
        d = p_off(ld_dst, L, r, c)
        out[d] = v
        np.add.at(cnt, d, 1)
        if I == J:                                     # p_store_sym: the mirror from the same value, by the same thread
            off = r != c
            dm = p_off(ld_dst, L, c[off], r[off])
            out[dm] = v[off]
            np.add.at(cnt, dm, 1)
    return out, cnt


def written_extent(n_old, n_new, ld_dst, E):
    """Boolean mask over dst's raw buffer: the offsets of the tiles (I, J), J <= I < Tw."""
    L = log2_edge(E)
    Td = ld_dst // E
    Tw = plan(n_old, n_new, ld_dst, E)[0]
    mask = np.zeros(Td * (Td + 1) // 2 * E * E, dtype=bool)
    for J in range(Tw):
        b = int(tile_base(J, J, Td, L))
        mask[b:b + (Tw - J) * E * E] = True            # a band's tiles I = J .. Tw - 1 are contiguous
    return mask
