"""Landmark removal (slam_ekf_remove_landmarks, csrc/ekf_compact.hip), the parts that need no GPU: the entry point is
declared where it belongs, exported and bound; its host-side argument check; the index maps; and a NumPy model of the
in-place band-group schedule on the tile-major, block-lower storage, which pins the ordering argument of ekf_compact.hip:

    walk the destination column bands in ascending order in groups [J0, J1); launch A forms every destination tile of the
    group from the matrix AS IT STANDS into a staging buffer, launch B copies staging over the group's bands.  A destination
    column c' reads source column keep[c'] >= c' (the upper part of a diagonal tile: its mirror, source column
    keep[r'] >= r'), i.e. only bands >= J0, none of which has been written yet.  Tile rows below I0 = f0 / E (f0: the first
    removed state index) and above I1 = (n_old - 1) / E are not touched.

The model runs that schedule literally (reads go to the ONE buffer that launch B of the earlier groups has already
overwritten), for every removal pattern of a few map sizes and several group sizes, against P[np.ix_(keep, keep)] laid out
by tests/strip_ref.expected_storage."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from tests import strip_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slam_ekf_remove_landmarks"


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", text))


def test_the_entry_point_is_declared_in_the_diag_header_exported_and_bound(pkg):
    assert NAME in _declared(os.path.join(ROOT, "include", "slamhip_diag.h"))
    assert NAME not in _declared(os.path.join(ROOT, "include", "slamhip.h"))          # the boundary header stays as it is
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    assert hasattr(lib, NAME)
    res, args = pkg._lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 4
    assert callable(pkg.EKFSlamState.remove_landmarks) and callable(pkg.remove_features) and callable(pkg.remove_features_)
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    assert "remove_features!" in src.split("const libslamhip")[0] and f"(:{NAME}, libslamhip)" in src     # exported, bound


def test_null_handle_is_a_status_code(pkg):
    lib = pkg._lib.lib
    ids = (ctypes.c_int32 * 1)(1)
    assert lib.slam_ekf_remove_landmarks(None, ids, 1, None) == pkg._lib.SLAM_E_BADARG
    assert "null handle" in pkg._lib.last_error()
    assert lib.slam_ekf_remove_landmarks(None, None, 0, None) == pkg._lib.SLAM_E_BADARG


@pytest.mark.parametrize("N", [1, 2, 7, 40])
def test_index_maps_against_np_delete(pkg, N):
    rng = np.random.default_rng(N)
    n = 3 + 2 * N
    sets = [[], [1], [N], list(range(1, N + 1)), list(range(N, 0, -1))]
    sets += [rng.choice(np.arange(1, N + 1), size=k, replace=False).tolist() for k in range(1, N + 1, max(1, N // 5))]
    for ids in sets:
        keep, new_index = pkg.removal_maps(N, ids)
        rm = np.asarray(sorted(ids), dtype=np.int64)
        gone_state = np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]) if rm.size else np.zeros(0, dtype=np.int64)
        assert keep.dtype == np.int32 and np.array_equal(keep, np.delete(np.arange(n), gone_state))
        assert np.all(np.diff(keep) > 0) and np.all(keep >= np.arange(len(keep)))      # monotone: keep[i] >= i
        assert new_index.dtype == np.int32 and new_index.shape == (N,)
        left = np.delete(np.arange(1, N + 1), rm - 1)
        assert np.array_equal(new_index[left - 1], np.arange(1, len(left) + 1)) and not new_index[rm - 1].any()
    for bad in ([0], [N + 1], [1, 1]):
        with pytest.raises(ValueError):
            pkg.removal_maps(N, bad)


# ---- the schedule, in NumPy ------------------------------------------------------------------------------------------------
def tiles_before(J0, J, I0, I1):
    """compact_tiles_before of csrc/ekf_compact.hip, restated: tiles of the bands [J0, J), band j holding tile rows max(j, I0) .. I1."""
    s = 0
    a = min(J, I0) - J0
    if a > 0:
        s += a * (I1 - I0 + 1)
    lo = max(J0, I0)
    cnt = J - lo
    if cnt > 0:
        s += cnt * (I1 + 1) - (cnt * (lo + J - 1)) // 2
    return s


def compact_in_place(buf, ld, E, keep, n_old, f0, cap_tiles, skip_prefix=True):
    """The schedule of ekf_compact.hip on the tile-major buffer `buf` (modified in place).  Returns the number of groups."""
    L = E.bit_length() - 1
    T = ld // E
    n_new = len(keep)
    I0 = (f0 >> L) if skip_prefix else 0
    I1 = (n_old - 1) >> L
    cap = max(cap_tiles, I1 - I0 + 1)
    groups = 0
    J0 = 0
    while J0 <= I1:
        J1 = J0 + 1
        while J1 <= I1 and tiles_before(J0, J1 + 1, I0, I1) <= cap:
            J1 += 1
        stage = np.full(tiles_before(J0, J1, I0, I1) * E * E, np.nan, dtype=buf.dtype)
        for J in range(J0, J1):                                                    # launch A: reads buf, writes stage
            for x, I in enumerate(range(max(J, I0), I1 + 1)):
                r = I * E + np.arange(E)[None, :]                                  # tile[column][row]
                c = J * E + np.arange(E)[:, None]
                hi, lo = np.maximum(r, c), np.minimum(r, c)                        # (above the diagonal: the mirror)
                live = hi < n_new
                kh = keep[np.where(live, hi, 0)]
                kl = keep[np.where(live, lo, 0)]
                tile = np.where(live, buf[SR.p_off(ld, L, kh, kl)], 0).astype(buf.dtype)
                o = (tiles_before(J0, J, I0, I1) + x) * E * E
                stage[o:o + E * E] = tile.reshape(-1)
        for J in range(J0, J1):                                                    # launch B: stage -> the group's bands
            lo_row = max(J, I0)
            cnt = I1 - lo_row + 1
            b = int(SR.tile_base(lo_row, J, T, L))
            o = tiles_before(J0, J, I0, I1) * E * E
            buf[b:b + cnt * E * E] = stage[o:o + cnt * E * E]
        groups += 1
        J0 = J1
    return groups


def test_tile_count_formula_against_a_plain_sum():
    for I1 in range(0, 7):
        for I0 in range(0, I1 + 1):
            for J0 in range(0, I1 + 2):
                for J in range(J0, I1 + 2):
                    assert tiles_before(J0, J, I0, I1) == sum(I1 - max(j, I0) + 1 for j in range(J0, J)), (J0, J, I0, I1)


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_band_group_schedule_reproduces_the_reduced_matrix(N):
    """E = 4, T = 5: every removal pattern, staging of one band / about two bands / everything, prefix below the first
    removed index skipped -- the buffer afterwards is the packed P[np.ix_(keep, keep)], padding +0.0."""
    E, T = 4, 5
    ld = E * T
    n = 3 + 2 * N
    assert n <= ld
    rng = np.random.default_rng(100 + N)
    A = rng.normal(size=(n, n))
    P = A + A.T
    start = SR.expected_storage(P, ld, E)
    cases = 0
    for k in range(1, N + 1):
        for ids in itertools.combinations(range(1, N + 1), k):
            rm = np.asarray(ids)
            keep = np.delete(np.arange(n), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))
            want = SR.expected_storage(P[np.ix_(keep, keep)], ld, E)
            f0 = 3 + 2 * (int(rm.min()) - 1)
            for cap in (1, 2 * T, T * (T + 1) // 2):
                buf = start.copy()
                groups = compact_in_place(buf, ld, E, keep, n, f0, cap)
                assert np.array_equal(SR._bits(buf), SR._bits(want)), (N, ids, cap)
                assert groups >= 1
                cases += 1
            # what the skipped prefix claims: no stored entry with row and column below f0 differs from the start
            r, c = np.meshgrid(np.arange(f0), np.arange(f0), indexing="ij")
            off = SR.stored_offsets(ld, E.bit_length() - 1, r, c)
            assert np.array_equal(SR._bits(want[off]), SR._bits(start[off]))
    assert cases == 3 * (2 ** N - 1)


def test_the_schedule_needs_its_order():
    """The model is sharp: the same launches over the bands in DESCENDING order read bands that are already overwritten
    and do not reproduce the reduced matrix."""
    E, T, N = 4, 5, 8
    ld, n = E * T, 3 + 2 * N
    rng = np.random.default_rng(3)
    A = rng.normal(size=(n, n))
    P = A + A.T
    keep = np.delete(np.arange(n), [3, 4])
    want = SR.expected_storage(P[np.ix_(keep, keep)], ld, E)
    L = 2
    buf = SR.expected_storage(P, ld, E)
    I1 = (n - 1) >> L
    for J in range(I1, -1, -1):                      # one band per group, wrong way round
        tiles = []
        for I in range(J, I1 + 1):
            r = I * E + np.arange(E)[None, :]
            c = J * E + np.arange(E)[:, None]
            hi, lo = np.maximum(r, c), np.minimum(r, c)
            live = hi < len(keep)
            tiles.append(np.where(live, buf[SR.p_off(ld, L, keep[np.where(live, hi, 0)], keep[np.where(live, lo, 0)])], 0).reshape(-1))
        b = int(SR.tile_base(J, J, T, L))
        buf[b:b + len(tiles) * E * E] = np.concatenate(tiles)
    assert not np.array_equal(buf, want)
