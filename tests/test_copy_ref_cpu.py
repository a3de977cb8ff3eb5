"""Copy, grow and select between EKF handles (slam_ekf_copy / slam_ekf_select / slam_ekf_capacity), the parts that need no GPU:
the layout arithmetic of tests/copy_ref.py against strip_ref's in int64, a literal NumPy run of the kernels' ownership rule with
the writes per destination offset counted, the expected buffers, the host-side argument checks, the growth policy, and the
declarations the host layers bind (the sixth companion library)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import copy_ref as CR
from tests import strip_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"slam_ekf_capacity", "slam_ekf_copy", "slam_ekf_select"}
EDGES = [(128, np.float32), (64, np.float64)]


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_offsets_agree_with_strip_ref_in_int64_up_to_800_tile_rows():
    rng = np.random.default_rng(1)
    for E in (128, 64):
        L = CR.log2_edge(E)
        for T in list(range(1, 41)) + [100, 255, 256, 391, 799, 800]:
            ld = T * E
            r = np.concatenate([rng.integers(0, ld, 400), [0, ld - 1, ld - 1, E - 1, min(E, ld - 1), ld - E]])
            c = np.concatenate([rng.integers(0, ld, 400), [0, 0, ld - 1, E - 1, E - 1, 0]])
            r, c = np.maximum(r, c), np.minimum(r, c)                  # tile-wise lower
            a, b = CR.p_off(ld, L, r, c), SR.p_off(ld, L, r, c)
            assert a.dtype == np.int64 and np.array_equal(a, b), (E, T)
            assert int(a.max()) < T * (T + 1) // 2 * E * E
    # the largest offset of T = 800, E = 128 does not fit 32 bits: the arithmetic is 64-bit
    top = int(CR.p_off(800 * 128, 7, 800 * 128 - 1, 800 * 128 - 1))
    assert top == 800 * 801 // 2 * 128 * 128 - 1 and top > 2 ** 32


def test_tile_numbering_is_inverted_exactly_up_to_800_tile_rows():
    for Tw in list(range(1, 41)) + [100, 255, 256, 391, 799, 800]:
        q = np.arange(Tw * (Tw + 1) // 2, dtype=np.int64)
        I, J = CR.tile_of(q, Tw)
        assert np.all((0 <= J) & (J <= I) & (I < Tw)), Tw
        assert np.array_equal(J * Tw - J * (J - 1) // 2 + (I - J), q), Tw       # the numbering the kernels stride over
        # and that numbering is memory order: tile_base of an allocation of exactly Tw tile rows
        assert np.array_equal(CR.tile_base(I, J, Tw, 0), q), Tw


def test_plan_counts_work_items_and_caps_the_grid():
    # N = 3000 fp32: n = 6003, 47 tile rows, 1128 tiles, 4 slices each = 4512 work items on 2048 workgroups
    Tw, Tn, items, grid = CR.plan(3, 6003, 6016 + 128, 128)
    assert (Tw, Tn, items, grid) == (47, 47, 4512, 2048)
    # a shrinking destination is cleared up to what it held, never beyond its allocation
    assert CR.plan(403, 143, 512, 128)[:2] == (4, 2) and CR.plan(403, 143, 384, 128)[:2] == (3, 2)
    assert CR.plan(3, 3, 128, 128) == (1, 1, 4, 4) and CR.plan(3, 3, 64, 64) == (1, 1, 2, 2)


# ---- the ownership rule ---------------------------------------------------------------------------------------------------------
def _state(rng, N, dtype):
    n = 3 + 2 * N
    A = rng.normal(0, 0.3, (n, 5))
    P = (A @ A.T + 0.02 * np.eye(n)).astype(dtype)
    return np.maximum(P, P.T)                                              # symmetric bit for bit after the rounding


def _dirty(rng, n_old, ld, E, dtype):
    """dst before the call: a dense state of n_old rows, padding zero (the storage invariant)."""
    A = rng.normal(0, 1.0, (n_old, n_old)).astype(dtype)
    return SR.expected_storage(np.maximum(A, A.T), ld, E)


@pytest.mark.parametrize("E,dtype", EDGES)
def test_copy_rule_writes_every_offset_below_the_extent_once_and_nothing_else(E, dtype):
    rng = np.random.default_rng(5)
    # (N_src, src capacity, N_old of dst, dst capacity): equal ld, growing, shrinking, stale larger state, empty source
    for Ns, caps, Nold, capd in ((70, 70, 0, 70), (70, 70, 0, 300), (70, 300, 0, 70), (70, 70, 200, 300), (0, 8, 100, 130),
                                 (130, 130, 40, 300)):
        P = _state(rng, Ns, dtype)
        n, n_old = 3 + 2 * Ns, 3 + 2 * Nold
        lds, ldd = -(-(3 + 2 * caps) // 128) * 128, -(-(3 + 2 * capd) // 128) * 128
        src = SR.expected_storage(P, lds, E)
        dst = _dirty(rng, n_old, ldd, E, dtype)
        out, cnt = CR.walk_copy(dst, ldd, n_old, src, lds, n, E, rng=rng)
        mask = CR.written_extent(n_old, n, ldd, E)
        assert np.array_equal(cnt[mask], np.ones(int(mask.sum()), dtype=np.int32)) and not cnt[~mask].any(), (Ns, capd)
        assert np.array_equal(SR._bits(out), SR._bits(CR.expected_copy(P, ldd, E))), (Ns, capd)
        out2, _ = CR.walk_copy(dst, ldd, n_old, src, lds, n, E)           # another order of work items and threads: the same
        assert np.array_equal(SR._bits(out), SR._bits(out2))


@pytest.mark.parametrize("E,dtype", EDGES)
def test_select_rule_equals_the_selected_matrix_for_permuted_subsets(E, dtype):
    rng = np.random.default_rng(9)
    Ns = 130 if E == 128 else 100
    strad = CR.straddlers(Ns, E)
    assert strad[0] == (63 if E == 128 else 31)                            # 0-based j = 62 / 30
    P = _state(rng, Ns, dtype)
    lds = -(-(3 + 2 * Ns) // 128) * 128
    src = SR.expected_storage(P, lds, E)
    # a lower and an upper entry of a source diagonal tile that DIFFER: the rule reads the lower one
    L = CR.log2_edge(E)
    src_marked = src.copy()
    src_marked[int(CR.p_off(lds, L, 5, 9))] += dtype(1.0)                # (5, 9): the upper copy inside diagonal tile 0
    subsets = {
        "shuffled": rng.permutation(np.arange(1, Ns + 1))[:Ns // 2],
        "reversed": np.arange(Ns, 0, -1),
        "none": np.zeros(0, dtype=np.int64),
        **CR.straddle_subsets(Ns, E),
    }
    for name, ids in subsets.items():
        s = CR.index_map(Ns, ids)
        nn = s.size
        for Nold, capd in ((0, max(ids.size, 1)), (120, 300)):
            n_old = 3 + 2 * Nold
            ldd = -(-(3 + 2 * capd) // 128) * 128
            dst = _dirty(rng, n_old, ldd, E, dtype)
            out, cnt = CR.walk_select(dst, ldd, n_old, src_marked, lds, s, E, rng=rng)
            mask = CR.written_extent(n_old, nn, ldd, E)
            assert np.array_equal(cnt[mask], np.ones(int(mask.sum()), dtype=np.int32)) and not cnt[~mask].any(), name
            assert np.array_equal(SR._bits(out), SR._bits(CR.expected_select(P, s, ldd, E))), name
            assert np.array_equal(SR._bits(out), SR._bits(SR.expected_storage(P[s][:, s], ldd, E))), name


def test_index_map_is_select_map_and_validates_ids(pkg):
    assert CR.index_map(4).tolist() == list(range(11))
    assert CR.index_map(4, [3, 1]).tolist() == [0, 1, 2, 7, 8, 3, 4]
    assert np.array_equal(pkg.select_map(4, [3, 1]), CR.index_map(4, [3, 1])) and pkg.select_map(4, []).tolist() == [0, 1, 2]
    for fn in (CR.index_map, pkg.select_map):
        for bad in ([0], [5], [2, 2], [1, 3, 1], [-1]):
            with pytest.raises(ValueError):
                fn(4, bad)


# ---- host side ----------------------------------------------------------------------------------------------------------------
def test_null_handles_and_one_handle_twice_are_status_codes(pkg):
    lib = pkg._lib.copy_lib()
    ids = (ctypes.c_int32 * 2)(1, 2)
    out = ctypes.c_int(-3)
    assert lib.slam_ekf_capacity(None, ctypes.byref(out)) == pkg._lib.SLAM_E_BADARG and out.value == -3
    assert lib.slam_ekf_copy(None, None) == pkg._lib.SLAM_E_BADARG and "null handle" in pkg._lib.last_error()
    assert lib.slam_ekf_select(None, None, ids, 2) == pkg._lib.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)                          # never dereferenced: dst == src is decided on the pointers
    assert lib.slam_ekf_copy(fake, None) == pkg._lib.SLAM_E_BADARG and lib.slam_ekf_copy(None, fake) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_copy(fake, fake) == pkg._lib.SLAM_E_BADARG and "one handle" in pkg._lib.last_error()
    assert lib.slam_ekf_select(fake, fake, ids, 2) == pkg._lib.SLAM_E_BADARG


def test_growth_policy():
    from __graft_entry__ import load_package
    g = load_package().grown_capacity
    assert [g(8, 9), g(16, 17), g(32, 33)] == [16, 32, 64]            # doubling while one more landmark arrives
    assert g(8, 40) == 40 and g(0, 5) == 5 and g(64, 128) == 128 and g(64, 129) == 129
    cap, seen = 8, []
    for need in range(9, 200):                                          # a map that grows one by one re-allocates log2 times
        if need > cap:
            cap = g(cap, need)
            seen.append(cap)
    assert seen == [16, 32, 64, 128, 256]
    with pytest.raises(ValueError):
        g(-1, 3)


def test_header_python_and_julia_name_the_same_symbols(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    assert set(pkg._lib.COPY_SIGNATURES) == NAMES
    with open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")) as f:
        src = f.read()
    for word in ("select", "reserve!", "capacity"):
        assert re.search(r"^export[^#]*?\b" + re.escape(word), src, flags=re.S | re.M), word
    for obj in (pkg.EKFSlamState.copy, pkg.EKFSlamState.select, pkg.EKFSlamState.copy_from, pkg.EKFSlamState.select_from,
                pkg.EKFSlamState.reserve, pkg.copy_state, pkg.select_features):
        assert callable(obj)
    assert isinstance(pkg.EKFSlamState.capacity, property)
