"""Duplicate search and merge (slam_ekf_find_duplicates, slam_ekf_merge_landmarks, csrc/ekf_merge.hip), the parts that need
no GPU.  tests/merge_ref.py is the fp64 oracle the GPU tests hold the kernels against; here the oracle itself is pinned --
a known answer in hand-chosen numbers, the generic Kalman update, the invariants of an exact merge, the index map, the
cheap bound of the search -- together with the declarations and the host-side batch splitter of
EKFSlamState.merge_landmarks."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import merge_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slam_ekf_find_duplicates", "slam_ekf_merge_landmarks")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", text))


def random_correlated(rng, N):
    n = 3 + 2 * N
    x = np.concatenate([[10.0, -4.0, 0.3], rng.uniform(-50, 50, 2 * N)])
    A = rng.normal(0, 0.3, (n, n))
    return x, A @ A.T + 0.05 * np.eye(n)


def test_entry_points_are_declared_in_the_diag_header_exported_and_bound(pkg):
    diag, boundary = _declared(os.path.join(ROOT, "include", "slamhip_diag.h")), _declared(os.path.join(ROOT, "include", "slamhip.h"))
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NAMES:
        assert name in diag and name not in boundary
        assert hasattr(lib, name)
        assert pkg._lib.SIGNATURES[name][0] is ctypes.c_int and len(pkg._lib.SIGNATURES[name][1]) == 5
    assert len(diag) == 22
    hdr = open(os.path.join(ROOT, "include", "slamhip_diag.h")).read()
    assert re.search(r"#define\s+SLAM_MERGE_MAX\s+8\b", hdr) and pkg._lib.SLAM_MERGE_MAX == 8
    assert callable(pkg.EKFSlamState.find_duplicates) and callable(pkg.EKFSlamState.merge_landmarks)
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    head = src.split("const libslamhip")[0]
    assert "find_duplicates" in head and "merge_landmarks!" in head
    assert all(f"(:{name}, libslamhip)" in src for name in NAMES)


def test_null_handle_and_bad_arguments_are_status_codes(pkg):
    lib = pkg._lib.lib
    cnt = ctypes.c_int(-5)
    pr = (ctypes.c_int32 * 2)(1, 2)
    assert lib.slam_ekf_find_duplicates(None, 9.0, None, 0, ctypes.byref(cnt)) == pkg._lib.SLAM_E_BADARG
    assert "null handle" in pkg._lib.last_error()
    assert lib.slam_ekf_merge_landmarks(None, pr, 1, None, None) == pkg._lib.SLAM_E_BADARG
    assert "null handle" in pkg._lib.last_error() and cnt.value == -5


def test_known_answer_two_uncorrelated_landmarks():
    """Landmarks with covariances A and B, uncorrelated with each other and with everything else, Rc = 0: the merged
    landmark is the product of the two Gaussians, the rest of the state is untouched.  Hand-chosen numbers."""
    A = np.array([[4.0, 1.0], [1.0, 2.0]])
    B = np.array([[1.0, -0.5], [-0.5, 3.0]])
    a, b = np.array([10.0, 20.0]), np.array([11.0, 18.5])
    x = np.concatenate([[1.0, 2.0, 0.25], a, [-7.0, 5.0], b])
    P = np.zeros((9, 9))
    P[:3, :3] = [[0.5, 0.1, 0.02], [0.1, 0.4, -0.01], [0.02, -0.01, 0.03]]
    P[3:5, 3:5] = A
    P[5:7, 5:7] = [[2.0, 0.3], [0.3, 1.0]]
    P[5:7, :3] = [[0.2, 0.0, 0.01], [0.0, 0.1, 0.0]]
    P[:3, 5:7] = P[5:7, :3].T
    P[7:9, 7:9] = B
    xm, Pm, ni = MR.merge(x, P, [[1, 3]])
    # (A^-1 + B^-1)^-1 by hand: A^-1 = [2 -1; -1 4] / 7, B^-1 = [3 .5; .5 1] / 2.75
    Ai = np.array([[2.0, -1.0], [-1.0, 4.0]]) / 7.0
    Bi = np.array([[3.0, 0.5], [0.5, 1.0]]) / 2.75
    info = Ai + Bi
    cov = np.array([[info[1, 1], -info[0, 1]], [-info[1, 0], info[0, 0]]]) / (info[0, 0] * info[1, 1] - info[0, 1] * info[1, 0])
    mean = cov @ (Ai @ a + Bi @ b)
    assert np.allclose(Pm[3:5, 3:5], cov, rtol=0, atol=1e-12) and np.allclose(xm[3:5], mean, rtol=0, atol=1e-12)
    keep = np.arange(7)
    rest = np.ones((7, 7), dtype=bool)
    rest[3:5, :] = rest[:, 3:5] = False
    assert np.allclose(Pm[rest], P[np.ix_(keep, keep)][rest], rtol=0, atol=1e-12)
    assert np.allclose(Pm[3:5, [0, 1, 2, 5, 6]], 0.0, atol=1e-12)                      # still uncorrelated with the rest
    assert np.allclose(np.delete(xm, [3, 4]), np.delete(x[:7], [3, 4]), rtol=0, atol=1e-12)
    assert ni.tolist() == [1, 2, 1]


def _generic(x, P, pairs, Rc):
    n = len(x)
    H = MR.dense_H(n, pairs)
    R = np.kron(np.eye(len(pairs)), Rc)
    S = H @ P @ H.T + R
    W = P @ H.T @ np.linalg.inv(S)
    xg, Pg = x + W @ (0.0 - H @ x), P - W @ S @ W.T
    rm = np.asarray(pairs)[:, 1]
    keep = np.delete(np.arange(n), np.concatenate([3 + 2 * (rm - 1), 4 + 2 * (rm - 1)]))
    return xg[keep], Pg[np.ix_(keep, keep)]


@pytest.mark.parametrize("cnt", [1, 3, 8])
@pytest.mark.parametrize("noisy", [False, True])
def test_merge_equals_the_generic_update(cnt, noisy):
    rng = np.random.default_rng(100 + cnt)
    N = 24
    x, P = random_correlated(rng, N)
    ids = rng.permutation(np.arange(1, N + 1))[:2 * cnt].reshape(cnt, 2)               # either order: the second leaves
    Rc = np.array([[0.3, 0.05], [0.05, 0.2]]) if noisy else np.zeros((2, 2))
    xm, Pm, _ni = MR.merge(x, P, ids, Rc)
    xg, Pg = _generic(x, P, ids, Rc)
    assert np.max(np.abs(xm - xg)) <= 1e-10 * np.max(np.abs(xg))
    assert np.max(np.abs(Pm - Pg)) <= 1e-10 * np.max(np.abs(Pg))
    assert np.allclose(Pm, Pm.T, rtol=0, atol=1e-12 * np.max(np.abs(Pm)))


@pytest.mark.parametrize("cnt", [1, 3, 8])
def test_after_an_exact_merge_the_two_landmarks_are_one_random_variable(cnt):
    rng = np.random.default_rng(200 + cnt)
    N = 20
    x, P = random_correlated(rng, N)
    ids = rng.permutation(np.arange(1, N + 1))[:2 * cnt].reshape(cnt, 2)
    xf, Pf = MR.fuse(x, P, ids, None)
    for a, b in ids:
        fa, fb = MR.f(a), MR.f(b)
        scale = np.max(np.abs(Pf[fa:fa + 2, fa:fa + 2]))
        assert np.max(np.abs(xf[fa:fa + 2] - xf[fb:fb + 2])) <= 1e-10 * np.max(np.abs(xf[fa:fa + 2]))
        for blk in (Pf[fb:fb + 2, fb:fb + 2], Pf[fa:fa + 2, fb:fb + 2]):
            assert np.max(np.abs(blk - Pf[fa:fa + 2, fa:fa + 2])) <= 1e-10 * scale
        # ... and every other entry sees them alike
        assert np.max(np.abs(Pf[fa:fa + 2, :] - Pf[fb:fb + 2, :])) <= 1e-10 * np.max(np.abs(Pf))


def test_new_index_semantics():
    assert MR.new_index_of(6, [[2, 5]]).tolist() == [1, 2, 3, 4, 2, 5]
    assert MR.new_index_of(6, [[5, 2]]).tolist() == [1, 4, 2, 3, 4, 5]                 # the one named second leaves
    assert MR.new_index_of(6, [[6, 1], [2, 3]]).tolist() == [4, 1, 1, 2, 3, 4]
    assert MR.new_index_of(4, []).tolist() == [1, 2, 3, 4]
    rng = np.random.default_rng(3)
    x, P = random_correlated(rng, 6)
    xm, Pm, ni = MR.merge(x, P, [[6, 1], [2, 3]])
    assert len(xm) == 3 + 2 * 4 and Pm.shape == (11, 11) and ni.tolist() == [4, 1, 1, 2, 3, 4]


def test_find_is_the_exhaustive_definition():
    rng = np.random.default_rng(11)
    N = 30
    x, P = random_correlated(rng, N)
    x[3 + 2 * 20:5 + 2 * 20] = x[3 + 2 * 4:5 + 2 * 4] + [0.05, -0.02]               # landmark 21 on top of landmark 5
    x[3 + 2 * 29:5 + 2 * 29] = x[3:5] + [0.01, 0.01]                                  # landmark 30 on top of landmark 1
    pairs, count = MR.find(x, P, 9.0)
    want = []
    for a in range(1, N + 1):
        for b in range(a + 1, N + 1):
            delta, D = MR.difference(x, P, a, b)
            if MR.d2_of(delta, D) < 9.0:
                want.append([a, b])
    assert count == len(want) and pairs.tolist() == want and [1, 30] in want and [5, 21] in want
    # a D that is not positive definite is never a duplicate, however close the means
    P2 = P.copy()
    fa, fb = MR.f(5), MR.f(21)
    P2[fb:fb + 2, :] = P2[fa:fa + 2, :]
    P2[:, fb:fb + 2] = P2[:, fa:fa + 2]
    P2[fb:fb + 2, fb:fb + 2] = P2[fa:fa + 2, fa:fa + 2]
    assert MR.d2_of(*MR.difference(x, P2, 5, 21)) == np.inf
    assert [5, 21] not in MR.find(x, P2, 9.0)[0].tolist()


def test_the_cheap_bound_never_rejects_a_duplicate():
    """10^4 random positive definite joint covariances of two landmarks, from nearly independent to nearly singular and
    strongly (anti-)correlated: whenever the exact d2 is inside the gate, |delta|^2 < 2 gate (tr P_aa + tr P_bb)."""
    rng = np.random.default_rng(2024)
    gate, inside, rejected = 9.0, 0, 0
    for i in range(10000):
        G = rng.normal(size=(4, 4)) * rng.uniform(0.05, 3.0, size=(4, 1))
        if i % 3 == 0:                                     # strong correlation between the two landmarks
            G[2:] = (-1.0 if i % 2 else 1.0) * G[:2] + 0.05 * rng.normal(size=(2, 4))
        J = G @ G.T + 1e-9 * np.eye(4)
        Paa, Pbb, Pab = J[:2, :2], J[2:, 2:], J[:2, 2:]
        D = Paa + Pbb - Pab - Pab.T
        delta = rng.normal(size=2) * rng.uniform(0.01, 4.0) * np.sqrt(np.trace(D))
        d2 = MR.d2_of(delta, (D + D.T) * 0.5)
        keeps = MR.prefilter_keeps(delta, Paa, Pbb, gate)
        if d2 < gate:
            inside += 1
            assert keeps, (i, d2)
        elif not keeps:
            rejected += 1
    assert inside > 1000 and rejected > 1000               # both branches were exercised


class FakeLibrary:
    """Stands where libslamhip stands under EKFSlamState.merge_landmarks: holds the landmarks as sets of original ids,
    refuses what slam_ekf_merge_landmarks refuses, returns its new_index."""

    def __init__(self, N, batch_max):
        self.members = [{j} for j in range(1, N + 1)]
        self.batch_max = batch_max
        self.calls = []

    def merge(self, batch):
        batch = np.asarray(batch)
        assert batch.dtype == np.int32 and batch.ndim == 2 and batch.shape[1] == 2
        N = len(self.members)
        assert 1 <= len(batch) <= self.batch_max
        flat = batch.reshape(-1).tolist()
        assert len(set(flat)) == len(flat) and min(flat) >= 1 and max(flat) <= N      # disjoint, in range
        self.calls.append(batch.tolist())
        for a, b in batch:
            self.members[a - 1] |= self.members[b - 1]
        ni = MR.new_index_of(N, batch)
        gone = set(batch[:, 1].tolist())
        self.members = [m for j, m in enumerate(self.members, start=1) if j not in gone]
        return ni


def test_batch_splitter_twenty_pairs_with_a_chain(pkg):
    N = 60
    pairs = [[2 * i + 1, 2 * i + 2] for i in range(17)]                  # 17 disjoint pairs (1,2) .. (33,34)
    pairs += [[40, 45], [45, 50], [50, 41]]                              # a chain 40 - 45 - 50 - 41
    assert len(pairs) == 20
    fake = FakeLibrary(N, pkg._lib.SLAM_MERGE_MAX)
    ni = pkg.merge_in_batches(N, pairs, fake.merge)
    assert len(fake.calls) >= 3 and all(len(c) <= 8 for c in fake.calls)
    groups = [{2 * i + 1, 2 * i + 2} for i in range(17)] + [{40, 41, 45, 50}]
    merged = set().union(*groups)
    expect_members = sorted([g for g in groups] + [{j} for j in range(1, N + 1) if j not in merged], key=min)
    assert fake.members == expect_members                                # survivors keep their order
    assert ni.dtype == np.int32 and ni.shape == (N,)
    for j in range(1, N + 1):                                            # every id lands on the landmark that holds it
        assert j in fake.members[ni[j - 1] - 1]
    # the survivor of a group is its lowest id: its final index is that of a never-merged landmark count below it
    for g in groups:
        low = min(g)
        assert ni[low - 1] == 1 + sum(1 for m in expect_members if min(m) < low)
    assert len(fake.members) == N - 17 - 3


def test_batch_splitter_order_of_a_lone_pair_and_bad_ids(pkg):
    fake = FakeLibrary(6, 8)
    ni = pkg.merge_in_batches(6, [[5, 2]], fake.merge)                  # a pair on its own goes down as given
    assert fake.calls == [[[5, 2]]] and ni.tolist() == [1, 4, 2, 3, 4, 5]
    fake = FakeLibrary(6, 8)
    ni = pkg.merge_in_batches(6, [[1, 4], [4, 1], [1, 4]], fake.merge)  # the same two landmarks again: dropped
    assert fake.calls == [[[1, 4]]] and ni.tolist() == [1, 2, 3, 1, 4, 5]
    assert pkg.merge_in_batches(3, np.zeros((0, 2)), fake.merge).tolist() == [1, 2, 3]
    for bad in ([[0, 1]], [[1, 7]], [[2, 2]]):
        with pytest.raises(ValueError):
            pkg.merge_in_batches(6, bad, fake.merge)
