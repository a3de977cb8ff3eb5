"""Map joining (slam_ekf_join), the parts that need no GPU: the entry point is declared, exported and bound where it belongs (the
second companion library); the host-side argument checks; csrc/dd_trig.h built for the host against exact arithmetic; the
blockwise formulas against the dense product and F, G against central differences; a known answer against the oracle's
add_features; and a literal NumPy run of the kernels' ownership rule (tests/join_ref.run_join)."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import join_ref as JR
from tests import strip_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slam_ekf_join"


def test_the_entry_point_is_declared_in_the_join_header_exported_and_bound(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    assert set(pkg._lib.JOIN_SIGNATURES) == {NAME}
    res, args = pkg._lib.JOIN_SIGNATURES[NAME]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    head = src.split("const libslamhip")[0]
    assert "join!" in head and "submap" in head
    for obj in (pkg.EKFSlamState.join, pkg.EKFSlamState.submap):
        assert callable(obj)


def test_null_handle_and_self_join_are_status_codes(pkg):
    lib = pkg._lib.join_lib()
    assert lib.slam_ekf_join(None, None, None) == pkg._lib.SLAM_E_BADARG
    assert "null handle" in pkg._lib.last_error()
    fake = ctypes.c_void_p(0x1000)                          # never dereferenced: a == b is decided on the pointers
    assert lib.slam_ekf_join(fake, None, None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_join(fake, fake, None) == pkg._lib.SLAM_E_BADARG
    assert "itself" in pkg._lib.last_error()


def test_sincos_and_dot_product_of_the_kernels_against_exact_arithmetic(tmp_path):
    """csrc/dd_trig.h, built for the host: sincos_rn returns the doubles nearest to sin and cos (join_ref.cs_of, decimal
    arithmetic), dot2_rn is within one rounding of the exact value where the two products cancel to 1e-9.
    This is the HOST build (g++, x86-64, no FMA contraction): it checks the algorithm, not the device compile.  What the device
    compiler makes of the same header -- contraction is switched off inside it by pragma -- is held only by the per-entry bound
    of tests/test_gpu_ekf_join.py, whose fp64 cases leave the bound when j is off by an ulp of its larger product."""
    exe = str(tmp_path / "join_trig_client")
    res = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "join_trig_client.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(1)
    ang = np.concatenate([rng.uniform(-math.pi, math.pi, 600), rng.uniform(-20, 20, 100), np.arange(-8, 9) * (math.pi / 4),
                          [0.0, 1e-9, -1e-300, 3.0, -3.0, 100.0]])
    cases = []
    for i in range(400):
        a, x, b, y = rng.uniform(-1, 1), rng.uniform(-100, 100), rng.uniform(-1, 1), rng.uniform(-100, 100)
        if i % 2:
            y = -a * x / b * (1 + rng.uniform(-1e-9, 1e-9))
        cases.append((a, x, b, y))
    inp = "".join(float(a).hex() + "\n" for a in ang) + "".join("dot " + " ".join(float(v).hex() for v in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=60).stdout.split("\n")
    for a, line in zip(ang, out):
        s, c = (float.fromhex(t) for t in line.split())
        assert (c, s) == JR.cs_of(a), (a, s, c)
    for (a, x, b, y), line in zip(cases, out[len(ang):]):
        exact = Fraction(a) * Fraction(x) + Fraction(b) * Fraction(y)
        assert abs(Fraction(float.fromhex(line)) - exact) <= abs(exact) * Fraction(1, 2 ** 52), (a, x, b, y)


def _state(rng, N, pose=None, scale=0.3):
    n = 3 + 2 * N
    p = [rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3)] if pose is None else pose
    x = np.concatenate([p, rng.uniform(-90, 90, 2 * N)])
    A = rng.normal(0, scale, (n, n))
    return x, A @ A.T + 0.01 * np.eye(n)


@pytest.mark.parametrize("NA,NB", [(0, 0), (0, 2), (3, 0), (4, 5)])
def test_blockwise_formulas_against_the_dense_product_and_central_differences(NA, NB):
    rng = np.random.default_rng(10 * NA + NB)
    xA, PA = _state(rng, NA)
    xB, PB = _state(rng, NB, pose=[1.5, -0.7, 0.2])
    xo, Po = JR.join(xA, PA, xB, PB)
    F, G, (c, s) = JR.FG(xA, xB)
    nA = 3 + 2 * NA
    got = np.full(Po.shape, np.nan, dtype=JR.LD)
    got[3:nA, 3:nA] = PA[3:nA, 3:nA]
    xb = xB.astype(JR.LD)
    for gr in range(NB + 2):
        r, nr = JR.dest_first(gr, NA), JR.grp_size(gr)
        for gc in range(NB + 2):
            q, nc = JR.dest_first(gc, NA), JR.grp_size(gc)
            rb, qb = JR.grp_first(gr), JR.grp_first(gc)
            got[r:r + nr, q:q + nc] = JR.block_new(PA[:3, :3].astype(JR.LD), PB[rb:rb + nr, qb:qb + nc], gr, gc, c, s, xb)
        for col in range(3, nA):
            got[r:r + nr, col] = JR.block_cross(PA[:3, col], gr, c, s, xb)
            got[col, r:r + nr] = got[r:r + nr, col]
    assert JR.worst_ratio(got, Po, JR.bound_P(xA, PA, xB, PB, "f64")) <= 1.0
    assert np.all(np.linalg.eigvalsh(Po.astype(np.float64)) > 0)
    # F = d x' / d x_A, G = d x' / d x_B by central differences (the wrap is off: headings chosen inside (-pi, pi))
    h = 1e-6
    for M, which in ((F, 0), (G, 1)):
        base = (xA, xB)[which]
        D = np.zeros(M.shape)
        for k in range(base.shape[0]):
            lo, hi = base.copy(), base.copy()
            lo[k] -= h
            hi[k] += h
            args = ((lo, xB), (hi, xB)) if which == 0 else ((xA, lo), (xA, hi))
            D[:, k] = ((JR.state_map(*args[1]) - JR.state_map(*args[0])) / (2 * h)).astype(np.float64)
        assert np.max(np.abs(D - M.astype(np.float64))) <= 1e-6 * max(1.0, float(np.max(np.abs(M)))), which


def test_known_answer_against_the_oracles_add_features():
    """P_B = 0, b's pose 0: b's landmark j is a noise-free feature at range-bearing (|b_j|, atan2(b_j)) from a's pose, so the new
    rows equal oracle.ekf_ref.add_features_sparse with R = 0."""
    rng = np.random.default_rng(77)
    xA, PA = _state(rng, 6)
    NB = 4
    xB = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-30, 30, 2 * NB)])
    PB = np.zeros((3 + 2 * NB, 3 + 2 * NB))
    xo, Po = JR.join(xA, PA, xB, PB)
    zn = np.stack([np.hypot(xB[3::2], xB[4::2]), np.arctan2(xB[4::2], xB[3::2])])
    xr, Pr = O.add_features_sparse(xA, PA, zn, np.zeros((2, 2)))
    assert np.allclose(xo.astype(np.float64), xr, rtol=0, atol=1e-11 * 100) and np.allclose(Po.astype(np.float64), Pr, rtol=0, atol=1e-10 * np.abs(Pr).max())


@pytest.mark.parametrize("E", [4, 8])
@pytest.mark.parametrize("NA", [0, 1, 2, 5])
@pytest.mark.parametrize("NB", [0, 1, 2, 7])
def test_ownership_rule_writes_every_owned_entry_once_and_matches_the_dense_result(E, NA, NB):
    rng = np.random.default_rng(1000 * E + 10 * NA + NB)
    L = E.bit_length() - 1
    nA, nB, n2 = 3 + 2 * NA, 3 + 2 * NB, 3 + 2 * (NA + NB)
    ldA, ldB = (((n2 - 1) >> L) + 2) * E, (((nB - 1) >> L) + 1) * E
    xA, PA = _state(rng, NA)
    xB, PB = _state(rng, NB, pose=[0.8, -1.1, 0.3])
    xo, Po = JR.join(xA, PA, xB, PB)
    want = SR.expected_storage(Po.astype(np.float64), ldA, E)
    owned = np.zeros(want.shape[0], dtype=np.int64)
    rows = np.concatenate([np.arange(3), np.arange(nA, n2)])
    owned[SR.stored_offsets(ldA, L, np.repeat(rows, n2), np.tile(np.arange(n2), len(rows)))] = 1
    perms = [None, lambda k: range(k - 1, -1, -1), lambda k: np.random.default_rng(k).permutation(k)]
    for order in perms:
        bufA, bufB = SR.expected_storage(PA, ldA, E), SR.expected_storage(PB, ldB, E)
        keepB = bufB.copy()
        xa = np.concatenate([xA, np.zeros(ldA - nA)])
        wP, wx = JR.run_join(bufA, ldA, xa, NA, bufB, ldB, xB, NB, E, order)
        assert np.array_equal(wP, owned), (np.flatnonzero(wP != owned)[:8], wP[wP != owned][:8])
        assert np.array_equal(wx, np.concatenate([np.ones(3), np.zeros(nA - 3), np.ones(2 * NB), np.zeros(ldA - n2)]))
        assert np.array_equal(bufB, keepB)
        pad = SR.expected_storage(np.ones((n2, n2)), ldA, E) == 0
        assert not bufA[pad].any() and not np.signbit(bufA[pad]).any()
        assert np.allclose(bufA, want, rtol=0, atol=1e-12 * max(np.abs(Po).max(), 1.0))
        assert np.allclose(xa[:n2], xo.astype(np.float64), rtol=0, atol=1e-12 * 100)
        T = ldA // E
        for J in range(T):
            b = int(SR.tile_base(J, J, T, L))
            tile = bufA[b:b + E * E].reshape(E, E)
            assert np.array_equal(tile, tile.T)
