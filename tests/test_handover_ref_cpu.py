"""tests/handover_ref.py, the literal form of include/slamhip_handover.h, against closed-form answers; the error bound against
wrong variants of the rule (each must exceed it by at least ten times on a designed case); the sampling rule's table against
numpy.linalg; the host layers (header, ctypes, Julia) naming the same symbols.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import handover_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"slam_pf_to_ekf", "slam_ekf_to_pf"}


def _particles(rng, n, nl, dtype="f64", spread=0.3, phi0=0.4):
    """A particle set with correlated poses and landmarks, rounded to the dtype."""
    T = HR.NP_DTYPE[dtype]
    base = rng.uniform(-20, 20, (nl, 2))
    e = rng.normal(0, spread, (3, n))
    pose = np.stack([5 + e[0], -3 + e[1], phi0 + 0.2 * e[2]])
    lm = np.zeros((nl, 5, n))
    for l in range(nl):
        lm[l, 0] = base[l, 0] + 0.7 * e[0] - 0.2 * e[2] + rng.normal(0, 0.05, n)
        lm[l, 1] = base[l, 1] + 0.5 * e[1] + 0.3 * e[2] + rng.normal(0, 0.05, n)
        a, b, c = rng.uniform(0.05, 0.2, n), rng.uniform(-0.02, 0.02, n), rng.uniform(0.05, 0.2, n)
        lm[l, 2], lm[l, 3], lm[l, 4] = a, b, c
    logw = rng.normal(-math.log(n), 1.0, n)
    return pose.astype(T).astype(np.float64), logw.astype(T).astype(np.float64), lm.astype(T).astype(np.float64)


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def test_two_particles_at_mu_plus_minus_a():
    a = np.array([0.5, -0.25, 0.125, 1.0, -2.0, 0.75, 0.5])
    mu = np.array([3.0, -1.0, 0.5, 10.0, 20.0, -5.0, 8.0])
    zs = np.stack([mu + a, mu - a], axis=1)                          # [D, 2]
    pose = zs[:3]
    lm = np.zeros((2, 5, 2))
    lm[0, :2], lm[1, :2] = zs[3:5], zs[5:7]
    lm[0, 2:] = [[0.5, 0.25], [0.125, -0.125], [1.0, 2.0]]
    lm[1, 2:] = [[2.0, 4.0], [0.0, 0.5], [0.25, 0.75]]
    r = HR.pf_to_ekf(pose, np.log([0.5, 0.5]), lm, [1, 2], "f64")
    want = np.outer(a, a)
    want[3:5, 3:5] += [[0.375, 0.0], [0.0, 1.5]]
    want[5:7, 5:7] += [[3.0, 0.25], [0.25, 0.5]]
    assert np.allclose(r["x"], mu, rtol=0, atol=1e-15) and np.allclose(r["P"], want, rtol=0, atol=1e-15)
    assert r["info"][0] == pytest.approx(1.0) and r["info"][1] == pytest.approx(2.0) and r["info"][2:] == (2, 2)
    assert r["counts"].tolist() == [2, 2]
    # the landmarks in the other order: a permutation of rows and columns
    r2 = HR.pf_to_ekf(pose, np.log([0.5, 0.5]), lm, [2, 1], "f64")
    s = [0, 1, 2, 5, 6, 3, 4]
    assert np.array_equal(r2["P"], r["P"][s][:, s]) and np.array_equal(r2["x"], r["x"][s])


def test_one_particle_with_all_the_mass():
    rng = np.random.default_rng(1)
    pose, _logw, lm = _particles(rng, 3, 2)
    logw = np.array([-np.inf, 0.0, -np.inf])
    r = HR.pf_to_ekf(pose, logw, lm, [1, 2], "f64")
    want = np.zeros((7, 7))
    for k in range(2):
        f = 3 + 2 * k
        want[f:f + 2, f:f + 2] = [[lm[k, 2, 1], lm[k, 3, 1]], [lm[k, 3, 1], lm[k, 4, 1]]]
    assert np.array_equal(r["P"], want) and np.array_equal(r["x"], np.concatenate([pose[:, 1], lm[0, :2, 1], lm[1, :2, 1]]))
    assert r["info"][1] == 1.0


def test_headings_across_pi_have_the_small_variance():
    eps = 1e-3
    pose = np.array([[0.0, 0.0], [0.0, 0.0], [math.pi - eps, -math.pi + eps]])
    r = HR.pf_to_ekf(pose, np.log([0.5, 0.5]), np.zeros((1, 5, 2)), [], "f64")
    assert abs(abs(r["x"][2]) - math.pi) < 1e-15
    assert r["P"][2, 2] == pytest.approx(eps * eps, rel=1e-9) and r["P"][2, 2] < 1e-5
    bad = HR.pf_to_ekf(pose, np.log([0.5, 0.5]), np.zeros((1, 5, 2)), [], "f64", variant="no_wrap")
    assert bad["P"][2, 2] > 9.0                                       # about pi^2 / ... : what the wrap is there for


def test_diagonal_blocks_and_means_are_finalise_map(pkg):
    from slam_jl_amd.pf import finalise_map
    rng = np.random.default_rng(2)
    n, nl = 257, 5
    pose, logw, lm = _particles(rng, n, nl)
    ids = [4, 1, 5]
    w = HR.weights(logw, 0.0, "f64")
    sums = np.zeros((1 + len(ids), 10))
    sums[0, 0] = w.sum()
    for i, l in enumerate(ids):
        mx, my = lm[l - 1, 0], lm[l - 1, 1]
        sums[1 + i] = [w.sum(), (w * mx).sum(), (w * my).sum(), (w * mx * mx).sum(), (w * mx * my).sum(), (w * my * my).sum(),
                       (w * lm[l - 1, 2]).sum(), (w * lm[l - 1, 3]).sum(), (w * lm[l - 1, 4]).sum(), n]
    fm = finalise_map(sums)
    r = HR.pf_to_ekf(pose, logw, lm, ids, "f64")
    for i in range(len(ids)):
        f = 3 + 2 * i
        got = [r["x"][f], r["x"][f + 1], r["P"][f, f], r["P"][f + 1, f], r["P"][f + 1, f + 1]]
        # (finalise_map forms E[m m'] - mean mean': cancellation of |mean|^2 u64 ~ 1e-13)
        assert np.allclose(got, fm[i, 1:6], rtol=0, atol=1e-11), (i, got, fm[i])
        assert r["P"][f, f + 1] == r["P"][f + 1, f]
    assert np.array_equal(r["P"], r["P"].T)


def test_pending_shift_and_counts():
    rng = np.random.default_rng(3)
    pose, logw, lm = _particles(rng, 64, 3)
    a = HR.pf_to_ekf(pose, logw, lm, [1, 2, 3], "f64")
    b = HR.pf_to_ekf(pose, logw + 5.0, lm, [1, 2, 3], "f64", pend=5.0)
    assert np.allclose(a["P"], b["P"], rtol=1e-12, atol=0) and a["info"][0] == pytest.approx(b["info"][0], rel=1e-12)
    lm[1, 2, 7] = -1.0                                               # an empty slot of the unknown-correspondence mode
    lm[2, 2:, 9] = 0.0                                               # Pxx == 0: in use only for a landmark that was seen
    c = HR.pf_to_ekf(pose, logw, lm, [1, 2, 3], "f64")
    assert c["counts"].tolist() == [64, 63, 64]
    assert HR.pf_to_ekf(pose, logw, lm, [3], "f64", seen=np.zeros(3, dtype=bool))["counts"].tolist() == [63]


# ---- the bound discriminates ------------------------------------------------------------------------------------------------------
def _designed(dtype):
    """Designed cases: name -> (pose, logw, lm, ids, pend)."""
    rng = np.random.default_rng(40)
    T = HR.NP_DTYPE[dtype]
    out = {}
    pose, logw, lm = _particles(rng, 515, 4, dtype)
    out["plain"] = (pose, logw, lm, [3, 1, 4, 2], 0.0)
    out["uniform_unnormalised"] = (pose, np.zeros(515), lm, [1, 2], 0.0)                  # W = n
    p2 = pose.copy()
    p2[2] = HR.wrap(math.pi + 0.05 * rng.normal(0, 1, 515)).astype(T).astype(np.float64)   # headings on both sides of +-pi
    out["across_pi"] = (p2, logw, lm, [1, 2], 0.0)
    lw = (-750.0 + rng.normal(0, 1.0, 515)).astype(T).astype(np.float64)
    out["pending_at_-750"] = (pose, lw, lm, [1, 2], -750.0)
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_wrong_variant_exceeds_the_bound_tenfold(dtype):
    cases = _designed(dtype)
    where = {"no_wrap": "across_pi", "no_within": "plain", "unnormalised": "uniform_unnormalised", "no_pending": "pending_at_-750",
             "unweighted_mean": "plain", "missing_mirror": "plain"}
    assert set(where) == set(HR.VARIANTS)
    for variant, name in where.items():
        pose, logw, lm, ids, pend = cases[name]
        good = HR.pf_to_ekf(pose, logw, lm, ids, dtype, pend=pend)
        assert np.all(np.isfinite(good["P"])) and np.all(good["Pbound"] > 0)
        with np.errstate(all="ignore"):
            bad = HR.pf_to_ekf(pose, logw, lm, ids, dtype, pend=pend, variant=variant)
        ratio = np.abs(bad["P"] - good["P"]) / good["Pbound"]
        worst = np.nanmax(np.where(np.isfinite(ratio), ratio, np.inf))
        assert worst >= 10.0, (variant, name, worst)
    # and the bound is not vacuous: far below the entries it guards
    for name, (pose, logw, lm, ids, pend) in cases.items():
        good = HR.pf_to_ekf(pose, logw, lm, ids, dtype, pend=pend)
        scale = np.sqrt(np.outer(np.diag(good["P"]), np.diag(good["P"])))
        assert np.max(good["Pbound"] / scale) < (1e-3 if dtype == "f32" else 1e-12), name


def test_fp32_rounding_of_the_rule_stays_inside_the_bound():
    """The rule carried out in float32 the way the kernel does it (inputs rounded as in steps 1 and 2, a sequential float32 chain per
    entry with the products rounded -- one rounding MORE per term than the fused chain) stays inside twice the bound; the chain is
    the longest the shapes of the GPU tests reach in one slab."""
    rng = np.random.default_rng(41)
    n = 2100
    pose, logw, lm = _particles(rng, n, 2, "f32")
    r = HR.pf_to_ekf(pose, logw, lm, [1, 2], "f32")
    w = HR.weights(logw, 0.0, "f32")
    sw = np.sqrt(w / w.sum()).astype(np.float32)
    z = np.concatenate([pose, lm[0, :2], lm[1, :2]]).T
    d = z - r["x"]
    d[:, 2] = HR.wrap(d[:, 2])
    Y = d.astype(np.float32) * sw[:, None]
    acc = np.zeros((7, 7), dtype=np.float32)
    for k in range(n):
        acc = acc + np.outer(Y[k], Y[k])                             # float32 products, float32 additions, in k order
    P = acc.astype(np.float64)
    for k in range(2):
        f = 3 + 2 * k
        within = [(w / w.sum() * lm[k, c]).sum() for c in (2, 3, 4)]
        P[f, f] += within[0]; P[f + 1, f] += within[1]; P[f, f + 1] += within[1]; P[f + 1, f + 1] += within[2]
    P = P.astype(np.float32).astype(np.float64)
    assert np.max(np.abs(P - r["P"]) / r["Pbound"]) <= 2.0


# ---- the sampling rule ----------------------------------------------------------------------------------------------------------------
def _state(rng, N):
    n = 3 + 2 * N
    x = np.concatenate([[50.0, 50.0, 0.3], rng.uniform(5, 95, 2 * N)])
    A = rng.normal(0, 0.2, (n, 6))
    P = A @ A.T + 0.01 * np.eye(n)
    return x, (P + P.T) / 2


def test_table_against_numpy_linalg():
    rng = np.random.default_rng(5)
    x, P = _state(rng, 9)
    ids = [7, 2, 9, 1]
    xv, Lv, m, B, Cm = HR.ekf_table(x, P, ids)
    Pvv = P[:3, :3]
    assert np.allclose(Lv @ Lv.T, Pvv, rtol=0, atol=1e-15) and np.array_equal(Lv, np.tril(Lv)) and np.array_equal(xv, x[:3])
    for j, l in enumerate(ids):
        f = 3 + 2 * (l - 1)
        Pjv = P[f:f + 2, :3]
        assert np.allclose(B[j] @ Pvv, Pjv, rtol=0, atol=1e-14)
        schur = P[f:f + 2, f:f + 2] - Pjv @ np.linalg.solve(Pvv, Pjv.T)
        assert np.allclose([Cm[j, 0], Cm[j, 1], Cm[j, 2]], [schur[0, 0], schur[1, 0], schur[1, 1]], rtol=0, atol=1e-12)
        assert np.array_equal(m[j], x[f:f + 2])


def test_table_refuses_what_is_not_positive_definite():
    rng = np.random.default_rng(6)
    x, P = _state(rng, 3)
    P0 = P.copy()
    P0[:3, :] = 0.0; P0[:, :3] = 0.0                                 # a vehicle known exactly
    with pytest.raises(HR.NotPD):
        HR.ekf_table(x, P0, [1])
    P1 = P.copy()
    P1[5, 5] = P1[5, 5] - 1.0                                        # landmark 2: an indefinite conditional block
    with pytest.raises(HR.NotPD):
        HR.ekf_table(x, P1, [1, 2, 3])
    HR.ekf_table(x, P1, [1, 3])                                      # ... which a call that leaves it out never sees


def test_philox_words_are_the_known_answers():
    # Random123's kat_vectors for philox4x32-10 (the ones tests/test_oracle_pf.py pins), through the hand-over's counter layout
    w = HR.words(np.array([0x85a308d3243f6a88], dtype=np.uint64), 0x13198a2e, 0x299f31d0a4093822, stream=0x03707344)
    assert [int(v[0]) for v in w] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    w = HR.words(np.array([0], dtype=np.uint64), 0, 0, stream=0)
    assert [int(v[0]) for v in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # the first two normals are the filter's normals2 on the hand-over stream
    from oracle.pf_ref import normals2
    xi, _rad = HR.normals3(np.arange(100, dtype=np.uint64), 7, 99, "f64")
    e1, e2 = normals2(np.arange(100), 7, HR.STREAM_HANDOVER, 99)
    assert np.array_equal(xi[0], e1) and np.array_equal(xi[1], e2)


def test_draw_has_the_moments_of_the_state_in_closed_form():
    """delta = L_v xi exactly, so with xi replaced by unit vectors the draw is the mean plus a column of [L_v; B_j L_v]."""
    rng = np.random.default_rng(7)
    x, P = _state(rng, 4)
    r = HR.ekf_to_pf(x, P, [1, 2, 3, 4], 1000, 0, 5, "f64")
    xv, Lv, m, B, Cm = r["table"]
    # the joint covariance the rule implies: [Pvv, Pvv B'; B Pvv, B Pvv B' + C] = P on the rows it touches
    for j in range(4):
        f = 3 + 2 * j
        assert np.allclose(B[j] @ P[:3, :3] @ B[j].T + [[Cm[j, 0], Cm[j, 1]], [Cm[j, 1], Cm[j, 2]]], P[f:f + 2, f:f + 2], rtol=0, atol=1e-12)
    assert np.all(r["pose_bound"] > 0) and np.all(r["lm_bound"] > 0) and np.max(r["lm_bound"]) < 1e-12
    assert np.all(r["logw"] == -math.log(1000)) and np.all(np.abs(r["pose"][2]) <= math.pi)
    # the same global ids give the same particles whatever the filter's size
    big = HR.ekf_to_pf(x, P, [1, 2, 3, 4], 1500, 0, 5, "f64")
    assert np.array_equal(big["pose"][:, :1000], r["pose"]) and np.array_equal(big["lm"][..., :1000], r["lm"])


# ---- host side ----------------------------------------------------------------------------------------------------------------
def test_null_handles_are_status_codes(pkg):
    lib = pkg._lib.handover_lib()
    assert lib.slam_pf_to_ekf(None, None, None, 0, None) == pkg._lib.SLAM_E_BADARG and "null handle" in pkg._lib.last_error()
    assert lib.slam_ekf_to_pf(None, None, None, 0) == pkg._lib.SLAM_E_BADARG and "null handle" in pkg._lib.last_error()
    fake = ctypes.c_void_p(0x1000)                                   # never dereferenced: the other handle is null
    assert lib.slam_pf_to_ekf(fake, None, None, 0, None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_to_pf(None, fake, None, 0) == pkg._lib.SLAM_E_BADARG


def test_header_python_and_julia_name_the_same_symbols(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    with open(os.path.join(ROOT, "include", "slamhip_handover.h")) as f:
        raw = f.read()
    assert set(pkg._lib.HANDOVER_SIGNATURES) == NAMES
    assert int(re.search(r"#define SLAM_HANDOVER_SLAB_F32 (\d+)", raw).group(1)) == HR.SLAB["f32"]
    assert int(re.search(r"#define SLAM_HANDOVER_SLAB_F64 (\d+)", raw).group(1)) == HR.SLAB["f64"]
    with open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")) as f:
        src = f.read()
    for word in ("to_ekf", "to_particles"):
        assert re.search(r"^export[^#]*?\b" + re.escape(word), src, flags=re.S | re.M), word
    for obj in (pkg.FastSLAM.to_ekf, pkg.PFSlamState.to_ekf, pkg.EKFSlamState.to_particles, pkg.particles_to_ekf, pkg.ekf_to_particles,
                pkg.PFShard.to_ekf_into, pkg.PFShard.from_ekf):
        assert callable(obj)
    from slam_jl_amd import pf
    assert pf.STREAM_HANDOVER == HR.STREAM_HANDOVER == 3
    with open(os.path.join(ROOT, "slam.jl_amd", "csrc", "pf_device.h")) as f:
        assert re.search(r"STREAM_HANDOVER = 3\b", f.read())
