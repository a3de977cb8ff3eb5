"""Joint-compatibility data association, the parts that need no GPU: the rule's two restatements (tests/jc_ref.py) against each
other on every scene, against exhaustive enumeration, on hand-made cases; the scenes' conditions; chi2_table; and the entry points
declared, exported and bound where they belong (the fourth companion library).

Largest relative difference in d2 between the literal form (S_H rebuilt, numpy.linalg.solve) and the incremental Cholesky twin over
every test of every scene: 6.6e-14 (recorded in DESIGN 5.8)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import assoc_scenes as AS
from tests import jc_ref as JR
from tests import jc_scenes as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"slam_ekf_jc_create", "slam_ekf_jc_destroy", "slam_ekf_associate_joint", "slam_ekf_joint_nis"}
R, GATE1, GATE2 = JS.R, JS.GATE1, JS.GATE2
FIELDS = ("pairings", "tests", "exhausted", "truncated", "candidates", "deepest")


def test_the_entry_points_are_declared_in_the_jc_header_exported_and_bound(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    L = pkg._lib
    assert set(L.JC_SIGNATURES) == NAMES
    res, args = L.JC_SIGNATURES["slam_ekf_associate_joint"]
    assert res is ctypes.c_int and args[7] is ctypes.c_int64 and len(args) == 10
    header = open(os.path.join(ROOT, "include", "slamhip_jc.h")).read()
    for name, val in (("SLAM_JC_MAXOBS", L.SLAM_JC_MAXOBS), ("SLAM_JC_MAXCAND", L.SLAM_JC_MAXCAND), ("SLAM_JC_NODE_CAP", L.SLAM_JC_NODE_CAP)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == val
    assert (L.SLAM_JC_MAXOBS, L.SLAM_JC_MAXCAND) == (JR.MAXOBS, JR.MAXCAND)
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    head = src.split("const libslamhip")[0]
    for name in ("associate_joint", "observe_joint!", "joint_nis", "chi2_table"):
        assert name in head
    for obj in (pkg.EKFSlamState.associate_joint, pkg.EKFSlamState.observe_joint, pkg.EKFSlamState.joint_nis, pkg.ekf.associate_joint,
                pkg.ekf.observe_joint, pkg.ekf.chi2_table):
        assert callable(obj)


def test_null_arguments_are_status_codes_without_a_device(pkg):
    lib = pkg._lib.jc_lib()
    out = ctypes.c_void_p()
    assert lib.slam_ekf_jc_create(ctypes.byref(out), None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_jc_create(None, None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_jc_destroy(None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_associate_joint(None, None, 0, None, 4.0, 25.0, None, 1, None, None) == pkg._lib.SLAM_E_BADARG
    assert lib.slam_ekf_joint_nis(None, None, None, 1, None, None) == pkg._lib.SLAM_E_BADARG


def test_chi2_table(pkg):
    want = (5.991464547, 9.487729037, 12.591587244)
    for table in (pkg.ekf.chi2_table(3, 0.95), JR.chi2_table(3, 0.95)):
        assert np.allclose(table, want, rtol=0, atol=5e-9)
    a, b = pkg.ekf.chi2_table(64, 0.95), JR.chi2_table(64, 0.95)
    assert np.allclose(a, b, rtol=1e-12, atol=0) and np.all(np.diff(a) > 0)
    # the closed form itself: the distribution function at the quantile is the confidence
    for k, q in enumerate(pkg.ekf.chi2_table(12, 0.99), start=1):
        cdf = 1.0 - math.exp(-q / 2) * sum((q / 2) ** i / math.factorial(i) for i in range(k))
        assert abs(cdf - 0.99) < 1e-12
    with pytest.raises(ValueError):
        pkg.ekf.chi2_table(3, 1.0)


@pytest.mark.parametrize("dtype", JS.DTYPES)
@pytest.mark.parametrize("kind,arg", JS.SCENES)
def test_scene_conditions_and_the_two_forms_agree(dtype, kind, arg):
    sc = JS.build(kind, arg, dtype)                        # (build() has verified the conditions: verify() again on the kept scene)
    assert JS.verify(dict(x=sc["x"], P=sc["P"], z=sc["z"], truncated_ok=sc.get("truncated_ok", False))) is not None
    ref = sc["ref"]
    inc = JR.associate_joint(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2, JS.CHI2, JS.MAX_NODES, form="incremental")
    assert np.array_equal(inc["assoc"], ref["assoc"])
    for key in FIELDS:
        assert inc[key] == ref[key], key
    assert len(inc["trace"]) == len(ref["trace"])
    worst = 0.0
    for (pa, da, _ta, oka, _ca), (pb, db, _tb, okb, _cb) in zip(ref["trace"], inc["trace"]):
        assert pa == pb and oka == okb
        worst = max(worst, abs(da - db) / abs(da))
    print(f"{sc['name']}: {ref['tests']} tests, literal against incremental d2: largest relative difference {worst:.2e}, "
          f"nearest margin {sc['worst_margin']:.2e}, 2k eps cond {sc['worst_cond_bar']:.2e}")
    assert worst <= 1e-10
    assert sc["worst_margin"] >= JS.DELTA and sc["worst_cond_bar"] <= JS.COND_BAR
    if kind == "pairs":
        nn, jc = sc["nn"], ref["assoc"]
        assert len(set(nn[nn > 0].tolist())) < int((nn > 0).sum()) and len(set(jc[jc > 0].tolist())) == int((jc > 0).sum())
    if kind == "sizes" and arg == 1:
        assert ref["assoc"][0] == sc["nn"][0]
    if kind == "trunc":
        assert ref["truncated"] == 1
    else:
        assert ref["truncated"] == 0


def _small_scene(seed, nz):
    """Five or fewer observations among paired landmarks: small enough to enumerate every hypothesis."""
    rng = np.random.default_rng(seed)
    pose = np.array([50.0, 50.0, 0.4])
    a = pose[:2] + rng.uniform(-25, 25, (6, 2))
    pts = np.stack([a, a + rng.normal(0, 0.8, (6, 2))], axis=1).reshape(-1, 2)
    x, P = AS.round_state(np.concatenate([pose, pts.reshape(-1)]), AS.scaled_cov(rng, 12, 1.0, 0.3, 0.2, 0.4), "f64")
    ids = rng.choice(np.arange(1, 13), nz, replace=False)
    return x, P, JS.observe(JS.true_state(x, P, rng), ids, rng)


@pytest.mark.parametrize("seed,nz", [(1, 1), (2, 3), (3, 4), (4, 5), (5, 5), (6, 5)])
def test_exhaustive_enumeration_confirms_the_pairing_count(seed, nz):
    x, P, z = _small_scene(seed, nz)
    ref = JR.associate_joint(x, P, z, R, GATE1, GATE2, JS.CHI2, 10 ** 6)
    assert ref["pairings"] == JR.exhaustive_best_count(x, P, z, R, GATE1, JS.CHI2) and not ref["exhausted"]
    used = ref["assoc"][ref["assoc"] > 0]
    assert len(set(used.tolist())) == len(used)
    if nz == 1:
        assert np.array_equal(ref["assoc"], JS.nn_vector(x, P, z))


def _two_landmarks(sep=0.6):
    x = np.array([0.0, 0.0, 0.0, 20.0, 0.0, 20.0, sep])
    P = np.diag([0.25, 0.25, 0.01, 0.01, 0.01, 0.01, 0.01])
    P[3, 0] = P[0, 3] = P[5, 0] = P[0, 5] = 0.0
    return x, P


def test_two_observations_that_prefer_one_landmark_come_out_distinct():
    """Both observations lie nearer to landmark 1 than to landmark 2 (the nearest neighbour gives both to landmark 1); the joint search
    pairs the second one with landmark 2."""
    x, P = _two_landmarks()
    zp1, _ = O.predict_observation(x, 1)
    zp2, _ = O.predict_observation(x, 2)
    z = np.stack([zp1 + [0.02, -0.001], zp1 + 0.35 * (zp2 - zp1)], axis=1)
    assert JS.nn_vector(x, P, z).tolist() == [1, 1]
    ref = JR.associate_joint(x, P, z, R, GATE1, GATE2, JS.CHI2, 1000)
    assert ref["assoc"].tolist() == [1, 2] and ref["pairings"] == 2
    assert ref["tests"] >= 2                                         # (obs 0 <-> 1; obs 1 skips the used landmark 1 and tests 2)


def test_an_individually_compatible_spurious_observation_is_rejected():
    """Three landmarks seen exactly where a shifted vehicle would see them (a common offset the pose covariance explains), and a fourth
    observation that is inside landmark 4's own gate but contradicts that common offset: alone it is compatible, jointly it is not."""
    N = 4
    pts = np.array([[20.0, 0.0], [0.0, 20.0], [-20.0, 0.0], [0.0, -20.0]])
    x = np.concatenate([[0.0, 0.0, 0.0], pts.reshape(-1)])
    P = np.diag([0.25, 0.25, 1e-4] + [1e-4] * (2 * N))
    xt = x.copy()
    xt[0] += 0.9                                                     # the vehicle really is 0.9 m further east
    f = lambda j: O.predict_observation(xt, j)[0]                    # noqa: E731
    z = np.stack([f(1), f(2), f(3), O.predict_observation(x, 4)[0]], axis=1)
    z[1] = np.arctan2(np.sin(z[1]), np.cos(z[1]))
    xg = x.copy()
    xg[0] -= 1.2                                                     # ... and observation 3 says it is 1.2 m further WEST
    z[:, 3] = O.predict_observation(xg, 4)[0]
    z[1, 3] = math.atan2(math.sin(z[1, 3]), math.cos(z[1, 3]))
    nis, _ = O.association_table_sparse(x, P, z, R)
    assert nis[3, 3] < GATE1                                         # individually compatible
    assert JS.nn_vector(x, P, z).tolist() == [1, 2, 3, 4]
    ref = JR.associate_joint(x, P, z, R, GATE1, GATE2, JS.CHI2, 1000)
    assert ref["assoc"].tolist() == [1, 2, 3, 0] and ref["pairings"] == 3


def test_max_nodes_stops_the_search_where_the_rule_says():
    sc = JS.build("pairs", 1, "f64")
    full = sc["ref"]
    for form in ("literal", "incremental"):
        for cut in (1, 2, full["tests"] // 2, full["tests"] - 1):
            part = JR.associate_joint(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2, JS.CHI2, cut, form=form, want_cond=False)
            assert part["exhausted"] == 1 and part["tests"] == cut
            assert [t[0] for t in part["trace"]] == [t[0] for t in full["trace"][:cut]]
            assert part["pairings"] <= full["pairings"]
        exact = JR.associate_joint(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2, JS.CHI2, full["tests"], form=form, want_cond=False)
        assert exact["exhausted"] == 0 and np.array_equal(exact["assoc"], full["assoc"])
    # with one node no hypothesis is completed: Best stays empty, the decisions are the unpaired ones
    one = JR.associate_joint(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2, JS.CHI2, 1)
    assert one["pairings"] == 0 and np.all(one["assoc"] <= 0)


def test_cross_matrix_blocks_are_the_blocks_of_the_dense_joint_covariance():
    x, P, _xt = JS.nis_state(31, "f64")
    ids = [7, 3, 31, 12]
    M, zp = JR.cross_matrix(x, P, R, ids)
    z = np.zeros((2, 4))
    _d2, S, ok = JR.joint_literal(x, P, z, R, list(enumerate(ids)))
    assert ok and np.allclose(M, S, rtol=0, atol=1e-13 * np.abs(S).max()) and np.allclose(M, M.T, rtol=0, atol=1e-15)
    for t, j in enumerate(ids):
        assert np.allclose(zp[t], O.predict_observation(x, j)[0], rtol=0, atol=1e-14)
