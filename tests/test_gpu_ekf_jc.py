"""Joint-compatibility data association on the device (libslamhip_jc.so, csrc/ekf_jc.hip) against the literal reference of
tests/jc_ref.py on the scenes of tests/jc_scenes.py: joint_nis on designed hypotheses, associate_joint decision for decision and
count for count, the state untouched bit for bit, observe_joint against the three calls made by hand, sim(association="joint"),
and the argument checks.

Measured on an MI355X (worst over the cases of a test, reference = the literal form):
    joint_nis       relative error of d2   fp64 6.2e-14   fp32 states 2.5e-14        (bar: TOL = 1e-9)
    associate_joint relative error of d2   fp64 1.9e-14   fp32 states 1.7e-14        (bar: TOL = 1e-9)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import jc_ref as JR
from tests import jc_scenes as JS
from tests import strip_ref as SR

pytestmark = pytest.mark.gpu

R = JS.R
GATE1, GATE2, TOL = JS.GATE1, JS.GATE2, JS.TOL
INFO_INT = ("pairings", "tests", "exhausted", "truncated", "candidates", "deepest")


def _state(pkg, sc, extra=8):
    return pkg.EKFSlamState(sc["x"], sc["P"], dtype=sc["dtype"], max_landmarks=max(sc["N"] + extra, 1))


def _eq_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(SR._bits(a.reshape(-1)), SR._bits(b.reshape(-1)))


def _frozen(st):
    return SR.snapshot(st), st.download("x"), st.landmark_blocks(), st.gate_info(), st.N


def _assert_frozen(st, before, what):
    snap, x0, blk0, gi0, N0 = before
    assert SR.changed_offsets(st, snap).size == 0, f"{what}: P changed"
    assert _eq_bits(st.download("x"), x0) and _eq_bits(st.landmark_blocks(), blk0) and st.N == N0, f"{what}: x or the side array changed"
    assert st.gate_info() == gi0, f"{what}: the gating's counters changed"


def _check_against(ref, assoc, info, what):
    assert np.array_equal(assoc, ref["assoc"]), (what, assoc.tolist(), ref["assoc"].tolist())
    for key in INFO_INT:
        assert info[key] == ref[key], (what, key, info[key], ref[key])
    err = abs(info["d2"] - ref["d2"]) / max(abs(ref["d2"]), 1e-300) if ref["pairings"] else abs(info["d2"])
    print(f"{what}: {ref['tests']} tests, {ref['pairings']} pairings, d2 {ref['d2']:.6f}, relative error {err:.2e}")
    assert err <= TOL, (what, info["d2"], ref["d2"])


@pytest.mark.parametrize("dtype", JS.DTYPES)
@pytest.mark.parametrize("N", JS.NIS_N)
def test_joint_nis_on_designed_hypotheses_against_the_literal_reference(pkg, dtype, N):
    x, P, xt = JS.nis_state(N, dtype)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 4)
    before = _frozen(st)
    rng = np.random.default_rng(N)
    worst = 0.0
    for name, ids in JS.nis_cases(N, dtype):
        z = JS.observe(xt, ids, rng)
        want = JR.joint_nis(x, P, z, R, ids)
        got = st.joint_nis(z, ids, R)
        err = abs(got - want) / abs(want)
        worst = max(worst, err)
        assert err <= TOL, (dtype, N, name, got, want)
    print(f"joint_nis {dtype} N = {N}: worst relative error {worst:.2e}")
    _assert_frozen(st, before, f"joint_nis {dtype} N = {N}")
    # duplicate, out-of-range and too many ids: the status code, and the handle goes on working
    lib, jc = pkg._lib.jc_lib(), st._jc_handle()
    r = np.ascontiguousarray(R.T).reshape(4)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = C.c_double(-7.0)
    for ids in ([1, 1], [0], [N + 1], [1] * 65):
        zz = np.ones((len(ids), 2))
        arr = np.asarray(ids, dtype=np.int32)
        assert lib.slam_ekf_joint_nis(jc, zz.ctypes.data_as(dp), arr.ctypes.data_as(ip), len(ids), r.ctypes.data_as(dp), C.byref(out)) == \
            pkg._lib.SLAM_E_BADARG, ids
    assert lib.slam_ekf_joint_nis(jc, None, None, 0, r.ctypes.data_as(dp), C.byref(out)) == pkg._lib.SLAM_E_BADARG
    assert out.value == -7.0
    name, ids = JS.nis_cases(N, dtype)[0]
    z = JS.observe(xt, ids, rng)
    assert abs(st.joint_nis(z, ids, R) / JR.joint_nis(x, P, z, R, ids) - 1.0) <= TOL
    st.close()


@pytest.mark.parametrize("dtype", JS.DTYPES)
def test_joint_nis_reports_a_matrix_that_is_not_positive_definite(pkg, dtype):
    x, P, xt = JS.nis_state(31, dtype)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=40)
    z = JS.observe(xt, [3, 9], np.random.default_rng(1))
    with pytest.raises(pkg.NotPositiveDefinite):
        st.joint_nis(z, [3, 9], -1.0 * np.eye(2))
    assert abs(st.joint_nis(z, [3, 9], R) / JR.joint_nis(x, P, z, R, [3, 9]) - 1.0) <= TOL
    st.close()


@pytest.mark.parametrize("dtype", JS.DTYPES)
@pytest.mark.parametrize("kind,arg", JS.SCENES)
def test_associate_joint_on_the_seeded_scenes(pkg, dtype, kind, arg):
    sc = JS.build(kind, arg, dtype)
    ref = sc["ref"]
    st = _state(pkg, sc)
    before = _frozen(st)
    assoc, info = st.associate_joint_vector(sc["z"], R, GATE1, GATE2, chi2=JS.CHI2, max_nodes=JS.MAX_NODES)
    _check_against(ref, assoc, info, sc["name"])
    _assert_frozen(st, before, sc["name"])
    nn = st.associate_vector(sc["z"], R, GATE1, GATE2)
    assert np.array_equal(nn, sc["nn"])
    if kind == "pairs":                                    # the nearest neighbour uses a landmark twice, the joint search does not
        used = assoc[assoc > 0]
        assert len(set(used.tolist())) == len(used) and len(set(nn[nn > 0].tolist())) < int((nn > 0).sum())
        # fewer nodes than the scene needs: exhausted, and the same partial result as the rule gives
        for cut in (1, ref["tests"] // 2, ref["tests"] - 1):
            part = JR.associate_joint(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2, JS.CHI2, cut, form="literal", want_cond=False)
            assert part["exhausted"] == 1 and part["tests"] == cut
            a2, i2 = st.associate_joint_vector(sc["z"], R, GATE1, GATE2, chi2=JS.CHI2, max_nodes=cut)
            _check_against(part, a2, i2, f"{sc['name']} max_nodes = {cut}")
        a3, i3 = st.associate_joint_vector(sc["z"], R, GATE1, GATE2, chi2=JS.CHI2, max_nodes=ref["tests"])
        assert i3["exhausted"] == 0 and np.array_equal(a3, ref["assoc"])
    if kind == "sizes" and arg == 1:
        assert assoc[0] == nn[0] > 0
    if kind == "sizes" and arg == 64:
        assert info["pairings"] == info["deepest"] == 64
    if kind == "empty":
        assert assoc.tolist() == [-1, -1, -1] and info["tests"] == 0
    if kind == "trunc":
        assert info["truncated"] == 1
    # the same call again: the workspace is re-armed
    a4, i4 = st.associate_joint_vector(sc["z"], R, GATE1, GATE2, chi2=JS.CHI2, max_nodes=JS.MAX_NODES)
    assert np.array_equal(a4, assoc) and i4 == info
    st.close()


@pytest.mark.parametrize("dtype", JS.DTYPES)
def test_observe_joint_equals_the_three_calls_made_by_hand(pkg, dtype):
    sc = JS.build("pairs", 0, dtype)
    a, b = _state(pkg, sc), _state(pkg, sc)
    assoc, info = a.observe_joint(sc["z"], R, GATE1, GATE2)
    zf, idf, zn, info_b = b.associate_joint(sc["z"], R, GATE1, GATE2)
    assert info == info_b and np.array_equal(idf.reshape(-1), assoc[assoc > 0])
    b.update(zf, R, idf)
    b.add_features(zn, R)
    xa, Pa = a.download()
    xb, Pb = b.download()
    assert a.N == b.N == sc["N"] + int((assoc < 0).sum()) and _eq_bits(xa, xb) and _eq_bits(Pa, Pb)
    # the module-level names
    c = _state(pkg, sc)
    zf2, idf2, zn2, info2 = pkg.ekf.associate_joint(c, sc["z"], R, GATE1, GATE2)
    assert np.array_equal(idf2, idf) and info2 == info
    assoc2, _ = pkg.ekf.observe_joint(c, sc["z"], R, GATE1, GATE2)
    assert np.array_equal(assoc2, assoc) and _eq_bits(c.download("cov"), Pa)
    for h in (a, b, c):
        h.close()


@pytest.mark.parametrize("dtype", JS.DTYPES)
def test_sim_with_joint_association_reuses_no_landmark(pkg, golden_dir, dtype):
    S = pkg.sim
    cfg = np.load(os.path.join(golden_dir, "config1.npz"))
    wp = S.get_waypoints(os.path.join(golden_dir, "course1.txt"))
    st = pkg.EKFSlamState(S.initial_pose(wp), np.zeros((3, 3)), dtype=dtype, max_landmarks=200)
    log = S.sim(st, wp, cfg["landmarks"], seed=int(cfg["seed"][1]), nlaps=1, max_steps=200, association="joint")
    assert len(log.obs_steps) >= 20 and st.N >= 1
    for idf, _nn in log.assoc:
        assert len(set(idf)) == len(idf)
    assert sum(len(idf) for idf, _nn in log.assoc) > 0
    np.linalg.cholesky(np.asarray(st.download("cov"), dtype=np.float64))
    st.close()


@pytest.mark.parametrize("dtype", JS.DTYPES)
def test_bad_arguments_return_the_code_and_leave_the_handle_usable(pkg, dtype):
    sc = JS.build("outer", 0, dtype)
    st = _state(pkg, sc)
    L = pkg._lib
    lib, jc = L.jc_lib(), st._jc_handle()
    before = _frozen(st)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    nz = sc["z"].shape[1]
    zc = np.ascontiguousarray(sc["z"].T)
    r = np.ascontiguousarray(R.T).reshape(4)
    chi = np.ascontiguousarray(JS.CHI2[:nz])
    assoc = np.full(nz, 99, dtype=np.int32)
    info = np.full(8, -3.0)
    P_ = lambda a: a.ctypes.data_as(dp)                    # noqa: E731

    def call(z=zc, n=nz, rr=r, g1=GATE1, g2=GATE2, ch=chi, nodes=100, out=assoc, inf=info, h=jc):
        return lib.slam_ekf_associate_joint(h, P_(z) if z is not None else None, n, P_(rr) if rr is not None else None, g1, g2,
                                            P_(ch) if ch is not None else None, nodes,
                                            out.ctypes.data_as(ip) if out is not None else None, P_(inf) if inf is not None else None)

    bad_r, bad_chi = r.copy(), chi.copy()
    bad_r[3] = math.nan
    bad_chi[nz - 1] = math.inf
    cases = dict(null_handle=dict(h=None), null_z=dict(z=None), null_R=dict(rr=None), null_chi2=dict(ch=None), null_assoc=dict(out=None),
                 null_info=dict(inf=None), nz_negative=dict(n=-1), nz_65=dict(n=65), R_nan=dict(rr=bad_r), gate1_inf=dict(g1=math.inf),
                 gate2_nan=dict(g2=math.nan), chi2_inf=dict(ch=bad_chi), nodes_0=dict(nodes=0), nodes_over=dict(nodes=L.SLAM_JC_NODE_CAP + 1))
    for name, kw in cases.items():
        assert call(**kw) == L.SLAM_E_BADARG, name
    assert np.all(assoc == 99) and np.all(info == -3.0)
    created = C.c_void_p()
    assert lib.slam_ekf_jc_create(None, st._h) == L.SLAM_E_BADARG and lib.slam_ekf_jc_create(C.byref(created), None) == L.SLAM_E_BADARG
    assert lib.slam_ekf_jc_destroy(None) == L.SLAM_E_BADARG
    _assert_frozen(st, before, "bad arguments")
    assert call(nodes=L.SLAM_JC_NODE_CAP) == L.SLAM_OK and np.array_equal(assoc, sc["ref"]["assoc"])
    a, i = st.associate_joint_vector(sc["z"], R, GATE1, GATE2, chi2=JS.CHI2)
    _check_against(sc["ref"], a, i, "after the refused calls")
    a0, i0 = st.associate_joint_vector(np.zeros((2, 0)), R, GATE1, GATE2)
    assert a0.size == 0 and i0["pairings"] == 0 and i0["tests"] == 0
    st.close()
