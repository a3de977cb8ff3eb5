"""csrc/ekf_strip.hip on the device, both dtypes: predict_kernel, augment_kernel (add_features) and the state movers
(pack / unpack / block_gather / side_rebuild / ellipse) against tests/strip_ref.py.

Every cell is RE-ANCHORED: the device's own state is read right before the call, the entry-wise reference repeats the call
from it in extended precision, and after the call
  * every entry the call owns is within the derived bound  u_T |ref| + c 2^-53 mag  (strip_ref: c = 16 / 32),
  * every other entry is bit-identical -- checked on the RAW tile-major buffer against a device snapshot, so it also
    holds for the padding and at sizes where the matrix is never downloaded,
  * the storage invariants hold (strip_ref.check_storage: padding +0.0, diagonal tiles bit-symmetric, get_block / download
    read what is stored, the packed side array equals the matrix),
  * P == P' where a full download is taken.
The largest (err - u_T |ref|) / (2^-53 mag) seen per operation and dtype is printed by the last test.

-0.0 in the padding: check_storage requires +0.0 (all bits clear) and the kernels meet that, so no reader has to care.
"""
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import strip_ref as S
from tests.test_gpu_ekf import DTYPES, noisy_obs, random_state, rounded

pytestmark = pytest.mark.gpu

# full symmetric matrices with correlation
RF = np.array([[0.1 ** 2, 0.4 * 0.1 * (math.pi / 180)], [0.4 * 0.1 * (math.pi / 180), (math.pi / 180) ** 2]])
QF = np.array([[0.5 ** 2, -0.3 * 0.5 * (3 * math.pi / 180)], [-0.3 * 0.5 * (3 * math.pi / 180), (3 * math.pi / 180) ** 2]])
WORST = {}                     # (kind, dtype) -> largest ratio seen, reported by the last test
F64 = np.float64


def _L(dtype):
    return 7 if dtype == "f32" else 6


def _eq_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(S._bits(a), S._bits(b))


def _only_owned(st, snap, owned, what):
    changed = S.changed_offsets(st, snap)
    stray = np.setdiff1d(changed, owned)
    assert stray.size == 0, f"{what}: {stray.size} stored entries the call does not own changed (first offsets {stray[:8]})"
    return changed


def predict_step(st, dtype, v, g, w, Qm, dt, what, full=True, storage=True):
    """One predict, re-anchored.  Returns (reference, changed raw offsets)."""
    n = st.n
    xb = st.download("x")
    Pb = st.download("cov") if full else None
    col = Pb[:, 0:3] if full else st.get_block(0, 0, n, 3)
    db = None if full else st.diag()
    _v, ld, _E = S.raw_view(st)
    snap = S.snapshot(st)
    st.predict(v, g, w, Qm, dt)
    ref = S.predict_ref(xb[:3].astype(F64), np.asarray(col, dtype=F64), v, g, w, Qm, dt)
    xg = st.download("x")
    assert _eq_bits(xg[3:], xb[3:]), f"{what}: landmark means moved"
    changed = _only_owned(st, snap, S.predict_owned_offsets(n, ld, _L(dtype)), what)
    Pg = None
    if full:
        Pg = st.download("cov")
        assert _eq_bits(Pg, Pg.T), f"{what}: P is not symmetric"
        assert _eq_bits(Pg[3:, 3:], Pb[3:, 3:]), f"{what}: the map block changed"
        colg = Pg[:, 0:3]
    else:
        colg = st.get_block(0, 0, n, 3)
        assert _eq_bits(st.get_block(0, 0, 3, n), colg.T), f"{what}: row strip and column strip differ"
        assert _eq_bits(st.diag()[3:], db[3:]), f"{what}: landmark variances changed"
    S.assert_within(colg[3:], ref["strip"], dtype, S.C_STRIP, "predict strip: " + what, WORST)
    S.assert_within(colg[0:3], ref["vv"], dtype, S.C_BLOCK, "predict P_vv: " + what, WORST)
    S.assert_within(xg[0:3], ref["x"], dtype, S.C_STRIP, "predict x: " + what, WORST)
    if storage:
        S.check_storage(st, Pg=Pg, what=what)
    return ref, changed


def add_step(st, dtype, zn, Rm, what, full=True, storage=True, through="add_features"):
    """One add_features (or observe on an empty map), re-anchored."""
    n0, N0 = st.n, st.N
    nn = zn.shape[1]
    xb = st.download("x")
    Pb = st.download("cov") if full else None
    col = Pb[:, 0:3] if full else st.get_block(0, 0, n0, 3)
    _v, ld, _E = S.raw_view(st)
    snap = S.snapshot(st)
    if through == "observe":
        assert N0 == 0
        a = st.observe(zn, Rm, 4.0, 25.0)
        assert a.tolist() == [-1] * nn
    else:
        st.add_features(zn, Rm)
    assert st.N == N0 + nn, what
    n1 = st.n
    ref = S.add_features_ref(xb[:3].astype(F64), np.asarray(col, dtype=F64), zn, Rm)
    xg = st.download("x")
    assert xg.shape == (n1,) and _eq_bits(xg[:n0], xb), f"{what}: old entries of x changed"
    _only_owned(st, snap, S.add_owned_offsets(n0, nn, ld, _L(dtype)), what)
    Pg = None
    if full:
        Pg = st.download("cov")
        assert _eq_bits(Pg, Pg.T), f"{what}: P is not symmetric"
        assert _eq_bits(Pg[:n0, :n0], Pb), f"{what}: the old block changed"
        cross, new = Pg[n0:, :n0], Pg[n0:, n0:]
    else:
        cross, new = st.get_block(n0, 0, 2 * nn, n0), st.get_block(n0, n0, 2 * nn, 2 * nn)
        assert _eq_bits(st.get_block(0, n0, n0, 2 * nn), cross.T), f"{what}: the cross blocks and their mirror differ"
        assert _eq_bits(new, new.T), f"{what}: the new corner is not symmetric"
    S.assert_within(cross, ref["cross"], dtype, S.C_STRIP, "add_features cross: " + what, WORST)
    S.assert_within(new, ref["new"], dtype, S.C_BLOCK, "add_features new: " + what, WORST)
    S.assert_within(xg[n0:], ref["x"], dtype, S.C_STRIP, "add_features x: " + what, WORST)
    if storage:
        S.check_storage(st, Pg=Pg, what=what)
    return ref


def device_state(pkg, N, dtype, max_landmarks, seed, heading=0.7):
    """A handle with a random map of N landmarks whose dense covariance exists on the DEVICE only: P = sum_k a_k a_k' + 0.01 I
    from element-wise outer products (bit-symmetric by construction), uploaded with slam_ekf_set_state_device."""
    import torch
    n = 3 + 2 * N
    st = pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype=dtype, max_landmarks=max_landmarks)
    rng = np.random.default_rng(seed)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    dev = torch.device("cuda", 0)
    L = 100.0 * math.sqrt(max(N, 35) / 35.0)
    x = np.concatenate([[L / 2, L / 2, heading], rng.uniform(0, L, 2 * N)]).astype(st.np_dtype)
    Pd = torch.zeros((n, n), dtype=tdt, device=dev)
    for _k in range(4):
        a = torch.from_numpy(rng.normal(0, 0.2, n).astype(st.np_dtype)).to(dev)
        Pd.addcmul_(a[:, None], a[None, :])
    Pd.diagonal().add_(0.01)
    xd = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    st.set_state_device(xd.data_ptr(), Pd.data_ptr(), n, n)       # symmetric: row-major == column-major
    st.sync()
    del Pd
    torch.cuda.empty_cache()
    return st


# ---- predict ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [0, 1, 62, 63, 126, 127, 128, 129, 1000])
def test_predict_sizes(pkg, dtype, N):
    """One and two workgroups (N = 128 -> 129), the first tile edge of each dtype, full Q with correlation."""
    rng = np.random.default_rng(3000 + N)
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 5)
    try:
        for k, (v, g) in enumerate(((7.5, 0.1), (-4.0, -0.35))):
            ref, _ = predict_step(st, dtype, v, g, 4.0, QF, 0.025, f"{dtype} N={N} call {k}")
            assert ref["wrapped"] == 0
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["g0", "v0", "vneg", "wide_dt"])
def test_predict_inputs(pkg, dtype, case):
    v, g, dt = {"g0": (8.0, 0.0, 0.025), "v0": (0.0, 0.3, 0.025), "vneg": (-6.0, 0.2, 0.05), "wide_dt": (9.0, -0.45, 0.8)}[case]
    rng = np.random.default_rng(17)
    for N in (40, 200):
        x, P = random_state(rng, N)
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
        try:
            predict_step(st, dtype, v, g, 4.0, QF, dt, f"{dtype} {case} N={N}")
        finally:
            st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_with_dt_zero_returns_the_state_bit_for_bit(pkg, dtype):
    rng = np.random.default_rng(18)
    for N, phi in ((0, 0.4), (150, -2.9), (150, math.pi)):
        x, P = random_state(rng, N)
        x[2] = phi                                      # inside (-pi, pi]: x[2] must come back too
        st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N + 3)
        try:
            xb, Pb = st.download()
            inside = -math.pi < float(xb[2]) <= math.pi      # (fp32 rounds pi upwards: then the one wrap applies, as in the reference)
            _ref, changed = predict_step(st, dtype, 8.0, 0.3, 4.0, QF, 0.0, f"{dtype} dt=0 N={N}")
            xg, Pg = st.download()
            assert changed.size == 0 and _eq_bits(Pg, Pb), "dt = 0 must not move the covariance"
            assert _eq_bits(xg[:2], xb[:2]) and _eq_bits(xg[3:], xb[3:])
            if inside:
                assert _eq_bits(xg[2:3], xb[2:3])
            else:
                assert dtype == "f32" and abs(float(xg[2]) - O.mpi_to_pi(float(xb[2]))) <= 2.0 ** -24 * math.pi
        finally:
            st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("phi,g,sign", [(math.pi - 5e-4, 0.3, 1), (-math.pi + 5e-4, -0.3, -1), (math.pi - 5e-4, -0.3, 0),
                                        (-math.pi + 5e-4, 0.3, 0)])
def test_predict_wraps_the_heading_once(pkg, dtype, phi, g, sign):
    """Heading within 1e-3 of +-pi and a steering angle that pushes it over (or back inside): exactly one conditional wrap
    (src/common.jl:102-110), x[2] within the bound of the reference's mpi_to_pi."""
    rng = np.random.default_rng(19)
    x, P = random_state(rng, 70)
    x[2] = phi
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=70)
    try:
        ref, _ = predict_step(st, dtype, 8.0, g, 4.0, QF, 0.025, f"{dtype} phi={phi:+.4f} g={g:+.1f}")
        assert ref["wrapped"] == sign
        assert -math.pi <= float(st.download("x")[2]) <= math.pi
        assert abs(float(st.download("x")[2])) > 3.1          # one wrap, not a reset
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_with_a_zero_heading_column_leaves_the_strip_bit_identical(pkg, dtype):
    rng = np.random.default_rng(20)
    N = 300
    x, P = random_state(rng, N)
    P[:, 2] = 0.0
    P[2, :] = 0.0
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    try:
        _v, ld, _E = S.raw_view(st)
        _ref, changed = predict_step(st, dtype, 8.0, 0.2, 4.0, QF, 0.025, f"{dtype} P[:, 2] = 0")
        pose_block = S.stored_offsets(ld, _L(dtype), np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3))
        assert changed.size and np.setdiff1d(changed, pose_block).size == 0, "only P_vv may move when P[:, 2] = 0"
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_at_10k_landmarks(pkg, dtype):
    """79 workgroups: the last arrival rewrites the pose.  Read through get_block(0, 0, n, 3), get_block(0, 0, 3, n), diag()."""
    N = 10000
    st = device_state(pkg, N, dtype, N, seed=51)
    try:
        for k in range(2):
            predict_step(st, dtype, 8.0, 0.1 - 0.3 * k, 4.0, QF, 0.025, f"{dtype} N={N} call {k}", full=False, storage=(k == 1))
    finally:
        st.close()


def test_predict_at_50k_landmarks_fp32(pkg):
    """C5 size in fp32: 391 workgroups, a 20 GB state.  The raw buffer is compared with its snapshot in full; the storage
    invariants on the first column band and the diagonal tiles."""
    N = 50000
    try:
        probe = pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype="f32", max_landmarks=N)
    except pkg.SlamHipError as e:
        if e.code == pkg._lib.SLAM_E_HIP:
            pytest.skip("the 20 GB state cannot be allocated on this device")
        raise
    probe.close()
    st = device_state(pkg, N, "f32", N, seed=52)
    try:
        predict_step(st, "f32", 8.0, 0.15, 4.0, QF, 0.025, f"f32 N={N}", full=False)
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N0,nn", [(120, 15), (250, 10)])
def test_predict_chain_across_grids_of_different_size(pkg, dtype, N0, nn):
    """9 predicts, an add_features that changes predict's grid (1 -> 2 and 2 -> 3 workgroups), 9 more predicts, five times
    on ONE handle: the arrival counter must be back at 0 after every launch.  Every call moves the pose -- a launch in
    which no workgroup is 'last' leaves x[0:3] and P_vv behind, and the bound on them catches it."""
    rng = np.random.default_rng(60 + N0)
    x, P = random_state(rng, N0)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N0 + nn)
    try:
        for rep in range(5):
            st.set_state(x, P)
            for k in range(19):
                what = f"{dtype} N0={N0} rep {rep} call {k}"
                if k == 9:
                    zn = np.vstack([rng.uniform(5, 60, nn), rng.uniform(-3, 3, nn)])
                    add_step(st, dtype, zn, RF, what)
                    continue
                pose = st.download("x")[:3].copy()
                predict_step(st, dtype, 8.0, 0.25 * math.sin(k + rep), 4.0, QF, 0.025, what, storage=(k in (8, 18)))
                assert not np.array_equal(st.download("x")[:2], pose[:2]), f"{what}: the pose did not move"
    finally:
        st.close()


# ---- add_features -------------------------------------------------------------------------------------------------------------
N0_EDGES = {"f32": (125, 127, 129, 255, 257, 513), "f64": (61, 63, 65, 127, 255, 257, 513)}
ADD_CELLS = [(dtype, n0, nn) for dtype in DTYPES for n0 in N0_EDGES[dtype] for nn in (1, 2, 23, 64)]


def _new_obs(rng, nn):
    """Ranges 5 .. 400 m, bearings well outside (-pi, pi]; from 23 observations on, one of them at range 0."""
    zn = np.vstack([rng.uniform(5, 400, nn), rng.uniform(-7, 7, nn)])
    if nn >= 23:
        zn[0, nn // 2] = 0.0
    return zn


@pytest.mark.parametrize("dtype,n0,nn", ADD_CELLS)
def test_add_features_at_tile_and_workgroup_edges(pkg, dtype, n0, nn):
    """First free row n0 = 3 + 2 N against the tile edge E (E - 3, E - 1: the new landmark's rows straddle two tile rows,
    E + 1, 2 E - 1) and the 256-thread edges of the cross-block threads; 23 new features are 276 pairs (the stride loop of
    workgroup 0 takes a second turn), 64 are 2080 and span a tile edge themselves.  nn = 2 and 64 fill the capacity
    exactly."""
    N = (n0 - 3) // 2
    rng = np.random.default_rng(7000 + 10 * n0 + nn)
    x, P = random_state(rng, N)
    cap = N + nn if nn in (2, 64) else N + nn + 37
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=cap)
    try:
        add_step(st, dtype, _new_obs(rng, nn), RF, f"{dtype} n0={n0} nn={nn}")
        if cap == N + nn:
            with pytest.raises(pkg.SlamHipError) as ei:
                st.add_features(np.array([[5.0], [0.1]]), RF)
            assert ei.value.code == pkg._lib.SLAM_E_CAPACITY and st.N == cap
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("through", ["add_features", "observe"])
@pytest.mark.parametrize("nn", [1, 2, 23, 64])
def test_add_features_to_an_empty_map(pkg, dtype, through, nn):
    rng = np.random.default_rng(80 + nn)
    Pvv = np.array([[0.3, 0.05, 0.02], [0.05, 0.2, -0.01], [0.02, -0.01, 0.01]])
    st = pkg.EKFSlamState(np.array([3.0, -2.0, 2.5]), Pvv, dtype=dtype, max_landmarks=nn)
    try:
        add_step(st, dtype, _new_obs(rng, nn), RF, f"{dtype} empty map nn={nn} via {through}", through=through)
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_features_at_10k_landmarks(pkg, dtype):
    """N = 10 000 -> 10 016: the new rows lie 78 (fp32) / 156 (fp64) tile rows below the pose strip they are formed from."""
    N, nn = 10000, 16
    st = device_state(pkg, N, dtype, N + nn, seed=53)
    try:
        rng = np.random.default_rng(54)
        add_step(st, dtype, _new_obs(rng, nn), RF, f"{dtype} N={N} nn={nn}", full=False)
        predict_step(st, dtype, 8.0, 0.1, 4.0, QF, 0.025, f"{dtype} N={N + nn} predict after add", full=False, storage=False)
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_features_after_the_map_shrank(pkg, dtype):
    """set_state of a larger map, then of a smaller one on the same handle, then add_features: the rows the larger map
    occupied are padding again and must read zero -- the new features' rows land there."""
    rng = np.random.default_rng(90)
    xl, Pl = random_state(rng, 300)
    xs, Ps = random_state(rng, 100)
    st = pkg.EKFSlamState(xl, Pl, dtype=dtype, max_landmarks=320)
    try:
        S.check_storage(st, Pg=st.download("cov"), what="large map")
        st.set_state(xs, Ps)
        S.check_storage(st, Pg=st.download("cov"), what="after the shrink")
        add_step(st, dtype, _new_obs(rng, 5), RF, f"{dtype} add_features after a shrink")
        predict_step(st, dtype, 8.0, 0.1, 4.0, QF, 0.025, f"{dtype} predict after a shrink")
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pre_gate_bound_follows_a_far_new_landmark(pkg, monkeypatch, dtype):
    """augment_kernel raises the pre-gate's variance bound (atomicMax on pmax) by the new landmarks' variances.  A landmark
    added 400 m away from a map with millimetre variances has a block more than 1e4 times larger than any other; observations of it that the oracle matches or drops
    (dead band) would be skipped by a pre-gate that still held the old bound -- and come back as new features.  Sweep
    (pre-gate forced on), grid and default mode against the oracle."""
    rng = np.random.default_rng(95)
    N = 300
    x, P = random_state(rng, N, spread=300.0)
    monkeypatch.setenv("SLAMHIP_X", "64")
    st = pkg.EKFSlamState(x, 1e-4 * P, dtype=dtype, max_landmarks=N + 1)
    monkeypatch.delenv("SLAMHIP_X", raising=False)
    try:
        xo, Po = rounded(st)
        old = rng.choice(np.arange(1, N + 1), 8, replace=False)
        for mode in ("sweep", "grid"):                                   # the bound of the OLD map is computed and kept
            st.set_gate_mode(mode)
            st.associate_vector(noisy_obs(rng, xo, old), RF, 4.0, 25.0)
        vmax = float(np.max(np.diag(Po)[3:]))
        add_step(st, dtype, np.array([[400.0], [0.4]]), RF, f"{dtype} far landmark")
        xo, Po = rounded(st)
        assert np.max(np.diag(Po)[-2:]) > 1e4 * vmax
        zp, _ = O.predict_observation(xo, N + 1)
        zold = O.obs_blocks(xo, old)[0].T + rng.normal(0, [0.03, math.pi / 540], (len(old), 2)).T     # far inside the inner gate
        z = np.hstack([zold, (zp + [0.0, 0.9 * math.pi / 180]).reshape(2, 1),
                       (zp + [0.0, 4.0 * math.pi / 180]).reshape(2, 1), (zp + [0.05, -0.5 * math.pi / 180]).reshape(2, 1)])
        nis, nd = O.association_table_sparse(xo, Po, z, RF)
        ao = O.assoc_vector(nis, nd, 4.0, 25.0)
        assert ao[-3] == N + 1 and ao[-2] == 0 and ao[-1] == N + 1, (ao[-3:], nis[-3:, N])
        assert nis[-3, N] < 3.0 and 6.0 < nis[-2, N] < 20.0                # decisions with a margin
        for mode in ("sweep", "grid", "auto"):
            st.set_gate_mode(mode)
            assert np.array_equal(st.associate_vector(z, RF, 4.0, 25.0), ao), mode
    finally:
        st.close()


# ---- state movers -------------------------------------------------------------------------------------------------------------
def test_fp32_state_upload_and_download_in_bands(pkg):
    """fp32 twin of test_state_upload_and_download_in_bands: n = 8203 columns of 32 812 bytes, so the 256 MiB staging buffer
    takes 8064 columns and a ragged band of 139 follows; the tile edge is 128.  Bit for bit."""
    rng = np.random.default_rng(13)
    N = 4100
    n = 3 + 2 * N
    assert n * n * 4 > (256 << 20)
    W = (256 << 20) // (4 * n) // 128 * 128
    assert 0 < n - W < W
    x, P = random_state(rng, N, rank=3)
    x, P = x.astype(np.float32), P.astype(np.float32)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N + 60)
    try:
        xg, Pg = st.download()
        assert _eq_bits(xg, x) and _eq_bits(Pg, P)
        for r0, c0, nr, nc in ((W - 70, W - 40, 140, 90),          # across the band edge, around the diagonal
                               (n - 300, W - 130, 300, 200),       # below the diagonal, across band and tile edge
                               (100, W - 5, 50, 60),               # above the diagonal, across the band edge
                               (127, 120, 3, 20), (120, 127, 20, 3), (8060, 0, 143, 3), (0, 8060, 3, 143)):
            assert _eq_bits(st.get_block(r0, c0, nr, nc), P[r0:r0 + nr, c0:c0 + nc]), (r0, c0, nr, nc)
        assert _eq_bits(st.diag(), np.diag(P).copy())
        S.check_storage(st, Pg=Pg, what="fp32 banded upload")
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_written_on_a_landmark_that_straddles_a_tile_row(pkg, dtype):
    """Landmark j = 62 (fp32) / 30 (fp64), 0-based: f = 3 + 2 j is the last row of the first tile, f + 1 the first of the
    next.  side_rebuild_kernel takes P[f + 1, f] from the tile BELOW the diagonal tile."""
    import torch
    rng = np.random.default_rng(14)
    E = S.TILE[dtype]
    j = (E - 4) // 2
    f = 3 + 2 * j
    assert f == E - 1
    N = 100
    x, P = random_state(rng, N)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    try:
        view, ld, _E = S.raw_view(st)
        L = _L(dtype)
        before = st.landmark_blocks()
        vals = np.array([3.25, -0.625, 7.5], dtype=st.np_dtype)
        idx = np.array([int(S.p_off(ld, L, f, f)), int(S.p_off(ld, L, f + 1, f)), int(S.p_off(ld, L, f + 1, f + 1))])
        assert idx[1] // (E * E) == 1 and idx[0] // (E * E) == 0          # tile (1, 0) below tile (0, 0)
        view[torch.as_tensor(idx, device="cuda")] = torch.as_tensor(vals, device="cuda")
        torch.cuda.synchronize()
        assert _eq_bits(st.landmark_blocks(), before)                     # stale until the library is told
        st.state_written()
        blk = st.landmark_blocks()
        assert _eq_bits(blk[:, j], vals)
        keep = np.arange(N) != j
        assert _eq_bits(blk[:, keep], before[:, keep])
        Pg = st.download("cov")
        assert Pg[f, f] == vals[0] and Pg[f + 1, f] == vals[1] and Pg[f, f + 1] == vals[1] and Pg[f + 1, f + 1] == vals[2]
        S.check_storage(st, Pg=Pg, what=f"{dtype} state_written")
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ellipses_at_10k_landmarks_after_add_features(pkg, dtype):
    """ellipse_kernel over 10 016 landmarks (straddling ones and ones beyond the first tile row included) against
    O.feature_ellipses, with the tolerances of test_telemetry_ellipses_and_monitor_schema.  The oracle is fed the 2 x 2
    diagonal blocks (check_storage has just shown that the packed blocks equal the matrix), 500 landmarks at a time."""
    N, nn = 10000, 16
    st = device_state(pkg, N, dtype, N + nn, seed=55)
    try:
        st.add_features(_new_obs(np.random.default_rng(56), nn), RF)
        S.check_storage(st, what=f"{dtype} before the ellipses")
        Ntot = st.N
        xg = st.download("x").astype(F64)
        blk = st.landmark_blocks().astype(F64)
        Eg = st.feature_ellipses()
        assert Eg.shape == (5, Ntot)
        Eo = np.empty((5, Ntot))
        for a in range(0, Ntot, 500):
            b = min(Ntot, a + 500)
            m = b - a
            xc = np.concatenate([xg[:3], xg[3 + 2 * a:3 + 2 * b]])
            Pc = np.zeros((3 + 2 * m, 3 + 2 * m))
            fi = 3 + 2 * np.arange(m)
            Pc[fi, fi], Pc[fi + 1, fi], Pc[fi, fi + 1], Pc[fi + 1, fi + 1] = blk[0, a:b], blk[1, a:b], blk[1, a:b], blk[2, a:b]
            Eo[:, a:b] = O.feature_ellipses(xc, Pc)
        tol = 1e-9 if dtype == "f64" else 1e-5
        assert np.allclose(Eg[:4], Eo[:4], rtol=tol, atol=tol)
        assert np.all(Eg[2] <= Eg[3] + 1e-15) and np.all(np.abs(Eg[4]) <= math.pi / 2 + 1e-12)
        aniso = (Eo[3] - Eo[2]) > 1e-3 * Eo[3]
        dphi = np.abs(np.angle(np.exp(2j * (Eg[4] - Eo[4])))) / 2
        assert aniso.sum() > Ntot // 2 and np.all(dphi[aniso] < (1e-7 if dtype == "f64" else 2e-3))
    finally:
        st.close()


def test_zz_report_the_largest_ratios(pkg):
    """Not a check of its own: prints, per operation and dtype, the largest (err - u_T |ref|) / (2^-53 mag) the cells above
    have seen, next to the committed c (run the module with -s to read it)."""
    for (kind, dtype), worst in sorted(WORST.items()):
        c = S.C_BLOCK if ("P_vv" in kind or "new" in kind) else S.C_STRIP
        print(f"largest ratio  {kind:24s} {dtype}: {worst:8.3f}   (committed c = {c:g})")
        assert worst <= c * S.C_FACTOR
