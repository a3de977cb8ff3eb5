"""The hand-over between the two filters on the device (slam_pf_to_ekf / slam_ekf_to_pf, csrc/handover.hip,
libslamhip_handover.so) against tests/handover_ref.py, the rule run literally in fp64 NumPy on what the device itself holds.

PARTICLES -> EKF.  The library has no particle upload, so a particle set is made by running the filter (init_landmarks with jitter,
predict, update_known, resampling); the reference then sees the downloaded set: exactly the rounded values the kernel read.  The
download flushes a pending normalisation shift into the stored log-weights -- (T)(logw - shift), the value the kernel forms -- so
where a shift is pending the hand-over comes FIRST and the download after it.  x and P come from slam_ekf_get_state.

TOLERANCE.  None is picked: every entry of x and P is held to the bound tests/handover_ref.py derives from the summation structure
include/slamhip_handover.h states (inputs 6 u, one fused chain of at most min(n, SLAB) terms per slab, the final rounding, the fp64
tail), |dP_ab| <= (Lc + 8) u sum what |d_a| |d_b| + u |P_ab| + F_ab.  tests/test_handover_ref_cpu.py shows that the bound
discriminates.  The largest observed error / bound per dtype is printed by the last test of each direction (profiles/handover_bounds.txt
records one run) and must be <= 1.

EKF -> PARTICLES.  The reference draws from the same Philox words in the arithmetic of the dtype; every pose and record value is held
to the rounding bound of the few operations of the rule (handover_ref.ekf_to_pf).  No statistical assertion anywhere.

Shapes: the smallest at which the kernels can go wrong -- n in {1, 3, 64, 65, 5013} (a partial wave, a partial chunk of 32, no
multiple of 4), one particle more than a slab and one more than two slabs; 31 landmarks in fp64 (D = 65: landmark 31's rows 63 | 64
straddle the tile edge), 63 and 70 in fp32 (rows 127 | 128), one landmark, none."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from oracle import pf_ref as F
from tests import handover_ref as HR
from tests import strip_ref as SR
from tests.strip_ref import check_storage
from tests.test_gpu_ekf import check_state, noisy_obs, random_state
from tests.test_gpu_pf import TOL as PF_TOL, close

pytestmark = pytest.mark.gpu

R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
GATE1, GATE2 = 4.0, 25.0
SLAB = HR.SLAB
MAP_BOUND = 4096 * 2.0 ** -53 * 2                                    # tests/test_gpu_pf_map.py: the bound of a sum of the read-out
RATIO = {"to_ekf": {"f32": 0.0, "f64": 0.0}, "to_pf": {"f32": 0.0, "f64": 0.0}}      # largest observed error / bound


def scene(nl, seed):
    return np.random.default_rng(seed).uniform(-40, 40, (nl, 2))


def observe(lm, pose, ids, rng):
    dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
    return np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))


def advance(pose, d, g=0.0):
    return np.array([pose[0] + d * math.cos(g + pose[2]), pose[1] + d * math.sin(g + pose[2]), pose[2] + d * math.sin(g) / 4.0])


def run_filter(f, lm, nseen, steps=3, pose0=(1.0, -2.0, 0.4), sharp=0):
    """The same short run for a PFShard and for the oracle: `nseen` landmarks initialised with jitter (a different map in every
    particle), `steps` predict + update_known steps (spread poses, unequal weights, records updated).  sharp > 0: the landmarks
    after `nseen` are initialised WITHOUT jitter at variance 1e-6 and `sharp` of them are then observed with R = diag(1e-6, 1e-8):
    the log-weights spread over thousands and one particle is left with the mass."""
    pose = np.array(pose0, dtype=np.float64)
    f.set_pose(pose)
    if sharp:
        f.init_landmarks(lm, 1e-6, 0.0)
    f.init_landmarks(lm[:nseen], 0.04, 0.3)
    rng = np.random.default_rng(3)
    for t in range(steps):
        f.predict(6.0, 0.05 * t, 4.0, Q, 0.1)
        pose = advance(pose, 0.6, 0.05 * t)
        ids = np.array([1 + t % nseen, 1 + (t + 2) % nseen])
        f.update_known(observe(lm, pose, ids, rng), ids, R)
    for k in range(sharp):
        ids = np.array([nseen + 1 + k])
        f.update_known(observe(lm, pose, ids, rng), ids, np.diag([1e-6, 1e-8]))
    return pose


def blank(pkg, dtype, cap):
    return pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype=dtype, max_landmarks=cap)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_to_ekf(pkg, sh, st, ids, dtype, what, seen_ids=None):
    """One slam_pf_to_ekf into `st`, then the download of `sh`, then the reference on that download.  Returns the reference."""
    info = sh.to_ekf_into(st, ids)
    xg, Pg = st.download()
    pose, logw, lm = sh.download()
    use = list(seen_ids) if ids is None else [int(i) for i in ids]
    ref = HR.pf_to_ekf(pose, logw, lm, use, dtype)
    D = 3 + 2 * len(use)
    assert st.N == len(use) and xg.shape == (D,) and Pg.shape == (D, D), what
    assert ref["counts"].tolist() == [sh.n] * len(use), what
    ex = np.abs(xg.astype(np.float64) - ref["x"])
    ex[2] = abs(float(HR.wrap(ex[2])))                                # (a mean heading at +-pi may come out on either side)
    eP = np.abs(Pg.astype(np.float64) - ref["P"])
    rx, rP = float(np.max(ex / ref["xbound"])), float(np.max(eP / ref["Pbound"]))
    print(f"{what}: x error / bound {rx:.3g}, P error / bound {rP:.3g} (largest bound / sqrt(P_aa P_bb) "
          f"{float(np.max(ref['Pbound'] / np.maximum(np.sqrt(np.outer(np.diag(ref['P']), np.diag(ref['P']))), 1e-300))):.3g})")
    RATIO["to_ekf"][dtype] = max(RATIO["to_ekf"][dtype], rx, rP)
    assert rx <= 1.0, (what, "x", int(np.argmax(ex / ref["xbound"])), rx)
    assert rP <= 1.0, (what, "P", np.unravel_index(int(np.argmax(eP / ref["Pbound"])), eP.shape), rP)
    assert bits_equal(Pg, Pg.T), what
    check_storage(st, pkg, Pg=Pg, what=what)
    W, neff, n, N = ref["info"]
    assert info["n"] == n == sh.n and info["N"] == N, what
    assert info["W"] == pytest.approx(W, rel=1e-12) and info["neff"] == pytest.approx(neff, rel=1e-10), what
    return ref


# ---- particles -> EKF: the shapes ------------------------------------------------------------------------------------------------
TO_EKF_CASES = [("f64", 1, 31), ("f64", 3, 31), ("f64", 64, 31), ("f64", 65, 31), ("f64", 5013, 31), ("f64", SLAB["f64"] + 1, 31),
                ("f64", 2 * SLAB["f64"] + 1, 1),
                ("f32", 1, 63), ("f32", 3, 70), ("f32", 64, 63), ("f32", 65, 70), ("f32", 5013, 63), ("f32", SLAB["f32"] + 1, 70),
                ("f32", 2 * SLAB["f32"] + 1, 1)]


@pytest.mark.parametrize("dtype,n,nl", TO_EKF_CASES)
def test_to_ekf_against_the_rule(pkg, dtype, n, nl):
    """All landmarks (ids = NULL), a shuffled subset, and the pose alone (cnt = 0), into one destination after another state."""
    E = SR.TILE[dtype]
    # landmark (E - 4) / 2 + 1 = 31 (fp64) / 63 (fp32) has its rows E - 1 | E on either side of the first tile edge
    assert nl == 1 or ((E - 4) % 2 == 0 and nl >= (E - 4) // 2 + 1 and 3 + 2 * ((E - 4) // 2) == E - 1)
    lm = scene(nl + 2, 21)
    sh = pkg.PFShard(n, nl + 2, 100 + n, dtype=dtype)                 # two slots more than landmarks: they stay unseen
    run_filter(sh, lm, nl)
    st = blank(pkg, dtype, nl + 5)
    every = list(range(1, nl + 1))
    ref = check_to_ekf(pkg, sh, st, None, dtype, f"{dtype} n={n} nl={nl} all", seen_ids=every)
    if n == 1:                                                        # one particle: no spread, P = blockdiag(P_i)
        # (the device forms mu = (w x) / w, which is x to a rounding: its pose block is of the order u64^2 |x|^2, inside the bound)
        assert not ref["P"][:3].any() and np.all(np.abs(st.download("cov")[:3]) <= 1e-25)
    # agreement with the per-landmark read-out on the same filter
    gm = sh.get_map(every)
    xg, Pg = (a.astype(np.float64) for a in st.download())
    for i in range(nl):
        f = 3 + 2 * i
        scale = MAP_BOUND * (gm[i, 1] ** 2 + gm[i, 2] ** 2 + 1.0)     # get_map forms E[m m'] - mean mean': its cancellation
        assert abs(xg[f] - gm[i, 1]) <= ref["xbound"][f] and abs(xg[f + 1] - gm[i, 2]) <= ref["xbound"][f + 1]
        for (a, b), col in (((f, f), 3), ((f + 1, f), 4), ((f + 1, f + 1), 5)):
            assert abs(Pg[a, b] - gm[i, col]) <= ref["Pbound"][a, b] + scale, (i, a, b)
    rng = np.random.default_rng(n)
    sub = rng.permutation(every)[:max(1, (2 * nl) // 3)]
    check_to_ekf(pkg, sh, st, sub, dtype, f"{dtype} n={n} nl={nl} shuffled subset of {len(sub)}")
    check_to_ekf(pkg, sh, st, [], dtype, f"{dtype} n={n} nl={nl} pose alone")
    assert st.N == 0
    st.close()
    sh.close()


# ---- the weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_uniform_weights_pending_shift_and_log_weights_at_minus_700(pkg, dtype):
    n, nl = 5013, 6
    lm = scene(nl, 22)
    sh = pkg.PFShard(n, nl, 7, dtype=dtype)
    sh.set_pose([1.0, -2.0, 0.4])
    sh.init_landmarks(lm, 0.04, 0.3)
    sh.predict(6.0, 0.02, 4.0, Q, 0.1)
    st = blank(pkg, dtype, 10)
    ref = check_to_ekf(pkg, sh, st, None, dtype, f"{dtype} uniform weights", seen_ids=range(1, nl + 1))
    assert ref["info"][1] == pytest.approx(n, rel=1e-6)               # Neff = n
    run_filter(sh, lm, nl)                                           # unequal weights, not normalised
    gm, s1, _ = sh.weight_stats()
    sh.normalize(gm, s1)                                             # the shift is PENDING: the hand-over must honour it
    info = sh.to_ekf_into(st, None)
    assert info["W"] == pytest.approx(1.0, rel=1e-5 if dtype == "f32" else 1e-12)
    P1 = st.download("cov")
    sh.download(landmarks=False)                                     # (applies the shift: the stored log-weights are (T)(logw - shift) now)
    ref = check_to_ekf(pkg, sh, st, None, dtype, f"{dtype} after the download applied the shift", seen_ids=range(1, nl + 1))
    # (the pending call formed (T)(logw - shift) itself, the second call read it stored: the same weights, the same bits)
    assert bits_equal(P1, st.download("cov"))
    # log-weights stored around -700 with a shift of -700 pending: w = exp(logw + 700)
    sh.normalize(700.0, 1.0)
    sh.weights()                                                     # (flushes: the stored log-weights are about -700 now)
    lw = sh.download(landmarks=False)[1]
    assert -760 < lw.min() and lw.max() < -690
    sh.normalize(-700.0, 1.0)
    info = sh.to_ekf_into(st, [2, 5, 1])
    assert 0.1 < info["W"] < 10.0 and np.all(np.isfinite(st.download("cov")))
    check_to_ekf(pkg, sh, st, [2, 5, 1], dtype, f"{dtype} log-weights at -700")
    st.close()
    sh.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_particle_holds_all_but_1e_30_of_the_mass(pkg, dtype):
    """Two sharp observations leave one particle with the mass (designed on the fp64 oracle: the runner-up lies 417 below in
    log-weight).  Asserted from the download: 0 < the others' share <= 1e-30."""
    n, nl, seed = 65, 8, 11
    lm = scene(nl, 21)
    sh = pkg.PFShard(n, nl, seed, dtype=dtype)
    run_filter(sh, lm, 5, sharp=2)
    st = blank(pkg, dtype, 8)
    # not normalised, the log-weights lie tens of thousands below zero: every weight underflows, W == 0 is refused
    with pytest.raises(pkg.SlamHipError, match="weights sum to zero"):
        sh.to_ekf_into(st, [1])
    assert st.N == 0
    gm, s1, _ = sh.weight_stats()
    sh.normalize(gm, s1)
    lw = np.sort(sh.download(landmarks=False)[1].astype(np.float64))[::-1]
    rest = float(np.exp(lw[1:] - lw[0]).sum())
    assert 0.0 < rest <= 1e-30, rest
    ref = check_to_ekf(pkg, sh, st, [3, 1, 5, 2, 4], dtype, f"{dtype} one particle with the mass")
    assert ref["info"][1] == pytest.approx(1.0, abs=1e-12)
    # (the pose block is the spread of one particle: at most the others' share of the squared distances)
    assert np.all(np.abs(st.download("cov")[:3, :3]) <= 1e-20)
    st.close()
    sh.close()


# ---- live ancestor tables, headings across +-pi --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_through_live_ancestor_tables_and_headings_across_pi(pkg, dtype):
    """After slam_pf_resample_local and before anything materialises: the first pass reads the records through the tables, the
    Gram kernel after pf_materialise.  The vehicle drives with its heading at +-pi, so the particles' headings lie on both sides."""
    n, nl = 5013, 9
    lm = scene(nl, 23)
    sh = pkg.PFShard(n, nl, 31, dtype=dtype)
    fs = pkg.FastSLAM(sh)
    turn = 6.0 * 0.1 * math.sin(0.3) / 4.0                           # the heading's advance per step: after three steps it stands at pi
    pose = np.array([2.0, 1.0, math.pi - 3 * turn])
    sh.set_pose(pose)
    sh.init_landmarks(lm, 0.04, 0.3)
    rng = np.random.default_rng(5)
    for t in range(3):
        pose = advance(pose, 0.6, 0.3)
        pose[2] = float(HR.wrap(pose[2]))
        ids = np.array([1 + t, 4 + t])
        fs.step(6.0, 0.3, 4.0, Q, 0.1, observe(lm, pose, ids, rng), ids, R, force_resample=(t == 1))
    # step 1 resampled (lazily), step 2 updated landmarks 3 and 6 only: the others still sit behind their tables
    st = blank(pkg, dtype, 12)
    info = sh.to_ekf_into(st, None)
    x1, P1 = st.download()
    ref = check_to_ekf(pkg, sh, st, None, dtype, f"{dtype} live tables, headings across pi", seen_ids=range(1, nl + 1))
    assert bits_equal(P1, st.download("cov")) and bits_equal(x1, st.download("x")), "materialised or not: the same bits"
    p = sh.download(landmarks=False)[0]
    assert p[2].max() > 3.0 and p[2].min() < -3.0, "headings on both sides of +-pi"
    assert abs(abs(ref["x"][2]) - math.pi) < 0.2 and ref["P"][2, 2] < 0.05 and info["n"] == n
    st.close()
    sh.close()


# ---- dst ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_larger_state_left_in_dst_is_cleared_and_calls_repeat_bit_for_bit(pkg, dtype):
    """dst of a larger capacity (another ld than ceil(D / E) tile rows) that held a LARGER state: what lies beyond the new state is
    +0.0 again (check_storage reads the raw buffer through slam_ekf_device_ptrs).  Two calls in a row give the same bits; the source's
    download is the same before and after."""
    E = SR.TILE[dtype]
    n, nl, N_old, cap = 300, 20, 150, 200
    rng = np.random.default_rng(8)
    x0, P0 = random_state(rng, N_old)
    st = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=cap)
    st.observe(noisy_obs(rng, st.download("x").astype(np.float64), [3, 50, 149]), R, GATE1, GATE2)      # (a used update workspace)
    st.sync()
    lm = scene(nl, 24)
    sh = pkg.PFShard(n, nl, 9, dtype=dtype)
    run_filter(sh, lm, nl)
    before = sh.download()
    ref = check_to_ekf(pkg, sh, st, None, dtype, f"{dtype} into a handle that held {N_old} landmarks", seen_ids=range(1, nl + 1))
    view, ld, _E = SR.raw_view(st)
    assert ld // E > (3 + 2 * nl + E - 1) // E and (3 + 2 * N_old + E - 1) // E > (3 + 2 * nl + E - 1) // E
    raw1 = view.cpu().numpy().copy()
    x1 = st.download("x")
    sh.to_ekf_into(st, None)
    raw2 = SR.raw_view(st)[0].cpu().numpy()
    assert bits_equal(raw1, raw2) and bits_equal(x1, st.download("x")), "two calls, different bits"
    after = sh.download()
    assert all(bits_equal(a, b) for a, b in zip(before, after)), "the particle set changed"
    # dst is a working filter: one observe against the oracle's update of the REFERENCE state
    xo, Po = ref["x"].copy(), ref["P"].copy()
    ids = [2, 7, 11, 19]
    # (every observation half a sigma beside its prediction: all four pass the gate, none starts a landmark)
    z = np.column_stack([O.predict_observation(xo, j)[0] for j in ids]) + np.array([[0.05], [0.5 * math.pi / 180]])
    nis, nd = O.association_table_sparse(xo, Po, z, R)
    want = O.assoc_vector(nis, nd, GATE1, GATE2)
    assert np.array_equal(want, ids), want
    a = st.observe(z, R, GATE1, GATE2)
    assert np.array_equal(a, want)
    zf, idf, _zn = O.split_assoc(z, want)
    xu, Pu = O.update_sparse(xo, Po, zf, R, idf)
    check_state(st, xu, Pu, dtype, f"{dtype} observe after the hand-over", prior=Po)
    check_storage(st, pkg, what="after the observe")
    st.close()
    sh.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_refusal_leaves_both_states_bit_identical(pkg, dtype):
    L = pkg._lib
    lib = L.handover_lib()
    n, nl = 257, 6
    lm = scene(nl, 25)
    sh = pkg.PFShard(n, nl, 12, dtype=dtype)
    run_filter(sh, lm, 4)                                            # landmarks 5 and 6 are never seen
    rng = np.random.default_rng(13)
    x0, P0 = random_state(rng, 3)
    st = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=3)
    other = blank(pkg, "f32" if dtype == "f64" else "f64", 8)
    snap, xs = SR.snapshot(st), st.download("x")
    before = sh.download()

    def refused(code, word, dst, ids):
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
        rc = lib.slam_pf_to_ekf(dst._h, sh._h, idv.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), None)
        assert rc == code and word in L.last_error(), (rc, L.last_error())
        assert SR.changed_offsets(st, snap).size == 0 and bits_equal(st.download("x"), xs) and st.N == 3
        assert all(bits_equal(a, b) for a, b in zip(before, sh.download()))

    refused(L.SLAM_E_BADARG, "landmark 5", st, [1, 5])               # unseen: in use in 0 of n particles
    refused(L.SLAM_E_BADARG, "duplicate", st, [2, 1, 2])
    refused(L.SLAM_E_BADARG, "out of range", st, [0])
    refused(L.SLAM_E_BADARG, "out of range", st, [nl + 1])
    refused(L.SLAM_E_BADARG, "dtype", other, [1])
    refused(L.SLAM_E_CAPACITY, "capacity", st, [1, 2, 3, 4])
    with pytest.raises(pkg.SlamHipError):
        sh.to_ekf_into(st, None)                                     # NULL: the four seen landmarks do not fit three either
    assert SR.changed_offsets(st, snap).size == 0
    # a filter run with unknown correspondences: slot 2 is empty in every particle, slot 1 is in use in all of them
    sh.clear_landmarks()
    sh.update_unknown(np.array([[12.0], [0.3]]), R, GATE1, GATE2)
    before = sh.download()
    refused(L.SLAM_E_BADARG, "landmark 2", st, [1, 2])
    assert sh.to_ekf_into(st, [1])["N"] == 1 and st.N == 1           # ... and with the identity given, the call goes through
    for s in (st, other):
        s.close()
    sh.close()


def test_to_ekf_through_the_drivers(pkg):
    pf = pkg.PFSlamState(300, 6, seed=3, dtype="f64", distributed=False)
    lm = scene(6, 26)
    run_filter(pf.shard, lm, 5)
    st = pf.to_ekf()
    assert isinstance(st, pkg.EKFSlamState) and st.N == 5 and st.handover_info["n"] == 300 and st.handover_info["N"] == 5
    s2 = pkg.particles_to_ekf(pf, ids=[4, 2], max_landmarks=7)
    assert s2.N == 2 and s2.capacity == 7
    sel = st.select([4, 2])                                          # the marginal of the joint Gaussian is the joint Gaussian of the subset
    assert np.allclose(sel.download("cov"), s2.download("cov"), rtol=1e-9, atol=1e-12)
    assert st.feature_ellipses().shape == (5, 5)
    for s in (st, s2, sel):
        s.close()
    pf.close()


def test_largest_to_ekf_ratio_is_recorded():
    print("handover bounds, slam_pf_to_ekf: largest observed error / bound " + ", ".join(f"{d} {v:.3g}" for d, v in RATIO["to_ekf"].items()))
    assert all(v <= 1.0 for v in RATIO["to_ekf"].values()), RATIO


# ---- EKF -> particles ------------------------------------------------------------------------------------------------------------------
def ekf_source(pkg, dtype, N, seed, cap=None):
    rng = np.random.default_rng(seed)
    x, P = random_state(rng, N)
    x[2] = 0.3 + 0.01 * N
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=cap or max(N, 1))
    xr, Pr = (a.astype(np.float64) for a in st.download())
    return st, xr, Pr


def check_particles(sh, ref, cnt, dtype, what, n=None):
    pose, logw, lm = sh.download()
    n = sh.n if n is None else n
    T = HR.NP_DTYPE[dtype]
    assert np.all(np.abs(pose[2]) <= T(math.pi)), what
    e = np.abs(pose[:, :n].astype(np.float64) - ref["pose"][:, :n])
    e[2] = np.abs(HR.wrap(e[2]))                                     # (a heading within rounding of +-pi may wrap on one side only)
    rp = float(np.max(e / ref["pose_bound"][:, :n]))
    rl = 0.0
    if cnt:
        el = np.abs(lm[:cnt, :2, :n].astype(np.float64) - ref["lm"][:, :2, :n])
        rl = float(np.max(el / ref["lm_bound"][:, :, :n]))
        # the conditional covariance: the same bits in every particle, the table's value rounded to the dtype
        assert np.all(lm[:cnt, 2:5, :] == lm[:cnt, 2:5, :1]), what
        Cm = ref["table"][4]
        assert np.all(np.abs(lm[:cnt, 2:5, 0].astype(np.float64) - Cm) <= (HR.U[dtype] + 1e-9) * np.abs(Cm) + 1e-14), what
    assert not lm[cnt:].any(), f"{what}: a slot beyond the hand-over is not the empty record"
    assert np.all(logw == T(-math.log(sh.n_global))), what
    print(f"{what}: pose error / bound {rp:.3g}, landmark error / bound {rl:.3g}")
    RATIO["to_pf"][dtype] = max(RATIO["to_pf"][dtype], rp, rl)
    assert rp <= 1.0 and rl <= 1.0, (what, rp, rl)


@pytest.mark.parametrize("n", [1, 4, 5013])
@pytest.mark.parametrize("N", [0, 1, 31, 70])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_to_pf_against_the_rule(pkg, dtype, N, n):
    st, xr, Pr = ekf_source(pkg, dtype, N, 200 + N)
    seed = 1000 + N
    pf = st.to_particles(n, seed=seed, max_landmarks=N + 2)
    sh = pf.shard
    ref = HR.ekf_to_pf(xr, Pr, np.arange(1, N + 1), n, 0, seed, dtype)
    check_particles(sh, ref, N, dtype, f"{dtype} N={N} n={n}")
    sums = sh.map_sums()
    assert np.array_equal(sums[1:, 9], np.where(np.arange(N + 2) < N, float(n), 0.0)), "landmarks 1 .. N in use in every particle"
    assert pf.resamples == 0 and sh.resample_count() == 0
    if N == 31 and n == 5013:
        # a second hand-over into the same filter consumes the next RNG step; a subset in another order
        ids = [9, 30, 2]
        sh.from_ekf(st, ids)
        check_particles(sh, HR.ekf_to_pf(xr, Pr, ids, n, 1, seed, dtype), 3, dtype, f"{dtype} subset, second RNG step")
    pf.close()
    st.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_particles_depend_on_their_global_id_alone_and_the_filter_runs_on(pkg, dtype):
    N, n, seed = 12, 5013, 77
    st, xr, Pr = ekf_source(pkg, dtype, N, 300)
    a = st.to_particles(n, seed=seed)
    b = st.to_particles(6000, seed=seed)                             # 6000 is a multiple of 4 (16-byte stores), 5013 is not
    pa, _wa, la = a.shard.download()
    pb, _wb, lb = b.shard.download()
    assert bits_equal(pa, np.ascontiguousarray(pb[:, :n])) and bits_equal(la, np.ascontiguousarray(lb[:, :, :n]))
    # one more step of the filter against the oracle started from the REFERENCE particles (the bars of tests/test_gpu_pf.py)
    ref = HR.ekf_to_pf(xr, Pr, np.arange(1, N + 1), n, 0, seed, dtype)
    orc = F.OraclePF(n, N, seed)
    orc.pose, orc.lm, orc.logw = ref["pose"].copy(), ref["lm"].copy(), ref["logw"].copy()
    orc.seen[:] = True
    orc.step = 1
    rng = np.random.default_rng(6)
    lmxy = xr[3:].reshape(N, 2)
    pose = advance(xr[:3], 0.6, 0.05)
    ids = np.array([3, 8, 3, 12])
    z = observe(lmxy, pose, ids, rng)
    a.shard.predict(6.0, 0.05, 4.0, Q, 0.1)
    orc.predict(6.0, 0.05, 4.0, Q, 0.1)
    a.shard.update_known(z, ids, R)
    orc.update_known(z, ids, R)
    p, lw, l = a.shard.download()
    tol = PF_TOL[dtype]
    assert close(p, orc.pose, tol) and close(l[:, 0:2], orc.lm[:, 0:2], tol)
    assert close(l[:, 2:5], orc.lm[:, 2:5], tol * 10, scale=float(np.max(np.abs(orc.lm[:, 2:5]))))
    assert close(lw, orc.logw, tol * 10, scale=max(1.0, float(np.max(np.abs(orc.logw)))))
    for f in (a, b):
        f.close()
    st.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_to_pf_refusals_leave_the_filter_as_it_was(pkg, dtype):
    L = pkg._lib
    N = 5
    st, xr, Pr = ekf_source(pkg, dtype, N, 400)
    sh = pkg.PFShard(260, 4, 5, dtype=dtype)
    run_filter(sh, scene(4, 27), 4)
    before = sh.download()

    def same():
        return all(bits_equal(a, b) for a, b in zip(before, sh.download()))

    with pytest.raises(pkg.SlamHipError) as e:
        sh.from_ekf(st)                                              # five landmarks, four slots
    assert e.value.code == L.SLAM_E_CAPACITY and same()
    for bad in ([0], [N + 1], [2, 2]):
        with pytest.raises(pkg.SlamHipError) as e:
            sh.from_ekf(st, bad)
        assert e.value.code == L.SLAM_E_BADARG and same()
    other = blank(pkg, "f32" if dtype == "f64" else "f64", 4)
    with pytest.raises(pkg.SlamHipError) as e:
        sh.from_ekf(other, [])
    assert e.value.code == L.SLAM_E_BADARG and same()
    # a vehicle known exactly
    P0 = Pr.copy()
    P0[:3, :] = 0.0
    P0[:, :3] = 0.0
    st.set_state(xr, P0)
    with pytest.raises(pkg.NotPositiveDefinite):
        sh.from_ekf(st, [1, 2])
    assert same()
    # an indefinite conditional block of landmark 2 -- refused only where landmark 2 is asked for
    P1 = Pr.copy()
    P1[5, 5] -= 1.0
    st.set_state(xr, P1)
    with pytest.raises(pkg.NotPositiveDefinite):
        sh.from_ekf(st, [1, 2, 3])
    assert same()
    # the RNG step was not consumed by any refusal: the first hand-over that succeeds draws with step = the filter's own (3 predicts)
    sh.from_ekf(st, [1, 3])
    ref = HR.ekf_to_pf(xr, P1, [1, 3], 260, 3, 5, dtype)
    check_particles(sh, ref, 2, dtype, f"{dtype} after the refusals")
    for s in (st, other):
        s.close()
    sh.close()


def test_largest_to_pf_ratio_is_recorded():
    print("handover bounds, slam_ekf_to_pf: largest observed error / bound " + ", ".join(f"{d} {v:.3g}" for d, v in RATIO["to_pf"].items()))
    assert all(v <= 1.0 for v in RATIO["to_pf"].values()), RATIO
    out = os.environ.get("HANDOVER_BOUNDS_OUT")
    if out:
        with open(out, "w") as f:
            for k, row in RATIO.items():
                f.write(f"{k}: " + ", ".join(f"{d} {v:.4g}" for d, v in row.items()) + "\n")
