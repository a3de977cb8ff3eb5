"""Every body of the EKF covariance down-date against the fp64 oracle.

The update (csrc/ekf_update.hip: update_typed) and the down-date launch (csrc/ekf_syrk.hip: launch_downdate) pick one of
about ten kernel bodies from the dtype, the form, k = 2m, the device's own matched count (observe), the pre-split panel
image and the SLAMHIP_X bits.  `expected_path` mirrors that choice on the host; tests/test_ekf_dispatch_table.py checks
that the grids below reach every body.  Every GPU cell here is RE-ANCHORED: the device state is downloaded (fp32-rounded
in f32 mode) right before each call, the oracle repeats the call in fp64 from it, and the result is held to the per-call
tolerance of tests/test_gpu_ekf.py -- also for the steps of a chained schedule on one handle.
"""
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import strip_ref as S
from tests.test_gpu_ekf import R, TOL, check_side, noisy_obs, random_state, relerr, relerr_cov, rounded

pytestmark = pytest.mark.gpu

Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])

# ---- host mirror of the dispatch ---------------------------------------------------------------------------------------
KPAD = 32                      # csrc/common.h: SLAM_KPAD
PRODUCT_XFLAGS = 4 | 8 | 16 | 32 | 64 | 128 | 512     # csrc/common.h: SLAM_XFLAGS_MASK of the product library

LABELS = ("f32_tile", "f32_stream2", "f32_stream3", "f32_stream4", "f32_stream4_joseph", "f32_bf16_claim", "f32_bf16_list",
          "f32_global_factor+tile", "f64")
FALLBACKS = (None, "dd_tile", "skip")


def _up(a, b):
    return (a + b - 1) // b * b


def expected_path(dtype, form, m, xflags=0, device_m=None):
    """(label, fallback): the down-date body the host launches for an update of m observations, and what the kernel does
    when observe() gives it the device's matched count `device_m` (the host's m is then only an upper bound):
    None = the label's body, "dd_tile" = the kernel's fp32 dd_tile fall-back inside the same launch, "skip" = nothing."""
    joseph = form == "joseph"
    x = xflags & PRODUCT_XFLAGS                                      # ekf_api.hip: slam_ekf_create reads SLAMHIP_X
    if dtype == "f64":
        # launch_downdate (ekf_syrk.hip:1300-1305): one body; downdate_f64_mfma returns at k == 0 (ekf_syrk.hip:992-994)
        return "f64", ("skip" if device_m == 0 else None)
    k = 2 * m
    kp = _up(k, KPAD)                                                # ekf_update.hip:1494
    use_img = not joseph and kp <= 128 and not (x & 16)             # ekf_update.hip:1561
    kp_total = 2 * kp if joseph else _up(k, 16)                     # ekf_update.hip:1563 / 1572 / 1578 / 1588
    stream = 0                                                       # the launch's STREAM template argument
    if kp > 128:
        # pht_compact_kernel + factor_kernel<T, false> (ekf_update.hip:1517-1519, 1551-1555); kp_total > 128 in both forms
        label = "f32_global_factor+tile"
    elif not (x & 4) and 32 < kp_total <= 128:                       # ekf_syrk.hip:1253
        nch = -(-kp_total // 32)                                    # ekf_syrk.hip:1255
        if nch >= 3 and not joseph and not (x & 8):                 # ekf_syrk.hip:1266
            label = "f32_bf16_claim" if use_img else "f32_bf16_list"   # ekf_syrk.hip:1277-1288
            stream = 4
        elif nch == 4:                                              # ekf_syrk.hip:1290
            label, stream = ("f32_stream4_joseph" if joseph else "f32_stream4"), 4
        elif nch == 3:                                              # ekf_syrk.hip:1291
            label, stream = "f32_stream3", 3
        else:                                                       # ekf_syrk.hip:1292
            label, stream = "f32_stream2", 2
    else:
        label = "f32_tile"                                          # ekf_syrk.hip:1296-1299: downdate_f32_mfma<>
    if device_m is None:
        return label, None
    # the kernel's own kp (ekf_syrk.hip:838-842) and the branch it then takes
    kd = 2 * device_m
    kpd = 2 * _up(kd, KPAD) if joseph else _up(kd, 16)
    if kpd == 0:
        return label, "skip"
    if label in ("f32_bf16_claim", "f32_bf16_list"):
        if 80 <= kpd <= 128:                                        # ekf_syrk.hip:875 / 913
            return label, None
    elif stream and -(-kpd // 32) == stream:                        # ekf_syrk.hip:942: c.nchunks == STREAM
        return label, None
    elif not stream:
        return label, None
    return label, "dd_tile"


# ---- the grids (the CPU test checks that they reach every label) ---------------------------------------------------------
F32_REF_M = (16, 17, 31, 32, 33, 39, 40, 47, 49, 55, 63, 64, 65)
F32_REF_CELLS = [(m, N, 0) for N in (64, 127, 700) for m in F32_REF_M if m <= N] + \
                [(m, N, x) for x in (8, 16, 4, 128) for N in (127, 700) for m in (33, 49, 64)]
F32_JOSEPH_CELLS = [(m, N) for N in (64, 127, 700) for m in (12, 16, 17, 24, 32, 33, 40)]
F64_CELLS = [(form, m, N) for form in ("cholesky", "joseph") for N in (32, 63, 300) for m in (1, 8, 16, 17, 32, 33, 64, 65)
             if m <= N]
OBSERVE_CELLS = [(N, nz, j) for N in (127, 700) for nz in (40, 64, 70) for j in (0, 5, 16, 17, 33, 40, 60, 64) if j <= nz]
SCHEDULE = (("update", 64), ("update", 33), ("update", 17), ("update", 2), ("update", 65), ("joseph", 24), ("update", 64),
            ("add", 30), ("update_new", 64), ("predict", 0), ("update", 49))


def grid_paths():
    """(label, fallback) of every cell of the grids above, as expected_path gives them."""
    out = [expected_path("f32", "cholesky", m, x) for m, _N, x in F32_REF_CELLS]
    out += [expected_path("f32", "joseph", m) for m, _N in F32_JOSEPH_CELLS]
    out += [expected_path("f64", form, m) for form, m, _N in F64_CELLS]
    out += [expected_path("f32", "cholesky", nz, 0, device_m=j) for _N, nz, j in OBSERVE_CELLS]
    for dtype in ("f32", "f64"):
        out += [expected_path(dtype, "joseph" if op == "joseph" else "cholesky", m) for op, m in SCHEDULE if m]
    return out


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _spread(N):
    return 90.0 if N < 127 else (300.0 if N < 700 else 600.0)


def _handle(pkg, monkeypatch, x, P, dtype, xflags=0, max_landmarks=None):
    """SLAMHIP_X is read when the handle is created (ekf_api.hip: slam_ekf_create)."""
    if xflags:
        monkeypatch.setenv("SLAMHIP_X", str(xflags))
    else:
        monkeypatch.delenv("SLAMHIP_X", raising=False)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=max_landmarks)
    monkeypatch.delenv("SLAMHIP_X", raising=False)
    return st


def _check(st, xo, Po, prior, dtype, what, fx=1.0, fP=1.0):
    """The state after one call against the oracle's result of the same call from the same (downloaded) state."""
    xg, Pg = st.download()
    assert xg.shape == xo.shape and Pg.shape == Po.shape, what
    assert np.array_equal(Pg, Pg.T), f"{what}: P must stay exactly symmetric"
    check_side(st, Pg, what)
    ex = relerr(xg, xo)
    eP = relerr_cov(Pg, Po, np.diag(prior))
    assert ex <= TOL[dtype]["x"] * fx, f"{what}: x rel err {ex:.3e}"
    assert eP <= TOL[dtype]["P"] * fP, f"{what}: P rel err {eP:.3e}"


def _update_step(st, dtype, form, z, ids, what):
    xo, Po = rounded(st)                                             # re-anchor: the device's own state
    st.update(z, R, ids, form=form)
    if form == "joseph":
        xn, Pn = O.update_joseph_sparse(xo, Po, z, R, ids)
    else:
        xn, Pn = O.update_sparse(xo, Po, z, R, ids)
    _check(st, xn, Pn, Po, dtype, what, fP=2.0 if form == "joseph" else 1.0)


def _update_cell(pkg, monkeypatch, dtype, form, m, N, xflags, seed):
    rng = np.random.default_rng(seed)
    x, P = random_state(rng, N, spread=_spread(N))
    st = _handle(pkg, monkeypatch, x, P, dtype, xflags, max_landmarks=N)
    try:
        ids = rng.permutation(N)[:m] + 1
        z = noisy_obs(rng, rounded(st)[0], ids)
        path = expected_path(dtype, form, m, xflags)[0]
        _update_step(st, dtype, form, z, ids, f"{dtype} {form} N={N} m={m} SLAMHIP_X={xflags} ({path})")
    finally:
        st.close()


# ---- (c) independent cells ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,N,xflags", F32_REF_CELLS)
def test_f32_reference_form_against_the_oracle(pkg, monkeypatch, m, N, xflags):
    _update_cell(pkg, monkeypatch, "f32", "cholesky", m, N, xflags, 10_000 * N + 100 * m + xflags)


@pytest.mark.parametrize("m,N", F32_JOSEPH_CELLS)
def test_f32_joseph_form_against_the_oracle(pkg, monkeypatch, m, N):
    _update_cell(pkg, monkeypatch, "f32", "joseph", m, N, 0, 20_000 * N + m)


@pytest.mark.parametrize("form,m,N", F64_CELLS)
def test_f64_against_the_oracle(pkg, monkeypatch, form, m, N):
    _update_cell(pkg, monkeypatch, "f64", form, m, N, 0, 30_000 * N + 100 * m + (form == "joseph"))


# ---- (d) observe: the host's bound and the device's count --------------------------------------------------------------
def _matched_obs(rng, x, ids):
    """Observations of landmarks `ids` with a third of R's noise: far inside the inner gate of their own landmark."""
    zp, _, _ = O.obs_blocks(x, ids)
    return zp.T + rng.normal(0, [0.1 / 3, math.pi / 180 / 3], (len(ids), 2)).T


def _dead_band_obs(x, P, ids):
    """One observation per landmark of `ids`, moved along the range so that its nis is 10: between the inner gate (4) and
    the outer one (25) of that landmark, i.e. neither matched nor a new feature."""
    zp, S = O._landmark_S(x, P, R, ids)
    t = np.sqrt(10.0 / np.linalg.inv(S)[:, 0, 0])
    return np.stack([zp[:, 0] + t, zp[:, 1]])


def observe_state(rng, N):
    """A map whose gates are unambiguous: random_state's covariance scaled down to a heading sigma of about 3 degrees."""
    x, P = random_state(rng, N, spread=_spread(N))
    return x, 0.01 * P


def observe_inputs(rng, xo, Po, N, nz, j, nnew=0):
    """z (2 x (nz + nnew)): j matched observations, nz - j in the dead band, nnew far beyond every landmark.  A dead-band
    observation that would fall inside the inner gate of ANOTHER landmark is not used (the oracle picks them)."""
    order = rng.permutation(N) + 1
    zd = _dead_band_obs(xo, Po, order[j:])
    nis, nd = O.association_table_sparse(xo, Po, zd, R)
    keep = np.flatnonzero(O.assoc_vector(nis, nd, 4.0, 25.0) == 0)[:nz - j]
    assert len(keep) == nz - j
    z = np.hstack([_matched_obs(rng, xo, order[:j]), zd[:, keep],
                   np.vstack([rng.uniform(2000, 2100, nnew), rng.uniform(-3, 3, nnew)])])
    return z[:, rng.permutation(nz + nnew)]


def _observe_oracle(xo, Po, z, j, nnew):
    nis, nd = O.association_table_sparse(xo, Po, z, R)
    ao = O.assoc_vector(nis, nd, 4.0, 25.0)
    # the construction: exactly j matched, nnew new, the rest dropped
    assert int(np.sum(ao > 0)) == j and int(np.sum(ao < 0)) == nnew, (j, nnew, ao)
    return ao


@pytest.mark.parametrize("N,nz,j", OBSERVE_CELLS)
def test_observe_device_count_against_the_oracle(pkg, monkeypatch, N, nz, j):
    rng = np.random.default_rng(40_000 * N + 100 * nz + j)
    x, P = observe_state(rng, N)
    st = _handle(pkg, monkeypatch, x, P, "f32", max_landmarks=N + 8)
    try:
        xo, Po = rounded(st)
        xb, Pb = st.download()
        z = observe_inputs(rng, xo, Po, N, nz, j)
        ao = _observe_oracle(xo, Po, z, j, 0)
        a = st.observe(z, R, 4.0, 25.0)
        assert np.array_equal(a, ao), "observe's decisions differ from the oracle's"
        assert st.N == N
        path = expected_path("f32", "cholesky", nz, 0, device_m=j)
        if j == 0:
            xg, Pg = st.download()
            assert np.array_equal(xg, xb) and np.array_equal(Pg, Pb), "no match: the state must not move"
            return
        zf, idf, _ = O.split_assoc(z, ao)
        xn, Pn = O.update_sparse(xo, Po, zf, R, idf)
        _check(st, xn, Pn, Po, "f32", f"observe N={N} nz={nz} j={j} {path}")
    finally:
        st.close()


def test_observe_device_count_with_new_features(pkg, monkeypatch):
    """The same regime (host bound 64, device count 40: the claiming grid) with the unmatched observations new features."""
    N, nz, j, nnew = 700, 64, 40, 16
    rng = np.random.default_rng(41)
    x, P = observe_state(rng, N)
    st = _handle(pkg, monkeypatch, x, P, "f32", max_landmarks=N + nnew)
    try:
        xo, Po = rounded(st)
        z = observe_inputs(rng, xo, Po, N, nz - nnew, j, nnew)
        ao = _observe_oracle(xo, Po, z, j, nnew)
        a = st.observe(z, R, 4.0, 25.0)
        assert np.array_equal(a, ao)
        assert st.N == N + nnew
        zf, idf, zn = O.split_assoc(z, ao)
        xn, Pn = O.update_sparse(xo, Po, zf, R, idf)
        xn, Pn = O.add_features_sparse(xn, Pn, zn, R)
        _check(st, xn, Pn, Po, "f32", "observe with new features", fx=4.0, fP=100.0)
    finally:
        st.close()


# ---- (e) one handle, one schedule --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_handle_through_a_schedule(pkg, monkeypatch, dtype):
    """k grows and shrinks on one handle (stale W1 columns and image chunks of a larger k must not leak into a smaller
    one), the Joseph form runs between reference updates (the reference form keeps the Jacobian blocks in Smat, the
    Joseph form its S), add_features grows N into the last tile's padding rows and the next update reads them."""
    N0 = 127
    rng = np.random.default_rng(50 + (dtype == "f64"))
    x, P = random_state(rng, N0, spread=_spread(N0))
    st = _handle(pkg, monkeypatch, x, P, dtype, max_landmarks=200)
    try:
        for step, (op, m) in enumerate(SCHEDULE):
            what = f"{dtype} step {step}: {op} m={m}"
            N = st.N
            if op in ("update", "joseph"):
                ids = rng.permutation(N)[:m] + 1
                _update_step(st, dtype, "joseph" if op == "joseph" else "cholesky", noisy_obs(rng, rounded(st)[0], ids), ids, what)
            elif op == "update_new":
                new = np.arange(N0 + 1, N + 1)
                ids = np.concatenate([new, rng.permutation(N0)[:m - len(new)] + 1])[rng.permutation(m)]
                _update_step(st, dtype, "cholesky", noisy_obs(rng, rounded(st)[0], ids), ids, what)
            elif op == "add":
                xo, Po = rounded(st)
                zn = np.vstack([rng.uniform(5, 40, m), rng.uniform(-3, 3, m)])
                st.add_features(zn, R)
                xn, Pn = O.add_features_sparse(xo, Po, zn, R)
                assert st.N == N + m
                _check(st, xn, Pn, Po, dtype, what)
                # ... and entry by entry, to the rounding-level bound of tests/strip_ref.py
                n0 = len(xo)
                xg, Pg = st.download()
                ref = S.add_features_ref(xo[:3], Po[:, 0:3], zn, R)
                S.assert_within(Pg[n0:, :n0], ref["cross"], dtype, S.C_STRIP, "add_features cross: " + what)
                S.assert_within(Pg[n0:, n0:], ref["new"], dtype, S.C_BLOCK, "add_features new: " + what)
                S.assert_within(xg[n0:], ref["x"], dtype, S.C_STRIP, "add_features x: " + what)
                assert np.array_equal(xg[:n0], xo) and np.array_equal(Pg[:n0, :n0], Po), what
            else:
                xo, Po = rounded(st)
                st.predict(8.0, 0.05, 4.0, Q, 0.025)
                xn, Pn = O.predict_sparse(xo.copy(), Po.copy(), 8.0, 0.05, 4.0, Q, 0.025)
                _check(st, xn, Pn, Po, dtype, what)
                xg, Pg = st.download()
                ref = S.predict_ref(xo[:3], Po[:, 0:3], 8.0, 0.05, 4.0, Q, 0.025)
                S.assert_within(Pg[3:, 0:3], ref["strip"], dtype, S.C_STRIP, "predict strip: " + what)
                S.assert_within(Pg[0:3, 0:3], ref["vv"], dtype, S.C_BLOCK, "predict P_vv: " + what)
                S.assert_within(xg[0:3], ref["x"], dtype, S.C_STRIP, "predict x: " + what)
                assert np.array_equal(xg[3:], xo[3:]) and np.array_equal(Pg[3:, 3:], Po[3:, 3:]), what
        # what the schedule leaves behind: zero padding, bit-symmetric diagonal tiles, readers and side array in step
        S.check_storage(st, Pg=st.download("cov"), what=f"{dtype} after the schedule")
    finally:
        st.close()
