"""GPU tests of the per-particle 2 x 2 landmark EKF (csrc/pf_device.h: lm_update, lm_init) on the designed records of
tests/lm_records.py: ONE call from injected per-particle state, every record against a longdouble evaluation of the oracle's formula
from bit-identical inputs, within margin x the record's OWN first-order rounding scale (margins from the CPU model, never from the
device; tests/test_lm_records_cpu.py shows what the bounds reject and what the suite's scene-wide tolerances let through).

INJECTION.  No entry point sets per-particle state; a shard takes the table as the "remote records" of a resampling in which every
ancestor lives on another rank (resample_apply, ancestor ids n .. 2 n - 1), after init_landmarks has marked landmarks 1 and 2 as seen
(`seen` is filter-wide and kept on the host).  The first download must be the table bit for bit.

a. the bound: per group of the table (an observation is filter-wide, see lm_records) one update_known call [landmark 1 seen,
   landmark 3 first sighted] on the freshly injected table; the group's particles are kept; compare_records on all of them, for the
   diagonal and the non-symmetric R; landmark 2 and the poses untouched bit for bit.
b. repeats: ids [1, 1] in one call == two calls.
c. the other forms of the step on the same records, bit for bit: step_fused == predict + update_known + weight_stats; the auto mode
   against the synchronous driver; fp32: four steps in one persistent launch == the four steps one by one.
d. the statistics and the normalisation on log-weights that spread over thousands (after the outlier class's observation), against
   float64 / longdouble evaluations from the downloaded log-weights.

MEASURED on the MI355X (worst error / bound per class, max over both noise matrices; printed by test a as "lm-record ..."):
see the table in DESIGN.md, "FastSLAM numerics: the landmark update against per-record bounds".
"""
import math

import numpy as np
import pytest

import lm_records as L
from test_gpu_pf import Q, _compare
from test_gpu_pf_batch import drive

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
WHEELBASE, DT = 4.0, 0.1                                   # the suite's motion (tests/test_gpu_pf.py)
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits(a):
    return np.ascontiguousarray(a).view(UINT[a.dtype])


def same_bits(a, b, what):
    """Two downloads (pose, logw, landmarks) bit for bit (NaN-proof: the bit patterns are compared)."""
    for x, y, part in zip(a, b, ("pose", "logw", "landmarks")):
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), f"{what}: {part} differ"


def inject(sh, t, clear=False):
    """The designed table as the state of shard `sh`; landmarks 1 and 2 seen, 3 not."""
    import torch
    if clear:
        sh.clear_landmarks()                               # (forgets `seen`: landmark 3 is a first sighting again)
    sh.init_landmarks(np.zeros((2, 2)), 0.01, 0.0)
    ids = torch.arange(t.n, 2 * t.n, dtype=torch.int32, device=sh.device)
    rec = torch.from_numpy(t.records.astype(sh.np_dtype)).to(sh.device)
    sh.resample_apply(ids, ids, rec)


def injected(pkg, t, dtype, n_global=None, seed=5):
    sh = pkg.PFShard(t.n, L.NL, seed, dtype=dtype, first=0, n_global=t.n if n_global is None else n_global)
    inject(sh, t)
    return sh


def assert_is_table(state, t, n_global):
    pose, logw, lm = state
    T = pose.dtype.type
    assert np.array_equal(bits(pose), bits(t.records[0:3].astype(T))), "injected poses"
    assert np.array_equal(bits(lm), bits(t.records[3:].reshape(L.NL, 5, t.n).astype(T))), "injected landmark records"
    assert np.all(logw == T(-math.log(n_global)))


# ---- a. the bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(L.NOISES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_landmark_update_and_first_sighting_within_per_record_bounds(pkg, dtype, which):
    cs = L.case(dtype, which)
    t = cs.t
    T = L.NP_DTYPE[dtype]
    sh = pkg.PFShard(t.n, L.NL, 5, dtype=dtype, first=0, n_global=2 * t.n)
    got = {q: np.full(cs.truth[q].shape, np.nan) for q in L.QUANTITIES}
    done = np.zeros(t.n, dtype=bool)
    for g in range(len(t.obs)):
        inject(sh, t, clear=g > 0)
        if g == 0:
            assert_is_table(sh.download(), t, 2 * t.n)
        z, ids = L.group_call(t, g)
        sh.update_known(z, ids, cs.R)
        pose, logw, lm = sh.download()
        assert np.array_equal(bits(pose), bits(t.records[0:3].astype(T))), f"group {g}: the update moved a pose"
        assert np.array_equal(bits(lm[1]), bits(t.records[8:13].astype(T))), f"group {g}: landmark 2 was not observed"
        m = t.group == g
        lm = lm.astype(np.float64)
        got["mean"][:, m], got["cov"][:, m] = lm[0, 0:2][:, m], lm[0, 2:5][:, m]
        got["init_mean"][:, m], got["init_cov"][:, m] = lm[2, 0:2][:, m], lm[2, 2:5][:, m]
        got["inc"][m] = logw.astype(np.float64)[m] - float(T(-math.log(2 * t.n)))
        done |= m
    sh.close()
    out = L.compare_case(got, cs, enforce=False, compared=done)
    for name in L.CLASSES:                                    # (printed before anything is asserted)
        print(f"lm-record {dtype} {which} {name}: error/bound " + " ".join(f"{q} {out[(name, q)]:.2g}" for q in L.QUANTITIES)
              + f"  lost-pd {out[(name, 'pd')]}")
    L.compare_case(got, cs, compared=done)


# ---- b. repeats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_repeat_inside_a_call_equals_two_calls(pkg, dtype):
    """ids [1, 1] (the second observation reads what the first one stored, at its turn, not from the record ring) against two calls
    on a twin shard, for a short-range, a nearly singular and an outlier group; every particle, whatever its class."""
    t = L.table(dtype)
    R = L.noise("full", dtype)
    a, b = (injected(pkg, t, dtype, n_global=2 * t.n) for _ in range(2))
    for k, name in enumerate(("near", "correlated", "outlier")):
        g = next(i for i, o in enumerate(t.obs) if L.CLASSES[o[0]] == name)
        if k:
            inject(a, t, clear=True)
            inject(b, t, clear=True)
        z, _ = L.group_call(t, g)
        z2 = np.stack([z[:, 0], z[:, 0] * np.array([1.001, 0.99])], axis=1)
        a.update_known(z2, [1, 1], R)
        b.update_known(z2[:, 0:1], [1], R)
        b.update_known(z2[:, 1:2], [1], R)
        same_bits(a.download(), b.download(), f"{name} group")
    a.close()
    b.close()


# ---- c. the other forms of the step, on the same records ------------------------------------------------------------------------------
def _steps(t, force):
    """Four steps with the suite's motion: observations made for a short-range, a far, a nearly singular and an outlier group; first
    sightings of landmark 3, then updates of what was first sighted; a repeat; landmark 2."""
    plan = (("near", [1, 3]), ("far", [3, 1]), ("correlated", [1, 1, 2]), ("outlier", [2, 1, 3]))
    steps = []
    for k, (name, ids) in enumerate(plan):
        g = next(i for i, o in enumerate(t.obs) if L.CLASSES[o[0]] == name)
        z13, _ = L.group_call(t, g)
        col = {1: z13[:, 0], 3: z13[:, 1], 2: np.array([30.0, -1.0])}
        steps.append((6.0, 0.02 * k - 0.03, np.stack([col[i] for i in ids], axis=1), np.array(ids, dtype=np.int32), force))
    return steps


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_equals_the_separate_calls_on_the_designed_records(pkg, dtype):
    t = L.table(dtype)
    R = L.noise("full", dtype)
    a, b = (injected(pkg, t, dtype) for _ in range(2))
    for k, (V, G, z, ids, _) in enumerate(_steps(t, False)):
        sa = a.step_fused(V, G, WHEELBASE, Q, DT, z, ids, R)
        b.predict(V, G, WHEELBASE, Q, DT)
        b.update_known(z, ids, R)
        sb = b.weight_stats()
        same_bits(a.download(), b.download(), f"step {k}")
        assert sa[0] == sb[0] and abs(sa[1] - sb[1]) <= 1e-12 * sb[1] and abs(sa[2] - sb[2]) <= 1e-12 * sb[2], f"step {k}"
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_mode_equals_the_normalised_fused_step_on_the_designed_records(pkg, dtype):
    """step_auto(force = 0) + flush against step_fused_normalized (FastSLAM.step_async / FastSLAM.step without resampling): poses and
    maps bit for bit, log-weights as tests/test_gpu_pf.py::_compare has them (the two shifts may differ in the last bit), Neff."""
    t = L.table(dtype)
    R = L.noise("full", dtype)
    f = {name: pkg.FastSLAM(injected(pkg, t, dtype), None) for name in ("auto", "sync")}
    for k, (V, G, z, ids, force) in enumerate(_steps(t, False)):
        f["auto"].step_async(V, G, WHEELBASE, Q, DT, z, ids, R, force_resample=force)
        want = f["sync"].step(V, G, WHEELBASE, Q, DT, z, ids, R, force_resample=force)
        neff, did = f["auto"].flush()
        assert did == want[1] and not did and neff == pytest.approx(want[0], rel=1e-12 if dtype == "f64" else 1e-6), f"step {k}"
        _compare(f["auto"].shard, f["sync"].shard, f"step {k}", exact_logw=False)
    for g in f.values():
        g.shard.close()


def test_persistent_batch_equals_the_steps_one_by_one_on_the_designed_records(pkg):
    """fp32: the four steps (none may resample) as one persistent launch against slam_pf_step_auto four times; the two filters run one
    after the other, as tests/test_gpu_pf_batch.py::drive has it (which also supplies the suite's R, Q and motion)."""
    t = L.table("f32")
    f = {name: pkg.FastSLAM(injected(pkg, t, "f32"), None, neff_frac=0.75) for name in ("batch", "single")}
    drive(pkg, f, _steps(t, False), 4, (3,), "designed records")
    for g in f.values():
        g.shard.close()


# ---- d. statistics and normalisation on spread weights ---------------------------------------------------------------------------------
def _stats_ld(logw):
    lw = logw.astype(np.longdouble)
    m = lw.max()
    e = np.exp(lw - m)
    return float(m), float(e.sum()), float((e * e).sum())


def _outlier_call(t):
    g = next(i for i, o in enumerate(t.obs) if L.CLASSES[o[0]] == "outlier")
    return L.group_call(t, g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_and_normalisation_on_spread_weights(pkg, dtype):
    t = L.table(dtype)
    R = L.noise("diag", dtype)
    T = L.NP_DTYPE[dtype]
    z, ids = _outlier_call(t)
    # weight_stats after the legacy update
    a = injected(pkg, t, dtype)
    a.update_known(z, ids, R)
    lw = a.download(landmarks=False)[1]
    assert np.all(np.isfinite(lw)) and lw.max() - np.median(lw) > 1e3, "the weights spread over thousands"
    want = _stats_ld(lw)
    gm, s1, s2 = a.weight_stats()
    print(f"lm-record {dtype} spread weights: max {want[0]:.6g} min {float(lw.min()):.6g} sum {want[1]:.6g} Neff {want[1] ** 2 / want[2]:.6g}")
    assert gm == want[0] and abs(s1 - want[1]) <= 1e-12 * want[1] and abs(s2 - want[2]) <= 1e-12 * want[2]
    # normalize: every stored log-weight within one ulp (of the largest magnitude involved, in the storage dtype: half an ulp for the
    # shift rounded to the dtype, half for the subtraction) of logw - (gmax + log gsum) in longdouble; the weights sum to one
    a.normalize(gm, s1)
    got = a.download(landmarks=False)[1]
    shift = np.longdouble(gm) + np.log(np.longdouble(s1))
    exact = lw.astype(np.longdouble) - shift
    ulp = np.spacing(np.maximum(np.maximum(np.abs(lw), np.abs(got)), T(abs(float(shift)))).astype(T)).astype(np.float64)
    err = np.abs((got.astype(np.longdouble) - exact).astype(np.float64))
    assert np.all(err <= ulp), float((err / ulp).max())
    w = np.exp(got.astype(np.longdouble))
    assert abs(float(w.sum()) - 1.0) <= 1.01 * float((w * ulp).sum()) + 1e-12
    assert abs(float(w.sum()) - 1.0) <= t.n * float(ulp[np.argmax(got)])
    a.close()
    # the statistics of the fused step, and the Neff and the normalisation of the normalised fused step (same sweep, bit for bit)
    b, c = (injected(pkg, t, dtype) for _ in range(2))
    sb = b.step_fused(6.0, 0.01, WHEELBASE, Q, DT, z, ids, R)
    lwb = b.download(landmarks=False)[1]
    want = _stats_ld(lwb)
    assert sb[0] == want[0] and abs(sb[1] - want[1]) <= 1e-12 * want[1] and abs(sb[2] - want[2]) <= 1e-12 * want[2]
    neff, gmax_norm = c.step_fused_normalized(6.0, 0.01, WHEELBASE, Q, DT, z, ids, R)
    assert abs(neff - want[1] ** 2 / want[2]) <= 1e-12 * neff
    got = c.download(landmarks=False)[1]
    shift = np.longdouble(want[0]) + np.log(np.longdouble(want[1]))
    ulp = np.spacing(np.maximum(np.maximum(np.abs(lwb), np.abs(got)), T(abs(float(shift)))).astype(T)).astype(np.float64)
    err = np.abs((got.astype(np.longdouble) - (lwb.astype(np.longdouble) - shift)).astype(np.float64))
    assert np.all(err <= ulp), float((err / ulp).max())
    assert gmax_norm == float(got.max())
    b.close()
    c.close()
