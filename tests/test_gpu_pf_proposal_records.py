"""GPU tests of the motion model and the FastSLAM-2.0 proposal (csrc/pf_device.h: normals2, motion_pose and its written-out copies,
proposal_core) on the designed records of tests/proposal_records.py: ONE call from injected per-particle state, every particle against
a longdouble evaluation of the oracle's formula from bit-identical inputs, within margin x the particle's OWN first-order rounding
scale (margins from the CPU model, never from the device; tests/test_proposal_records_cpu.py shows what the bounds reject).

INJECTION as in tests/test_gpu_pf_records.py (resample_apply with remote ancestors), after init_landmarks has marked landmarks
1 .. 64 as seen.  Group g of the table is the shard's g-th stepping call: the Philox step word is the call's index.

a. the bound: per group one step_proposal call (predict for the motion class) on the freshly injected table; the group's particles
   are kept; P.compare on all of them, for the diagonal and the non-symmetric R.
b. motion: predict, step_fused without observation and step_proposal without observation land on the same bits, inside the bound.
c. the other forms on the same records: step_auto(proposal) + flush and step_async_batch(proposal) against step_proposal + normalize,
   on every group of the near, many, mixed and outlier classes.
d. beyond: wherever the model's pose is finite the device's must be, under both noise matrices; the counts are printed.

MEASURED on the MI355X (worst error / bound per class; printed by test a as "proposal-record ..."): see the table in DESIGN.md,
"FastSLAM numerics: predict and the 2.0 proposal against per-particle bounds".
"""
import math

import numpy as np
import pytest

import lm_records as L
import proposal_records as P
from test_gpu_pf import _compare
from test_gpu_pf_records import bits, inject, same_bits

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]


def shard(pkg, t, dtype):
    return pkg.PFShard(t.n, P.NL, P.SHARD_SEED, dtype=dtype, first=0, n_global=t.n)


def load(sh, t, clear=False, rec=None):
    """The designed table as the state of shard `sh`: landmarks 1 .. NSEEN seen (filter-wide, kept on the host), 65 and 66 not.
    `rec`: the table already on the device (many loads in a row), else tests/test_gpu_pf_records.py::inject uploads it."""
    if clear:
        sh.clear_landmarks()
    sh.init_landmarks(np.zeros((P.NSEEN, 2)), 0.01, 0.0)
    if rec is None:
        inject(sh, t)
    else:
        sh.resample_apply(rec[0], rec[0], rec[1])


def on_device(sh, t):
    import torch
    return (torch.arange(t.n, 2 * t.n, dtype=torch.int32, device=sh.device), torch.from_numpy(t.records.astype(sh.np_dtype)).to(sh.device))


def assert_is_table(state, t):
    pose, logw, lm = state
    T = pose.dtype.type
    assert np.array_equal(bits(pose), bits(t.records[0:3].astype(T))), "injected poses"
    assert np.array_equal(bits(lm), bits(t.records[3:].reshape(P.NL, 5, t.n).astype(T))), "injected landmark records"
    assert np.all(logw == T(-math.log(t.n)))


def call_args(call, R):
    return (call.V, call.G, P.WHEELBASE, call.Q, call.dt, call.z, call.ids, R)


def run_groups(pkg, cs):
    """Every group's call, in order, each on the freshly injected table; the group's particles are kept.  Returns got (as P.compare
    takes it, float64), the log-weights [N] in the dtype, which particles were run."""
    t, dtype = cs.t, cs.dtype
    T = L.NP_DTYPE[dtype]
    sh = shard(pkg, t, dtype)
    rec = on_device(sh, t)
    got = {"pose": np.full((3, t.n), np.nan), "inc": np.full(t.n, np.nan), "lm": np.full((P.NL, 5, t.n), np.nan)}
    logw = np.full(t.n, np.nan, dtype=T)
    done = np.zeros(t.n, dtype=bool)
    base = T(-math.log(t.n))
    for g, call in enumerate(t.calls):
        load(sh, t, clear=g > 0, rec=rec)
        if g == 0:
            assert_is_table(sh.download(), t)
        R = P.noise(cs.which, dtype, call.rs)
        if len(call.ids):
            sh.step_proposal(*call_args(call, R))
        else:                                                 # the motion class (test b: the other forms give the same bits)
            sh.predict(call.V, call.G, P.WHEELBASE, call.Q, call.dt)
        m = t.group == g
        pose, lw, lm = sh.download()
        got["pose"][:, m], got["lm"][:, :, m], logw[m] = pose[:, m], lm[:, :, m], lw[m]
        got["inc"][m] = lw.astype(np.float64)[m] - float(base)
        done |= m
    sh.close()
    return got, logw, done


def report(out, cs, tag):
    for name in P.classes_of(cs.which):                       # (printed before anything is asserted)
        print(f"proposal-record {tag} {cs.dtype} {cs.which} {name}: error/bound "
              + " ".join(f"{q} {out[(name, q)]:.2g}" for q in P.QUANTITIES + P.LM_QUANTITIES) + f"  lost-pd {out[(name, 'pd')]} non-finite {out[(name, 'nonfinite')]}")


# ---- a. the bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(L.NOISES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_and_proposal_within_per_particle_bounds(pkg, dtype, which):
    cs = P.case(dtype, which)
    t = cs.t
    T = L.NP_DTYPE[dtype]
    got, logw, done = run_groups(pkg, cs)
    # (every group ran, fullQR under the diagonal R too: the call index is the Philox step; its particles are not compared there)
    out = P.compare(got, cs, enforce=False, compared=done)
    report(out, cs, "proposal")
    print(f"proposal-record proposal {dtype} {which} beyond: non-finite poses where the model's is finite {out[('beyond', 'nonfinite')]}")
    motion = t.cls == P.CLASSES.index("motion")
    assert np.array_equal(bits(logw[motion]), bits(np.full(int(motion.sum()), T(-math.log(t.n)), dtype=T))), "no observation: the log-weight stays bit for bit"
    P.compare(got, cs, compared=done)


# ---- b. motion -----------------------------------------------------------------------------------------------------------------------
def run_motion(pkg, cs, form):
    """The motion groups (the table's first calls) through `form`; (pose, logw, lm) of the motion particles."""
    t = cs.t
    sh = shard(pkg, t, cs.dtype)
    rec = on_device(sh, t)
    motion = t.cls == P.CLASSES.index("motion")
    T = L.NP_DTYPE[cs.dtype]
    pose, logw, lmk = np.zeros((3, t.n), dtype=T), np.zeros(t.n, dtype=T), np.zeros((P.NL, 5, t.n), dtype=T)
    none = (np.zeros((2, 0)), np.zeros(0, dtype=np.int32))
    for g, call in enumerate(t.calls):
        if P.CLASSES[call.cls] != "motion":
            break
        load(sh, t, clear=g > 0, rec=rec)
        R = P.noise(cs.which, cs.dtype)
        if form == "predict":
            sh.predict(call.V, call.G, P.WHEELBASE, call.Q, call.dt)
        elif form == "fused":
            sh.step_fused(call.V, call.G, P.WHEELBASE, call.Q, call.dt, *none, R)
        else:
            sh.step_proposal(call.V, call.G, P.WHEELBASE, call.Q, call.dt, *none, R)
        m = t.group == g
        p, w, l = sh.download()
        pose[:, m], logw[m], lmk[:, :, m] = p[:, m], w[m], l[:, :, m]
    sh.close()
    return pose[:, motion], logw[motion], lmk[:, :, motion]


@pytest.mark.parametrize("dtype", DTYPES)
def test_motion_is_the_same_bits_in_every_form_and_within_the_pose_bound(pkg, dtype):
    cs = P.case(dtype, "diag")
    t = cs.t
    motion = t.cls == P.CLASSES.index("motion")
    assert all(P.CLASSES[c.cls] == "motion" for c in t.calls[:P.SPEC["motion"]["groups"]])
    forms = {form: run_motion(pkg, cs, form) for form in ("predict", "fused", "proposal")}
    same_bits(forms["predict"], forms["fused"], "predict / step_fused without observation")
    same_bits(forms["predict"], forms["proposal"], "predict / step_proposal without observation")
    pose = forms["predict"][0].astype(np.float64)
    ratio = P.ratios({"pose": _spread(pose, motion, t.n), "inc": np.zeros(t.n)}, cs)["pose"][motion] / P.MARGINS[dtype]["motion"]["pose"]
    print(f"proposal-record motion {dtype}: pose error/bound {ratio.max():.2g}")
    assert np.all(np.isfinite(pose)) and ratio.max() <= 1.0, float(ratio.max())
    assert np.array_equal(bits(forms["predict"][2]), bits(t.records[3:].reshape(P.NL, 5, t.n)[:, :, motion].astype(forms["predict"][2].dtype)))


def _spread(pose, sel, n):
    full = np.full((3, n), np.nan)
    full[:, sel] = pose
    return full


# ---- c. the other forms on the same records ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["near", "many", "mixed", "outlier"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_and_batch_forms_equal_the_legacy_proposal_step_on_the_designed_records(pkg, dtype, name):
    """step_auto(proposal) + flush, and step_async_batch(proposal) (which goes step by step), against step_proposal + normalize on
    every group of the class: poses and maps bit for bit, log-weights as tests/test_gpu_pf.py::_compare has them (the two shifts may
    differ in the last bit).  Every particle of the table takes part, whatever its class."""
    t = P.table(dtype)
    groups = [i for i, c in enumerate(t.calls) if P.CLASSES[c.cls] == name]
    assert len(groups) == P.SPEC[name]["groups"]
    f = {form: shard(pkg, t, dtype) for form in ("sync", "auto", "batch")}
    rec = on_device(f["sync"], t)
    for k, g in enumerate(groups):
        call = t.calls[g]
        R = P.noise("full", dtype, call.rs)
        for sh in f.values():
            load(sh, t, clear=k > 0, rec=rec)
        d = {form: pkg.FastSLAM(sh, None) for form, sh in f.items()}
        want = d["sync"].step(*call_args(call, R), force_resample=False, proposal=True)
        d["auto"].step_async(*call_args(call, R), force_resample=False, proposal=True)
        batch = pkg.PFShard.prepare_batch([(call.V, call.G)], [(call.z, call.ids)], [False])
        d["batch"].step_async_batch(batch, P.WHEELBASE, call.Q, call.dt, R, proposal=True)
        for form in ("auto", "batch"):
            neff, did = d[form].flush()
            assert not did and neff == pytest.approx(want[0], rel=1e-12 if dtype == "f64" else 1e-6), (form, g)
            _compare(f[form], f["sync"], f"{name} group {g} {form}", exact_logw=False)
        same_bits(f["auto"].download(), f["batch"].download(), f"{name} group {g}: auto / batch")
    for sh in f.values():
        sh.close()


# ---- d. beyond the fp32 model's limit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(L.NOISES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_beyond_the_limit_the_device_is_finite_wherever_the_model_is(pkg, dtype, which):
    """The finiteness rule in the class past the fp32 model's own limit (Sig 6e-9 of the prior, below 2^-24): wherever the model of
    the dtype yields a finite pose, the device must.  Before proposal_core kept Sig positive semi-definite the fp32 device lost 7
    of 1001 particles here with the diagonal R, 6 of them where the correctly rounded model (which loses 20) is finite, and 14 such
    particles with the non-symmetric R; see DESIGN.md 5.2b.  (Test a asserts the same count through P.compare.)"""
    cs = P.case(dtype, which)
    t = cs.t
    sel = t.cls == P.CLASSES.index("beyond")
    sh = shard(pkg, t, dtype)
    rec = on_device(sh, t)
    finite = np.zeros(t.n, dtype=bool)
    first = next(g for g, c in enumerate(t.calls) if P.CLASSES[c.cls] == "beyond")
    for _ in range(first):                                    # group g is the g-th stepping call: the model drew its normals for that
        sh.predict(0.0, 0.0, P.WHEELBASE, P.Q_SUITE, 0.1)
    for g in range(first, len(t.calls)):
        call = t.calls[g]
        load(sh, t, clear=True, rec=rec)
        sh.step_proposal(*call_args(call, P.noise(which, dtype, call.rs)))
        m = t.group == g
        finite[m] = np.isfinite(sh.download(landmarks=False)[0]).all(axis=0)[m]
    sh.close()
    print(f"proposal-record beyond {dtype} {which}: non-finite poses: device {int((~finite[sel]).sum())}, model of the dtype {int((~cs.model_finite[sel]).sum())},"
          f" device only {int((cs.model_finite & ~finite)[sel].sum())} of {int(sel.sum())}")
    assert not (cs.model_finite & ~finite)[sel].any()
