"""CPU tests of tests/lm_records.py: the designed landmark records are as hard as they claim, the reference is the oracle, the
margins follow their rule, the exclusion stays under its cap, compare_records rejects every planted defect -- and the bounds of
tests/test_gpu_pf.py, applied to the same records, accept several of them (OLD_BOUNDS_ACCEPT below: the gap this closes).
No GPU."""
import math

import numpy as np
import pytest

import lm_records as L
from oracle import pf_ref as F

DTYPES = ("f64", "f32")


def test_the_suites_numbers():
    import test_gpu_pf as G
    assert np.array_equal(L.R_DIAG, G.R) and L.OLD_TOL == G.TOL
    assert L.R_FULL[0, 1] != L.R_FULL[1, 0]
    s = 0.5 * (L.R_FULL[0, 1] + L.R_FULL[1, 0])
    assert L.R_FULL[0, 0] * L.R_FULL[1, 1] > s * s
    assert L.N % 64 != 0 and all(np.count_nonzero(L.table("f32").cls == ci) >= 1000 for ci in range(len(L.CLASSES)))


@pytest.mark.parametrize("which", list(L.NOISES))
def test_reference_is_the_oracle_on_every_class(which):
    """The float64 instance of the reference against OraclePF.update_known itself, group by group (one observation per call),
    to 1e-12 relative (of the entry, or of the record's own scale where an entry cancels to nothing)."""
    t = L.table("f64")
    R = L.noise(which, "f64")
    ref = L.as_f64(L.reference(np.float64, t, R))
    got = {q: np.full_like(v, np.nan) for q, v in ref.items()}
    for g in range(len(t.obs)):
        orc = F.OraclePF(t.n, L.NL, 1, first_id=0, n_global=2 * t.n)
        orc.pose = t.records[0:3].copy()
        orc.lm = t.records[3:].reshape(L.NL, 5, t.n).copy()
        orc.seen[:2] = True
        z, ids = L.group_call(t, g)
        orc.update_known(z, ids, R)
        m = t.group == g
        got["mean"][:, m], got["cov"][:, m] = orc.lm[0, 0:2][:, m], orc.lm[0, 2:5][:, m]
        got["init_mean"][:, m], got["init_cov"][:, m] = orc.lm[2, 0:2][:, m], orc.lm[2, 2:5][:, m]
        got["inc"][m] = (orc.logw + math.log(2 * t.n))[m]
        assert np.array_equal(orc.lm[1], t.records[8:13]) and np.array_equal(orc.pose, t.records[0:3])
    floor = {"mean": 1.0, "cov": np.maximum(t.pxx, t.pyy), "inc": 10.0, "init_mean": 1.0, "init_cov": L.R_DIAG[0, 0]}
    for q in L.QUANTITIES:
        assert np.all(np.isfinite(got[q]))
        err = np.abs(got[q] - ref[q]) / np.maximum(np.abs(ref[q]), floor[q])
        assert err.max() <= 1e-12, (q, float(err.max()))


def test_classes_are_as_hard_as_they_claim():
    for dtype in DTYPES:
        cs = L.case(dtype, "diag")
        t, tr = cs.t, cs.truth_ld
        d = np.asarray(tr.d, dtype=np.float64)
        nis = np.asarray(tr.nis, dtype=np.float64)
        raw = np.asarray(tr.raw_v1, dtype=np.float64)
        rho = t.pxy / np.sqrt(t.pxx * t.pyy)
        pvar = np.maximum(t.pxx, t.pyy)
        dx, dy = t.lx - t.x, t.ly - t.y
        assert np.all(np.abs(t.x) <= 5.001) and np.all(np.abs(t.y) <= 5.001)
        assert t.phi.min() < -3.0 and t.phi.max() > 3.0 and np.all(np.abs(t.phi) < math.pi)
        assert np.all(np.abs(t.b) <= math.pi * (1 + 1e-7)) and np.abs(t.b).max() > 3.1 and np.abs(t.b3).max() > 2.5
        for ci, name in enumerate(L.CLASSES):
            s = t.cls == ci
            lo, hi = L.SPEC[name]["rng"]
            vlo, vhi = L.SPEC[name]["var"]
            assert lo * 0.999 - 1.5 / L.GRID <= d[s].min() and d[s].max() <= hi * 1.001 + 1.5 / L.GRID, (name, d[s].min(), d[s].max())   # (the grid of the exact directions)
            if name != "outlier":                                     # the class's interval is used, not one corner of it
                assert d[s].min() < lo * 1.3 and d[s].max() > hi / 1.3, (name, d[s].min(), d[s].max())
            assert vlo * 0.999 <= pvar[s].min() and pvar[s].max() <= vhi * 1.001
            if vhi > vlo:
                assert pvar[s].min() < vlo * 3 and pvar[s].max() > vhi / 3
            if name == "correlated":
                one = 1.0 - np.abs(rho[s])
                assert 0 < one.min() < 3e-6 and one.max() <= 1.01e-2 and one.max() > 3e-3
                assert (rho[s] > 0).sum() > 300 and (rho[s] < 0).sum() > 300
            else:
                assert np.abs(rho[s]).max() <= 0.9001 and np.abs(rho[s]).max() > 0.8
            # the wrap: a stated share of bearing innovations beyond pi before it, on both sides
            assert np.mean(np.abs(raw[s]) > math.pi) >= L.WRAP_SHARE_MIN, (name, np.mean(np.abs(raw[s]) > math.pi))
            assert (raw[s] > math.pi).sum() > 30 and (raw[s] < -math.pi).sum() > 30
            # every branch and tie of the fp32 atan2: |dy| <> |dx|, both signs of dx and dy, the axes and the diagonals exactly
            ax, ay = np.abs(dx[s]), np.abs(dy[s])
            for cond in (ay > ax, ay < ax, dx[s] < 0, dx[s] > 0, dy[s] < 0, dy[s] > 0):
                assert cond.sum() > 100, name
            for sx in (1, -1):
                for sy in (1, -1):
                    assert ((np.sign(dx[s]) == sx) & (np.sign(dy[s]) == sy)).sum() > 100, name
                    assert ((dx[s] == sx * ax) & (dy[s] == sy * ay) & (ax == ay) & (ax > 0)).sum() >= 1, (name, "diagonal", sx, sy)
                assert ((dy[s] == 0) & (np.sign(dx[s]) == sx)).sum() >= 1 and ((dx[s] == 0) & (np.sign(dy[s]) == sx)).sum() >= 1, (name, "axis")
            if name == "outlier":
                sig = np.sqrt(nis[s])
                assert sig.max() > 0.9 * math.sqrt(2) * L.OUTLIER_SIGMAS and np.median(sig) > 20
                assert cs.truth["inc"][s].min() < -3.0e3 and cs.truth["inc"][s].max() > -50.0      # the log-weight span
            else:
                assert np.median(nis[s]) < 4.0 and np.percentile(nis[s], 90) < 25.0, (name, np.median(nis[s]))
        big = t.cls == L.CLASSES.index("bigP")
        assert (pvar[big] / L.R_DIAG[0, 0]).max() > 3e5 and np.asarray(tr.cond, dtype=np.float64)[big].max() > 1e5
        tiny = t.cls == L.CLASSES.index("tinyP")
        assert (pvar[tiny] / L.R_DIAG[0, 0]).max() < 1.1e-4
        assert d[t.cls == L.CLASSES.index("near")].min() < 0.06 and d[t.cls == L.CLASSES.index("far")].max() > 1500


@pytest.mark.parametrize("dtype", DTYPES)
def test_margins_table_follows_its_rule(dtype):
    rule = L.derive_margins(dtype)
    for name in L.CLASSES:
        for q in L.QUANTITIES:
            have, want = L.MARGINS[dtype][name][q], rule[name][q]
            assert have >= want, f"{dtype} {name} {q}: committed {have} below the rule's {want:.3f}"
            assert have <= 1.5 * want, f"{dtype} {name} {q}: committed {have} is slack against the rule's {want:.3f}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_exclusion_stays_under_its_cap_and_the_model_passes(dtype):
    for which in L.NOISES:
        cs = L.case(dtype, which)
        for ci, name in enumerate(L.CLASSES):
            s = cs.t.cls == ci
            assert cs.excluded[s].sum() <= L.EXCLUDE_CAP * s.sum(), (name, int(cs.excluded[s].sum()))
        if dtype == "f64":
            assert not cs.excluded.any()
        out = L.compare_case(cs.model, cs)                       # the correctly rounded model is inside its own bounds, with room
        assert max(out.values()) <= 0.25 + 1e-9
        assert L.compare_case(cs.truth, cs)[("benign", "cov")] == 0.0
        some = np.ones(cs.t.n, dtype=bool)
        some[5] = False
        with pytest.raises(AssertionError, match="never run"):
            L.compare_case(cs.model, cs, compared=some)
        bad = {q: v.copy() for q, v in cs.model.items()}
        bad["inc"][17] = np.nan
        with pytest.raises(AssertionError, match="not finite"):
            L.compare_case(bad, cs)
        neg = {q: v.copy() for q, v in cs.model.items()}
        k = int(np.nonzero(cs.t.cls == L.CLASSES.index("tinyP"))[0][3])
        neg["cov"][0, k] = -neg["cov"][0, k]
        with pytest.raises(AssertionError):
            L.compare_case(neg, cs)


# (defect, class) pairs that the bounds of tests/test_gpu_pf.py accept on these records in fp32 -- close() with TOL, 10 x on
# covariances and log-weights, the class's records taken as the filter -- while compare_records rejects the defect.  Re-derived and
# compared by the test below.
OLD_BOUNDS_ACCEPT = {
    "cov_1e-4": ["benign", "correlated", "far", "near", "outlier", "tinyP"],
    "h_over_d": ["tinyP"],
    "log2pi_1.84": ["benign", "correlated", "far", "near", "outlier", "tinyP"],
    "pxy_cross_sign": ["far", "tinyP"],
}


def test_every_planted_defect_is_rejected_and_the_old_bounds_accept_some():
    accepted = {}
    for defect in L.DEFECTS:
        rejected_on = set()
        for which in L.NOISES:
            cs = L.case("f32", which)
            got = L.planted(defect, "f32", which)
            if which == "full":                                   # (with the diagonal R the symmetrisation changes nothing)
                with pytest.raises(AssertionError):
                    L.compare_case(got, cs)
            out = L.compare_case(got, cs, enforce=False)
            for ci, name in enumerate(L.CLASSES):
                worst = max(out[(name, q)] for q in L.QUANTITIES)
                if worst > 1.0 or out[(name, "pd")] > 0:
                    rejected_on.add(name)
                if which == "full" or defect != "no_symmetrisation":
                    if L.old_bounds_accept(got, cs, cs.t.cls == ci):
                        accepted.setdefault(defect, set()).add(name)
        assert rejected_on, f"{defect}: no class rejects it"
        print(f"planted {defect}: rejected on {sorted(rejected_on)}; the old bounds accept it on {sorted(accepted.get(defect, ()))}")
    assert "tinyP" in accepted["cov_1e-4"] and "tinyP" in accepted["pxy_cross_sign"]
    assert {k: sorted(v) for k, v in accepted.items()} == {k: sorted(v) for k, v in OLD_BOUNDS_ACCEPT.items()}
    # the defect-free model is accepted by both, so neither verdict above is an artefact of the comparison
    for which in L.NOISES:
        cs = L.case("f32", which)
        for ci, name in enumerate(L.CLASSES):
            # (bigP: P - W1 W1' cancels six digits, the correctly rounded fp32 model is 3e-3 off on posteriors of at most 0.8 --
            #  the documented fp32 limit; the old bound takes its scale from the largest POSTERIOR entry and misses)
            assert L.old_bounds_accept(cs.model, cs, cs.t.cls == ci) == (name != "bigP"), name
