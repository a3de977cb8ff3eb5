"""GPU tests of the per-particle association with unknown correspondences (pf_update_unknown_kernel, pf_step_unknown_kernel) on the
designed table of tests/pf_assoc_records.py: per-particle maps injected bit for bit, ONE call, every decision inside the set its
pair's rounding bounds can reach, every decided pair equal to the longdouble truth -- no agreement quota -- and the state after the
call against a longdouble replay of the device's OWN decisions, record by record (tests/test_pf_assoc_records_cpu.py shows what
this rejects and what the quiet scenes of tests/test_gpu_pf_unknown_step.py let through).

INJECTION as in tests/test_gpu_pf_records.py: the table is the "remote records" of a resampling in which every ancestor lives on
another rank, after clear_landmarks; the first download must be the table bit for bit.  The fused step runs with V = G = dt = 0:
no motion, and the poses must come back bit for bit.

a. decisions: update_unknown at m = 5, 16; step_unknown_fused at m = 5, 16, 17, 33, 48, 49, 64 (one to four groups; fp64: the second
   sweep with an idle and with a busy second group), both dtypes, the diagonal R; the non-symmetric R_FULL at m = 64.
b. the state after those calls given the device's decisions: used slots exact, untouched records bit for bit, touched records and
   log-weight increments within the replay's bounds, records touched twice at the suite's TOL; the fused call's statistics are
   weight_stats() right after it, bit for bit.
c. fused == legacy bit for bit at m = 5 and 16 (decisions, state, statistics).
d. degenerate gates on the table, exact.

MEASURED on the MI355X (printed by a and b as "assoc-record ..."): no decision outside its set, no decided pair off the truth; fp32
decides about 1 % of its open pairs the other way than the truth (488 of 46 987 at m = 64), fp64 has none; state error / bound at
most 0.23 (fp32) and 0.36 (fp64).  The table is in DESIGN.md, "5.2c FastSLAM numerics: the association against per-pair bounds".
"""
import math

import numpy as np
import pytest

import pf_assoc_records as A
from test_gpu_pf import Q, TOL, close
from test_gpu_pf_records import bits, same_bits

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
CASES = [("legacy", 5, "diag"), ("legacy", 16, "diag")] + [("fused", m, "diag") for m in (5, 16, 17, 33, 48, 49, 64)] + [("fused", 64, "full")]
IDS = [f"{e}-{m}-{w}" for e, m, w in CASES]
_RUNS = {}


def inject(sh, t):
    import torch
    sh.clear_landmarks()
    ids = torch.arange(t.n, 2 * t.n, dtype=torch.int32, device=sh.device)
    sh.resample_apply(ids, ids, torch.from_numpy(t.records.astype(sh.np_dtype)).to(sh.device))


def assert_is_table(state, t):
    pose, logw, lm = state
    T = pose.dtype.type
    assert np.array_equal(bits(pose), bits(t.pose.astype(T))), "injected poses"
    assert np.array_equal(bits(lm), bits(t.lm.astype(T))), "injected maps"
    assert np.all(logw == T(-math.log(t.n)))


def call(sh, t, entry, m, gate1=None, gate2=None):
    """One call on the injected shard: (decisions [m, n], statistics of the call or of weight_stats() after the legacy call)."""
    g1, g2 = t.gate1 if gate1 is None else gate1, t.gate2 if gate2 is None else gate2
    if entry == "legacy":
        dec = sh.update_unknown(t.z[:, :m], t.R, g1, g2, want_assoc=True).cpu().numpy()
        return dec, sh.weight_stats()
    stats, dec = sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.0, t.z[:, :m], t.R, g1, g2, want_assoc=True)
    return dec.cpu().numpy(), stats


def run(pkg, entry, m, dtype, which):
    """The call of a case on a freshly injected shard, once per session: decisions, statistics, weight_stats() after it, the state."""
    key = (entry, m, dtype, which)
    if key not in _RUNS:
        t = A.table(dtype, which)
        sh = pkg.PFShard(t.n, A.NL, 5, dtype=dtype)
        inject(sh, t)
        assert_is_table(sh.download(), t)
        dec, stats = call(sh, t, entry, m)
        after = sh.weight_stats()
        _RUNS[key] = dict(dec=dec, stats=stats, after=after, state=sh.download())
        sh.close()
    return _RUNS[key]


# ---- a. decisions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,m,which", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_decision_is_admissible_and_every_decided_pair_is_the_truth(pkg, dtype, entry, m, which):
    c = A.case(dtype, which)
    out = run(pkg, entry, m, dtype, which)
    dec = out["dec"]
    assert dec.shape == (m, c.t.n)
    outside, wrong = A.check_decisions(c, dec, m)
    edge = ~c.decided[:m]
    as_truth = int(np.sum(dec[edge] == c.dec[:m][edge]))
    print(f"assoc-record {dtype} {entry} m={m} {which}: {int(c.decided[:m].sum())} decided pairs, {int(wrong.sum())} differ from the truth; "
          f"{int(edge.sum())} open pairs, {as_truth} decided as the truth does, {int(edge.sum()) - as_truth} the other way; "
          f"{int(outside.sum())} decisions outside their admissible set")
    for name, s in (("exact", A.EXACT), ("twin", A.TWIN)):
        sel = c.sit[:m] == s
        print(f"assoc-record {dtype} {entry} m={m} {which}: {name} pairs {int(sel.sum())}, as the truth {int(np.sum(dec[sel] == c.dec[:m][sel]))}")
    assert not outside.any(), f"first: observation, particle {np.argwhere(outside)[0]}: {dec[tuple(np.argwhere(outside)[0])]}"
    assert not wrong.any()


# ---- b. the state, given the device's own decisions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,m,which", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_state_after_the_call_given_the_devices_decisions(pkg, dtype, entry, m, which):
    t = A.table(dtype, which)
    T = A.NP_DTYPE[dtype]
    out = run(pkg, entry, m, dtype, which)
    pose, logw, lm = out["state"]
    assert np.array_equal(bits(pose), bits(t.pose.astype(T))), "the poses moved (dt = 0)"
    rp = A.replay(t, out["dec"], m)
    inc = logw.astype(np.float64) - float(T(-math.log(t.n)))
    st = A.check_state(t, rp, lm.astype(np.float64), inc)
    print(f"assoc-record {dtype} {entry} m={m} {which}: state error/bound records {st['worst_lm']:.2g} increments {st['worst_inc']:.2g}; "
          f"{int((rp.touch == 1).sum())} records touched once, {int(st['twice'].sum())} twice, {int(rp.dropped.sum())} new landmarks found no slot")
    assert st["used_wrong"] == 0 and st["untouched_changed"] == 0 and st["out_of_bound"] == 0, {k: v for k, v in st.items() if not isinstance(v, np.ndarray)}
    want = np.asarray(rp.lm, dtype=np.float64)
    tw = st["twice"]
    if tw.any():                                                   # the second touch has a rounded prior: the suite's tolerance
        assert close(lm[:, 0:2, :].transpose(0, 2, 1)[tw], want[:, 0:2, :].transpose(0, 2, 1)[tw], TOL[dtype])
        assert close(lm[:, 2:5, :].transpose(0, 2, 1)[tw], want[:, 2:5, :].transpose(0, 2, 1)[tw], TOL[dtype])
        p2 = st["twice_p"]
        assert close(inc[p2], np.asarray(rp.inc, dtype=np.float64)[p2], TOL[dtype], scale=max(1.0, float(np.max(np.abs(logw)))))
    if m >= 16:
        assert int(rp.dropped.sum()) > 0 and int(st["twice"].sum()) > 0
    assert out["stats"] == out["after"], "the call's statistics against weight_stats() right after it"


# ---- c. fused against legacy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_equals_legacy_on_the_table(pkg, dtype, m):
    a, b = run(pkg, "legacy", m, dtype, "diag"), run(pkg, "fused", m, dtype, "diag")
    assert np.array_equal(a["dec"], b["dec"]), "decisions"
    same_bits(a["state"], b["state"], f"m = {m}")
    assert a["stats"] == b["stats"]


# ---- d. degenerate gates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,m", [("legacy", 16), ("fused", 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_gates_on_the_table(pkg, dtype, entry, m):
    t = A.table(dtype, "diag")
    holds = (t.lm[:, 2, :] >= 0).any(axis=0)
    assert holds.sum() > 2900 and (~holds).sum() >= 10
    sh = pkg.PFShard(t.n, A.NL, 5, dtype=dtype)
    inf = float("inf")
    for g1, g2, with_map in ((0.0, 0.0, -1), (0.0, inf, -2), (inf, t.gate2, None)):
        inject(sh, t)
        dec, _ = call(sh, t, entry, m, g1, g2)
        assert np.all(dec[:, ~holds] == -1), (g1, g2, "particles without a landmark")
        if with_map is None:
            assert np.all(dec[:, holds] >= 0) and np.all(dec[:, holds] < A.NL), (g1, g2)
            p = np.broadcast_to(np.arange(t.n)[None, :], dec.shape)
            assert np.all(t.lm[np.maximum(dec, 0), 2, p][:, holds] >= 0), "matched to an unused slot"
        else:
            assert np.all(dec[:, holds] == with_map), (g1, g2)
    sh.close()
