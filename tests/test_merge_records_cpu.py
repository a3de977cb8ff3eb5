"""CPU half of tests/test_gpu_ekf_merge_records.py: the designed states, the extended-precision restatement against
tests/merge_ref.py, the committed margins against the rule they come from, and the planted defects -- which ones the per-entry
bounds reject and which ones the acceptance of tests/test_gpu_ekf_merge.py lets through on the same records (run with -s to
read the tables)."""
import numpy as np
import pytest

from tests import merge_records as M
from tests import merge_ref as MR
from tests import update_records as U

DEFECT_CELL = dict(N=127, cnt=3, dtype="f32", noisy=True)      # n = 257: two fp32 tile rows, a second block of merge_panel_kernel
GAIN_CLASSES = ("independent", "slam", "rank6")                # where the present tolerance must be SHOWN to accept a wrong gain


@pytest.fixture(scope="module")
def needs():
    return M.model_needs()


def test_restatement_agrees_with_the_float64_reference():
    """`restate` (hand-written longdouble Cholesky and solves) against merge_ref.merge on every cell, to 1e-10 of mag."""
    for c in M.CELLS:
        x, P, pairs, Rc = M.make_inputs(*c)
        ref = M.restate_cell(c)
        xr, Pr, _ni = MR.merge(x, P, pairs, Rc)
        (xe, xm, _), (Pe, Pm, _) = ref["x"], ref["P"]
        assert xe.shape == xr.shape and Pe.shape == Pr.shape, M.cell_id(c)
        assert np.all(np.abs(np.asarray(xe, dtype=np.float64) - xr) <= 1e-10 * xm), M.cell_id(c)
        assert np.all(np.abs(np.asarray(Pe, dtype=np.float64) - Pr) <= 1e-10 * Pm), M.cell_id(c)
        assert np.all(Pm >= np.abs(Pe) * (1 - 1e-12)) and np.all(xm >= np.abs(xe) * (1 - 1e-12))


def test_designed_states_have_their_properties():
    """Every cell: values of the dtype, positive definite (asserted while it is built), disjoint pairs whose D is positive
    definite and whose d2 is the planted one; the pair lists hold what they are meant to; `echo`'s P H' is exactly zero off
    b's rows and its P_bb = P_aa + D0 exactly."""
    seen = set()
    for c in M.CELLS:
        x, P, pairs, Rc = M.make_inputs(*c)
        t = U.NP_DTYPE[c.dtype]
        what = M.cell_id(c)
        assert np.array_equal(x.astype(t).astype(np.float64), x) and np.array_equal(P.astype(t).astype(np.float64), P), what
        assert not x.flags.writeable and not P.flags.writeable
        flat = [j for p in pairs for j in p]
        assert len(pairs) == c.cnt and len(set(flat)) == 2 * c.cnt and min(flat) >= 1 and max(flat) <= c.N, what
        for i, (a, b) in enumerate(pairs):
            delta, D = MR.difference(x, P, a, b)
            d2 = MR.d2_of(delta, D)
            tt = M.T_SET[i % 3]                                  # (x_b was rounded to the dtype: 2e-6 m beside `mixed`'s 1e-3 m)
            assert (tt / 2 <= d2 <= 2 * tt) if c.dtype == "f32" else abs(d2 - tt) <= 1e-6 * tt, (what, a, b, d2)
        assert (Rc is None) == (not c.noisy)
        if c.N >= 66:
            assert pairs[0] == (1, c.N)
            S = M.straddlers(c.dtype, c.N)
            if c.cnt >= 3:
                assert pairs[1][0] in S and any(b < a for a, b in pairs), what
                seen.add((c.dtype, "b straddles") if (pairs[2][1] in S or c.N in S) else (c.dtype, "b opens a tile"))
            if c.cnt == 8 and c.cls != "mixed":
                assert any(b == a + 1 for a, b in pairs), what
            if c.cnt == 8 and c.cls == "mixed":
                sc = [((a - 1) % 5, (b - 1) % 5) for a, b in pairs]
                assert {s for s, u in sc if s == u} == set(range(5)) and any(s != u for s, u in sc), what
        if c.cls == "echo":
            _v, A, _S = M.front(x, P, pairs, Rc, np.float64)
            rows_b = np.concatenate([[MR.f(b), MR.f(b) + 1] for _a, b in pairs])
            off = np.setdiff1d(np.arange(len(x)), rows_b)
            assert not A[off].any(), f"{what}: P H' must be exactly zero off b's rows"
            src = np.arange(len(x))                              # where every row was copied from
            for a, b in pairs:
                src[MR.f(b):MR.f(b) + 2] = [MR.f(a), MR.f(a) + 1]
            for a, b in pairs:
                fa, fb = MR.f(a), MR.f(b)
                others = np.setdiff1d(np.arange(len(x)), [fb, fb + 1])
                assert np.array_equal(P[fb:fb + 2][:, others], P[fa:fa + 2][:, src[others]]), f"{what}: b's rows are not copies of a's"
                D0 = P[fb:fb + 2, fb:fb + 2] - P[fa:fa + 2, fa:fa + 2]
                exact = np.asarray(P[fb:fb + 2, fb:fb + 2], dtype=U.LD) - np.asarray(P[fa:fa + 2, fa:fa + 2], dtype=U.LD)
                assert np.array_equal(np.asarray(D0, dtype=U.LD), exact) and np.linalg.cond(D0) < 4, what
                s = D0[0, 0]
                assert np.array_equal(D0, s * np.array([[1.0, 0.25], [0.25, 0.75]])), f"{what}: P_aa + D0 was rounded"
                assert 0.5 <= s / ((P[fa, fa] + P[fa + 1, fa + 1]) / 2) <= 1.0 + 1e-3, what
                assert np.array_equal(MR.difference(x, P, a, b)[1], D0), what
        if c.cls == "independent":
            _v, A, _S = M.front(x, P, pairs, Rc, np.float64)
            assert not A[M.untouched_rows(c.N, pairs)].any() and not A[0:3].any(), what
    assert {("f32", "b straddles"), ("f64", "b straddles"), ("f32", "b opens a tile")} <= seen
    assert {(c.N, c.cnt) for c in M.CELLS} == set(M.SHAPES) and len(M.CELLS) == 60
    for cls in M.CLASSES:
        mine = [c for c in M.CELLS if c.cls == cls]
        assert {(c.dtype, c.noisy) for c in mine} == set(M.COMBOS), cls
        assert {c.dtype for c in mine if c.cnt == 8} == {"f32", "f64"}, cls
    assert {M.echo_base(c.N, c.cnt) for c in M.CELLS} == {"independent", "slam"}


def test_committed_margins_follow_the_rule(needs):
    """MARGINS = max(4, 4 x the model's need) per class; the committed table may round up by a quarter at most.  Also:
    c 2^-53 kappa stays below KAPPA_SLACK on every cell, so no bound goes slack."""
    need, rows = needs
    rule = M.margins_from(need)
    print("\nMARGINS by the rule (c_x, c_P, c_32):")
    for c in M.CLASSES:
        print(f"  {c:12s} " + ", ".join(f"{v:.4g}" for v in rule[c]) + "      model needs " +
              ", ".join(f"{q}={v:.3g}" for q, v in sorted(need[c].items())) +
              f"      largest kappa {max(k for cell, k, _ in rows if cell.cls == c):.3g}")
    for c in M.CLASSES:
        for got, want in zip(M.MARGINS[c], rule[c]):
            assert want <= got <= 1.25 * want, (c, M.MARGINS[c], rule[c])
    for cell, kap, _r in rows:
        cx, cP, _ = U.bound_constants(cell.cls, cell.dtype, "cholesky", cell.cnt, M._as_form(None))
        assert max(cx, cP) * U.EPS53 * kap < U.KAPPA_SLACK * U.C_FACTOR, (cell, kap)


def test_the_models_stay_within_a_quarter_of_their_bounds(needs):
    """By construction of the margins where the derived limit does not cap them (then: within the bound) -- every class and
    cell, every entry, nothing excluded; the rows that must come back bit for bit do."""
    _need, rows = needs
    for cell, _kap, _r in rows:
        x, P, pairs, Rc = M.make_inputs(*cell)
        ref = M.restate_cell(cell)
        xm, Pm, side = M.model_merge(x, P, pairs, Rc, cell.dtype)
        w = M.judge(xm, Pm, ref, cell.cls, cell.dtype, cell.cnt, what=M.cell_id(cell))
        capped = cell.dtype == "f32" and M.MARGINS[cell.cls][2] > U.derived_limit_p32("cholesky", cell.cnt)
        assert w["x"] <= 0.25 + 1e-9 and (w["P"] <= 0.25 + 1e-9 or capped), (M.cell_id(cell), w)
        assert U.structure_ok(Pm, side)
        keep = M.keep_index(len(x), pairs)
        if cell.cls == "independent":
            un = np.flatnonzero(np.isin(keep, np.concatenate([[0, 1, 2], M.untouched_rows(cell.N, pairs)])))
            assert np.array_equal(xm[un], x[keep][un]) and np.array_equal(Pm[un], P[np.ix_(keep, keep)][un])
        if cell.cls == "echo":
            assert np.array_equal(xm, x[keep]) and np.array_equal(Pm, P[np.ix_(keep, keep)])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_schedule_with_the_models_in_the_devices_place(dtype, needs):
    """Update 64, merge 1, update 17, merge 8, merge 3 on one state: the updates stay inside update_records' own bounds, the
    merges within a quarter of this file's (their need is part of `independent`'s margins), kappa stays small."""
    rows = M.model_schedule(dtype)
    assert [(kind, m) for kind, m, _r, _k in rows] == list(M.SCHEDULE)
    cx, cP, c32 = M.MARGINS[M.SCHEDULE_CLASS]
    for kind, m, r, kap in rows:
        print(f"\nschedule {dtype} {kind} {m}: kappa {kap:.3g} " + ", ".join(f"{q}={v:.3g}" for q, v in sorted(r.items())), end="")
        assert max(cx, cP) * U.EPS53 * kap < U.KAPPA_SLACK
        if kind == "update":
            assert r["x"] <= 1.0 and r["P"] <= 1.0, (kind, m, r)
        else:
            assert r["x"] <= cx / 4 and r.get("P", 0.0) <= cP / 4 and r.get("P32", 0.0) <= c32 / 4, (kind, m, r)


def _previous(cls, x, N, m, seed):
    rng = np.random.default_rng(seed)
    ids = U.choose_ids(cls, rng, N, m)
    return U.observations(cls, rng, x, ids), ids


def _defect_results(cls, defect):
    c = M.Cell(cls, **DEFECT_CELL)
    x, P, pairs, Rc = M.make_inputs(*c)
    ref = M.restate_cell(c)
    previous = None
    if defect in ("stale_columns", "stale_image"):
        previous = _previous(cls, x, c.N, 8 if defect == "stale_columns" else 64, 5)
    xm, Pm, side = M.model_merge(x, P, pairs, Rc, c.dtype, defect=defect, previous=previous)
    return (M.accepted(xm, Pm, side, ref, cls, c.dtype, c.cnt),
            M.tol_accepts(xm, Pm, side, ref, P, M.keep_index(len(x), pairs), c.dtype))


def test_planted_defects_are_rejected_and_what_the_tolerances_accept():
    """Every planted defect leaves the per-entry bounds on the class designed for it (one cell: N = 127, three pairs, fp32, Rc
    set).  Printed: what the present acceptance (TOL, symmetry, check_side) lets through on the same records."""
    tol_list = []
    print("\ndefect                    class         per-entry bounds   acceptance of test_gpu_ekf_merge")
    for defect in (None,) + M.DEFECTS:
        for cls in (M.CLASSES if defect is None else tuple(dict.fromkeys((M.DEFECT_CLASS[defect], "rank6")))):
            ok_new, ok_tol = _defect_results(cls, defect)
            print(f"{str(defect):25s} {cls:12s}  {'accept' if ok_new else 'REJECT':16s}   {'ACCEPT' if ok_tol else 'reject'}")
            if defect is None:
                assert ok_new and ok_tol, cls
                continue
            if ok_tol:
                tol_list.append((defect, cls))
            if cls == M.DEFECT_CLASS[defect]:
                assert not ok_new, f"{defect} passes the per-entry bounds on {cls}"
    print("accepted by the present tolerance:", tol_list)


def test_a_gain_wrong_by_a_thousandth_on_every_fp32_cell():
    """The mean correction scaled by 1.001: rejected by the per-entry bounds on EVERY fp32 cell (but `echo`'s, where the
    correction moves only the landmarks that leave), accepted by TOL of tests/test_gpu_ekf_merge.py on cells of `independent`,
    `slam` and `rank6` -- and that test allows max(TOL, 4 x an update's error), which is wider still."""
    let_through = []
    print("\ngain_1e-3, fp32              relerr(x)   TOL['f32']['x'] = 5e-6   per-entry bounds")
    for c in M.CELLS:
        if c.dtype != "f32" or c.cls == "echo":
            continue
        x, P, pairs, Rc = M.make_inputs(*c)
        ref = M.restate_cell(c)
        xm, Pm, side = M.model_merge(x, P, pairs, Rc, c.dtype, defect="gain_1e-3")
        ok_new = M.accepted(xm, Pm, side, ref, c.cls, c.dtype, c.cnt)
        ok_tol = M.tol_accepts(xm, Pm, side, ref, P, M.keep_index(len(x), pairs), c.dtype)
        ex = M.relerr(xm, np.asarray(ref["x"][0], dtype=np.float64))
        print(f"{M.cell_id(c):28s} {ex:.2e}    {'ACCEPT' if ok_tol else 'reject'}                   {'accept' if ok_new else 'REJECT'}")
        assert not ok_new, M.cell_id(c)
        if ok_tol:
            let_through.append(c)
    print("accepted by the present tolerance:", [M.cell_id(c) for c in let_through])
    assert set(GAIN_CLASSES) <= {c.cls for c in let_through}


def test_the_transposed_cross_block_is_invisible_to_find():
    """D holds P_ab + P_ab' and does not change when the block is transposed; the merge's column differences do."""
    c = M.Cell("slam", **DEFECT_CELL)
    x, P, pairs, Rc = M.make_inputs(*c)
    _v, A, S = M.front(x, P, pairs, Rc, np.float64)
    _v, At, St = M.front(x, P, pairs, Rc, np.float64, transposed=True)
    for p in range(len(pairs)):
        assert np.array_equal(S[2 * p:2 * p + 2, 2 * p:2 * p + 2], St[2 * p:2 * p + 2, 2 * p:2 * p + 2])
    assert not np.array_equal(A, At)
