"""CPU half of tests/test_gpu_ekf_update_records.py: the designed states, the extended-precision restatement, the committed
margins against the rule they come from, and the planted defects -- which ones the per-entry bounds reject and which ones the
tolerances of tests/test_gpu_ekf_dispatch.py accept on the same records (run with -s to read the tables)."""
import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import update_records as U

DEFECT_CELL = dict(N=127, m=64, dtype="f32", form="cholesky")      # n = 257: two fp32 tile rows, k = 128: the claiming grid


@pytest.fixture(scope="module")
def needs():
    return U.model_needs()


def test_restatement_agrees_with_the_float64_oracle():
    """The hand-written longdouble Cholesky / solves against oracle/ekf_ref.py on a benign cell, both forms."""
    x, P, z, ids = U.make_inputs("rank6", 66, 17, "f64")
    for form, fn in (("cholesky", O.update_sparse), ("joseph", O.update_joseph_sparse)):
        ref = U.restate(x, P, z, ids, form)
        xo, Po = fn(x, P, z, U.R, ids)
        assert np.max(np.abs(np.asarray(ref["x"][0], dtype=np.float64) - xo)) <= 1e-11 * np.max(np.abs(xo))
        assert np.max(np.abs(np.asarray(ref["P"][0], dtype=np.float64) - Po)) <= 1e-10 * np.max(np.abs(Po))
        assert np.all(ref["P"][1] >= np.abs(ref["P"][0]) * (1 - 1e-12)) and np.all(ref["x"][1] >= np.abs(ref["x"][0]) * (1 - 1e-12))


@pytest.mark.parametrize("cls", U.CLASSES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_designed_states_have_their_properties(cls, dtype):
    N, m = 127, 32
    x, P, z, ids = U.make_inputs(cls, N, m, dtype)           # (positive definite after the rounding: asserted inside)
    t = U.NP_DTYPE[dtype]
    assert np.array_equal(x.astype(t).astype(np.float64), x) and np.array_equal(P.astype(t).astype(np.float64), P)
    assert len(set(ids.tolist())) == m and ids.min() >= 1 and ids.max() <= N
    v, A, S = U.front(x, P, z, U.R, ids, np.float64, wrap=False)
    if cls != "rank6":
        assert np.all(np.abs(z[1]) <= U.PI)
    if cls == "independent":
        un = U.untouched_rows(N, ids)
        assert len(un) == 2 * (N - m) and not A[un].any(), "an unobserved landmark's row of P H' must be exactly zero"
        assert not P[3:, 0:3].any()
        d = np.array([np.linalg.eigvalsh(P[f:f + 2, f:f + 2]) for f in range(3, 3 + 2 * N, 2)])
        assert d[:, 1].min() < 1e-2 and d[:, 1].max() > 3.0 and (d[:, 1] / d[:, 0]).max() > 30
    if cls == "slam":
        kap = U.scaled_condition(S)
        assert 1e4 <= kap <= 1e7, kap
    if cls == "mixed":
        dv = np.diag(P)[3::2]
        assert dv.min() < 5e-6 and dv.max() > 1e2
        obs = set(((ids - 1) % 5).tolist())
        uno = set(((np.setdiff1d(np.arange(1, N + 1), ids) - 1) % 5).tolist())
        assert obs == uno == set(range(5)), "every scale needs observed and unobserved landmarks"
    if cls == "geometry":
        assert U.PI - abs(x[2]) < 5e-4
        f = 3 + 2 * (ids - 1)
        dx, dy = x[f] - x[0], x[f + 1] - x[1]
        r = np.hypot(dx, dy)
        assert r.min() == 0.5 and r.max() == 2000.0
        assert np.any(dx == 0) and np.any(dy == 0) and np.any(dx == dy)
        assert np.any(np.abs(v[1::2]) > U.PI), "no bearing innovation needs the wrap"


def test_committed_margins_follow_the_rule(needs):
    """MARGINS = max(4, 4 x the model's need), per form and class; the committed table may round up by a quarter at most.
    Also: c 2^-53 kappa stays below KAPPA_SLACK on every cell, so no bound goes slack."""
    need, rows = needs
    rule = U.margins_from(need)
    print("\nMARGINS by the rule (c_x, c_P, c_32):")
    for f in U.FORMS:
        for c in U.CLASSES:
            print(f"  {f:9s} {c:12s} " + ", ".join(f"{v:.4g}" for v in rule[f][c]) + "      model needs " +
                  ", ".join(f"{q}={v:.3g}" for q, v in sorted(need[(f, c)].items())))
    for f in U.FORMS:
        for c in U.CLASSES:
            for got, want in zip(U.MARGINS[f][c], rule[f][c]):
                assert want <= got <= 1.25 * want, (f, c, U.MARGINS[f][c], rule[f][c])
    for cell, kap, _r in rows:
        cx, cP, _ = U.bound_constants(cell.cls, cell.dtype, cell.form, cell.m)
        assert max(cx, cP) * U.EPS53 * kap < U.KAPPA_SLACK * U.C_FACTOR, (cell, kap)


def test_the_models_stay_within_a_quarter_of_their_bounds(needs):
    """By construction of the margins -- on every class, cell and form, every entry, nothing excluded."""
    _need, rows = needs
    for cell, _kap, _r in rows:
        x, P, z, ids = U.make_inputs(cell.cls, cell.N, cell.m, cell.dtype)
        ref = U.restate_cell(cell.cls, cell.N, cell.m, cell.dtype, cell.form)
        xm, Pm, side = U.model_update(x, P, z, ids, cell.dtype, cell.form)
        w = U.judge(xm, Pm, ref, cell.cls, cell.dtype, cell.form, cell.m, what=U.cell_id(cell))
        assert w["P"] <= 0.25 + 1e-9 and w["x"] <= 0.25 + 1e-9, (U.cell_id(cell), w)
        assert U.structure_ok(Pm, side)
        if cell.cls == "independent":
            un = U.untouched_rows(cell.N, ids)
            assert np.array_equal(xm[un], x[un]) and np.array_equal(Pm[un], P[un])


def _defect_results(cls, defect):
    c = DEFECT_CELL
    x, P, z, ids = U.make_inputs(cls, c["N"], c["m"], c["dtype"])
    ref = U.restate_cell(cls, c["N"], c["m"], c["dtype"], c["form"])
    rng = np.random.default_rng(5)
    ids_prev = U.choose_ids(cls, rng, c["N"], c["m"])
    previous = (U.observations(cls, rng, x, ids_prev), ids_prev)
    xm, Pm, side = U.model_update(x, P, z, ids, c["dtype"], c["form"], defect=defect, previous=previous)
    return (U.accepted(xm, Pm, side, ref, cls, c["dtype"], c["form"], c["m"]),
            U.tol_accepts(xm, Pm, side, ref, P, c["dtype"], c["form"]))


def test_planted_defects_are_rejected_and_what_the_tolerances_accept():
    """Every planted defect leaves the per-entry bounds on the class designed for it.  Printed: what TOL accepts on the same
    records -- expected non-empty: at least the gain error and the 0.99 column on `rank6`."""
    tol_list = []
    print("\ndefect                    class         per-entry bounds   TOL of test_gpu_ekf_dispatch")
    for defect in (None,) + U.DEFECTS:
        for cls in ((U.DEFECT_CLASS[defect], "rank6") if defect else U.CLASSES):
            ok_new, ok_tol = _defect_results(cls, defect)
            print(f"{str(defect):25s} {cls:12s}  {'accept' if ok_new else 'REJECT':16s}   {'ACCEPT' if ok_tol else 'reject'}")
            if defect is None:
                assert ok_new and ok_tol, cls
                continue
            if ok_tol:
                tol_list.append((defect, cls))
            if cls == U.DEFECT_CLASS[defect]:
                assert not ok_new, f"{defect} passes the per-entry bounds on {cls}"
    print("accepted by TOL:", tol_list)
    assert ("gain_1e-3", "rank6") in tol_list and ("w1_last_column_0.99", "rank6") in tol_list


def test_a_stale_padding_column_is_rejected_after_the_panel_shrank():
    """64 -> 17 observations on one handle: the earlier panel's columns 34 .. 47 (the padding up to the next multiple of 16)
    must not enter the down-date."""
    cls, N = "independent", 127
    x, P, z, ids = U.make_inputs(cls, N, 17, "f32")
    rng = np.random.default_rng(9)
    idp = U.choose_ids(cls, rng, N, 64)
    previous = (U.observations(cls, rng, x, idp), idp)
    ref = U.restate(x, P, z, ids, "cholesky")
    good = U.model_update(x, P, z, ids, "f32", "cholesky")
    bad = U.model_update(x, P, z, ids, "f32", "cholesky", defect="stale_columns", previous=previous)
    assert U.accepted(*good, ref, cls, "f32", "cholesky", 17)
    assert not U.accepted(*bad, ref, cls, "f32", "cholesky", 17)


def test_the_cells_reach_every_downdate_body():
    """In the style of tests/test_ekf_dispatch_table.py: over the GPU file's cells expected_path reaches every label and
    fallback, and every class meets every body that needs no SLAMHIP_X bit."""
    paths = U.cell_paths()
    assert {label for label, _ in paths} == set(U.LABELS)
    assert {fb for _, fb in paths} == set(U.FALLBACKS)
    plain = {U.expected_path(d, f, m)[0] for d in ("f32", "f64") for f in U.FORMS for m in U.MS}
    assert plain == set(U.LABELS) - {"f32_stream3", "f32_stream4", "f32_bf16_list"}
    for cls in U.CLASSES:
        got = {U.expected_path(c.dtype, c.form, c.m)[0] for c in U.CELLS if c.cls == cls}
        assert got == plain, (cls, plain - got)
    for m in U.MS:                                           # every m in both dtypes and both forms
        assert {(c.dtype, c.form) for c in U.CELLS if c.m == m} == {(d, f) for d in ("f32", "f64") for f in U.FORMS}, m
    assert {c.N for c in U.CELLS} == set(U.NS)
    for xf in (4, 8, 16, 128):
        assert sum(c.xflags == xf for c in U.X_CELLS) == 2


@pytest.mark.parametrize("N,nz,j", U.OBSERVE_CELLS)
def test_observe_cases_give_the_intended_counts(N, nz, j):
    """The oracle matches exactly j of the nz observations on the `independent` state (asserted inside) and no new feature
    appears: the device count is j while the host's bound is nz."""
    _x, _P, z, ao = U.observe_case(N, nz, j)
    assert z.shape == (2, nz) and int(np.sum(ao > 0)) == j and not np.any(ao < 0)
    assert len(set(ao[ao > 0].tolist())) == j


def test_the_floor_is_needed_where_the_panel_cancels():
    """`slam`, one observation, kappa = 2: the rows of P H' of the other landmarks cancel to rounding level, and the correctly
    rounded fp64 model is then off by far more than 2^-53 kappa mag on entries of P -- the term the floor carries."""
    cls, N, m = "slam", 200, 1
    x, P, z, ids = U.make_inputs(cls, N, m, "f64")
    ref = U.restate_cell(cls, N, m, "f64", "joseph")
    _xm, Pm, _side = U.model_update(x, P, z, ids, "f64", "joseph")
    Pr, Pmag, Pfl = ref["P"]
    err = np.abs(np.asarray(Pm, dtype=U.LD) - Pr)
    assert ref["kappa"] < 4
    assert float(np.max(U._over(err, U.LD(U.EPS53 * ref["kappa"]) * Pmag))) > 100, "kappa mag alone would have been enough"
    assert float(np.max(U._over(err, U.LD(U.EPS53) * (ref["kappa"] * Pmag + Pfl)))) < 1
