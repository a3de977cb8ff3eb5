"""slam_ekf_merge_landmarks on the device, entry by entry, against tests/merge_records.py -- through the C ABI, as `lib_merge`
of tests/test_gpu_ekf_merge.py calls it.

Every cell is ONE merge call from a designed state: the download must equal the upload bit for bit, the merge is restated from
that state in extended precision, and after the call
  * new_index equals merge_ref.new_index_of,
  * EVERY entry of x and P is within its derived bound against ref[keep] (merge_records: u_T |ref| + c_x 2^-53 (kappa mag +
    floor) for x, c_32 2^-24 mag + c_P 2^-53 (kappa mag + floor) for P; margins from the CPU model, none from a device),
  * P is exactly symmetric, the packed side array equals the matrix (check_side), the storage invariants hold
    (strip_ref.check_storage),
  * on `independent` the pose and every landmark outside the pairs, on `echo` every survivor, come back bit for bit.
One handle then runs update m = 64 (in fp32: the bf16 path with its pre-split image and a 128-column panel), merge of 1 pair,
update m = 17, merge of 8, merge of 3: a column of a wider panel or an image left behind would carry a landmark's whole
down-date on `independent`.  The last test prints the worst error / bound per class, dtype and quantity (run with -s).
"""
import numpy as np
import pytest

from tests import merge_records as M
from tests import merge_ref as MR
from tests import strip_ref as S
from tests import update_records as U
from tests.test_gpu_ekf import R, check_side, rounded
from tests.test_gpu_ekf_merge import lib_merge

pytestmark = pytest.mark.gpu

WORST = {}                     # (class, dtype) -> {"x": .., "P": ..}: largest error / bound seen


def _structure(st, pkg, Pg, what):
    assert np.array_equal(Pg, Pg.T), f"{what}: P must stay exactly symmetric"
    check_side(st, Pg, what)
    S.check_storage(st, pkg, Pg, what=what)


def _merge_and_judge(pkg, st, xo, Po, pairs, Rc, cls, dtype, what, ref=None):
    """One merge call from the state (xo, Po) the handle holds; returns (x, P, new_index) after it."""
    N = st.N
    if ref is None:
        ref = M.after_removal(M.restate(xo, Po, pairs, Rc))
    code, ni = lib_merge(pkg, st, pairs, Rc)
    assert code == 0 and st.N == N - len(pairs), what
    assert np.array_equal(ni, MR.new_index_of(N, pairs)), (what, ni.tolist())
    xg, Pg = st.download()
    _structure(st, pkg, Pg, what)
    M.judge(xg, Pg, ref, cls, dtype, len(pairs), what=what, log=WORST.setdefault((cls, dtype), {}))
    return xg, Pg, ni


@pytest.mark.parametrize("cell", M.CELLS, ids=M.cell_id)
def test_merge_entry_by_entry(pkg, cell):
    x, P, pairs, Rc = M.make_inputs(*cell)
    what = M.cell_id(cell)
    st = pkg.EKFSlamState(x, P, dtype=cell.dtype, max_landmarks=cell.N + 4)
    try:
        xo, Po = rounded(st)
        assert np.array_equal(xo, x) and np.array_equal(Po, P), f"{what}: upload / download is not the identity"
        xg, Pg, _ni = _merge_and_judge(pkg, st, x, P, pairs, Rc, cell.cls, cell.dtype, what, ref=M.restate_cell(cell))
        keep = M.keep_index(len(x), pairs)
        if cell.cls == "independent":
            un = np.flatnonzero(np.isin(keep, np.concatenate([[0, 1, 2], M.untouched_rows(cell.N, pairs)])))
            assert np.array_equal(xg[un], x[keep][un]), f"{what}: x of the pose or of a landmark in no pair moved"
            assert np.array_equal(Pg[un], P[np.ix_(keep, keep)][un]), f"{what}: a row of P of the pose or of a landmark in no pair moved"
        if cell.cls == "echo":
            assert np.array_equal(xg, x[keep]), f"{what}: a survivor's x moved"
            assert np.array_equal(Pg, P[np.ix_(keep, keep)]), f"{what}: a survivor's row of P moved"
    finally:
        st.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_merge_after_wide_updates_on_one_handle(pkg, dtype):
    """M.SCHEDULE on one handle, re-anchored from the device's own state before every call.  Updates are judged by
    update_records with its margins, merges by merge_records; landmarks never observed and never paired keep x and their
    rows of P bit for bit throughout, followed through new_index."""
    cls, N0 = M.SCHEDULE_CLASS, M.SCHEDULE_N
    x0, P0, rng = M.schedule_start(dtype)
    st = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=N0 + 4)
    try:
        xo, Po = rounded(st)
        assert np.array_equal(xo, x0) and np.array_equal(Po, P0), "upload / download is not the identity"
        orig = np.arange(1, N0 + 1)                      # orig[j - 1]: the first id of the landmark that is j now
        touched = np.zeros(N0 + 1, dtype=bool)           # by original id
        for step, (kind, m) in enumerate(M.SCHEDULE):
            N = st.N
            xo, Po = rounded(st)                         # re-anchor
            if kind == "update":
                what = f"{dtype} step {step}: update m={m} {U.expected_path(dtype, 'cholesky', m)[0]}"
                z, ids = M.schedule_update(rng, xo, N, m)
                ref = U.restate(xo, Po, z, ids, "cholesky")
                st.update(z, R, ids)
                xg, Pg = st.download()
                _structure(st, pkg, Pg, what)
                U.judge(xg, Pg, ref, cls, dtype, "cholesky", m, what=what)
                touched[orig[ids - 1]] = True
            else:
                what = f"{dtype} step {step}: merge cnt={m} at N={N}"
                x2, pairs, Rc = M.schedule_merge(rng, xo, Po, dtype, N, m, step)
                st.set_state(x2, Po)                     # the same N: the panels are left as they are
                xo, Po = rounded(st)
                assert np.array_equal(xo, x2), what
                xg, Pg, ni = _merge_and_judge(pkg, st, xo, Po, pairs, Rc, cls, dtype, what)
                touched[orig[np.asarray(pairs).reshape(-1) - 1]] = True
                gone = np.asarray(pairs)[:, 1]
                stay = np.setdiff1d(np.arange(1, N + 1), gone)
                assert np.array_equal(ni[stay - 1], np.arange(1, len(stay) + 1)), what
                orig = orig[stay - 1]
            # the landmarks nobody has touched: x and the whole row of P, as uploaded
            cur = np.flatnonzero(~touched[orig]) + 1
            assert len(cur) >= 10, what
            f_then = np.concatenate([[0, 1, 2], np.stack([3 + 2 * (orig - 1), 4 + 2 * (orig - 1)], axis=1).reshape(-1)])
            rows = np.sort(np.concatenate([3 + 2 * (cur - 1), 4 + 2 * (cur - 1)]))
            assert np.array_equal(xg[rows], x0[f_then[rows]]), f"{what}: x of an untouched landmark moved"
            assert np.array_equal(Pg[rows], P0[np.ix_(f_then[rows], f_then)]), f"{what}: a row of P of an untouched landmark moved"
    finally:
        st.close()


def test_zz_report_the_worst_error_over_bound(pkg):
    """Not a check of its own: the largest error / bound per class, dtype and quantity the cells above have seen."""
    print("\nworst error / bound   class         dtype      x        P")
    for (cls, dtype), w in sorted(WORST.items()):
        print(f"                      {cls:12s}  {dtype}   {w.get('x', 0.0):8.3f} {w.get('P', 0.0):8.3f}")
        assert w.get("x", 0.0) <= 1.0 and w.get("P", 0.0) <= 1.0
