"""The EKF update on the device, entry by entry, against tests/update_records.py -- through the C ABI (EKFSlamState).

Every cell is ONE call, re-anchored as `_update_step` of tests/test_gpu_ekf_dispatch.py does it: the device's own state is
downloaded (for a designed state it must equal the upload bit for bit), the update is restated from it in extended precision,
and after the call
  * EVERY entry of x and P is within its derived bound (update_records: u_T |ref| + c_x 2^-53 (kappa mag + floor) for x,
    c_32 2^-24 mag + c_P 2^-53 (kappa mag + floor) for P; margins from the CPU model, none from a device) -- no entry is
    excluded,
  * P is exactly symmetric, the packed side array equals the matrix (check_side), the storage invariants hold
    (strip_ref.check_storage),
  * on `independent` the rows of P and the entries of x of every unobserved landmark are bit-identical.
The cells cross every body of the down-date dispatch (tests/test_update_records_cpu.py checks the table), SLAMHIP_X's product
bits, observe() with a device count below the host's bound (each fallback), and a grow-and-shrink schedule on one handle.
The last test prints the worst error / bound per class, dtype and quantity (run with -s).
"""
import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import strip_ref as S
from tests import update_records as U
from tests.test_gpu_ekf import R, check_side, rounded
from tests.test_gpu_ekf_dispatch import _handle

pytestmark = pytest.mark.gpu

WORST = {}                     # (class, dtype) -> {"x": .., "P": ..}: largest error / bound seen


def _after(st, ref, cls, dtype, form, m, what, x0, P0, untouched=None):
    xg, Pg = st.download()
    assert np.array_equal(Pg, Pg.T), f"{what}: P must stay exactly symmetric"
    check_side(st, Pg, what)
    S.check_storage(st, Pg=Pg, what=what)
    U.judge(xg, Pg, ref, cls, dtype, form, m, what=what, log=WORST.setdefault((cls, dtype), {}))
    if untouched is not None:
        assert np.array_equal(xg[untouched], x0[untouched]), f"{what}: x of an unobserved landmark moved"
        assert np.array_equal(Pg[untouched], P0[untouched]), f"{what}: a row of P of an unobserved landmark moved"


def _uploaded(st, x, P, what):
    """The handle holds the designed state bit for bit: the restatement cached per cell IS the re-anchored one."""
    xo, Po = rounded(st)
    assert np.array_equal(xo, x) and np.array_equal(Po, P), f"{what}: upload / download is not the identity"


@pytest.mark.parametrize("cell", U.CELLS + U.X_CELLS, ids=U.cell_id)
def test_update_entry_by_entry(pkg, monkeypatch, cell):
    x, P, z, ids = U.make_inputs(cell.cls, cell.N, cell.m, cell.dtype)
    what = f"{U.cell_id(cell)} {U.expected_path(cell.dtype, cell.form, cell.m, cell.xflags)[0]}"
    st = _handle(pkg, monkeypatch, x, P, cell.dtype, cell.xflags, max_landmarks=cell.N)
    try:
        _uploaded(st, x, P, what)
        ref = U.restate_cell(cell.cls, cell.N, cell.m, cell.dtype, cell.form)
        st.update(z, R, ids, form=cell.form)
        _after(st, ref, cell.cls, cell.dtype, cell.form, cell.m, what, x, P,
               U.untouched_rows(cell.N, ids) if cell.cls == "independent" else None)
    finally:
        st.close()


@pytest.mark.parametrize("N,nz,j", U.OBSERVE_CELLS)
def test_observe_with_a_device_count_below_the_bound(pkg, monkeypatch, N, nz, j):
    x, P, z, ao = U.observe_case(N, nz, j)
    path = U.expected_path("f32", "cholesky", nz, 0, device_m=j)
    what = f"observe independent N={N} nz={nz} j={j} {path}"
    st = _handle(pkg, monkeypatch, x, P, "f32", max_landmarks=N + 8)
    try:
        _uploaded(st, x, P, what)
        a = st.observe(z, R, 4.0, 25.0)
        assert np.array_equal(a, ao), f"{what}: observe's decisions differ from the oracle's"
        assert st.N == N
        if j == 0:
            xg, Pg = st.download()
            assert np.array_equal(xg, x) and np.array_equal(Pg, P), f"{what}: no match, the state must not move"
            return
        zf, idf, _ = O.split_assoc(z, ao)
        idf = idf.reshape(-1)
        ref = U.restate(x, P, zf, idf, "cholesky")
        _after(st, ref, "independent", "f32", "cholesky", j, what, x, P, U.untouched_rows(N, idf))
    finally:
        st.close()


def test_the_panel_grows_and_shrinks_on_one_handle(pkg, monkeypatch):
    """64 -> 17 -> 64 observations: a column of the earlier, wider panel (or of its pre-split image) that stayed behind would
    carry a landmark's whole down-date on this state.  Landmarks never observed keep their rows bit for bit throughout."""
    cls, N, dtype = "independent", 127, "f32"
    x, P, _z, _ids = U.make_inputs(cls, N, U.SCHEDULE_MS[0], dtype)
    rng = np.random.default_rng(77)
    st = _handle(pkg, monkeypatch, x, P, dtype, max_landmarks=N)
    try:
        _uploaded(st, x, P, "schedule")
        seen = np.zeros(0, dtype=np.int64)
        for step, m in enumerate(U.SCHEDULE_MS):
            what = f"schedule step {step}: m={m} {U.expected_path(dtype, 'cholesky', m)[0]}"
            xo, Po = rounded(st)                                         # re-anchor
            ids = U.choose_ids(cls, rng, N, m)
            z = U.observations(cls, rng, xo, ids)
            ref = U.restate(xo, Po, z, ids, "cholesky")
            st.update(z, R, ids)
            seen = np.union1d(seen, ids)
            _after(st, ref, cls, dtype, "cholesky", m, what, x, P, U.untouched_rows(N, seen))
    finally:
        st.close()


def test_zz_report_the_worst_error_over_bound(pkg):
    """Not a check of its own: the largest error / bound per class, dtype and quantity the cells above have seen."""
    print("\nworst error / bound   class         dtype      x        P")
    for (cls, dtype), w in sorted(WORST.items()):
        print(f"                      {cls:12s}  {dtype}   {w.get('x', 0.0):8.3f} {w.get('P', 0.0):8.3f}")
        assert w.get("x", 0.0) <= 1.0 and w.get("P", 0.0) <= 1.0
