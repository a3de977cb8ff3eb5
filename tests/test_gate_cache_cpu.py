"""The table of map-changing calls (tests/gate_cache_scenes.py) held to account without a GPU:

  * completeness -- every entry point of the sixteen signature tables that takes an EKF handle, or an object attached to one, is
    either the call of a table row or a member of the explicit READ_ONLY set, never both and never neither: the next side library
    gets its row here;
  * sensitivity -- for every row that claims it, from the builder's states and the fp64 oracle alone: the oracle matches at least
    one landmark and finds one new feature on the expected state after the call, every decision is at least 1 % clear of both
    gates, and for each target the side state of BEFORE the call would have missed it by a factor of 2
    (tests/gate_cache_ref.stale_would_miss); for condition (r), where a stale bound is merely too large, that the grid query would
    evaluate at least twice the landmarks (tests/gate_cache_ref.evaluated_bounds).  Conditions on the input, not measurements: without them a row would pass with the
    line it is there for deleted."""
import math
import os

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import gate_cache_ref as GR
from tests import gate_cache_scenes as S

DTYPES = ["f64", "f32"]
FACTOR = 2.0


def _takes_an_ekf_handle(header):
    """The slam_* prototypes of a header with a parameter of type slam_ekf_t or of an object attached to one (slam_ekf_fej_t,
    slam_ekf_local_t, slam_ekf_jc_t, slam_ekf_factor_t), pointers to them included (the create calls)."""
    import re
    from tests.abi_surface import ROOT, _code
    protos = re.findall(r"\b(slam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _code(os.path.join(ROOT, header)))
    return {name for name, params in protos if re.search(r"\bslam_ekf(_[a-z]+)?_t\b", params)}


def _entry_points(pkg):
    """name -> table, of every entry point of the product library's table and the side libraries' that takes an EKF handle or an
    object attached to one: by the parameter types of its prototype in the library's header (the ctypes tables have one opaque
    handle type), and -- a second net -- by `_ekf` in its name."""
    L = pkg._lib
    tables = {"product": (L.SIGNATURES, ("include/slamhip.h", "include/slamhip_diag.h"))}
    tables.update({name: (c.signatures, (c.header,)) for name, c in L.LIBRARIES.items()})
    assert len(tables) == 16
    out = {}
    for lib, (sigs, headers) in tables.items():
        typed = set().union(*(_takes_an_ekf_handle(h) for h in headers))
        assert typed <= set(sigs), (lib, sorted(typed - set(sigs)))
        for name in sigs:
            if name in typed or "_ekf" in name:
                assert name not in out
                out[name] = lib
    return out


def test_every_entry_point_on_an_ekf_handle_is_classified_exactly_once(pkg):
    eps = _entry_points(pkg)
    rows = {}
    for r in S.ROWS:
        for e in r.entries:
            rows.setdefault(e, []).append(r)
    unknown = sorted((set(rows) | S.READ_ONLY) - set(eps))
    assert not unknown, f"classified but not an entry point: {unknown}"
    both = sorted(set(rows) & S.READ_ONLY)
    assert not both, f"a table row AND read-only: {both}"
    unclassified = sorted(set(eps) - set(rows) - S.READ_ONLY)
    print(f"{len(eps)} entry points on an EKF handle: {len(rows)} in table rows, {len(S.READ_ONLY)} read-only, "
          f"{len(unclassified)} unclassified")
    assert not unclassified, f"neither a row of tests/gate_cache_scenes.py nor READ_ONLY: {unclassified}"
    for e, rs in rows.items():                         # a row lives in the library its call lives in
        for r in rs:
            assert r.lib == eps[e], (r.name, e, eps[e])
    assert len({r.name for r in S.ROWS}) == len(S.ROWS)


def _margins(nis, what):
    """tests/test_gpu_ekf_transform._margins: every decision at least 1 % clear of both gates."""
    with np.errstate(invalid="ignore"):
        rel = min(float(np.nanmin(np.abs(nis - S.GATE1) / S.GATE1)),
                  float(np.nanmin(np.abs(np.nanmin(nis, axis=1) - S.GATE2) / S.GATE2)))
    assert rel >= 0.01, f"{what}: a decision lies within 1 % of a gate ({rel:.4f})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_the_scene_is_one_a_stale_cache_would_decide_differently(row, dtype):
    sc = row.build(dtype)
    x1, P1 = sc.after
    what = f"{row.name} {dtype}"
    assert np.array_equal(P1, P1.T) or np.allclose(P1, P1.T, rtol=0, atol=1e-12 * np.abs(P1).max()), what
    assert np.linalg.eigvalsh((P1 + P1.T) / 2).min() > -1e-9 * np.abs(P1).max(), f"{what}: the expected covariance is not one"
    nis, nd = O.association_table_sparse(x1, P1, sc.z, S.R)
    _margins(nis, what)
    want = O.assoc_vector(nis, nd, S.GATE1, S.GATE2)
    assert np.any(want > 0) and np.any(want < 0), (what, want.tolist())
    if row.sensitive == "control":
        assert not sc.targets and row.why, what
        return
    pmax_old = GR.true_pmax(sc.before[1])
    seen = set()
    if "r" in row.sensitive:
        # the bound of before the call is still valid afterwards, only far too large: the grid query would evaluate at least twice
        # the landmarks it may evaluate under the recomputed one (items of before the call, the call's own displacement as drift)
        assert row.recomputed and sc.stale_bound == pytest.approx(pmax_old, rel=0.01) and len(sc.x_old) == len(x1), what
        drift = float(np.max(np.abs(x1[3:] - sc.x_old[3:])))
        cols = [sc.z[:, i] for i in range(sc.z.shape[1])]
        most = sum(GR.evaluated_bounds(x1, P1, z, sc.x_old[3:], GR.true_pmax(P1), S.R, S.GATE2, drift)[1] for z in cols)
        least = sum(GR.evaluated_bounds(x1, P1, z, sc.x_old[3:], sc.stale_bound, S.R, S.GATE2)[0] for z in cols)
        print(f"{what}: bound {pmax_old:.3g} -> {GR.true_pmax(P1):.3g}; landmarks evaluated: at most {most} under the new bound, "
              f"at least {least} under the old one  (r) {least / max(most, 1):.2f}")
        assert most >= 1 and least >= FACTOR * most, (what, least, most)
        seen.add("r")
    assert sc.targets or "r" in row.sensitive, what
    for i, j, conds in sc.targets:
        assert want[i] == j, f"{what}: observation {i} should match landmark {j}, the oracle says {want[i]}"
        assert nis[i, j - 1] < S.GATE1
        miss = GR.stale_would_miss(x1, P1, sc.z[:, i], j, S.R, S.GATE2, pmax_old, sc.x_old, recomputed=row.recomputed)
        print(f"{what}: observation {i} -> landmark {j}, nis {nis[i, j - 1]:.3f}; stale cache misses by  "
              + "  ".join(f"({k}) {miss[k]:.2f}" for k in conds))
        for k in conds:
            assert miss[k] >= FACTOR, f"{what}: condition ({k}) holds only by {miss[k]:.3f} for landmark {j}"
        seen |= set(conds)
    assert seen == set(row.sensitive), f"{what}: the row names {row.sensitive}, its targets carry {sorted(seen)}"


def test_the_restatement_of_the_reach_on_the_recipe():
    """The figures the recipe quotes, from the restated formulas: rho about 0.5 m under a bound of 1e-4 and about 14 m under 4;
    the pre-gate's range bound under the old bound; and the bound itself."""
    x, P = S.base()
    z = S.obs(x, S.T)
    assert GR.true_pmax(P) == pytest.approx(1e-4, rel=0.02)
    assert GR.grid_reach(x, P, z, 1e-4, S.R, S.GATE2)["rho"] == pytest.approx(0.5, rel=0.05)
    wide = GR.grid_reach(x, P, z, 4.0, S.R, S.GATE2)
    assert wide["rho"] == pytest.approx(14.16, rel=0.01) and wide["lo"] == pytest.approx(z[0] - wide["rho"]) and wide["beta"] < 0.5
    b0, b1 = GR.pre_gate_bounds(x, P, S.T, 1e-4, S.R, S.GATE2)
    assert 0.25 < b0 < 0.26 and 0.0 < b1 < 0.01
    assert GR.grid_reach(x, P, np.array([0.3, 0.0]), 1e-4, S.R, S.GATE2)["beta"] == math.pi      # r <= rho: the whole annulus
    # a landmark on top of the vehicle (d = 0) or a negative variance: the bound is not usable, nothing is skipped
    x0 = x.copy()
    x0[GR.f(1):GR.f(1) + 2] = x0[0:2]
    assert GR.pre_gate_bounds(x0, P, 1, 1e-4, S.R, S.GATE2) == (math.inf, math.inf)
