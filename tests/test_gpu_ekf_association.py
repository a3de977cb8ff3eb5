"""The three forms of the device gating (csrc/ekf_gate.hip: the sweep, the sweep with the spatial pre-gate, the uniform
grid) against the fp64 oracle on the scenes of tests/assoc_scenes.py: clutter (several candidates per observation, arg-min
nis != arg-min nd), observations DELTA = 1e-7 (relative) off either gate, exact and near ties inside a wave, across
workgroups and in the ragged last workgroup, and the rims of the grid's sector and annulus.  tests/test_assoc_scenes.py
checks, on the CPU, that the scenes are what they claim.

Decisions must be array_equal to the oracle's (evaluated from the DOWNLOADED state) and across the forms; values
(slam_ekf_nis) within 1e-9 of the oracle's, the fp64 tolerance of tests/test_gpu_ekf.py -- in f32 mode too, where the state
is stored in fp32 but the gating evaluates it in fp64 like the oracle does from the same rounded numbers.
"""
import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import assoc_scenes as A
from tests.assoc_scenes import GATE1, GATE2, R
from tests.test_gpu_ekf import Q, TOL, rounded
from tests.test_gpu_ekf_dispatch import _check, _handle

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
FORMS = ("sweep", "pregate", "grid")
VALUE_TOL = TOL["f64"]["x"]                      # 1e-9


def _open(pkg, monkeypatch, form, x, P, dtype, max_landmarks):
    """sweep: SLAMHIP_X=32 (never the pre-gate), pregate: SLAMHIP_X=64 (always), grid: set_gate_mode("grid")."""
    st = _handle(pkg, monkeypatch, x, P, dtype, xflags={"sweep": 32, "pregate": 64, "grid": 0}[form], max_landmarks=max_landmarks)
    st.set_gate_mode("grid" if form == "grid" else "sweep")
    return st


def _oracle(st, z):
    xo, Po = rounded(st)
    nis, nd = O.association_table_sparse(xo, Po, z, R)
    return O.assoc_vector(nis, nd, GATE1, GATE2)


def _decisions(pkg, monkeypatch, sc, dtype, extra=0):
    """associate_vector of the scene in the three forms: each equal to the oracle's vector, the form as asked for.
    Returns the open handles."""
    sts = {}
    try:
        for form in FORMS:
            st = sts[form] = _open(pkg, monkeypatch, form, sc["x"], sc["P"], dtype, sc["N"] + extra)
            xg, Pg = st.download()
            assert np.array_equal(xg, sc["x"]) and np.array_equal(Pg, sc["P"]), "the scene is not representable in " + dtype
            want = _oracle(st, sc["z"])
            assert np.array_equal(want, sc["want"])
            a = st.associate_vector(sc["z"], R, GATE1, GATE2)
            bad = np.flatnonzero(a != want)
            assert len(bad) == 0, f"{sc['name']} {form}: observations {bad[:8]} device {a[bad[:8]]} oracle {want[bad[:8]]}"
            assert st.gate_info()["form"] == ("grid" if form == "grid" else "sweep")
            again = st.associate_vector(sc["z"], R, GATE1, GATE2)       # cnt, near and arrive were re-armed
            assert np.array_equal(again, a), f"{sc['name']} {form}: the second call differs"
    except BaseException:
        for st in sts.values():
            st.close()
        raise
    return sts


def _close(sts):
    for st in sts.values():
        st.close()


def _values(st, sc, rng):
    """slam_ekf_nis for every pair the scene placed at a prescribed nis plus 16 random pairs (at least 32 in all)."""
    xo, Po = rounded(st)
    nis, nd = O.association_table_sparse(xo, Po, sc["z"], R)
    nz = sc["z"].shape[1]
    pairs = [(i, j) for i, j, _t in sc["pairs"]]
    pairs += [(int(rng.integers(nz)), int(rng.integers(1, sc["N"] + 1))) for _ in range(max(16, 32 - len(pairs)))]
    for i, j in pairs:
        if not np.isfinite(nis[i, j - 1]):
            continue
        g_nis, g_nd = st.compute_association(sc["z"][:, i], R, j)
        assert abs(g_nis - nis[i, j - 1]) <= VALUE_TOL * abs(nis[i, j - 1]), (sc["name"], i, j, g_nis, nis[i, j - 1])
        assert abs(g_nd - nd[i, j - 1]) <= VALUE_TOL * max(abs(nd[i, j - 1]), 1.0), (sc["name"], i, j, g_nd, nd[i, j - 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which,arg", A.SCENES)
def test_decisions_and_values_against_the_oracle(pkg, monkeypatch, which, arg, dtype):
    sc = A.build(which, arg, dtype)
    sts = _decisions(pkg, monkeypatch, sc, dtype)
    try:
        info = sts["grid"].gate_info()
        nz = sc["z"].shape[1]
        # gate_info's counters accumulate over the handle's life: _decisions has called associate_vector TWICE
        calls = 2
        assert info["queries"] == calls * -(-nz // 128) and info["in_grid"] == sc["N"] and info["tail"] == 0
        assert info["evaluated"] <= info["visited"]
        if sc["selective"] and which == "reach":
            # a sweep evaluates N landmarks per observation; the grid pruned
            assert info["visited"] < 0.25 * sc["N"] * nz * calls, info       # i.e. a quarter of the map per query
        _values(sts["sweep"], sc, np.random.default_rng(7))
    finally:
        _close(sts)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", A.PARTITION_N)
def test_partition_cells(pkg, monkeypatch, N, dtype):
    """N and nz around the edges of the sweep's partition: 64 landmarks per workgroup, eight observation waves, chunks of
    128 observations.  One handle per form walks through every nz, largest first (a 257-observation call is followed by
    smaller ones down to a single observation)."""
    x, P = A.partition_state(N, dtype)
    sts = {form: _open(pkg, monkeypatch, form, x, P, dtype, N) for form in FORMS}
    try:
        for nz in sorted(A.PARTITION_NZ, reverse=True):
            sc = A.partition_cells(N, nz, dtype)
            for form, st in sts.items():
                a = st.associate_vector(sc["z"], R, GATE1, GATE2)
                assert np.array_equal(a, sc["want"]), f"N={N} nz={nz} {form}: {a} against {sc['want']}"
        for form, st in sts.items():                                    # 257 observations, then one
            big, one = A.partition_cells(N, 257, dtype), A.partition_cells(N, 1, dtype)
            assert np.array_equal(st.associate_vector(big["z"], R, GATE1, GATE2), big["want"]), form
            assert np.array_equal(st.associate_vector(one["z"], R, GATE1, GATE2), one["want"]), form
            assert st.gate_info()["form"] == ("grid" if form == "grid" else "sweep")
    finally:
        _close(sts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_after_the_map_changed(pkg, monkeypatch, dtype):
    """The grid's tail, drift and rebuild are separate code: 40 landmarks are appended, the vehicle moves, 16 known
    landmarks are updated; then a second draw of edge observations from the state as the device now holds it."""
    sc = A.cluster_scene(A.CLUSTER_SEEDS[0], dtype)
    sts = _decisions(pkg, monkeypatch, sc, dtype, extra=40)
    try:
        rng = np.random.default_rng(21)
        znew = np.vstack([rng.uniform(160, 200, 40), rng.uniform(-3, 3, 40)])
        ids = rng.choice(np.arange(1, sc["N"] + 1), 16, replace=False)
        r0 = sts["grid"].gate_info()["rebuilds"]
        states = []
        for form, st in sts.items():
            st.add_features(znew, R)
            st.predict(8.0, 0.05, 4.0, Q, 0.025)
            xo, _ = rounded(st)
            zp, _, _ = O.obs_blocks(xo, ids)
            st.update(zp.T + np.array([[0.05], [0.004]]), R, ids)
            states.append(st.download())
            assert st.N == sc["N"] + 40
        for xg, Pg in states[1:]:                                       # the gating form does not touch the filter
            assert np.array_equal(xg, states[0][0]) and np.array_equal(Pg, states[0][1])
        xo, Po = rounded(sts["sweep"])
        z, pairs = A.cluster_draw(xo, Po, sc["isolated"], np.random.default_rng(22))
        nis, nd = O.association_table_sparse(xo, Po, z, R)
        want = O.assoc_vector(nis, nd, GATE1, GATE2)
        assert (want > 0).sum() >= 8 and (want == 0).sum() >= 8 and (want < 0).sum() >= 4
        for form, st in sts.items():
            a = st.associate_vector(z, R, GATE1, GATE2)
            bad = np.flatnonzero(a != want)
            assert len(bad) == 0, f"{form}: observations {bad[:8]} device {a[bad[:8]]} oracle {want[bad[:8]]}"
        info = sts["grid"].gate_info()
        assert info["form"] == "grid" and (info["tail"] > 0 or info["rebuilds"] > r0), info
    finally:
        _close(sts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_keeps_landmarks_that_moved_towards_the_pose(pkg, monkeypatch, dtype):
    """The annulus is tested on the means AT BUILD TIME, widened by the recorded drift.  An update moves the deciding
    landmarks of the reach scene inwards by decimetres -- more than the slack of the annulus, less than what makes the
    device rebuild the grid -- and they are then observed on its outer and inner rim (tests/test_assoc_scenes.py shows on
    the host restatement that they are lost without the drift term)."""
    sc = A.reach_scene("inside", dtype)
    sts = _decisions(pkg, monkeypatch, sc, dtype)
    try:
        zu, ids = A.reach_update_inputs(sc)
        r0 = sts["grid"].gate_info()["rebuilds"]
        for st in sts.values():
            st.update(zu, R, ids)
        xo, Po = rounded(sts["grid"])
        moved = np.max(np.abs(xo[3:] - sc["x"][3:]))
        assert moved > 0.1
        z, zid = A.reach_rim_after(xo, Po, sc["dec_ids"])
        assert z.shape[1] >= len(sc["dec_ids"])
        nis, nd = O.association_table_sparse(xo, Po, z, R)
        want = O.assoc_vector(nis, nd, GATE1, GATE2)
        assert np.all(want == 0)
        for form, st in sts.items():
            a = st.associate_vector(z, R, GATE1, GATE2)
            assert np.array_equal(a, want), f"{form}: {a}"
        info = sts["grid"].gate_info()
        assert info["form"] == "grid" and info["rebuilds"] == r0, info   # the grid of BEFORE the update answered
    finally:
        _close(sts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_observe_on_the_cluster_scene(pkg, monkeypatch, dtype):
    """observe() on clutter: 61 matched observations, 7 of them a second one of a landmark already matched (duplicate ids in
    the update; tests/test_assoc_scenes.py holds the scene to that), ~10 new features.  Decisions against the oracle, the
    state against update_sparse + add_features_sparse from the downloaded prior, the sweep's and the grid's handle
    bit-identical."""
    sc = A.cluster_scene(A.CLUSTER_SEEDS[0], dtype, True)
    want = sc["want"]
    matched = want[want > 0]
    assert 56 <= len(matched) <= 64 and len(matched) - len(set(matched.tolist())) >= 5
    nnew = int((want < 0).sum())
    out = {}
    for form in ("sweep", "grid"):
        st = _open(pkg, monkeypatch, form, sc["x"], sc["P"], dtype, sc["N"] + nnew)
        try:
            xo, Po = rounded(st)
            a = st.observe(sc["z"], R, GATE1, GATE2)
            assert np.array_equal(a, want), f"{form}: observations {np.flatnonzero(a != want)[:8]}"
            assert st.gate_info()["form"] == form and st.N == sc["N"] + nnew
            zf, idf, zn = O.split_assoc(sc["z"], want)
            xn, Pn = O.update_sparse(xo, Po, zf, R, idf)
            xn, Pn = O.add_features_sparse(xn, Pn, zn, R)
            _check(st, xn, Pn, Po, dtype, f"observe on the cluster scene ({form})", fx=4.0, fP=100.0)
            out[form] = st.download()
        finally:
            st.close()
    assert np.array_equal(out["sweep"][0], out["grid"][0]) and np.array_equal(out["sweep"][1], out["grid"][1])
