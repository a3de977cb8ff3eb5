"""CPU half of tests/test_gpu_ekf_association.py: with the oracle alone, every scene of tests/assoc_scenes.py is as hard as
it claims, so that the GPU test cannot pass vacuously.  The counts below are CONDITIONS on the scenes (chosen below what a
prototype of the cluster scene reached: 35-39 observations with two or more candidates, 20-22 where arg-min nis and arg-min nd
differ), not measurements of the device.

The grid's pruning is restated on the host (assoc_scenes.grid_reach, from the formulas in the header of the grid form in
csrc/ekf_gate.hip); the tests below also show, on that restatement, that the reach scenes would tell a grid with half the
sector angle, without one of the four arc tests or without the drift term of the annulus from a correct one.
"""
import math

import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import assoc_scenes as A
from tests.assoc_scenes import DELTA, GATE1, GATE2, R

DTYPES = ["f64", "f32"]


def _table(sc):
    return O.association_table_sparse(sc["x"], sc["P"], sc["z"], R)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", A.CLUSTER_SEEDS)
def test_cluster_scene_is_cluttered(seed, dtype):
    sc = A.cluster_scene(seed, dtype)
    t = np.float32 if dtype == "f32" else np.float64
    assert np.array_equal(sc["x"], sc["x"].astype(t).astype(np.float64)) and np.array_equal(sc["P"], sc["P"].astype(t).astype(np.float64))
    assert np.all(np.linalg.eigvalsh(sc["P"]) > 0)
    d = np.diag(sc["P"])[3::2]
    assert d.max() / d.min() > 30.0                                       # per-landmark variances over a wide range
    nis, nd = _table(sc)
    assert sc["z"].shape == (2, 96)
    cand = nis < GATE1
    multi = np.flatnonzero(cand.sum(axis=1) >= 2)
    assert len(multi) >= 25
    differ = sum(int(np.argmin(np.where(cand[i], nis[i], np.inf)) != np.argmin(np.where(cand[i], nd[i], np.inf))) for i in multi)
    assert differ >= 10
    want = sc["want"]
    assert (want > 0).sum() >= 8 and (want == 0).sum() >= 8 and (want < 0).sum() >= 4
    # every edge target on both flanks of both gates, placed to 1e-10
    targets = {t for _, _, t in sc["pairs"]}
    assert set(A.EDGE_TARGETS) <= targets
    for i, j, t in sc["pairs"]:
        assert abs(nis[i, j - 1] / t - 1.0) <= 1e-10
    # the isolated landmarks: nothing else within gate2 of their observations, so the outer gate alone decides them
    iso = set(int(j) for j in sc["isolated"])
    for i, j, t in sc["pairs"]:
        if j in iso:
            row = nis[i].copy()
            row[j - 1] = np.inf
            assert row.min() > GATE2
            assert want[i] == (-1 if t > GATE2 else 0)
    assert sum(1 for i, j, t in sc["pairs"] if j in iso and t == GATE2 * (1 + DELTA)) >= 2
    assert sum(1 for i, j, t in sc["pairs"] if j in iso and t == GATE2 * (1 - DELTA)) >= 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_with_landmarks_observed_twice(dtype):
    """What observe() is run on: about 60 matched observations (one update of k ~ 120 rows, below the 64-observation
    switch of the down-date) with several landmarks matched more than once, and new features beside them."""
    sc = A.cluster_scene(A.CLUSTER_SEEDS[0], dtype, True)
    want = sc["want"]
    matched = want[want > 0]
    assert sc["z"].shape == (2, 96) and 56 <= len(matched) <= 64
    assert len(matched) - len(set(matched.tolist())) >= 5
    assert (want < 0).sum() >= 4 and (want == 0).sum() >= 8
    assert set(A.EDGE_TARGETS) <= {t for _, _, t in sc["pairs"]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["placed", "all", "all_small"])
def test_copy_scenes_have_exact_ties_that_the_lowest_index_decides(kind, dtype):
    sc = A.copies_scene(kind, dtype)
    nis, nd = _table(sc)
    want, group = sc["want"], sc["group"]
    ties = 0
    for i in range(sc["z"].shape[1]):
        if want[i] <= 0:
            continue
        b = want[i] - 1
        same = np.flatnonzero((nd[i] == nd[i, b]) & (nis[i] < GATE1))
        if len(same) >= 2:
            ties += 1
            assert b == same.min() and np.all(group[same] == group[b])
            # a fold that took the LAST arrival, or the higher index, would answer differently
            assert same.max() + 1 != want[i]
    if kind == "placed":
        assert ties >= 3 * len(A.COPY_PAIRS)
        lo_hi = {(int(group[j]), j) for j in range(sc["N"]) if group[j] != j}
        assert lo_hi == set(A.COPY_PAIRS)
        dist = {hi - lo for lo, hi in A.COPY_PAIRS}
        assert {1, 63, 64, 192} <= dist                                   # one wave; neighbouring and distant workgroups
        assert any(hi >= 320 > lo for lo, hi in A.COPY_PAIRS) and any(lo >= 320 for lo, hi in A.COPY_PAIRS)   # the ragged last one
    else:
        assert sc["N"] % 64 == 1 and np.all(group == 0)
        assert ties == len(sc["tie_obs"]) and np.all(want[sc["tie_obs"]] == 1)
        # every workgroup holds a candidate of every matched observation: ceil(N / 64) equal list entries
        assert np.all((nis[sc["tie_obs"]] < GATE1).sum(axis=1) == sc["N"])
        assert {-1, 0, 1} == set(want.tolist())
    assert np.all(np.linalg.eigvalsh(sc["P"]) > -1e-9 * np.abs(sc["P"]).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_near_ties_are_decided_by_the_inflated_block_alone(dtype):
    sc = A.copies_scene("near", dtype)
    nis, nd = _table(sc)
    x, P = sc["x"], sc["P"]
    for k, (lo, hi) in enumerate(A.COPY_PAIRS):
        flo, fhi = 3 + 2 * lo, 3 + 2 * hi
        # the pair differs in the lower landmark's own 2 x 2 block and nowhere else
        assert np.array_equal(x[flo:flo + 2], x[fhi:fhi + 2])
        rows_lo, rows_hi = P[flo:flo + 2].copy(), P[fhi:fhi + 2].copy()
        blk_lo, blk_hi = rows_lo[:, flo:flo + 2].copy(), rows_hi[:, fhi:fhi + 2].copy()
        assert np.array_equal(rows_lo[:, fhi:fhi + 2], blk_hi)           # cross block = the original block
        rows_lo[:, flo:flo + 2] = 0; rows_lo[:, fhi:fhi + 2] = 0; rows_hi[:, flo:flo + 2] = 0; rows_hi[:, fhi:fhi + 2] = 0
        assert np.array_equal(rows_lo, rows_hi)
        ratio = blk_lo / blk_hi
        assert np.all(ratio > 1.0) and np.all(np.abs(ratio - (1 + 1e-6)) < 2e-7)
        for i in (2 * k, 2 * k + 1):
            # the inflated (lower) landmark has the SMALLER nis and the larger nd: nd = nis decides wrongly, and so does
            # "lowest index on a tie"
            assert sc["want"][i] == hi + 1
            assert nis[i, lo] <= nis[i, hi] < GATE1
            assert nd[i, lo] - nd[i, hi] >= 1e-9 * max(1.0, abs(nd[i, hi]))
            assert nd[i, lo] - nd[i, hi] < 1e-5
        assert nis[2 * k, hi] < 1e-20                                    # v = 0: log det S alone


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["inside", "outside", "huge"])
def test_reach_scene_cases(kind, dtype):
    sc = A.reach_scene(kind, dtype)
    nis, nd = _table(sc)
    x, z, cases, want = sc["x"], sc["z"], sc["cases"], sc["want"]
    lx, ly = x[3::2], x[4::2]
    dist = np.hypot(lx - x[0], ly - x[1])
    inside_box = lx.min() <= x[0] <= lx.max() and ly.min() <= x[1] <= ly.max()
    assert inside_box == (kind != "outside")
    assert not sc["d0_finite"]                      # the oracle has no S for a landmark AT the pose: no scene holds one
    assert dist.min() > 0.0
    assert math.sqrt(sc["P"][2, 2]) > 0.04          # a large heading variance ...
    seen = {c.split(":")[0] for c in cases}
    assert {"sector_rim", "annulus_rim", "outside", "inner_edge", "match", "unwrapped", "unwrapped_rim", "beyond", "negative_far"} <= seen
    geo = A.grid_geometry(x)
    axes_in_arc = {0.0: 0, math.pi: 0, math.pi / 2: 0, -math.pi / 2: 0}
    cut = 0
    half_beta_misses = 0
    arc_needed = [0, 0, 0, 0]
    for i, c in enumerate(cases):
        tag = c.split(":")[0]
        reach = A.grid_reach(x, sc["P"], z[:, i], geo)
        # the restated reach is sound: it sees every landmark within gate2 of the observation
        with np.errstate(invalid="ignore"):
            for j in np.flatnonzero(nis[i] <= GATE2) + 1:
                assert A.reach_sees(reach, x, x, j, geo), (c, j)
        if tag in ("sector_rim", "annulus_rim", "outside", "inner_edge", "match"):
            k = int(c.split(":")[1])
            j = int(sc["dec_ids"][k])
            assert 200.0 <= dist[j - 1] <= 360.0
            assert want[i] == {"sector_rim": 0, "annulus_rim": 0, "outside": -1, "inner_edge": j, "match": j}[tag]
            if kind == "huge":
                continue
            assert not reach["whole_annulus"] and reach["beta"] < 1.0
            if tag == "sector_rim":
                # ... so the deciding landmark lies tens of metres sideways of the observation's ray, within the sector
                side = dist[j - 1] * abs(math.sin(math.atan2(ly[j - 1] - x[1], lx[j - 1] - x[0]) - reach["th"]))
                assert side > 30.0, side
                for t in axes_in_arc:
                    axes_in_arc[t] += A._arc_has(reach["a"], reach["b"], t)
                cut += (reach["a"] < math.pi < reach["b"]) or (reach["a"] < -math.pi < reach["b"])
                half = A.grid_reach(x, sc["P"], z[:, i], geo, beta_scale=0.5)
                half_beta_misses += not A.reach_sees(half, x, x, j, geo)
            if tag in ("annulus_rim", "inner_edge", "match"):
                # looking straight at a landmark on an axis: only the arc test for that axis keeps its cell in the box
                for q in range(4):
                    arcs = [True] * 4
                    arcs[q] = False
                    arc_needed[q] += not A.reach_sees(A.grid_reach(x, sc["P"], z[:, i], geo, arcs=tuple(arcs)), x, x, j, geo)
            if tag == "annulus_rim":
                assert 0.3 < abs(z[0, i] - dist[j - 1]) < reach["rho"]
        elif tag == "unwrapped":
            assert abs(z[1, i]) > math.pi and want[i] > 0
        elif tag == "unwrapped_rim":
            assert want[i] == 0 and abs(reach["th"]) > math.pi
        elif tag == "beyond":
            assert z[0, i] > dist.max() + 100.0 and want[i] == -1
        elif tag == "negative_far":
            assert want[i] == -1 and (kind == "huge" or reach["empty"])
        elif tag == "r_le_rho":
            assert 0.0 < z[0, i] <= reach["rho"] and reach["whole_annulus"] and want[i] == sc["near_id"]
        elif tag == "negative_near":
            assert z[0, i] < 0.0 and not reach["empty"] and want[i] == 0 and nis[i, sc["near_id"] - 1] < GATE2
    if kind == "inside":
        assert {"r_le_rho", "negative_near"} <= seen
        assert all(n >= 1 for n in axes_in_arc.values()), axes_in_arc     # th +- beta contains 0, pi/2, pi and -pi/2
        assert cut >= 2                                                  # ... and straddles the +-pi cut
        assert half_beta_misses >= 2
        assert all(n >= 1 for n in arc_needed), arc_needed               # each arc test is what keeps some landmark in the box
    if kind != "huge":
        # the grid is selective on this scene (restated reach: cells of the box over all cells, averaged over the observations)
        G = geo["G"]
        frac = []
        for i in range(z.shape[1]):
            r = A.grid_reach(x, sc["P"], z[:, i], geo)
            cx0, cx1, cy0, cy1 = r["box"]
            frac.append(0.0 if r["empty"] else (cx1 - cx0 + 1) * (cy1 - cy0 + 1) / (G * G))
        assert np.mean(frac) < 0.15, np.mean(frac)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reach_scene_after_an_update_needs_the_drift_term(dtype):
    """The update of reach_update_inputs moves deciding landmarks TOWARDS the pose by more than the slack of the annulus
    (rho against the true reach), by less than a quarter of a cell (no rebuild): observed on the outer rim afterwards,
    their means at build time lie beyond z0 + rho, inside it only with the drift term."""
    sc = A.reach_scene("inside", dtype)
    xb, Pb = sc["x"], sc["P"]
    zu, ids = A.reach_update_inputs(sc)
    xn, Pn = O.update_sparse(xb, Pb, zu, R, ids)
    xn, Pn = A.round_state(xn, Pn, dtype)
    geo = A.grid_geometry(xb)
    drift = float(np.max(np.abs(xn[3:] - xb[3:])))
    assert 0.1 < drift < 0.25 * min(geo["cwx"], geo["cwy"])
    z, zid = A.reach_rim_after(xn, Pn, sc["dec_ids"])
    assert z.shape[1] >= len(sc["dec_ids"])
    nis, nd = O.association_table_sparse(xn, Pn, z, R)
    assert np.all(O.assoc_vector(nis, nd, GATE1, GATE2) == 0)
    lost = 0
    for i, j in enumerate(zid):
        assert A.reach_sees(A.grid_reach(xn, Pn, z[:, i], geo, drift=drift), xn, xb, int(j), geo)
        lost += not A.reach_sees(A.grid_reach(xn, Pn, z[:, i], geo, drift=drift, use_drift=False), xn, xb, int(j), geo)
    assert lost >= 2, lost


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", A.PARTITION_N)
def test_partition_cells_yield_their_intended_decisions(N, dtype):
    for nz in A.PARTITION_NZ:
        sc = A.partition_cells(N, nz, dtype)
        assert sc["z"].shape == (2, nz) and sc["N"] == N
        assert np.array_equal(sc["want"], sc["intended"]), (N, nz)
        if nz >= 2:
            assert 1 in sc["want"] and N in sc["want"]                   # the first and the last landmark are matched
        if nz >= 9:
            assert {-1, 0} <= set(sc["want"].tolist())


def _literal(sc):
    zf, idf, zn = O.associate(sc["x"], sc["P"], sc["z"], R, GATE1, GATE2)
    zf_o, idf_o, zn_o = O.split_assoc(sc["z"], sc["want"])
    assert np.array_equal(idf, idf_o) and np.array_equal(zf, zf_o) and np.array_equal(zn, zn_o), sc["name"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_literal_scan_agrees_on_every_small_scene(dtype):
    """The oracle's dense, sequential restatement of the reference (every pair through a dense 2 x n Jacobian) against the
    order-independent vector form the GPU tests compare with, on every scene of N <= 130 landmarks: the all-copies scene
    of N = 129 (exact ties) and every partition cell of N <= 129, the ones of 127 .. 257 observations included."""
    small = [A.copies_scene("all_small", dtype)]
    small += [A.partition_cells(N, nz, dtype) for N in A.PARTITION_N if N <= 130 for nz in A.PARTITION_NZ]
    assert len(small) == 1 + 7 * len(A.PARTITION_NZ) and all(sc["N"] <= 130 for sc in small)
    for sc in small:
        _literal(sc)
