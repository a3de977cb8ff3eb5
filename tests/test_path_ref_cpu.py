"""CPU tests of tests/path_ref.py, the NumPy restatement of the per-particle trajectory history (include/slamhip_path.h): known
answers written out by hand, the composition of resamplings, the ring, the circular mean -- and the declarations the host layers
bind, and the property the mean kernel's memory access leans on (systematic resampling yields non-decreasing ancestors)."""
import math
import os
import re

import numpy as np
import pytest

import path_ref as PR
import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poses(r, n=4):
    """Record r: particle p at x = 10 r + p, y = -p, phi = 0.1 p."""
    p = np.arange(n, dtype=np.float64)
    return np.vstack([10.0 * r + p, -p, 0.1 * p])


def _xs(path):
    return path[..., 0].tolist()


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_four_particles_three_records_by_hand():
    """record, resample [0, 0, 2, 3], record, resample [1, 1, 1, 3], record.  By hand: the current particles 0 1 2 3 sit at
    1 1 1 3 at record 1 (the second map) and at 0 0 0 3 at record 0 (the first map applied to that)."""
    ref = PR.PathRef(4, 8)
    ref.record(_poses(0))
    ref.resample([0, 0, 2, 3])
    ref.record(_poses(1))
    ref.resample([1, 1, 1, 3])
    ref.record(_poses(2))
    assert ref.indices().tolist() == [[0, 0, 0, 3], [1, 1, 1, 3], [0, 1, 2, 3]]
    tr = ref.trace([0, 1, 2, 3])
    assert tr.shape == (4, 3, 3)
    assert _xs(tr) == [[0.0, 11.0, 20.0], [0.0, 11.0, 21.0], [0.0, 11.0, 22.0], [3.0, 13.0, 23.0]]
    assert tr[2, :, 1].tolist() == [0.0, -1.0, -2.0] and tr[3, :, 2].tolist() == pytest.approx([0.3, 0.3, 0.3])
    assert ref.survivors().tolist() == [2, 2, 4]
    assert ref.info() == dict(L=3, records=3, cap=8, resamples=2)
    # the slots: record 0 has no ancestors, records 1 and 2 the maps as they were given
    assert ref.get(2)[2] is False and ref.get(2)[1].tolist() == [0, 1, 2, 3]
    assert ref.get(1)[2] is True and ref.get(1)[1].tolist() == [0, 0, 2, 3]
    assert ref.get(0)[2] is True and ref.get(0)[1].tolist() == [1, 1, 1, 3]
    # the best particle: the largest log-weight, the lowest index on a tie, NaN never
    b, path = ref.best([-1.0, float("nan"), -0.5, -0.5])
    assert b == 2 and _xs(path) == [0.0, 11.0, 22.0]
    assert PR.PathRef.best_index([float("nan")] * 3) == 0


def test_two_resamplings_between_two_records_compose():
    ref = PR.PathRef(4, 8)
    ref.record(_poses(0))
    ref.resample([0, 0, 2, 3])
    ref.resample([1, 1, 1, 3])                     # particle p now descends from a1[a2[p]]
    assert ref.pending.tolist() == [0, 0, 0, 3]
    ref.record(_poses(1))
    assert ref.get(0)[1].tolist() == [0, 0, 0, 3] and ref.pending is None
    assert _xs(ref.trace([0, 1, 2, 3])) == [[0.0, 10.0], [0.0, 11.0], [0.0, 12.0], [3.0, 13.0]]
    assert ref.survivors().tolist() == [2, 4]


def test_no_resampling_is_the_identity_everywhere():
    ref = PR.PathRef(4, 8)
    for r in range(3):
        ref.record(_poses(r))
    assert all(not ref.get(k)[2] for k in range(3))
    assert ref.survivors().tolist() == [4, 4, 4]
    assert _xs(ref.trace([3])) == [[3.0, 13.0, 23.0]]


def test_resampling_before_the_first_record_and_after_the_last():
    """Before the first record the map is held pending and lands in the first slot, where no read-out applies it (nothing lies
    further back).  After the last record it is pending only: the trace shows it, no slot does."""
    ref = PR.PathRef(4, 8)
    ref.resample([2, 2, 0, 1])
    assert ref.pending.tolist() == [2, 2, 0, 1] and ref.L == 0
    ref.record(_poses(0))
    assert ref.get(0)[2] is True and ref.get(0)[1].tolist() == [2, 2, 0, 1]
    assert _xs(ref.trace([0, 1, 2, 3])) == [[0.0], [1.0], [2.0], [3.0]] and ref.survivors().tolist() == [4]
    ref.record(_poses(1))
    ref.resample([3, 3, 1, 3])
    assert _xs(ref.trace([0, 1, 2, 3])) == [[3.0, 13.0], [3.0, 13.0], [1.0, 11.0], [3.0, 13.0]]
    assert ref.survivors().tolist() == [2, 2]
    assert ref.get(0)[2] is False and ref.get(1)[1].tolist() == [2, 2, 0, 1]      # the slots are what they were
    ref.resample([2, 2, 2, 2])                                                    # composes with the pending one
    assert _xs(ref.trace([0, 3])) == [[1.0, 11.0], [1.0, 11.0]] and ref.survivors().tolist() == [1, 1]


def test_ring_wraps_at_cap_two_and_cap_one():
    ref = PR.PathRef(4, 2)
    ref.record(_poses(0))
    ref.resample([0, 0, 2, 3])
    ref.record(_poses(1))
    ref.resample([1, 1, 1, 3])
    ref.record(_poses(2))                            # record 0 is gone
    assert ref.info() == dict(L=2, records=3, cap=2, resamples=2)
    assert _xs(ref.trace([0, 1, 2, 3])) == [[11.0, 20.0], [11.0, 21.0], [11.0, 22.0], [13.0, 23.0]]
    assert ref.survivors().tolist() == [2, 4]
    assert ref.get(1)[1].tolist() == [0, 0, 2, 3]    # the oldest held slot keeps its map; it is never applied
    one = PR.PathRef(4, 1)
    one.record(_poses(0))
    one.resample([0, 0, 2, 3])
    one.record(_poses(1))
    one.resample([1, 1, 1, 3])
    assert one.L == 1 and _xs(one.trace([0, 1, 2, 3])) == [[11.0], [11.0], [11.0], [13.0]]
    assert one.survivors().tolist() == [2]


def test_mean_is_weighted_and_circular():
    """Headings either side of +-pi: pi - 0.1 and -pi + 0.2 with equal weights have the mean direction pi + 0.05 = -pi + 0.05,
    not 0.05 (their arithmetic mean); R = cos(0.15)."""
    ref = PR.PathRef(2, 4)
    ref.record(np.array([[1.0, 3.0], [0.0, 8.0], [math.pi - 0.1, -math.pi + 0.2]]))
    out, detail = ref.mean([-2.0, -2.0])
    assert out[0, 0] == 2.0 and out[0, 1] == 4.0
    assert abs(out[0, 2] - (-math.pi + 0.05)) < 1e-14 and abs(out[0, 3] - math.cos(0.15)) < 1e-14
    # weights 3 : 1 through the log-weights, and through an ancestor map
    ref.resample([1, 1])
    ref.record(np.array([[5.0, 9.0], [1.0, 1.0], [0.0, 0.0]]))
    out, _ = ref.mean([math.log(3.0), 0.0])
    assert out[:, 0] == pytest.approx([3.0, 6.0]) and out[:, 1] == pytest.approx([8.0, 1.0])      # record 0: both at particle 1
    assert out[0, 2] == pytest.approx(-math.pi + 0.2) and out[0, 3] == pytest.approx(1.0)
    b = PR.mean_bounds(2, detail)
    assert b[0]["x"] == 18 * 2.0 ** -52 * 2.0 and b[0]["phi"] == pytest.approx((b[0]["S"] + b[0]["C"]) / math.cos(0.15))


def test_recover_ancestors_needs_distinct_poses():
    pre = np.array([[0.0, 1.0, 2.0], [5.0, 5.0, 5.0], [0.1, 0.1, 0.1]])
    assert PR.recover_ancestors(pre, pre[:, [2, 2, 0]]).tolist() == [2, 2, 0]
    with pytest.raises(AssertionError):
        PR.recover_ancestors(pre[:, [0, 0, 1]], pre)


# ---- the property the mean kernel's gathers lean on -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depleted", "uniform"])
@pytest.mark.parametrize("n", [65, 1025, 5000])
def test_systematic_resampling_yields_non_decreasing_ancestors(name, n):
    """The exact table and both device-order models, at the three offsets; and a composition of non-decreasing maps is
    non-decreasing (what a slot's ancestor array is after several resamplings)."""
    sc = RR.scene(name, n, "f32")                  # (asserts that the scene has a meaning at this size)
    tables = []
    for u0 in RR.U0S:
        tables.append(np.asarray(sc.exact(u0).anc, dtype=np.int64))
        tables.extend(np.asarray(t, dtype=np.int64) for t in RR.model_tables(sc.logw, sc.gmax, u0))
    for t in tables:
        assert t.shape == (n,) and t.min() >= 0 and t.max() < n and np.all(np.diff(t) >= 0)
    comp = tables[0][tables[3]][tables[6]]
    assert np.all(np.diff(comp) >= 0)
    if name == "uniform":
        assert all(np.array_equal(t, np.arange(n)) for t in tables)


# ---- the declarations the host layers bind -------------------------------------------------------------------------------------
NAMES = {"slam_pf_path_create", "slam_pf_path_destroy", "slam_pf_path_record", "slam_pf_path_resample", "slam_pf_path_info",
         "slam_pf_path_get", "slam_pf_path_trace", "slam_pf_path_best", "slam_pf_path_mean", "slam_pf_path_survivors"}


def test_header_python_and_julia_name_the_same_symbols(pkg):
    """(That the header, the library, this table and the Julia binding name the same symbols: tests/test_companions_cpu.py.)"""
    assert set(pkg._lib.PATH_SIGNATURES) == NAMES
    with open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")) as f:
        src = f.read()
    for word in ("PathHistory", "record!", "resample!", "trace", "best_path", "mean_path", "survivors"):
        assert re.search(r"^export[^#]*?\b" + re.escape(word), src, flags=re.S | re.M), word
    assert callable(pkg.PathHistory) and callable(pkg.FastSLAM.track_path)
    assert callable(pkg.PFSlamState.path) and callable(pkg.PFSlamState.mean_path)
    for method in ("record", "resample", "info", "get", "trace", "best", "mean", "survivors", "close"):
        assert callable(getattr(pkg.PathHistory, method))


def test_null_arguments_are_status_codes(pkg):
    lib = pkg._lib.path_lib()
    BAD = pkg._lib.SLAM_E_BADARG
    assert lib.slam_pf_path_create(None, None, 4) == BAD
    assert lib.slam_pf_path_destroy(None) == BAD
    assert lib.slam_pf_path_record(None) == BAD
    assert "null path object" in pkg._lib.last_error()
    assert lib.slam_pf_path_resample(None, 0.0, 0.5) == BAD
    assert lib.slam_pf_path_info(None, None) == BAD
    assert lib.slam_pf_path_get(None, 0, None, None, None) == BAD
    assert lib.slam_pf_path_trace(None, None, 1, None) == BAD
    assert lib.slam_pf_path_best(None, None, None) == BAD
    assert lib.slam_pf_path_mean(None, None) == BAD
    assert lib.slam_pf_path_survivors(None, None) == BAD


def test_the_sim_log_has_room_for_the_best_path(pkg):
    log = pkg.sim.SimLog()
    assert log.best_path is None
