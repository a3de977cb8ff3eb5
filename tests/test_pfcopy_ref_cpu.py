"""CPU checks of tests/pfcopy_ref.py (the literal model of include/slamhip_pfcopy.h) and of the boundary of the eighth companion
library: ExactInto against resample_ref.Exact and the device-order model, the undecided cap on the cells the GPU test uses, every
mutant of the model caught, the KLD count against hand values, the bins against np.unique, the Julia ccalls and the exports."""
import math
import os

import numpy as np
import pytest

from tests import abi_surface as ABI
from tests import pfcopy_ref as PR
from tests import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slamhip_pfcopy.h")
DTYPES = ("f32", "f64")


def cells():
    return [(name, n) for n in PR.RESIZE_NS for name in RR.SCENES if RR.fits(name, n)]


# ---- ExactInto --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 65, 1025, 2049))
def test_exact_into_equals_exact_at_equal_counts(n):
    for name in RR.SCENES:
        if not RR.fits(name, n):
            continue
        for dt in DTYPES:
            sc = RR.scene(name, n, dt)
            for u0 in RR.U0S:
                a, b = PR.ExactInto(sc.logw, sc.gmax, u0, n), sc.exact(u0)
                assert np.array_equal(a.anc, b.anc) and np.array_equal(a.undecided, b.undecided), (name, n, dt, u0)
                assert np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi) and a.delta == b.delta


@pytest.mark.parametrize("name,n", cells())
def test_undecided_cap_and_the_device_order_model_on_the_gpu_cells(name, n):
    """What tests/test_gpu_pfcopy.py relies on: at most max(2, 1e-4 m) undecided slots per scene, and the device-order model (the
    scan's order of additions, the binary search, the target with m) passes ExactInto.check on every cell."""
    for dt in DTYPES:
        sc = RR.scene(name, n, dt)
        for m in PR.resize_ms(n):
            for u0 in RR.U0S:
                ex = PR.ExactInto(sc.logw, sc.gmax, u0, m)
                assert ex.n_undecided <= PR.undecided_cap(m), (name, n, m, dt, u0, ex.n_undecided)
                assert ex.delta * m < 0.25
                ex.check(PR.model_table(ex.w, u0, m), what=f"{name} n={n} m={m} {dt} u0={u0}")


def test_exact_into_by_hand():
    """Four particles of weights 1, 0, 2, 1 into six slots at u0 = 0.5: targets (q + 0.5) / 6 * 4 = 1/3, 1, 5/3, 7/3, 3, 11/3 against
    the cdf 1, 1, 3, 4: ancestors 0, 0, 2, 2, 2, 3 (the target 1 meets the step exactly: >= takes particle 0; the target 3
    likewise takes particle 2)."""
    w = np.array([1.0, 0.0, 2.0, 1.0])
    ex = PR.ExactInto(None, 0.0, 0.5, 6, w=w)
    assert ex.anc.tolist() == [0, 0, 2, 2, 2, 3]
    assert ex.undecided.tolist() == [False, True, False, False, True, False]   # the two slots whose target meets a step exactly
    assert PR.model_table(w, 0.5, 6).tolist() == [0, 0, 2, 2, 2, 3]
    assert PR.ExactInto(None, 0.0, 0.25, 1, w=w).anc.tolist() == [0] and PR.ExactInto(None, 0.0, 0.26, 1, w=w).anc.tolist() == [2]


def _caught(ex, table):
    try:
        ex.check(table)
    except AssertionError:
        return True
    return False


def test_table_mutants_are_caught():
    """The target formed with n in place of m, and > in place of >=."""
    hit = {"target_with_n": 0, "gt_for_ge": 0}
    for name, n in (("depleted", 1025), ("edge_survivors", 5013), ("two_level", 65), ("uniform", 65)):
        sc = RR.scene(name, n, "f32")
        for m in PR.resize_ms(n):
            ex = PR.ExactInto(sc.logw, sc.gmax, 0.37, m)
            hit["target_with_n"] += _caught(ex, PR.model_table(ex.w, 0.37, m, mutant="target_with_n"))
    # > for >=: a tie that is exact in floating point -- equal weights 2^-k, a dyadic u0 -- must go to the lower particle
    for n, m in ((64, 128), (1024, 64), (65, 1), (4, 2)):
        w = np.full(n, 0.5)
        for u0 in (0.0, 0.5):
            ex = PR.ExactInto(None, 0.0, u0, m, w=w)
            good, bad = PR.model_table(w, u0, m), PR.model_table(w, u0, m, mutant="gt_for_ge")
            assert np.array_equal(good, ex.anc)
            hit["gt_for_ge"] += int(not np.array_equal(bad, ex.anc))
    assert hit["target_with_n"] >= 20 and hit["gt_for_ge"] >= 3, hit


# ---- select / resize -------------------------------------------------------------------------------------------------------------
def _source(n, nl, dt, seed, pend=None):
    rng = np.random.default_rng(seed)
    pose = PR.designed((3, n), dt, seed)
    logw = PR.designed((n,), dt, seed + 1)
    seen = rng.integers(0, 2, nl)
    return PR.scatter(pose, logw, nl, seen, rng, pend=pend, seed=77, step=5, resamples=3, cur=0)


@pytest.mark.parametrize("dt", DTYPES)
def test_select_runs_the_rule(dt):
    src = _source(67, 7, dt, 3)
    plain = src.plain()
    d = PR.select(src, [5, 1, 7], 6, 1)
    assert PR.bits_equal(d["lm"][:3], plain[[4, 0, 6]]) and d["seen"][:3].tolist() == src.seen[[4, 0, 6]].tolist()
    assert np.all(d["lm"][3:, 2] == -1) and not d["lm"][3:, [0, 1, 3, 4]].any() and not d["seen"][3:].any()
    assert PR.bits_equal(d["pose"], src.pose) and PR.bits_equal(d["logw"], src.logw)
    assert (d["seed"], d["step"], d["resamples"]) == (77, 5, 3)
    d0 = PR.select(src, None, 9, 0)
    assert PR.bits_equal(d0["lm"][:7], plain) and not d0["lm"][7:].any()
    # the plain view of a plain source is itself
    flat = PR.LazySource.from_plain(src.pose, src.logw, plain, src.seen)
    assert PR.bits_equal(PR.select(flat, None, 7, 0)["lm"], plain)


def test_pending_shift_is_the_downloaded_value():
    src = _source(65, 2, "f32", 4, pend=0.1)
    want = (src.logw - np.float32(0.1)).astype(np.float32)
    assert PR.bits_equal(PR.select(src, None, 2, 0)["logw"], want) and not PR.bits_equal(want, src.logw)


@pytest.mark.parametrize("dt", DTYPES)
def test_resize_runs_the_rule(dt):
    src = _source(65, 3, dt, 5)
    anc = np.sort(np.random.default_rng(0).integers(0, 65, 131))
    d = PR.resize(src, anc, 4, 0)
    assert PR.bits_equal(d["lm"][:3], src.plain()[:, :, anc]) and not d["lm"][3].any()
    assert PR.bits_equal(d["pose"], src.pose[:, anc])
    assert np.all(d["logw"] == PR.NP_DTYPE[dt](-math.log(131))) and d["resamples"] == 4 and d["step"] == 5 and d["seed"] == 77


def test_gather_and_fill_mutants_are_caught():
    src = _source(67, 7, "f32", 6)
    assert (src.ltab >= 0).any() and (src.lbuf != src.cur).any()         # the scene has records behind tables and in the other buffer
    good = PR.select(src, None, 9, 1)
    for mutant in ("table_ignored", "buffer_cur_only", "fill_swapped"):
        assert not PR.bits_equal(PR.select(src, None, 9, 1, mutant=mutant)["lm"], good["lm"]), mutant
        anc = np.arange(67)[::-1].copy()
        assert not PR.bits_equal(PR.resize(src, anc, 9, 1, mutant=mutant)["lm"], PR.resize(src, anc, 9, 1)["lm"]), mutant
    assert set(PR.MUTANTS) == {"target_with_n", "gt_for_ge", "table_ignored", "buffer_cur_only", "fill_swapped"}


def test_designed_values_hold_the_special_cases():
    for dt in DTYPES:
        a = PR.designed((3, 65), dt, 1).reshape(-1)
        tiny = np.finfo(a.dtype).tiny
        assert np.any((a == 0) & np.signbit(a)) and np.any((a != 0) & (np.abs(a) < tiny)) and np.all(np.isfinite(a))
        assert np.unique(a.view(np.uint32 if dt == "f32" else np.uint64)).size == a.size
        assert not PR.bits_equal(np.zeros(1, a.dtype), -np.zeros(1, a.dtype))


# ---- bins and the KLD count --------------------------------------------------------------------------------------------------
def test_pose_bins_against_unique_and_by_hand():
    pose = np.array([[0.0, 0.49, 0.5, -0.01, -0.5, 0.0],
                     [0.0, 0.0, 0.0, 0.0, -0.51, 0.0],
                     [0.0, 0.1, 0.0, 0.0, 0.0, math.pi]])
    keys = PR.pose_keys(pose, 0.5, math.pi / 2)
    # phi = pi falls into cell 4 of 4 and is clamped to 3; -0.01 / 0.5 floors to -1, -0.51 / 0.5 to -2
    assert keys.tolist() == [[0, 0, 2], [0, 0, 2], [1, 0, 2], [-1, 0, 2], [-1, -2, 2], [0, 0, 3]]
    assert PR.pose_bins(pose, 0.5, math.pi / 2) == 5
    rng = np.random.default_rng(1)
    p = np.vstack([rng.normal(0, 3, (2, 5013)), rng.uniform(-math.pi, math.pi, (1, 5013))]).astype(np.float32)
    k = PR.pose_keys(p, 0.25, 0.1)
    assert PR.pose_bins(p, 0.25, 0.1) == len({tuple(r) for r in k.tolist()})
    for bad in (np.array([[2.0 ** 20 * 0.5], [0.0], [0.0]]), np.array([[0.0], [-2.0 ** 19 - 0.5], [0.0]]), np.array([[np.nan], [0.0], [0.0]]),
                np.array([[0.0], [0.0], [np.inf]])):
        with pytest.raises(ValueError):
            PR.pose_bins(bad, 0.5, 0.1)
    assert PR.pose_bins(np.array([[-2.0 ** 19 + 0.5], [0.0], [0.0]]), 0.5, 0.1) == 1       # ix = -2^20 + 1: the last cell inside
    with pytest.raises(ValueError):
        PR.pose_bins(pose, 0.0, 0.1)


def test_kld_count_by_hand(pkg):
    """k = 2: a = 2/9, (1 - 2/9 + sqrt(2/9) 2.326)^3 = 1.874286^3 = 6.58428, times 1 / 0.1: 65.8 -> 66.  k = 100, eps = 0.05,
    z = 2.326: a = 2 / 891, 1 - a + sqrt(a) z = 1.107954, cubed 1.360094, times 990: 1346.49 -> 1347.  k = 11, eps = 0.1,
    z = 1.645: a = 1/45, 1 - a + 0.149071 * 1.645 = 1.223000, cubed 1.829276, times 50: 91.46 -> 92."""
    for f in (pkg.kld_particle_count, PR.kld_count):
        assert f(2, n_min=1) == 66 and f(100, n_min=1) == 1347 and f(11, eps=0.1, z=1.645, n_min=1) == 92
        assert f(0, n_min=17) == 17 and f(1, n_min=17) == 17 and f(2, n_min=100) == 100 and f(100, n_min=1, n_max=1000) == 1000
    for k in (2, 3, 10, 1000, 12345):
        assert pkg.kld_particle_count(k) == PR.kld_count(k)


# ---- the boundary of the eighth companion library -----------------------------------------------------------------------------------
def test_the_library_exports_exactly_what_its_header_declares(pkg):
    """Seven entry points.  (That the header, the library, the ctypes table and the Julia binding name the same symbols, that the
    library needs neither torch nor python and that the product library has none of the names: tests/test_companions_cpu.py.)"""
    assert ABI.declared(HEADER) == set(pkg._lib.PFCOPY_SIGNATURES) and len(ABI.declared(HEADER)) == 7


def test_bad_arguments_are_status_codes(pkg):
    lib = pkg._lib.pfcopy_lib()
    E = pkg._lib.SLAM_E_BADARG
    assert lib.slam_pf_copy(None, None, 0) == E and lib.slam_pf_select(None, None, None, 0, 0) == E
    assert lib.slam_pf_resize(None, None, 0.0, 0.5, 0, None) == E and lib.slam_pf_upload(None, None, None, None, None) == E
    assert lib.slam_pf_get_meta(None, None, None) == E and lib.slam_pf_set_rng(None, 0, 0) == E
    assert lib.slam_pf_pose_bins(None, 1.0, 1.0, None) == E


def test_julia_binding_of_the_new_library(pkg):
    """(Every ccall's name, return type and number of argument types: tests/test_companions_cpu.py.)"""
    src = open(os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")).read()
    assert len(ABI.julia_ccalls("libslamhip_pfcopy")) >= 7
    for word in ("upload!", "resize", "pose_bins", "kld_particle_count", "reserve!(s::PFSlamState", "Base.copy!(dst::PFSlamState", "select(s::PFSlamState"):
        assert word in src, word
