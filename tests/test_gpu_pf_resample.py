"""GPU tests of the systematic resampling in every form against the EXACT ancestor table (tests/resample_ref.py: integer
arithmetic on the doubles, decided / undecided slots): depleted weights, one survivor, dead scan blocks, survivors on the
probe rounds' boundaries, and the structural sizes of the kernels.

  (a) the legacy table (slam_pf_ancestors) at the wave, scan-block and multi-block sizes, every scene that fits, the extreme
      offsets; then slam_pf_resample_apply and a download
  (b) shards with first != 0 (slam_pf_ancestors / slam_pf_ancestors_all), 2 and 3 ranks, n_global no multiple of 1024
  (c) depleted weights reached through the real API -- one step with a tight R -- resampled by the auto mode's conditional
      kernels (step_async), the batch entry (step_async_batch) and the synchronous driver (step -> slam_pf_resample_local);
      sizes either side of PF_BOFF_MIN_NB = 192 scan blocks, in the second 1024-block round of the offset hand-over, at
      AUTO_NB_MAX = 2048 blocks and one particle beyond (there the auto step halts and the library resamples through
      slam_pf_resample_local: the same table is expected); three consecutive depleted resamplings with composed tables.

On a decided slot the device must return the exact ancestor; on an undecided one a neighbouring live particle; the table is
non-decreasing, has no dead ancestor, and every particle's copy count lies next to n w / W.  The reference alone decides what
is undecided, and at most max(2, 1e-4 n) slots per scene may be (asserted here and, for the builder scenes, on the CPU).

Largest undecided count per scene, as the reference computes it (CPU, every scene, size and offset used here, both dtypes): 0
for depleted, one_survivor, dead_blocks, edge_survivors, uniform, two_level, and 0 for the float64 oracle's weights of the API
cells; each test prints the count it met on the device's own weights (run with -s).
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR                                          # noqa: E402

pytestmark = pytest.mark.gpu

Q = RR.API_Q
LM4 = np.array([[20.0, 5.0], [-8.0, 15.0]])
SEEN = {}                                                          # scene -> largest number of undecided slots met (reported)


def _note(scene, count):
    SEEN[scene] = max(SEEN.get(scene, 0), int(count))
    print(f"undecided[{scene}] = {count}")


def _distinct_shard(pkg, n, dtype, seed=5):
    """A filter whose particles all differ: jittered landmarks and one predict."""
    sh = pkg.PFShard(n, 2, seed, dtype=dtype)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.init_landmarks(LM4, 0.02, 0.3)
    sh.predict(5.0, 0.0, 4.0, Q, 0.1)
    return sh


def _uniform_logw(lw, n):
    return bool(np.all(lw == lw[0])) and abs(float(lw[0]) + math.log(n)) <= 1e-6 * max(1.0, math.log(n))


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", RR.GPU_SIZES)
def test_legacy_table_against_the_exact_reference(pkg, dtype, n):
    import torch
    sh = _distinct_shard(pkg, n, dtype)
    for name in RR.SCENES:
        if not RR.fits(name, n):
            continue
        sc = RR.scene(name, n, dtype)
        t = torch.from_numpy(sc.logw).to(sh.device)
        for u0 in RR.U0S:
            ex = sc.exact(u0)
            assert ex.n_undecided <= RR.undecided_cap(n)
            anc_t = sh.ancestors(t, sc.gmax, u0)
            anc = anc_t.cpu().numpy()
            ex.check(anc, what=f"{name} n={n} u0={u0}")
            _note(name, ex.n_undecided)
            if name == "uniform":
                assert np.array_equal(anc, np.arange(n))
        pose0, _, lm0 = sh.download()
        sh.resample_apply(anc_t, None, None)                       # (the last offset's table)
        pose1, lw1, lm1 = sh.download()
        assert np.array_equal(pose1, pose0[:, anc]) and np.array_equal(lm1, lm0[:, :, anc]), name
        assert _uniform_logw(lw1, n), name
        sh.predict(5.0, 0.0, 4.0, Q, 0.1)                          # copies become distinct poses again for the next scene
    sh.close()


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("world,per", [(2, 2500), (3, 1667)])
def test_shard_tables_are_slices_of_the_one_rank_table(pkg, dtype, world, per):
    import torch
    n = world * per
    assert n % RR.SCAN_BLOCK != 0
    full = pkg.PFShard(n, 2, 9, dtype=dtype)
    parts = [pkg.PFShard(per, 2, 9, dtype=dtype, first=r * per, n_global=n) for r in range(world)]
    for name in ("depleted", "dead_blocks"):
        sc = RR.scene(name, n, dtype)
        t = torch.from_numpy(sc.logw).to(full.device)
        for u0 in RR.U0S:
            ex = sc.exact(u0)
            one = full.ancestors(t, sc.gmax, u0).cpu().numpy()
            ex.check(one, what=f"{name} one rank u0={u0}")
            got = [h.ancestors(t, sc.gmax, u0).cpu().numpy() for h in parts]
            for r, (h, a) in enumerate(zip(parts, got)):
                ex.check(a, first=h.first, what=f"{name} rank {r} of {world} u0={u0}")
                assert np.array_equal(h.ancestors_all(t, sc.gmax, u0).cpu().numpy(), one), (name, r, u0)
            assert np.array_equal(np.concatenate(got), one), (name, u0)
            _note(name, ex.n_undecided)
    for h in parts + [full]:
        h.close()


# ---- (c) ----------------------------------------------------------------------------------------------------------------
def _keys(pose):
    u = pose.view(np.uint32 if pose.dtype == np.float32 else np.uint64).astype(np.uint64)
    with np.errstate(over="ignore"):
        return (u[0] * np.uint64(0x9E3779B97F4A7C15)) ^ (u[1] * np.uint64(0xC2B2AE3D27D4EB4F)) ^ (u[2] * np.uint64(0x165667B19E3779F9))


def _recover(pose_pre, pose_post):
    """The ancestor table from the resampled poses; asserts that the pre-resampling pose columns are pairwise distinct."""
    key = _keys(pose_pre)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    assert np.all(ks[1:] != ks[:-1]), "pose columns before the resampling are not pairwise distinct"
    pos = np.minimum(np.searchsorted(ks, _keys(pose_post)), ks.shape[0] - 1)
    anc = order[pos]
    assert np.array_equal(pose_post, pose_pre[:, anc]), "a resampled pose is no pose of the filter before the resampling"
    return anc


def _api_filter(pkg, n, dtype, var):
    sh = pkg.PFShard(n, 2, RR.API_SEED, dtype=dtype)
    sh.set_pose([0.0, 0.0, 0.0])
    sh.init_landmarks(RR.API_LM, var, RR.API_JITTER)
    return pkg.FastSLAM(sh, None)


def _step(pkg, f, form, z, ids, R, force):
    V, G, wb, dt = RR.API_CTL
    if form == "auto":
        f.step_async(V, G, wb, Q, dt, z, ids, R, force_resample=force)
        return f.flush()
    if form == "batch":
        f.step_async_batch(pkg.PFShard.prepare_batch([(V, G)], [(z, ids)], [force]), wb, Q, dt, R)
        return f.flush()
    return f.step(V, G, wb, Q, dt, z, ids, R, force_resample=force)


def _check_neff(kind, neff, logw):
    live = int(np.sum(logw.astype(np.float64) - float(logw.max()) > -700.0))
    if kind == "few":
        assert RR.NEFF_FEW[0] <= neff <= RR.NEFF_FEW[1], f"Neff {neff}"
        assert live < 0.05 * logw.shape[0] + 3000, f"{live} particles keep weight"
    else:
        assert neff == pytest.approx(1.0, abs=1e-12) and live == 1, (neff, live)


@pytest.mark.parametrize("kind", ["few", "one"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", RR.API_SIZES)
def test_depleted_step_resampled_by_auto_batch_and_synchronous_forms(pkg, dtype, n, kind):
    var, z, ids, R = RR.api_cell(kind, n)
    u0 = pkg.philox_uniform(0, 2, RR.API_SEED)
    twin = _api_filter(pkg, n, dtype, var)
    neff, did = _step(pkg, twin, "auto", z, ids, R, False)
    assert not did
    pose_pre, logw_pre, lm_pre = twin.shard.download()
    twin.shard.close()
    _check_neff(kind, neff, logw_pre)
    ex = RR.Exact(logw_pre, float(logw_pre.max()), u0)
    assert ex.n_undecided <= RR.undecided_cap(n)
    _note(f"api-{kind}", ex.n_undecided)
    tables, poses = {}, {}
    for form in ("auto", "batch", "sync"):
        f = _api_filter(pkg, n, dtype, var)
        neff_f, did = _step(pkg, f, form, z, ids, R, True)
        assert did and neff_f == pytest.approx(neff, rel=1e-12 if dtype == "f64" else 1e-6), form
        assert f.resamples == 1
        pose, lw, lm = f.shard.download()                          # (materialises the lazy tables)
        f.shard.close()
        anc = _recover(pose_pre, pose)
        ex.check(anc, what=f"{form} n={n} {kind}")
        assert np.array_equal(lm, lm_pre[:, :, anc]), f"{form}: landmark records"
        assert _uniform_logw(lw, n), form
        if kind == "one":
            assert np.all(anc == ex.live[0])
        tables[form], poses[form] = anc, pose
        del lm
    for form in ("batch", "sync"):
        assert np.array_equal(tables[form], tables["auto"]) and np.array_equal(poses[form], poses["auto"]), form


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_consecutive_depleted_resamplings_compose_their_tables(pkg, monkeypatch, dtype):
    """Three forced resamplings on depleted weights, landmarks 1, 2, 2: landmark 1's table is composed twice with tables
    of mostly identical entries before the final download reads through it.  The twins (the first k steps resampled, step
    k + 1 not) gather eagerly (SLAMHIP_PF_EAGER=1), so nothing they hold went through a table."""
    n, kind = 65536 + 77, "few"
    cells = [RR.api_cell(kind, n, step=k) for k in range(3)]
    main = _api_filter(pkg, n, dtype, cells[0][0])
    monkeypatch.setenv("SLAMHIP_PF_EAGER", "1")
    twins = [_api_filter(pkg, n, dtype, cells[0][0]) for _ in range(3)]
    monkeypatch.delenv("SLAMHIP_PF_EAGER", raising=False)
    for k, (_, z, ids, R) in enumerate(cells):
        for j in range(k, 3):
            neff, did = _step(pkg, twins[j], "auto", z, ids, R, j > k)
            assert did == (j > k)
        pose_pre, logw_pre, lm_pre = twins[k].shard.download()
        twins[k].shard.close()
        assert neff <= 0.01 * n, f"step {k}: Neff {neff} is no depleted filter"
        ex = RR.Exact(logw_pre, float(logw_pre.max()), pkg.philox_uniform(k, 2, RR.API_SEED))
        assert ex.n_undecided <= RR.undecided_cap(n)
        _note("api-three-steps", ex.n_undecided)
        _, did = _step(pkg, main, "auto", z, ids, R, True)
        assert did and main.resamples == k + 1
        pose, lw, lm = main.shard.download(landmarks=(k == 2))     # (poses only: the tables stay lazy until the last step)
        anc = _recover(pose_pre, pose)
        ex.check(anc, what=f"step {k}")
        assert _uniform_logw(lw, n)
    assert np.array_equal(lm, lm_pre[:, :, anc]), "landmark records behind the composed tables"
    main.shard.close()
