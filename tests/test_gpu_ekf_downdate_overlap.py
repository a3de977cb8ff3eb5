"""The split-bf16 down-date's LDS-DMA pipeline with two fragment register sets (csrc/ekf_syrk.hip: dd_stream_dma_ovl): in
the steps 0 .. nch - 3 of a tile the fragment reads of chunk c + 1 are issued in front of the MFMAs of chunk c, the P tile is
requested at step nch - 2 and the last two steps run with one set.  The buffers, the requests, the products and their order
are those of the one-set schedule, so the covariance must be the same BITS as

  * the register-staged pipeline (SLAMHIP_X=512), computed once in a fresh child process for every case below, and
  * the one-set LDS-DMA schedule kept behind SLAMHIP_X bit 65536,

at every chunk count nch = 5 .. 8 (matched counts m = 40, 48, 56, 64: every position of the peeled steps), with a ragged last
chunk (m = 41, 63), over three consecutive updates (a chunk read before it landed, or a buffer refilled before every wave had
read it, is a wrong P), at two map sizes: N = 300 (n = 603, five tile rows, ten off-diagonal tiles: no workgroup has more than
one, the first-tile and last-tile wait counts at once) and N = 2600 (n = 5203, 41 tile rows, 820 off-diagonal tiles for 512
workgroups: some stream two tiles, some one -- the counts with the previous tile's stores in the queue, the first tile's and
the last tile's).  The whole state is compared: a SHA-256 over the bytes of the mean and of the full covariance.

Run as a script (`python tests/test_gpu_ekf_downdate_overlap.py OUT.json`) the module computes those digests for every case
under the SLAMHIP_X of its environment: that is the child process.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ekf_ref as O                                                            # noqa: E402
from tests.test_gpu_ekf import R, noisy_obs, random_state, relerr, relerr_cov, rounded     # noqa: E402

MATCHED = (40, 48, 56, 64, 41, 63)          # k = 2 m = 80, 96, 112, 128 (nch = 5, 6, 7, 8); 82 -> nch 6 and 126 -> nch 8, ragged
SIZES = (300, 2600)
CASES = [(m, N) for N in SIZES for m in MATCHED]
FALLBACK_BIT = 65536                        # the LDS-DMA pipeline with one fragment set


def run_case(pkg, m, N):
    """Three updates of m matched landmarks each on a fresh fp32 state of N landmarks (Cholesky form); the state as downloaded."""
    rng = np.random.default_rng(7000 + 10 * m + N)
    x, P = random_state(rng, N, spread=400.0 if N < 1000 else 1200.0)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
    r2 = np.random.default_rng(17)
    for _ in range(3):
        xo = st.download("x").astype(np.float64)
        ids = r2.permutation(N)[:m] + 1
        st.update(noisy_obs(r2, xo, ids), R, ids)
    xg, Pg = st.download()
    st.close()
    return np.ascontiguousarray(xg), np.ascontiguousarray(Pg)


def digest(xg, Pg):
    h = hashlib.sha256()
    h.update(str((xg.dtype, xg.shape, Pg.dtype, Pg.shape)).encode())
    h.update(xg.tobytes())
    h.update(Pg.tobytes())
    return h.hexdigest()


def _with_flag(monkeypatch, flag):
    if flag:
        monkeypatch.setenv("SLAMHIP_X", str(flag))          # (read when a handle is created)
    else:
        monkeypatch.delenv("SLAMHIP_X", raising=False)


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """{(m, N): digest} of the register-staged pipeline, one child process for all cases."""
    out = tmp_path_factory.mktemp("downdate_overlap") / "staged.json"
    env = dict(os.environ, SLAMHIP_X="512")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = json.loads(out.read_text())
    assert got["SLAMHIP_X"] == "512"
    return {tuple(int(v) for v in k.split(",")): d for k, d in got["digests"].items()}


@pytest.fixture(scope="module")
def default_runs():
    """{(m, N): digest} of the default schedule, computed once per case and shared by the tests below."""
    return {}


def _default_digest(pkg, monkeypatch, cache, m, N):
    if (m, N) not in cache:
        _with_flag(monkeypatch, None)
        xg, Pg = run_case(pkg, m, N)
        assert np.array_equal(Pg, Pg.T)
        assert np.isfinite(Pg).all() and np.isfinite(xg).all()
        cache[(m, N)] = digest(xg, Pg)
    return cache[(m, N)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,N", CASES)
def test_two_fragment_sets_against_the_register_staged_pipeline(pkg, monkeypatch, staged, default_runs, m, N):
    assert _default_digest(pkg, monkeypatch, default_runs, m, N) == staged[(m, N)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,N", CASES)
def test_one_set_schedule_behind_the_fallback_bit(pkg, monkeypatch, default_runs, m, N):
    ovl = _default_digest(pkg, monkeypatch, default_runs, m, N)
    _with_flag(monkeypatch, FALLBACK_BIT)
    xg, Pg = run_case(pkg, m, N)
    _with_flag(monkeypatch, None)
    assert digest(xg, Pg) == ovl


@pytest.mark.gpu
def test_two_fragment_sets_against_the_fp64_oracle(pkg, monkeypatch):
    """N = 300, m = 56 (nch = 7), one update, against the fp64 oracle on the state as the device holds it, with the bounds of
    tests/test_gpu_ekf.py::test_split_bf16_downdate_against_the_fp32_matrix_cores: inside the fp32 tolerance (5e-6 of the
    entries' scale), rms error at most 1.1 x and max error at most 1.5 x those of the fp32 matrix cores (SLAMHIP_X=8) on the same
    state."""
    m, N = 56, 300
    rng = np.random.default_rng(100 + m)
    x, P = random_state(rng, N, spread=400.0)
    ids = rng.permutation(N)[:m] + 1
    got = {}
    for name, flag in (("ovl", None), ("fp32", 8)):
        _with_flag(monkeypatch, flag)
        st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
        xo, Po = rounded(st)
        z = noisy_obs(np.random.default_rng(7), xo, ids)
        st.update(z, R, ids)
        got[name] = st.download()
        st.close()
    _with_flag(monkeypatch, None)
    xn, Pn = O.update_sparse(xo, Po, z, R, ids)
    err = {}
    for name, (xg, Pg) in got.items():
        assert relerr(xg, xn) <= 5e-6, name
        d = np.asarray(Pg, dtype=np.float64) - Pn
        err[name] = (float(np.abs(d).max()), float(np.sqrt((d * d).mean())))
        assert relerr_cov(Pg, Pn, np.diag(Po)) <= 5e-6, name
        assert np.array_equal(Pg, Pg.T)
    print(f"P error vs fp64 (max, rms): two fragment sets {err['ovl']}, fp32 matrix cores {err['fp32']}")
    assert not np.array_equal(got["ovl"][1], got["fp32"][1])                 # the split path did run
    assert err["ovl"][1] <= 1.1 * err["fp32"][1], err
    assert err["ovl"][0] <= 1.5 * err["fp32"][0], err


if __name__ == "__main__":
    from __graft_entry__ import load_package
    package = load_package()
    digests = {f"{m},{N}": digest(*run_case(package, m, N)) for m, N in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump({"SLAMHIP_X": os.environ.get("SLAMHIP_X", ""), "digests": digests}, f)
