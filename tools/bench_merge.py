#!/usr/bin/env python3
"""Time of slam_ekf_find_duplicates and slam_ekf_merge_landmarks (csrc/ekf_merge.hip).

    python tools/bench_merge.py [--runs 5] [--n-find 10000,50000] [--n-merge 10000] [--out profiles/ekf_merge_bench.txt]

fp32, each figure the median over --runs runs after one warm-up, wall clock around the synchronising calls:
  find      at every N of --n-find with 0, 8 and 64 duplicates planted (landmark b moved onto landmark a); beside the time the
            number of pairs the cheap bound keeps -- the only pairs whose cross blocks are read -- counted on the host with the
            kernel's own inequality from the downloaded means and diagonal blocks (the library has no hook that returns it)
  merge     of 1 and of 8 pairs at --n-merge, the state uploaded again before every run, against
            (i)  an ordinary 8-observation update on the same state (one down-date pass) and a removal of 8 landmarks,
            (ii) the host round trip: get_state, the fusion in NumPy, set_state.
The find states are built on the device (torch) and handed over with set_state_device: no host buffer holds the 40 GB of a
dense fp32 matrix at N = 50 000; the merge state (N = 10 000, 1.6 GB) is uploaded from the host before every run.
One JSON line per measurement; the same lines go to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package                      # noqa: E402

pkg = load_package()
GATE = 9.0
R = np.array([[0.1 ** 2, 0.0], [0.0, (np.pi / 180) ** 2]])


def make_state(rng, N):
    """Means on a jittered 5 m grid, covariance = rank 4 + diagonal (fp32)."""
    n = 3 + 2 * N
    side = int(np.ceil(np.sqrt(N)))
    cells = rng.permutation(side * side)[:N]
    x = np.zeros(n, dtype=np.float32)
    x[:3] = [2.5 * side, 2.5 * side, 0.3]
    x[3::2] = 5.0 * (cells % side) + rng.uniform(-0.5, 0.5, N)
    x[4::2] = 5.0 * (cells // side) + rng.uniform(-0.5, 0.5, N)
    A = rng.normal(0, 0.05, (n, 4)).astype(np.float32)
    P = A @ A.T
    P[np.diag_indices(n)] += np.float32(0.01)
    return x, np.maximum(P, P.T)


def survivors(x, blocks, gate, chunk=2048):
    """Pairs a < b with |delta|^2 < 2 gate (tr P_aa + tr P_bb): what the kernel's first test keeps."""
    m = x[3:].astype(np.float64).reshape(-1, 2)
    g = 2.0 * gate * (blocks[0].astype(np.float64) + blocks[2].astype(np.float64))
    N, total = len(g), 0
    for a0 in range(0, N, chunk):
        a1 = min(N, a0 + chunk)
        d2 = (m[a0:a1, None, 0] - m[None, :, 0]) ** 2 + (m[a0:a1, None, 1] - m[None, :, 1]) ** 2
        keep = d2 < g[a0:a1, None] + g[None, :]
        keep &= np.arange(a0, a1)[:, None] < np.arange(N)[None, :]
        total += int(keep.sum())
    return total


def wall(fn, runs, before=None):
    ts = []
    for k in range(runs + 1):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if k:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def bench_find(N, runs, emit):
    """The state is built ON THE DEVICE (torch) and handed over with set_state_device: at N = 50 000 the dense fp32 matrix is
    40 GB, which no host buffer should have to hold."""
    import torch
    rng = np.random.default_rng(2024)
    n = 3 + 2 * N
    side = int(np.ceil(np.sqrt(N)))
    cells = rng.permutation(side * side)[:N]
    x = np.zeros(n, dtype=np.float32)
    x[:3] = [2.5 * side, 2.5 * side, 0.3]
    x[3::2] = 5.0 * (cells % side) + rng.uniform(-0.5, 0.5, N)
    x[4::2] = 5.0 * (cells // side) + rng.uniform(-0.5, 0.5, N)
    gen = torch.Generator(device="cuda").manual_seed(2024)
    A = torch.randn(n, 4, device="cuda", generator=gen) * 0.05
    Pt = A @ A.T
    Pt.diagonal().add_(0.01)
    st = pkg.EKFSlamState(x[:5], np.eye(5, dtype=np.float32), dtype="f32", max_landmarks=N)
    order = rng.permutation(np.arange(1, N + 1))
    for planted in (0, 8, 64):
        x2 = x.copy()
        for a, b in order[:2 * planted].reshape(planted, 2):
            x2[3 + 2 * (b - 1):5 + 2 * (b - 1)] = x2[3 + 2 * (a - 1):5 + 2 * (a - 1)] + np.float32(0.02)
        xt = torch.from_numpy(x2).cuda()
        torch.cuda.synchronize()
        st.set_state_device(xt.data_ptr(), Pt.data_ptr(), n, n)
        count = [0]

        def run():
            count[0] = st.find_duplicates(GATE, cap=4096)[1]

        med, lo, hi = wall(run, runs)
        surv = survivors(st.download("x"), st.landmark_blocks(), GATE)
        emit({"what": "find", "dtype": "f32", "N": N, "planted": planted, "found": count[0], "pairs": N * (N - 1) // 2,
              "survivors_of_the_cheap_bound": surv, "cross_block_bytes_read": surv * 16, "stored_matrix_bytes": int(2 * N + 3) ** 2 * 2,
              "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "runs": runs})
    st.close()
    del Pt


def numpy_fusion(x, P, pairs):
    """The host path: the same update with dense rows, then the deletion (float64 on the host)."""
    x = x.astype(np.float64)
    k = 2 * len(pairs)
    PHt = np.zeros((len(x), k))
    for p, (a, b) in enumerate(pairs):
        fa, fb = 3 + 2 * (a - 1), 3 + 2 * (b - 1)
        PHt[:, 2 * p:2 * p + 2] = P[:, fa:fa + 2].astype(np.float64) - P[:, fb:fb + 2]
    rows = np.concatenate([[3 + 2 * (a - 1), 4 + 2 * (a - 1)] for a, _ in pairs])
    rowsb = np.concatenate([[3 + 2 * (b - 1), 4 + 2 * (b - 1)] for _, b in pairs])
    S = PHt[rows] - PHt[rowsb]
    v = -(x[rows] - x[rowsb])
    W = PHt @ np.linalg.inv((S + S.T) / 2)
    x = x + W @ v
    P -= (W @ PHt.T).astype(P.dtype)
    keep = np.delete(np.arange(len(x)), rowsb)
    return x[keep].astype(np.float32), P[np.ix_(keep, keep)]


def bench_merge(N, runs, emit):
    rng = np.random.default_rng(77)
    x, P = make_state(rng, N)
    order = rng.permutation(np.arange(1, N + 1))
    pairs8 = order[:16].reshape(8, 2)
    for a, b in pairs8:
        x[3 + 2 * (b - 1):5 + 2 * (b - 1)] = x[3 + 2 * (a - 1):5 + 2 * (a - 1)] + np.float32(0.05)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
    upload = lambda: (st.set_state(x, P), st.sync())             # noqa: E731
    floor_ms, _form = st.copy_floor(5)
    emit({"what": "copy_floor", "dtype": "f32", "N": N, "ms": round(floor_ms, 4)})
    for cnt in (1, 8):
        med, lo, hi = wall(lambda: st.merge_landmarks(pairs8[:cnt]), runs, before=upload)
        emit({"what": "merge", "dtype": "f32", "N": N, "pairs": cnt, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "runs": runs})
    ids = order[100:108]
    z = np.zeros((2, 8))
    for i, j in enumerate(ids):
        dx, dy = x[3 + 2 * (j - 1)] - x[0], x[4 + 2 * (j - 1)] - x[1]
        z[:, i] = [np.hypot(dx, dy), np.arctan2(dy, dx) - x[2]]
    med, lo, hi = wall(lambda: st.update(z, R, ids.reshape(1, -1)), runs, before=upload)
    emit({"what": "update of 8 observations", "dtype": "f32", "N": N, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "runs": runs})
    med, lo, hi = wall(lambda: st.remove_landmarks(pairs8[:, 1]), runs, before=upload)
    emit({"what": "removal of 8 landmarks", "dtype": "f32", "N": N, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "runs": runs})

    def host():
        xd, Pd = st.download()
        xn, Pn = numpy_fusion(xd, Pd, pairs8)
        st.set_state(xn, Pn)
        st.sync()

    med, lo, hi = wall(host, min(runs, 2), before=upload)
    emit({"what": "host round trip (get_state, NumPy fusion of 8 pairs, set_state)", "dtype": "f32", "N": N, "ms_median": round(med, 1),
          "ms_min": round(lo, 1), "ms_max": round(hi, 1), "runs": min(runs, 2)})
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n-find", default="10000,50000")
    ap.add_argument("--n-merge", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ekf_merge_bench.txt"))
    a = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        with open(a.out, "w") as f:                               # rewritten after every figure: a cut-short run keeps what it has
            f.write("# tools/bench_merge.py: wall-clock milliseconds around the synchronising calls, fp32\n" + "\n".join(lines) + "\n")

    for N in [int(v) for v in a.n_find.split(",") if v]:
        bench_find(N, a.runs, emit)
    if a.n_merge:
        bench_merge(a.n_merge, a.runs, emit)


if __name__ == "__main__":
    main()
