#!/usr/bin/env python3
"""Time of slam_ekf_transform (csrc/ekf_transform.hip) against the copy floor and the host round trip, and of
slam_pf_transform (csrc/pf_transform.hip) against its algorithmic bytes.

    python tools/bench_transform.py [--runs 25] [--n32 10000] [--n64 10000] [--pf-n 262144] [--pf-nl 512] [--no-host]

Per EKF shape (fp32 N = --n32, fp64 N = --n64; 0 skips one):
  t_transform  slam_ekf_transform with theta != 0 (the pass over P runs), wall clock around a sync, median of --runs after a warm-up
  floor        slam_ekf_copy_floor of the same handle in the same run (one read + one write of the stored tiles)
  t_host       download, NumPy (T P T' blockwise), set_state: what the library offered before (wall clock, median of 3)
The figure to compare across boxes is t_transform / floor.  FastSLAM (fp32, --pf-n particles x --pf-nl landmarks, every record in
use): t against (40 B per record + 24 B per pose) read + written.  One JSON line per shape at the end."""
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


def make_state(rng, N, npdt):
    n = 3 + 2 * N
    x = rng.uniform(0, 1000, n).astype(npdt)
    A = rng.normal(0, 0.05, (n, 4)).astype(npdt)
    P = A @ A.T
    P[np.diag_indices(n)] += npdt(0.01)
    return x, np.maximum(P, P.T)


def wall_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def host_transform(st, tx, ty, theta):
    x, P = st.download()
    c, s = np.cos(theta), np.sin(theta)
    a = np.concatenate([[0], np.arange(3, x.shape[0], 2)])    # first index of every pair
    b = a + 1

    def rot(M):                                               # the pairs' rows of M
        u, v = M[a], M[b]
        M[a], M[b] = c * u - s * v, s * u + c * v
    rot(P)
    P = np.ascontiguousarray(P.T)
    rot(P)
    xx = x.astype(np.float64)
    rot(xx)
    xx[a] += tx
    xx[b] += ty
    st.set_state(xx.astype(x.dtype), P.astype(x.dtype))


def bench_ekf(dtype, N, runs, with_host):
    npdt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(12345)
    x, P = make_state(rng, N, npdt)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    del P
    floor_ms, form = st.copy_floor(10)
    ts = [wall_ms(lambda: st.transform(1.0, -2.0, 0.3 if k % 2 else -0.3), st.sync) for k in range(runs + 1)][1:]
    tt = [wall_ms(lambda: st.transform(1.0, -2.0, 0.0), st.sync) for k in range(runs + 1)][1:]
    floor2_ms, _ = st.copy_floor(10)
    floor = min(floor_ms, floor2_ms)
    out = {"what": "slam_ekf_transform", "dtype": dtype, "N": N, "runs": runs, "copy_floor_ms": floor, "copy_floor_form": form,
           "t_transform_ms": statistics.median(ts), "t_transform_min_ms": min(ts), "t_translation_ms": statistics.median(tt)}
    out["transform_over_floor"] = out["t_transform_ms"] / floor
    print(f"{dtype} N={N}: slam_ekf_transform median {out['t_transform_ms']:.3f} ms wall (min {min(ts):.3f}, max {max(ts):.3f}); "
          f"copy floor {floor:.3f} ms ({form}); ratio {out['transform_over_floor']:.2f}; pure translation {out['t_translation_ms']:.3f} ms",
          flush=True)
    if with_host:
        hs = [wall_ms(lambda: host_transform(st, 1.0, -2.0, 0.3), st.sync) for _ in range(3)]
        out["t_host_ms"] = statistics.median(hs)
        out["host_over_transform"] = out["t_host_ms"] / out["t_transform_ms"]
        print(f"{dtype} N={N}: host round trip (download, NumPy, set_state) median {out['t_host_ms']:.0f} ms wall", flush=True)
    st.close()
    return out


def bench_pf(n, nl, runs):
    sh = pkg.PFShard(n, nl, 7, dtype="f32")
    sh.set_pose([0.0, 0.0, 0.1])
    sh.init_landmarks(np.random.default_rng(1).uniform(-200, 200, (nl, 2)), 0.01, 0.1)
    ts = [wall_ms(lambda: sh.transform(1.0, -2.0, 0.3 if k % 2 else -0.3), sh.sync) for k in range(runs + 1)][1:]
    nbytes = 2 * 4 * (5 * nl + 3) * n
    t = statistics.median(ts)
    out = {"what": "slam_pf_transform", "dtype": "f32", "particles": n, "landmarks": nl, "runs": runs, "t_ms": t, "t_min_ms": min(ts),
           "algorithmic_bytes": nbytes, "TB_per_s": nbytes / (t * 1e-3) / 1e12}
    print(f"FastSLAM f32 {n} x {nl}: slam_pf_transform median {t:.3f} ms wall (min {min(ts):.3f}); {nbytes / 1e9:.3f} GB read + written: "
          f"{out['TB_per_s']:.2f} TB/s", flush=True)
    sh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--n32", type=int, default=10000)
    ap.add_argument("--n64", type=int, default=10000)
    ap.add_argument("--pf-n", type=int, default=262144)
    ap.add_argument("--pf-nl", type=int, default=512)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lines = []
    if a.n32:
        lines.append(bench_ekf("f32", a.n32, a.runs, not a.no_host))
    if a.n64:
        lines.append(bench_ekf("f64", a.n64, a.runs, not a.no_host))
    if a.pf_n:
        lines.append(bench_pf(a.pf_n, a.pf_nl, a.runs))
    for l in lines:
        print(json.dumps(l))


if __name__ == "__main__":
    main()
