#!/usr/bin/env python3
"""Time of slam_ekf_remove_landmarks (csrc/ekf_compact.hip) against the copy floor and against the host round trip.

    python tools/bench_remove.py [--runs 10] [--n32 10000] [--n64 0]

Per shape (fp32 N = --n32; fp64 N = --n64 when given, 50 000 is the C5 shape and needs ~45 GB of device memory and a few
minutes of uploads), each figure the median over --runs runs after one warm-up, HIP events on the handle's stream, the
state uploaded again (fresh random mean, covariance diagonal re-drawn) before every run:
  t_first   remove landmark 1: every stored tile moves, twice (matrix -> staging -> matrix)
  t_last    remove landmark N: the last tile row only
  floor     slam_ekf_copy_floor on the same handle in the same run (one read + one write of the stored tiles)
  t_host    fp32 only: download, np.delete rows / columns, set_state -- what the library offered before (wall clock)
One JSON line per shape at the end."""
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
import torch                                                   # noqa: E402


def make_state(rng, N, npdt):
    n = 3 + 2 * N
    x = rng.uniform(0, 1000, n).astype(npdt)
    A = rng.normal(0, 0.05, (n, 4)).astype(npdt)
    P = A @ A.T
    P[np.diag_indices(n)] += npdt(0.01)
    return x, np.maximum(P, P.T)


def timed_remove(st, stream, ids):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.sync()
    t0 = time.perf_counter()
    a.record(stream)
    st.remove_landmarks(ids)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def bench_shape(dtype, N, runs, with_host):
    npdt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(12345)
    x, P = make_state(rng, N, npdt)
    st = pkg.EKFSlamState(x, P, dtype=dtype, max_landmarks=N)
    stream = torch.cuda.ExternalStream(st.device_ptrs()[3])
    floor_ms, form = st.copy_floor(10)
    out = {"dtype": dtype, "N": N, "runs": runs, "copy_floor_ms": floor_ms, "copy_floor_form": form}
    for what, ids in (("first", [1]), ("last", [N])):
        dev, wall = [], []
        for k in range(runs + 1):
            x[:] = rng.uniform(0, 1000, x.shape[0]).astype(npdt)
            P[np.diag_indices(x.shape[0])] = rng.uniform(0.02, 0.03, x.shape[0]).astype(npdt)
            st.set_state(x, P)
            d, w = timed_remove(st, stream, ids)
            if k:                                              # (run 0: warm-up)
                dev.append(d)
                wall.append(w)
        out[f"t_{what}_ms"] = statistics.median(dev)
        out[f"t_{what}_wall_ms"] = statistics.median(wall)
        out[f"t_{what}_all_ms"] = [round(v, 4) for v in dev]
        print(f"{dtype} N={N} remove {what}: median {out[f't_{what}_ms']:.3f} ms on the stream "
              f"(min {min(dev):.3f}, max {max(dev):.3f}), {out[f't_{what}_wall_ms']:.3f} ms wall; copy floor {floor_ms:.3f} ms", flush=True)
    out["first_over_floor"] = out["t_first_ms"] / floor_ms
    out["last_over_first"] = out["t_last_ms"] / out["t_first_ms"]
    if with_host:
        hs = []
        for _ in range(3):
            st.set_state(x, P)
            st.sync()
            t0 = time.perf_counter()
            xd, Pd = st.download()
            keep = np.delete(np.arange(len(xd)), [3, 4])
            st.set_state(xd[keep], Pd[np.ix_(keep, keep)])
            st.sync()
            hs.append((time.perf_counter() - t0) * 1e3)
        out["t_host_ms"] = statistics.median(hs)
        out["host_over_first"] = out["t_host_ms"] / out["t_first_wall_ms"]
        print(f"{dtype} N={N} host round trip (download, np.delete, set_state): median {out['t_host_ms']:.0f} ms wall", flush=True)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--n32", type=int, default=10000)
    ap.add_argument("--n64", type=int, default=0)
    a = ap.parse_args()
    lines = [bench_shape("f32", a.n32, a.runs, True)]
    if a.n64:
        lines.append(bench_shape("f64", a.n64, a.runs, False))
    for l in lines:
        print(json.dumps(l))


if __name__ == "__main__":
    main()
