#!/usr/bin/env python3
"""Time of slam_ekf_join (csrc/ekf_join.hip) against the byte floor and against the host round trip it replaces.

    python tools/bench_join.py [--runs 25] [--na 10000] [--nb 100 1000] [--dtypes f32 f64] [--out profiles/ekf_join_bench.txt]

Per dtype and N_B, N_A landmarks in the global map:
  t_join    wall clock around join + synchronise, median of --runs after one warm-up; the appended landmarks are removed again
            outside the timed region
  t_host    the round trip it replaces: download of both states, NumPy (F P_a F' + G P_b G' blockwise), set_state; median of 3
  t_empty   the same call with an EMPTY b (N_B = 0: the trig launch, the vehicle strip, the pose block, the side rebuild and the two
            events, no new row): the part of t_join that does not depend on N_B, same handle, same run, median of --runs
  floor     the copy rate slam_ekf_copy_floor gives on the same handle (bytes of the stored tiles read + written per second)
            applied to the bytes the join reads and writes: the new rows written (2 N_b x n'), b's matrix read, the strip read and written
One JSON line per case; --out also writes the lines to a file."""
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


def make_state(rng, N, npdt, pose, spread):
    n = 3 + 2 * N
    x = np.concatenate([pose, rng.uniform(-spread, spread, 2 * N)]).astype(npdt)
    A = rng.normal(0, 0.05, (n, 4)).astype(npdt)
    P = A @ A.T
    P[np.diag_indices(n)] += npdt(0.01)
    return x, np.maximum(P, P.T)


def host_join(xa, Pa, xb, Pb):
    """The same result on the host, blockwise (the dense F and G would be 20 000 x 20 000)."""
    nA, NB = len(xa), (len(xb) - 3) // 2
    c, s = np.cos(np.float64(xa[2])), np.sin(np.float64(xa[2]))
    Rm = np.array([[c, -s], [s, c]])
    pts = np.concatenate([xb[0:2], xb[3:]]).reshape(-1, 2).astype(np.float64)            # vehicle, then b's landmarks
    J = np.zeros((len(pts), 2, 3))
    J[:, 0, 0] = J[:, 1, 1] = 1.0
    J[:, 0, 2] = -(s * pts[:, 0] + c * pts[:, 1])
    J[:, 1, 2] = c * pts[:, 0] - s * pts[:, 1]
    Fn = np.concatenate([J[0], [[0.0, 0.0, 1.0]], J[1:].reshape(-1, 3)])                 # rows: new vehicle (3), new landmarks
    Gn = np.kron(np.eye(NB + 1), Rm)
    Gn = np.insert(np.insert(Gn, 2, 0.0, axis=0), 2, 0.0, axis=1)
    Gn[2, 2] = 1.0
    out = np.zeros((nA + 2 * NB, nA + 2 * NB), dtype=Pa.dtype)
    out[3:nA, 3:nA] = Pa[3:nA, 3:nA]
    new = Fn @ Pa[:3, :3].astype(np.float64) @ Fn.T + Gn @ Pb.astype(np.float64) @ Gn.T
    cross = Fn @ Pa[:3, 3:nA].astype(np.float64)
    idx = np.concatenate([np.arange(3), np.arange(nA, nA + 2 * NB)])
    out[np.ix_(idx, idx)] = new
    out[idx[:, None], np.arange(3, nA)[None, :]] = cross
    out[np.arange(3, nA)[:, None], idx[None, :]] = cross.T
    g = xa[:2].astype(np.float64) + pts @ Rm.T
    x = np.concatenate([g[0], [xa[2] + xb[2]], xa[3:], g[1:].reshape(-1)]).astype(xa.dtype)
    return x, out


def bench_case(dtype, NA, NB, runs):
    npdt = np.float32 if dtype == "f32" else np.float64
    esz = 4 if dtype == "f32" else 8
    E = 128 if dtype == "f32" else 64
    rng = np.random.default_rng(12345)
    xa, Pa = make_state(rng, NA, npdt, [500.0, 500.0, 0.6], 1000.0)
    xb, Pb = make_state(rng, NB, npdt, [1.0, -2.0, 0.1], 30.0)
    a = pkg.EKFSlamState(xa, Pa, dtype=dtype, max_landmarks=NA + NB)
    b = pkg.EKFSlamState(xb, Pb, dtype=dtype, max_landmarks=NB)
    floor_ms, form = a.copy_floor(10)
    T = a.device_ptrs()[2] // E
    tile_bytes = T * (T + 1) // 2 * E * E * esz
    rate = 2.0 * tile_bytes / (floor_ms * 1e-3)                     # bytes per second, read + write
    nA, n2 = 3 + 2 * NA, 3 + 2 * (NA + NB)
    join_bytes = esz * (2 * NB * nA + 2 * NB * (2 * NB + 1) // 2 * 2 + 2 * 3 * nA)       # new rows written, b read, strip read + written
    ts = []
    for k in range(runs + 1):
        a.sync()
        b.sync()
        t0 = time.perf_counter()
        a.join(b)
        a.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if k:
            ts.append(dt)
        a.remove_landmarks(np.arange(NA + 1, NA + NB + 1))          # (the composed vehicle stays: the next join costs the same)
    empty = a.submap(1)
    te = []
    for k in range(runs + 1):
        a.sync()
        t0 = time.perf_counter()
        a.join(empty)
        a.sync()
        if k:
            te.append((time.perf_counter() - t0) * 1e3)
    empty.close()
    hs = []
    for _ in range(3):
        a.sync()
        t0 = time.perf_counter()
        x1, P1 = a.download()
        x2, P2 = b.download()
        xj, Pj = host_join(x1, P1, x2, P2)
        a.set_state(xj, Pj)
        a.sync()
        hs.append((time.perf_counter() - t0) * 1e3)
        a.set_state(xa, Pa)
    out = {"dtype": dtype, "N_A": NA, "N_B": NB, "runs": runs, "t_join_ms": statistics.median(ts), "t_join_min_ms": min(ts),
           "t_empty_ms": statistics.median(te), "t_host_ms": statistics.median(hs), "copy_floor_ms": floor_ms, "copy_floor_form": form, "copy_rate_GBps": rate / 1e9,
           "join_bytes": join_bytes, "byte_floor_ms": join_bytes / rate * 1e3}
    out["join_over_byte_floor"] = out["t_join_ms"] / out["byte_floor_ms"]
    out["rows_over_byte_floor"] = (out["t_join_ms"] - out["t_empty_ms"]) / out["byte_floor_ms"]       # what N_B adds, against the floor
    out["host_over_join"] = out["t_host_ms"] / out["t_join_ms"]
    print(f"{dtype} N_A={NA} N_B={NB}: join {out['t_join_ms']:.3f} ms (min {out['t_join_min_ms']:.3f}), byte floor {out['byte_floor_ms']:.3f} ms "
          f"at {out['copy_rate_GBps']:.0f} GB/s, empty join {out['t_empty_ms']:.3f} ms, host round trip {out['t_host_ms']:.0f} ms", flush=True)
    a.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--na", type=int, default=10000)
    ap.add_argument("--nb", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(bench_case(d, args.na, nb, args.runs)) for d in args.dtypes for nb in args.nb]
    for l in lines:
        print(l)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
