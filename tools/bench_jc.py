#!/usr/bin/env python3
"""Time of the joint-compatibility association (slam_ekf_associate_joint, csrc/ekf_jc.hip) beside the nearest neighbour it stands
next to (slam_ekf_associate), on the bench workload.

    python tools/bench_jc.py [--runs 200] [--out profiles/ekf_jc_bench.txt] [--no-trace]

Per configuration (C2: N = 1000, 16 observations; C3: N = 10000, 64 observations; fp32 state, bench.make_workload_on_device):
  t_joint_us      wall clock of one associate_joint call (upload, four launches, download, synchronise): median over --runs calls
                  after 10 warm-up calls, cycling through the workload's observation sets
  t_nearest_us    the same for slam_ekf_associate on the same inputs, same handle, same run: the existing baseline
  tests           joint tests evaluated per call (median, max), pairings, distinct candidate landmarks
  launches        per kernel of the call: mean device time from a kernel trace of a child process (rocprofv3 --kernel-trace --stats);
                  "not measured" where the tracer is not available
Time per joint test at depth d (d = 8, 32, 64): slam_ekf_joint_nis on a hypothesis of d pairings runs d tests at depths 1 .. d, so
the median of the call with d pairings minus the median with d - 1 is the cost of the test at depth d (plus d more threads in the
cross launch, which runs in parallel); medians over --runs calls each, interleaved.
One JSON line per record; --out also writes them to a file, the device's name first."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B                                             # noqa: E402
from __graft_entry__ import load_package                      # noqa: E402

CONFIGS = {"C2": (1000, 16), "C3": (10000, 64)}
WARMUP = 10


def wall_us(fn, runs):
    ts = []
    for k in range(WARMUP + runs):
        t0 = time.perf_counter()
        fn(k)
        if k >= WARMUP:
            ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def open_config(pkg, name):
    N, nz = CONFIGS[name]
    st, zs = B.make_workload_on_device(pkg, N, nz, 40, B.SEED, "f32", 0)          # (the bench's workload, P formed on the device)
    return st, zs, N, nz


def child(name, calls):
    """What the kernel trace watches: `calls` joint associations and as many nearest-neighbour ones."""
    pkg = load_package()
    st, zs, _N, _nz = open_config(pkg, name)
    for k in range(calls):
        st.associate_joint_vector(zs[k % len(zs)], B.R, B.GATE1, B.GATE2)
        st.associate_vector(zs[k % len(zs)], B.R, B.GATE1, B.GATE2)
    st.close()


def trace_launches(name, calls=60):
    tool = shutil.which("rocprofv3")
    if tool is None:
        return "not measured: no rocprofv3 on this machine"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--calls", str(calls)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if res.returncode != 0 or not files:
            return f"not measured: the tracer returned {res.returncode}"
        out = {}
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                kname = row.get("Name", "")
                for key in ("jc_sweep_kernel", "jc_lists_kernel", "jc_cross_kernel", "jc_search_kernel", "gate_kernel"):
                    if key in kname and "grid" not in kname:
                        out[key] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return out or "not measured: no jc kernel in the trace"


def bench_config(pkg, name, runs, trace):
    st, zs, N, nz = open_config(pkg, name)
    infos = []

    def joint(k):
        infos.append(st.associate_joint_vector(zs[k % len(zs)], B.R, B.GATE1, B.GATE2)[1])

    tj = wall_us(joint, runs)
    tn = wall_us(lambda k: st.associate_vector(zs[k % len(zs)], B.R, B.GATE1, B.GATE2), runs)
    infos = infos[WARMUP:]
    tests = [i["tests"] for i in infos]
    rec = {"config": name, "dtype": "f32", "N": N, "nz": nz, "runs": runs, "t_joint_us": statistics.median(tj), "t_joint_min_us": min(tj),
           "t_nearest_us": statistics.median(tn), "t_nearest_min_us": min(tn), "tests_median": statistics.median(tests),
           "tests_max": max(tests), "pairings_median": statistics.median(i["pairings"] for i in infos),
           "candidates_median": statistics.median(i["candidates"] for i in infos), "deepest_max": max(i["deepest"] for i in infos),
           "exhausted_calls": sum(i["exhausted"] for i in infos), "truncated_calls": sum(i["truncated"] for i in infos)}
    st.close()
    rec["launches"] = trace_launches(name) if trace else "not measured: --no-trace"
    print(f"{name}: joint {rec['t_joint_us']:.1f} us, nearest neighbour {rec['t_nearest_us']:.1f} us, tests median {rec['tests_median']} "
          f"max {rec['tests_max']}", flush=True)
    return rec


def bench_depth(pkg, runs):
    """Per-test time at depth 8, 32 and 64 from joint_nis on d and d - 1 pairings (module docstring)."""
    N = 1000
    x, P, _zs = B.make_workload(N, 16, 2, B.SEED)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
    xs = np.asarray(st.download("x"), dtype=np.float64)
    rng = np.random.default_rng(5)
    ids = rng.permutation(np.arange(1, N + 1))[:64]
    f = 3 + 2 * (ids - 1)
    dx, dy = xs[f] - xs[0], xs[f + 1] - xs[1]
    z = np.stack([np.hypot(dx, dy) + 0.05, np.arctan2(dy, dx) - xs[2] + 0.005])
    sizes = (7, 8, 31, 32, 63, 64)
    ts = {m: [] for m in sizes}
    for k in range(WARMUP + runs):
        for m in sizes:
            t0 = time.perf_counter()
            st.joint_nis(z[:, :m], ids[:m], B.R)
            if k >= WARMUP:
                ts[m].append((time.perf_counter() - t0) * 1e6)
    st.close()
    med = {m: statistics.median(v) for m, v in ts.items()}
    rec = {"record": "time per joint test", "N": N, "dtype": "f32", "runs": runs, "call_us": {str(m): med[m] for m in sizes},
           "test_us_at_depth": {str(d): med[d] - med[d - 1] for d in (8, 32, 64)},
           "mean_test_us_over_depths_1_to_64": (med[64] - med[7]) / 57.0}
    print(f"joint_nis call {med}; per test {rec['test_us_at_depth']}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--calls", type=int, default=60)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    pkg = load_package()
    import torch
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP})]
    lines += [json.dumps(bench_config(pkg, name, args.runs, not args.no_trace)) for name in CONFIGS]
    lines.append(json.dumps(bench_depth(pkg, args.runs)))
    for l in lines:
        print(l)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
