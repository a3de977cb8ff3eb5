#!/usr/bin/env python3
"""Time of the FastSLAM map read-out (slam_pf_map_sums) at the C4 shape (262144 particles x 512 landmarks, fp32) on one GPU:
  (a) all 512 landmarks, records without ancestor tables (16-byte loads),
  (b) the same after 8 resampling steps: every landmark behind a live ancestor table (particle-by-particle reads),
  (c) a 16-landmark subset, in both states,
and, as the only way to the same answer without it, slam_pf_download with the landmark records.
Wall time around the synchronising call, after a warm-up, median of 25 calls.  Beside each time: the bytes the algorithm
needs (records + table words + log-weights) and their rate against the 6.3 TB/s a streaming kernel reaches on this GPU.
  python tools/bench_pf_map.py [n] [nl] [--only a|b]       (--only: one state, for a kernel trace)"""
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package                      # noqa: E402

HBM = 6.3e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
if only:
    args = [a for a in args if a != only]
n = int(args[0]) if len(args) > 0 else 262144
nl = int(args[1]) if len(args) > 1 else 512
pkg = load_package()
Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
rng = np.random.default_rng(20240602)
lm = rng.uniform(-200, 200, (nl, 2))
pf = pkg.PFSlamState(n, nl, seed=20240602, dtype="f32", distributed=False)
pf.shard.set_pose([0.0, 0.0, 0.3])
pf.shard.init_landmarks(lm, 0.01, 0.1)
sub = list(range(1, nl + 1, max(1, nl // 16)))[:16]


def timed(call, reps=25, warm=3):
    for _ in range(warm):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def report(name, cnt, tables, call):
    med, lo, hi = timed(call)
    byts = cnt * n * 20 + (cnt * n * 4 if tables else 0) + n * 4
    print(f"{name:58s} {med * 1e6:9.1f} us  (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  {byts / 1e6:9.1f} MB  "
          f"{byts / med / 1e12:5.2f} TB/s = {100 * byts / med / HBM:4.1f} % of 6.3 TB/s", flush=True)
    return med


print(f"n = {n}, nl = {nl}, fp32; wall time around the synchronising call, median of 25 after 3 warm-up calls")
ta = tb = None
if only in (None, "a"):
    ta = report("(a) all landmarks, no tables", nl, False, lambda: pf.shard.map_sums())
    report("(c) 16 landmarks, no tables", len(sub), False, lambda: pf.shard.map_sums(sub))
if only in (None, "b"):
    pose = np.array([0.0, 0.0, 0.3])
    for t in range(8):
        pose = np.array([pose[0] + 0.2 * math.cos(pose[2]), pose[1] + 0.2 * math.sin(pose[2]), pose[2]])
        ids = (np.arange(16) + 16 * t) % nl + 1
        dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
        z = np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, 16))
        pf.step_async(8.0, 0.0, 4.0, Q, 0.025, z, ids, R, force_resample=True)
    _neff, _did = pf.flush()
    print(f"8 steps, {pf.resamples} resamplings: every landmark's records sit behind an ancestor table")
    tb = report("(b) all landmarks, through live ancestor tables", nl, True, lambda: pf.shard.map_sums())
    report("(c) 16 landmarks, through live ancestor tables", len(sub), True, lambda: pf.shard.map_sums(sub))
    report("    the pose row alone", 0, False, lambda: pf.shard.map_sums([]))
    report("    best particle with its records (slam_pf_get_particle)", 0, False, lambda: pf.shard.particle(-1))
if ta and tb:
    print(f"(b) / (a) = {tb / ta:.2f}  ({'within' if tb <= 1.5 * ta else 'NOT within'} 1.5 x)")
if only is None:
    ts = []
    for _ in range(3):                                         # (the first one materialises the maps: listed separately)
        t0 = time.perf_counter()
        pf.shard.download()
        ts.append(time.perf_counter() - t0)
    print(f"slam_pf_download with the records ({nl * n * 20 / 1e9:.2f} GB to the host; no reduction yet): first call "
          f"(materialises) {ts[0] * 1e3:.0f} ms, then {ts[1] * 1e3:.0f} ms, {ts[2] * 1e3:.0f} ms")
pf.close()
