#!/usr/bin/env python3
"""Time of the FastSLAM step with UNKNOWN correspondences on one GPU: fp32, 262144 particles x 64 slots, map about half full
(32 landmarks), every observation a revisit:
  m = 16   the three calls slam_pf_predict + slam_pf_update_unknown + slam_pf_weight_stats, and the fused slam_pf_step_unknown,
  m = 32, m = 64   the fused call alone (the legacy call takes at most 16).
Wall time around the synchronising step, after a warm-up, median of 25 steps.  Beside each time: the bytes the algorithm
needs -- the slot sweep as 5 rows x slots x n x 4 B plus the written records (5 x m x n x 4 B) -- and their rate.
Every case is a process of its own under `timeout -k 10`; the first one that fails ends the run.
  python tools/bench_pf_unknown.py [n] [slots]            all four cases
  python tools/bench_pf_unknown.py --case calls|fused --m M [n] [slots]      one case, in this process"""
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12
CASES = [("calls", 16), ("fused", 16), ("fused", 32), ("fused", 64)]
CASE_TIMEOUT_S = 180


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def positional():
    out, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a in ("--case", "--m"):
            skip = True
        elif not a.startswith("--"):
            out.append(a)
    return out


def run_case(case, m, n, slots):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
    R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
    rng = np.random.default_rng(20240602)
    nlm = slots // 2
    ang = 2 * math.pi * (np.arange(nlm) + 0.5) / nlm                  # a ring of well separated landmarks around the vehicle
    lm = np.stack([(20.0 + 10.0 * (np.arange(nlm) % 3)) * np.cos(ang), (20.0 + 10.0 * (np.arange(nlm) % 3)) * np.sin(ang)], axis=1)
    pose = np.array([0.0, 0.0, 0.3])

    def observe(ids):
        dx, dy = lm[ids, 0] - pose[0], lm[ids, 1] - pose[1]
        return np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + 0.3 * rng.normal(0, [[0.1], [math.pi / 180]], (2, len(ids)))

    sh = pkg.PFShard(n, slots, 20240602, dtype="f32")
    sh.set_pose(pose)
    sh.clear_landmarks()
    for lo in range(0, nlm, 64):                                       # the map: every landmark once (all new)
        sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.025, observe(np.arange(lo, min(lo + 64, nlm))), R, 4.0, 25.0)
    z = observe(np.arange(m) % nlm)

    def calls():
        sh.predict(0.0, 0.0, 4.0, Q, 0.025)
        sh.update_unknown(z, R, 4.0, 25.0)
        return sh.weight_stats()

    def fused():
        return sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.025, z, R, 4.0, 25.0)

    step = calls if case == "calls" else fused
    for _ in range(3):
        step()
    ts = []
    for _ in range(25):
        t0 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t0)
    _, assoc = sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.025, z, R, 4.0, 25.0, want_assoc=True)
    matched = float((assoc >= 0).float().mean().item())
    used = float((sh.download()[2][:, 2, :] >= 0).sum(axis=0).mean())
    sh.close()
    med = statistics.median(ts)
    byts = 5 * slots * n * 4 + 5 * m * n * 4
    name = "predict + update_unknown + weight_stats" if case == "calls" else "slam_pf_step_unknown (fused)"
    print(f"m = {m:2d}  {name:42s} {med * 1e6:9.1f} us  (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f})  {byts / 1e6:7.1f} MB  "
          f"{byts / med / 1e12:5.2f} TB/s = {100 * byts / med / HBM:4.1f} % of 6.3 TB/s   matched {matched:.3f}, slots in use {used:.1f}",
          flush=True)
    print(json.dumps({"case": case, "m": m, "n": n, "slots": slots, "dtype": "f32", "us_per_step": med * 1e6, "us_min": min(ts) * 1e6,
                      "us_max": max(ts) * 1e6, "bytes": byts, "tb_per_s": byts / med / 1e12, "matched": matched, "slots_in_use": used}),
          flush=True)


def main():
    pos = positional()
    n = int(pos[0]) if len(pos) > 0 else 262144
    slots = int(pos[1]) if len(pos) > 1 else 64
    case = opt("--case")
    if case is not None:
        run_case(case, int(opt("--m", "16")), n, slots)
        return 0
    print(f"n = {n}, slots = {slots}, fp32; wall time around the synchronising step, median of 25 after 3 warm-up steps", flush=True)
    for case, m in CASES:
        cmd = ["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--case", case, "--m", str(m),
               str(n), str(slots)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"case {case} m = {m} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
