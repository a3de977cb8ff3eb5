#!/usr/bin/env python3
"""Time of the landmark-evidence pass (slam_pf_evidence_update, libslamhip_evidence.so) beside the step it follows, on one GPU:
fp32, 262144 particles x 64 slots, map half full (32 landmarks), m = 16 observations, every one a revisit.  In ONE run:
  slam_pf_step_unknown                 the fused unknown-correspondence step (the yardstick: same run, same box)
  slam_pf_evidence_update              the pass alone, with the step's decisions: as a synchronising call (counts wanted), and
                                       enqueued 20 times back to back behind one synchronisation (the pass without the host)
  slam_pf_step_unknown_evidence        the combined call
The rule is set so that the pass does all of its arithmetic and changes nothing from call to call: r_max = 100 m takes every
unmatched record through the range AND the bearing, half_fov = 0.001 rad lets none of them be in view, so no counter decays and
no record is pruned while the clock runs (16 of the 32 landmarks are matched and sit at `cap`).
Beside each time of the pass: its algorithmic bytes -- three rows and the counter of every (slot, particle), (3 x 4 + 1) B, the
decisions 4 m n B, the poses 12 n B -- and their rate.  Wall time, median of 25 after 3 warm-up calls.
The measuring process runs under `timeout -k 10`.
  python tools/bench_pf_evidence.py [n] [slots] [--out FILE]      (FILE: default profiles/pf_evidence_bench.txt)"""
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12
TIMEOUT_S = 240
M = 16
BACK_TO_BACK = 20


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def positional():
    out, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a == "--out":
            skip = True
        elif not a.startswith("--"):
            out.append(a)
    return out


def median_us(fn, reps=25, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6


def measure(n, slots, out_path):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
    R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
    rng = np.random.default_rng(20240602)
    nlm = slots // 2
    ang = 2 * math.pi * (np.arange(nlm) + 0.5) / nlm                  # the ring of tools/bench_pf_unknown.py
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
    z = observe(np.arange(M) % nlm)
    ev = pkg.LandmarkEvidence(sh, 100.0, 1e-3, inc=1, dec=1, init=1, cap=5)
    step = lambda: sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.025, z, R, 4.0, 25.0)
    _, assoc = sh.step_unknown_fused(0.0, 0.0, 4.0, Q, 0.025, z, R, 4.0, 25.0, want_assoc=True)
    first = ev.update(assoc).tolist()

    def back_to_back():
        for _ in range(BACK_TO_BACK):
            ev.update(assoc, want_counts=False, assume_ready=True)
        sh.sync()

    t_step = median_us(step)
    t_sync = median_us(lambda: ev.update(assoc, assume_ready=True))
    t_b2b = tuple(t / BACK_TO_BACK for t in median_us(back_to_back, reps=10, warm=1))
    t_both = median_us(lambda: ev.step(0.0, 0.0, 4.0, Q, 0.025, z, R, 4.0, 25.0))
    last = ev.update(assoc).tolist()
    matched = float((assoc >= 0).float().mean().item())
    used = float((sh.download()[2][:, 2, :] >= 0).sum(axis=0).mean())
    c = ev.counters()
    ev.close()
    sh.close()
    byts = (3 * 4 + 1) * slots * n + 4 * M * n + 12 * n
    sweep = 5 * slots * n * 4 + 5 * M * n * 4
    rate = lambda us: f"{byts / (us * 1e-6) / 1e9:7.1f} GB/s = {100 * byts / (us * 1e-6) / HBM:4.1f} % of 6.3 TB/s"
    lines = [
        f"landmark evidence pass beside the step it follows: fp32, n = {n}, slots = {slots}, m = {M}, map half full "
        f"(slots in use {used:.1f}, matched {matched:.3f})",
        "wall time, median of 25 after 3 warm-up calls (min, max); back to back: 20 enqueued passes behind one synchronisation, per pass",
        f"rule: r_max = 100, half_fov = 0.001, inc = dec = init = 1, cap = 5: every unmatched record goes through range and bearing, "
        f"none is in view; counts of the first pass {first}, of the last {last}; counters at cap: {int((c == 5).sum())}, "
        f"at init: {int((c == 1).sum())}, empty: {int((c == -128).sum())}",
        f"slam_pf_step_unknown (yardstick)          {t_step[0]:9.1f} us  (min {t_step[1]:.1f}, max {t_step[2]:.1f})   "
        f"its sweep: {sweep / 1e6:.1f} MB, {sweep / (t_step[0] * 1e-6) / 1e9:.1f} GB/s",
        f"slam_pf_evidence_update, synchronising    {t_sync[0]:9.1f} us  (min {t_sync[1]:.1f}, max {t_sync[2]:.1f})   "
        f"{byts / 1e6:.1f} MB  {rate(t_sync[0])}",
        f"slam_pf_evidence_update, back to back     {t_b2b[0]:9.1f} us  (min {t_b2b[1]:.1f}, max {t_b2b[2]:.1f})   "
        f"{byts / 1e6:.1f} MB  {rate(t_b2b[0])}",
        f"slam_pf_step_unknown_evidence (combined)  {t_both[0]:9.1f} us  (min {t_both[1]:.1f}, max {t_both[2]:.1f})",
        f"pass / step: {t_b2b[0] / t_step[0]:.2f} (back to back), {t_sync[0] / t_step[0]:.2f} (synchronising); "
        f"combined - step: {t_both[0] - t_step[0]:.1f} us",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    pos = positional()
    n = int(pos[0]) if len(pos) > 0 else 262144
    slots = int(pos[1]) if len(pos) > 1 else 64
    out_path = opt("--out", os.path.join(ROOT, "profiles", "pf_evidence_bench.txt"))
    if "--measure" in sys.argv:
        measure(n, slots, out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", str(n), str(slots),
           "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
