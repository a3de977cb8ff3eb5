#!/usr/bin/env python3
"""Time of slam_ekf_copy / slam_ekf_select (libslamhip_copy.so, csrc/ekf_copy.hip) beside the copy floor of the same matrix, on one
GPU: fp32, N = 10 000 landmarks (n = 20 003, 157 tile rows, 12 403 tiles of 64 KiB = 813 MB).  In ONE process:
  (1) slam_ekf_copy_floor of the source: every stored tile read once and written back, the fastest of 10 passes between events --
      the same bytes as a copy into equal capacity;
  (2) slam_ekf_copy into a handle of equal capacity and into one of double capacity (other block numbers, the same bytes);
  (3) slam_ekf_select of 1 000 and of 5 000 landmarks, ids ascending and shuffled, into a handle of capacity 5 000.
(2), (3): wall time around call + synchronise, median of 15 after 2 warm-up calls (min, max), and per call over 10 calls enqueued back
to back behind one synchronisation.  A call is the matrix launch plus the x copy, the side-array rebuild, two events and two stream
waits.  Bytes: the tiles the launch reads plus the tiles it writes; "byte floor": those bytes at the rate (1) reached, which for a
copy is (1) itself.
The measuring process runs under `timeout -k 10`.
  python tools/bench_ekf_copy.py [N] [--out FILE]      (FILE: default profiles/ekf_copy_bench.txt)"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12
TIMEOUT_S = 420
B2B = 10
E, ESZ = 128, 4


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def median_ms(fn, reps=15, warm=2, per=1):
    for _ in range(warm):
        fn()
    ts = [wall(fn) / per * 1e3 for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def tiles(n):
    t = (n + E - 1) // E
    return t * (t + 1) // 2


def measure(N, out_path):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    rng = np.random.default_rng(20240607)
    n = 3 + 2 * N
    x = np.concatenate([[500.0, 500.0, 0.6], rng.uniform(-1000, 1000, 2 * N)]).astype(np.float32)
    A = rng.normal(0, 0.05, (n, 4)).astype(np.float32)
    P = A @ A.T
    P[np.diag_indices(n)] += np.float32(0.01)
    src = pkg.EKFSlamState(x, np.maximum(P, P.T), dtype="f32", max_landmarks=N)
    del P
    blank = lambda cap: pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype="f32", max_landmarks=cap)   # noqa: E731
    tile_mb = E * E * ESZ / 1e6
    lines = [f"slam_ekf_copy / slam_ekf_select beside the copy floor: fp32, N = {N}, n = {n}, {tiles(n)} stored tiles = "
             f"{tiles(n) * tile_mb:.0f} MB",
             f"(2), (3): ms around call + synchronise, median of 15 after 2 warm-up calls (min, max); b2b = per call over {B2B} calls "
             f"behind one synchronisation; GB/s = bytes read + written over the b2b time"]
    floor_ms, form = src.copy_floor(10)
    byts = 2 * tiles(n) * tile_mb * 1e6
    floor_rate = byts / (floor_ms * 1e-3)                            # bytes per second, read + written
    lines.append(f"(1) slam_ekf_copy_floor ({form})          {floor_ms:8.3f} ms   {byts / 1e6:7.0f} MB  "
                 f"{byts / (floor_ms * 1e-3) / 1e9:6.0f} GB/s = {100 * byts / (floor_ms * 1e-3) / HBM:4.1f} % of 6.3 TB/s")

    def timed(label, dst, call, byts):
        def one():
            call()
            dst.sync()

        def many():
            for _ in range(B2B):
                call()
            dst.sync()
        t1 = median_ms(one)
        tb = median_ms(many, reps=7, warm=1, per=B2B)
        own = byts / floor_rate * 1e3                                  # these bytes at the floor's rate
        lines.append(f"{label:44s} {t1[0]:8.3f} ms (min {t1[1]:.3f}, max {t1[2]:.3f})   b2b {tb[0]:8.3f} ms (min {tb[1]:.3f})   "
                     f"{byts / 1e6:7.0f} MB  {byts / (tb[0] * 1e-3) / 1e9:6.0f} GB/s   byte floor {own:6.3f} ms   b2b / byte floor {tb[0] / own:5.2f}")
        return tb[0]

    for label, cap in (("(2) slam_ekf_copy, equal capacity", N), ("(2) slam_ekf_copy, double capacity", 2 * N)):
        dst = blank(cap)
        timed(label, dst, lambda d=dst: d.copy_from(src), byts)
        dst.close()
    floor2, _ = src.copy_floor(10)
    lines.append(f"(1) slam_ekf_copy_floor again                 {floor2:8.3f} ms")
    dst = blank(5000)
    for cnt in (1000, 5000):
        asc = np.sort(rng.choice(np.arange(1, N + 1), size=cnt, replace=False))
        for name, ids in (("ascending", asc), ("shuffled", rng.permutation(asc))):
            nn = 3 + 2 * cnt
            sel_bytes = 2 * tiles(nn) * tile_mb * 1e6                 # dst's tiles written, as many source values read
            timed(f"(3) slam_ekf_select, {cnt} landmarks, {name}", dst, lambda i=ids: dst.select_from(src, i), sel_bytes)
    dst.close()
    src.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--out"]
    N = int(pos[0]) if pos else 10000
    out_path = opt("--out", os.path.join(ROOT, "profiles", "ekf_copy_bench.txt"))
    if "--measure" in sys.argv:
        measure(N, out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", str(N), "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
