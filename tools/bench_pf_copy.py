#!/usr/bin/env python3
"""Times of moving a particle set on the device (libslamhip_pfcopy.so, csrc/pf_copy.hip) at the C4 shape of bench.py: fp32,
262 144 particles x 512 landmarks, after 20 steps of the bench's scene under the Neff rule -- ancestor tables live, records in
both buffers -- and once more on plain maps (after a download has materialised them).  In ONE process:
  (1) slam_pf_copy into a second filter of the same shape, beside hipMemcpyAsync device-to-device of the same chunks, poses and
      log-weights (the floor); the ratio is the figure;
  (2) slam_pf_select of 256 landmarks, ids ascending and shuffled;
  (3) slam_pf_resize to n / 2 and to 2 n particles;
  (4) slam_pf_pose_bins;
  (5) slam_pf_upload and slam_pf_download of the whole set (the host round trip a clone had to take before), once each.
(1) - (4): wall time around the call (each synchronises), median of 7 after 2 warm-up calls (min, max).
The measuring process runs under `timeout -k 10`.
  python tools/bench_pf_copy.py [--np N] [--out FILE]      (FILE: default profiles/pf_copy_bench.txt)"""
import ctypes
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 540
NL, M, STEPS = 512, 16, 20


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def median_ms(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = [wall(fn) * 1e3 for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def loaded_hip():
    """The HIP runtime this process already uses (torch's, which libslamhip.so shares), for hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        return None
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int
    return hip


def chunk_bytes(n, nl, esz=4):
    """The chunk sizes slam_pf_create cuts [nl][5][n] into (csrc/pf_legacy.hip: pf_create_impl)."""
    per = esz * 5 * n
    shift = 0
    while shift < 20 and (per << (shift + 1)) <= (1 << 30):
        shift += 1
    while ((nl + (1 << shift) - 1) >> shift) > 16:
        shift += 1
    return [per * min(1 << shift, nl - (k << shift)) for k in range((nl + (1 << shift) - 1) >> shift)]


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def measure(NP, out_path):
    sys.path.insert(0, ROOT)
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
    R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
    rng = np.random.default_rng(20240602)                      # bench.py's scene
    lm = rng.uniform(-200, 200, (NL, 2))
    pose = np.array([0.0, 0.0, 0.3])
    pf = pkg.PFSlamState(NP, NL, seed=20240602, dtype="f32", distributed=False)
    pf.shard.set_pose(pose)
    pf.shard.init_landmarks(lm, 0.01, 0.1)
    for t in range(STEPS):
        pose = np.array([pose[0] + 0.2 * math.cos(pose[2]), pose[1] + 0.2 * math.sin(pose[2]), pose[2]])
        ids = (np.arange(M) + M * t) % NL + 1
        dx, dy = lm[ids - 1, 0] - pose[0], lm[ids - 1, 1] - pose[1]
        z = np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, M))
        pf.step_async(8.0, 0.0, 4.0, Q, 0.025, z, ids, R)
    neff, _ = pf.flush()
    sh = pf.shard
    gm, s1, _ = sh.weight_stats()
    sh.normalize(gm, s1)
    gmax = float(np.float32(gm) - np.float32(gm + math.log(s1)))
    rec_bytes = 4.0 * NP * (5 * NL + 4)
    lines = [f"particle set moved on the device at the C4 shape: fp32, {NP} particles x {NL} landmarks, after {STEPS} bench steps under the Neff "
             f"rule (Neff {neff:.0f}, {pf.resamples} resamplings); records + poses + log-weights {rec_bytes / 1e9:.2f} GB, "
             f"{len(chunk_bytes(NP, NL))} chunks a buffer",
             "ms around a synchronising call, median of 7 after 2 warm-up calls (min, max); GB/s counts the bytes written (as many are read)"]
    hip = loaded_hip()
    sizes = chunk_bytes(NP, NL) + [12 * NP, 4 * NP]
    a = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in sizes]
    b = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in sizes]
    for t in a:
        t.zero_()

    def floor():
        for x, y in zip(a, b):
            if hip is not None:
                assert hip.hipMemcpyAsync(ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(x.data_ptr()), x.numel(), 3, None) == 0
            else:
                y.copy_(x)
        if hip is not None:
            assert hip.hipDeviceSynchronize() == 0
        else:
            torch.cuda.synchronize()

    same = pkg.PFShard(NP, NL, 1, dtype="f32")
    half = pkg.PFShard(NP // 2, NL, 1, dtype="f32")
    sel = pkg.PFShard(NP, 256, 1, dtype="f32")
    asc = np.arange(1, 257) * 2 - 1
    shuf = np.random.default_rng(1).permutation(NL)[:256] + 1
    sel_bytes = 4.0 * NP * (5 * 256 + 4)

    def block(tag):
        t_floor = median_ms(floor)
        t_copy = median_ms(lambda: same.copy_from(sh))
        lines.append(f"[{tag}]")
        lines.append(f"(1) slam_pf_copy                         {fmt(t_copy)}   {rec_bytes / (t_copy[0] * 1e-3) / 1e9:.0f} GB/s")
        lines.append(f"    {'hipMemcpyAsync' if hip is not None else 'torch copy_'} d2d of the same chunks     {fmt(t_floor)}   "
                     f"{rec_bytes / (t_floor[0] * 1e-3) / 1e9:.0f} GB/s;  (1) / floor = {t_copy[0] / t_floor[0]:.2f}")
        for name, ids in (("ascending", asc), ("shuffled ", shuf)):
            t = median_ms(lambda: sel.select_from(sh, ids))
            lines.append(f"(2) slam_pf_select, 256 ids {name}    {fmt(t)}   {sel_bytes / (t[0] * 1e-3) / 1e9:.0f} GB/s")
        t = median_ms(lambda: half.resize_from(sh, gmax, 0.37))
        lines.append(f"(3) slam_pf_resize to n / 2              {fmt(t)}   {rec_bytes / 2 / (t[0] * 1e-3) / 1e9:.0f} GB/s")
        dbl = pkg.PFShard(2 * NP, NL, 1, dtype="f32")
        t = median_ms(lambda: dbl.resize_from(sh, gmax, 0.37), reps=5, warm=1)
        lines.append(f"    slam_pf_resize to 2 n (median of 5)  {fmt(t)}   {rec_bytes * 2 / (t[0] * 1e-3) / 1e9:.0f} GB/s")
        dbl.close()

    block("ancestor tables live, as the filter stands after the steps")
    t = median_ms(lambda: sh.pose_bins(0.05, math.radians(2.0)))
    lines.append(f"(4) slam_pf_pose_bins (5 cm, 2 deg)      {fmt(t)}   k = {sh.pose_bins(0.05, math.radians(2.0))}, "
                 f"KLD count {pkg.kld_particle_count(sh.pose_bins(0.05, math.radians(2.0)))}")
    t0 = time.perf_counter()
    p, lw, l = sh.download()                                   # materialises: plain maps from here on
    t_down = time.perf_counter() - t0
    seen = sh.meta()["seen"]
    t0 = time.perf_counter()
    same.upload(p, lw, l, seen)
    t_up = time.perf_counter() - t0
    lines.append(f"(5) slam_pf_download {t_down * 1e3:.0f} ms (with its materialise pass), slam_pf_upload {t_up * 1e3:.0f} ms, once each: the host round trip of a "
                 f"clone {(t_down + t_up) * 1e3:.0f} ms")
    del p, lw, l
    sh.normalize(0.0, 1.0)                                     # (a pending shift again, as in the first block)
    block("plain maps, after the download")
    for f in (same, half, sel):
        f.close()
    pf.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    NP = int(opt("--np", 262144))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "pf_copy_bench.txt"))
    if "--measure" in sys.argv:
        measure(NP, out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", "--np", str(NP), "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
