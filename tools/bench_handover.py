#!/usr/bin/env python3
"""Times of the hand-over between the two filters (libslamhip_handover.so, csrc/handover.hip) at the C4 shape of bench.py: fp32,
262 144 particles x 512 landmarks, after 20 steps of the bench's scene under the Neff rule.  In ONE process:
  (1) slam_pf_to_ekf of all 512 landmarks (D = 1027: 45 tiles of 128 x 128, 32 slabs of 8192 particles);
  (2) slam_pf_get_map of the same landmarks: one pass over the records, the comparator (it is also the hand-over's first pass);
  (3) the host route: slam_pf_download, the weighted covariance in NumPy (float64, the BLAS of the installation on 16 threads),
      slam_ekf_set_state -- timed piece by piece, once;
  (4) slam_ekf_to_pf into a second filter of the same shape, beside hipMemsetAsync of the bytes it writes (the store floor).
(1), (2), (4): wall time around the call (each synchronises), median of 7 after 2 warm-up calls (min, max).
"useful flop" = 2 n D (D + 1) / 2, the lower triangle; "executed" = 2 n E^2 per computed tile.  (1) - (2) bounds the Gram and fold
kernels from above (the rest of the call: the weights, two events, the side array); kernel times proper come from a rocprofv3 run.
The measuring process runs under `timeout -k 10`.
  python tools/bench_handover.py [--np N] [--out FILE]      (FILE: default profiles/handover_bench.txt)"""
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
MFMA_F32_PEAK = 157.3e12              # MI355X_MICROARCH: fp32 matrix rate (the guide's 155-157 TF)


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
    """The HIP runtime this process already uses (torch's, which libslamhip.so shares), for hipMemsetAsync."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        return None
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int
    return hip


def measure(NP, out_path, quick):
    sys.path.insert(0, ROOT)
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    os.environ.setdefault("OMP_NUM_THREADS", "16")
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
    D = 3 + 2 * NL
    E, slab = 128, 8192
    T = (D + E - 1) // E
    useful = 2.0 * NP * D * (D + 1) / 2
    executed = 2.0 * NP * E * E * T * (T + 1) / 2
    rec_bytes = 4.0 * NP * (5 * NL + 4)
    lines = [f"hand-over at the C4 shape: fp32, {NP} particles x {NL} landmarks (D = {D}), after {STEPS} bench steps under the Neff rule "
             f"(Neff {neff:.0f}, {pf.resamples} resamplings); records {rec_bytes / 1e9:.2f} GB",
             "ms around a synchronising call, median of 7 after 2 warm-up calls (min, max)"]
    st = pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype="f32", max_landmarks=NL)
    every = np.arange(1, NL + 1)
    t1 = median_ms(lambda: sh.to_ekf_into(st, every))
    t2 = median_ms(lambda: sh.get_map(every))
    lines.append(f"(1) slam_pf_to_ekf, {NL} landmarks          {t1[0]:9.3f} ms (min {t1[1]:.3f}, max {t1[2]:.3f})   useful {useful / 1e9:.0f} Gflop, "
                 f"executed {executed / 1e9:.0f} Gflop in {T * (T + 1) // 2} tiles x {(NP + slab - 1) // slab} slabs")
    lines.append(f"(2) slam_pf_get_map, {NL} landmarks         {t2[0]:9.3f} ms (min {t2[1]:.3f}, max {t2[2]:.3f})   {rec_bytes / 1e9:.2f} GB read: "
                 f"{rec_bytes / (t2[0] * 1e-3) / 1e9:.0f} GB/s")
    rest = max(t1[0] - t2[0], 1e-9)
    lines.append(f"    (1) - (2) = {rest:.3f} ms >= Gram + fold kernels: useful {useful / (rest * 1e-3) / 1e12:.1f} TFLOP/s, executed "
                 f"{executed / (rest * 1e-3) / 1e12:.1f} TFLOP/s = {100 * executed / (rest * 1e-3) / MFMA_F32_PEAK:.0f} % of the fp32 matrix peak "
                 f"({MFMA_F32_PEAK / 1e12:.0f} TF); floor of the useful flop at that peak {useful / MFMA_F32_PEAK * 1e3:.2f} ms; "
                 f"(1) / (2) = {t1[0] / t2[0]:.2f}")
    xg, Pg = st.download()
    if not quick:
        # (3) the host route, once, piece by piece
        t0 = time.perf_counter()
        p, lw, l = sh.download()
        t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        w = np.exp(lw.astype(np.float64))
        w /= w.sum()
        z = np.empty((NP, D))
        z[:, :3] = p.T
        z[:, 3::2] = l[:, 0].T
        z[:, 4::2] = l[:, 1].T
        mu = w @ z
        mu[2] = math.atan2(w @ np.sin(z[:, 2]), w @ np.cos(z[:, 2]))
        z -= mu
        z[:, 2] = np.where(z[:, 2] > math.pi, z[:, 2] - 2 * math.pi, np.where(z[:, 2] < -math.pi, z[:, 2] + 2 * math.pi, z[:, 2]))
        Ph = z.T @ (w[:, None] * z)
        k = np.arange(NL)
        Ph[3 + 2 * k, 3 + 2 * k] += w @ l[:, 2].T.astype(np.float64)
        Ph[4 + 2 * k, 3 + 2 * k] += w @ l[:, 3].T.astype(np.float64)
        Ph[3 + 2 * k, 4 + 2 * k] += w @ l[:, 3].T.astype(np.float64)
        Ph[4 + 2 * k, 4 + 2 * k] += w @ l[:, 4].T.astype(np.float64)
        t_cov = time.perf_counter() - t0
        s2 = pkg.EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype="f32", max_landmarks=NL)
        t0 = time.perf_counter()
        s2.set_state(mu, (Ph + Ph.T) / 2)
        s2.sync()
        t_up = time.perf_counter() - t0
        s2.close()
        host = t_down + t_cov + t_up
        scale = np.sqrt(np.outer(np.diag(Ph), np.diag(Ph)))
        lines.append(f"(3) host route, all {NP} particles         {host * 1e3:9.1f} ms = download {t_down * 1e3:.1f} + NumPy float64 covariance "
                     f"({os.environ['OMP_NUM_THREADS']} threads) {t_cov * 1e3:.1f} + set_state {t_up * 1e3:.1f};  (3) / (1) = {host * 1e3 / t1[0]:.0f}")
        lines.append(f"    device against host result: max |dP| / sqrt(P_aa P_bb) = {float(np.max(np.abs(Pg - Ph) / scale)):.2e}, "
                     f"max |dx| = {float(np.max(np.abs(xg - mu))):.2e}")
        del p, lw, l, z, Ph
    # (4) the other direction, into a second filter of the same shape
    dst = pkg.PFShard(NP, NL, 7, dtype="f32")
    t4 = median_ms(lambda: dst.from_ekf(st))
    lines.append(f"(4) slam_ekf_to_pf, {NL} landmarks          {t4[0]:9.3f} ms (min {t4[1]:.3f}, max {t4[2]:.3f})   {rec_bytes / 1e9:.2f} GB written: "
                 f"{rec_bytes / (t4[0] * 1e-3) / 1e9:.0f} GB/s")
    hip = loaded_hip()
    buf = torch.empty(int(rec_bytes), dtype=torch.uint8, device="cuda")
    if hip is not None:
        def fill():
            assert hip.hipMemsetAsync(ctypes.c_void_p(buf.data_ptr()), 0, int(rec_bytes), None) == 0
            assert hip.hipDeviceSynchronize() == 0
        name = "hipMemsetAsync"
    else:
        def fill():
            buf.zero_()
            torch.cuda.synchronize()
        name = "torch zero_ (the runtime's library was not found among the mapped files)"
    t5 = median_ms(fill)
    lines.append(f"    {name} of the same bytes            {t5[0]:9.3f} ms (min {t5[1]:.3f}, max {t5[2]:.3f})   {rec_bytes / (t5[0] * 1e-3) / 1e9:.0f} GB/s;  "
                 f"(4) / store floor = {t4[0] / t5[0]:.2f}")
    dst.close()
    st.close()
    pf.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    NP = int(opt("--np", 262144))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "handover_bench.txt"))
    if "--measure" in sys.argv:
        measure(NP, out_path, "--quick" in sys.argv)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", "--np", str(NP), "--out", out_path]
    if "--quick" in sys.argv:
        cmd.append("--quick")
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
