#!/usr/bin/env python3
"""Time of slam_ekf_factor_compute / solve / multiply (libslamhip_factor.so, csrc/ekf_factor.hip) on the C3 state -- fp32, N = 10 000
landmarks (n = 20 003) after 20 bench steps -- beside the host route and the traffic floor, on one GPU.  In ONE process:
  (1) the host route: download() of the matrix, then numpy.linalg.cholesky (LAPACK potrf on the threads OMP_NUM_THREADS allows);
  (2) slam_ekf_copy_floor of the state: every stored tile read once and written back, the fastest of 10 passes;
  (3) per panel_tiles in 1, 2, 4: compute into an fp32 factor and into an fp64 factor of the same state, median of 5 after one
      warm-up.  compute synchronises (it reads info back), so the time is the wall time around the call: the launches, the device
      work and one read-back.  Beside it: the launches of one factorisation, the passes over the trailing matrix it makes (target
      tiles read and written, in units of the whole matrix), those passes at the floor's rate, TFLOP/s of n^3 / 3;
  (4) solve and multiply at r = 1 and 64 on the default fp32 factor, beside one read of L at the floor's rate.
The kernel families' shares come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_factor.py
--measure --once PT DTYPE` (one compute, one solve and one multiply at r = 64).
C5 (fp64, N = 50 000) is run once (--c5) only if the fp64 time at C3 scaled by (n_C5 / n_C3)^3 predicts under a minute; otherwise the
prediction is recorded as a prediction.
The only assertion: the device route (download not needed) is faster than the host route measured beside it.
The measuring process runs under `timeout -k 10`.
  python tools/bench_factor.py [N] [--out FILE] [--c5]      (FILE: default profiles/factor_bench.txt)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 900
EDGE = {"f32": 128, "f64": 64}
ESZ = {"f32": 4, "f64": 8}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    ts = [wall_ms(fn) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def schedule(n, dtype, pt):
    """(launches, passes over the trailing matrix) of one factorisation: the loop of enqueue_factor (csrc/ekf_factor.hip)."""
    E = EDGE[dtype]
    T = (n + E - 1) // E
    launches, target_tiles = 2, 0                                     # the copy-in and the x snapshot
    for k0 in range(0, T, pt):
        k1 = min(k0 + pt, T)
        for k in range(k0, k1):
            launches += 1 + (k + 1 < T) + (k + 1 < k1)
            if k + 1 < k1:
                target_tiles += sum(T - J for J in range(k + 1, k1))
        if k1 < T:
            launches += 1
            target_tiles += (T - k1) * (T - k1 + 1) // 2
    return launches, target_tiles / (T * (T + 1) / 2)


def c3_state(pkg, N):
    import bench as B
    x, P, zs = B.make_workload(N, 64, 20, 11)
    st = pkg.EKFSlamState(x, P, dtype="f32", max_landmarks=N)
    del P
    for z in zs:
        B.gpu_step(st, z)
    st.sync()
    return st


def measure(N, out_path, once=None, c5=False):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    st = c3_state(pkg, N)
    n = st.n
    if once is not None:                                              # one compute for a kernel trace
        f = pkg.CovarianceFactor(once[1], N, panel_tiles=int(once[0]))
        print(f.compute(st))
        B = np.random.default_rng(1).standard_normal((n, 64))
        f.whiten(B)                                                   # (the trace then also holds one solve and one multiply)
        f.colour(B)
        f.close()
        st.close()
        return
    stored = lambda d: (lambda t: t * (t + 1) // 2 * EDGE[d] ** 2 * ESZ[d])((n + EDGE[d] - 1) // EDGE[d])   # noqa: E731
    lines = [f"slam_ekf_factor_compute on the C3 state after 20 bench steps: fp32 state, N = {N}, n = {n}; "
             f"OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}",
             "times: wall ms around the synchronising call, median of 5 after one warm-up (min, max)"]
    t_dl = wall_ms(lambda: st.download("cov"))
    P = st.download("cov")
    t_chol = wall_ms(lambda: np.linalg.cholesky(P))
    del P
    host_ms = t_dl + t_chol
    lines.append(f"(1) host route: download {t_dl:9.1f} ms + numpy.linalg.cholesky (fp32) {t_chol:9.1f} ms = {host_ms:9.1f} ms")
    floor_ms, form = st.copy_floor(10)
    rate = 2 * stored("f32") / (floor_ms * 1e-3)                      # bytes per second, read + written
    lines.append(f"(2) slam_ekf_copy_floor ({form}): {floor_ms:8.3f} ms per pass over {stored('f32') / 1e6:.0f} MB, "
                 f"{rate / 1e12:5.2f} TB/s read + written")
    best = {}
    for dtype in ("f32", "f64"):
        for pt in (1, 2, 4):
            f = pkg.CovarianceFactor(dtype, N, panel_tiles=pt)
            med, lo, hi = median_ms(lambda: f.compute(st))
            launches, passes = schedule(n, dtype, pt)
            fl = passes * 2 * stored(dtype) / rate * 1e3
            lines.append(f"(3) compute {dtype} panel_tiles {pt}: {med:9.2f} ms (min {lo:.2f}, max {hi:.2f})   {launches:5d} launches   "
                         f"{passes:6.1f} passes = {passes * 2 * stored(dtype) / 1e9:7.1f} GB   floor {fl:8.2f} ms   time / floor {med / fl:5.2f}   "
                         f"{passes * 2 * stored(dtype) / (med * 1e-3) / 1e12:5.2f} TB/s   {n ** 3 / 3 / (med * 1e-3) / 1e12:6.2f} TFLOP/s   "
                         f"logdet {f.logdet:.6f}")
            if dtype not in best or med < best[dtype][1]:
                best[dtype] = (pt, med)
            f.close()
    for dtype in ("f32", "f64"):
        lines.append(f"    fastest for {dtype}: panel_tiles {best[dtype][0]} ({best[dtype][1]:.2f} ms)")
    f = pkg.CovarianceFactor("f32", N)
    f.compute(st)
    read_ms = stored("f32") / rate * 1e3
    rng = np.random.default_rng(1)
    for r in (1, 64):
        B = rng.standard_normal((n, r))
        ts = median_ms(lambda: f.whiten(B))
        tm = median_ms(lambda: f.colour(B))
        lines.append(f"(4) r = {r:2d}: solve {ts[0]:8.2f} ms (min {ts[1]:.2f})   multiply {tm[0]:8.2f} ms (min {tm[1]:.2f})   "
                     f"one read of L at the floor's rate {read_ms:6.2f} ms   (default panel_tiles {f.panel_tiles})")
    f.close()
    n5 = 3 + 2 * 50000
    pred = best["f64"][1] * 1e-3 * (n5 / n) ** 3
    lines.append(f"C5 (fp64, N = 50 000, n = {n5}): the fp64 time at C3 times (n_C5 / n_C3)^3 PREDICTS {pred:.1f} s"
                 + ("" if pred < 60 else " -- above a minute: not run, a prediction only"))
    if pred < 60 and c5:
        import bench as B
        st.close()
        st5, _zs = B.make_workload_on_device(pkg, 50000, 64, 1, 11, "f64", 0)
        f5 = pkg.CovarianceFactor("f64", 50000, panel_tiles=best["f64"][0])
        t5 = wall_ms(lambda: f5.compute(st5))
        lines.append(f"C5 measured once: {t5 / 1e3:.2f} s, logdet {f5.logdet:.6f}")
        f5.close()
        st5.close()
    else:
        st.close()
    dev_ms = best["f32"][1]
    lines.append(f"device route {dev_ms:.2f} ms against host route {host_ms:.1f} ms: {host_ms / dev_ms:.1f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write(text)
    assert dev_ms < host_ms, "the device route is not faster than the host route"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("landmarks", nargs="?", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_bench.txt"))
    ap.add_argument("--c5", action="store_true", help="run C5 once if the prediction is under a minute")
    ap.add_argument("--measure", action="store_true", help="measure in this process (otherwise: a child under a time limit)")
    ap.add_argument("--once", nargs=2, metavar=("PT", "DTYPE"), help="with --measure: one compute, one solve, one multiply")
    args = ap.parse_args()
    if args.measure:
        measure(args.landmarks, args.out, once=args.once, c5=args.c5)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), str(args.landmarks), "--measure",
           "--out", args.out] + (["--c5"] if args.c5 else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
