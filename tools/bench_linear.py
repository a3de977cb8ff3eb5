#!/usr/bin/env python3
"""Times of the caller-supplied models (libslamhip_linear.so, csrc/ekf_linear.hip) at the C3 shape of bench.py: fp32, 10 000
landmarks, after 20 bench steps.  In ONE process, on ONE state:
  (1) update_linear with k = 2 and k = 16 rows: the rows and innovations of 1 and of 8 range-bearing observations, taken from
      slam_ekf_predict_observation (innovation mode), i.e. the SAME measurement as the yardstick's;
  (2) the yardstick: slam_ekf_update with m = 1 and m = 8 observations of those landmarks (k = 2 m);
  (3) slam_ekf_copy_floor: the bare read + rewrite of the stored tiles, the memory side of any down-date;
  (4) predict_odometry beside slam_ekf_predict (neither synchronises: CALLS calls, then one slam_ekf_sync, per call).
Protocol: every contender is warmed up (WARM calls), then REPEATS = 5 repeats; a repeat visits the contenders in turn (alternating,
so that drift of the machine hits all alike) and times CALLS calls of each, wall clock around calls that end in a device
synchronise; per contender the median of its five repeat means is reported with (min, max).  The margin of the comparison is the
spread (max - min) of the yardstick's own five repeats.  Then, with the library's event timers on, the mean time of every
bracketed launch of one more round of (1) and (2): where a difference lies.
The measuring process runs under `timeout -k 10`.
  python tools/bench_linear.py [--landmarks N] [--out FILE]      (FILE: default profiles/linear_bench.txt)"""
import ctypes
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 420
STEPS, NZ = 20, 64
WARM, REPEATS, CALLS = 5, 5, 20


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def mean_ms(fn, calls, after=None):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    if after is not None:
        after()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(N, out_path):
    sys.path.insert(0, ROOT)
    import bench as B
    from __graft_entry__ import load_package
    pkg = load_package()
    O = __import__("oracle.ekf_ref", fromlist=["ekf_ref"])
    st, zs = B.make_workload_on_device(pkg, N, NZ, STEPS, B.SEED, "f32", 0)
    matched = [B.gpu_step(st, z) for z in zs]
    a = st.associate_vector(zs[0], B.R, B.GATE1, B.GATE2)
    ids = a[a > 0][:8]
    z = zs[0][:, a > 0][:, :8]
    assert ids.size == 8, "the bench scene matches fewer than 8 observations"
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
    Q3 = np.diag([0.01, 0.01, 0.0004])

    L = pkg._lib
    fn_linear = L.linear_lib().slam_ekf_update_linear
    keep = []
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def linear(m):
        Hs, v = [], []
        for i in range(m):
            zp, H = st.predict_observation(int(ids[i]))
            nz = np.flatnonzero(H.any(axis=0))
            Hs.append([{int(c): float(H[r, c]) for c in nz if H[r, c] != 0.0} for r in range(2)])
            v += [z[0, i] - zp[0], O.mpi_to_pi(z[1, i] - zp[1])]
        # the C entry point itself, its arguments marshalled once: the yardstick below is called the same way
        ptr, idx, val = pkg.ekf.linear_rows([r for pair in Hs for r in pair], st.n)
        vv, RR, out = np.array(v), np.ascontiguousarray(np.kron(np.eye(m), B.R)), np.zeros(4)
        args = (st._h, 2 * m, ip(ptr), ip(idx), dp(val), dp(vv), dp(RR), L.SLAM_LINEAR_INNOVATION, 0, dp(out))
        keep.append((ptr, idx, val, vv, RR, out))
        return lambda: L.check(fn_linear(*args))

    def update(m):
        zz = np.ascontiguousarray(z[:, :m].T)
        ii = np.ascontiguousarray(ids[:m], dtype=np.int32)
        rr = np.ascontiguousarray(B.R.T).reshape(4)
        args = (st._h, dp(zz), ip(ii), m, dp(rr), L.SLAM_FORM_CHOLESKY)
        keep.append((zz, ii, rr))
        return lambda: L.check(L.lib.slam_ekf_update(*args))

    contenders = {
        "update_linear k = 2": linear(1),
        "slam_ekf_update m = 1": update(1),
        "update_linear k = 16": linear(8),
        "slam_ekf_update m = 8": update(8),
    }
    for fn in contenders.values():
        for _ in range(WARM):
            fn()
    times = {name: [] for name in contenders}
    for _ in range(REPEATS):
        for name, fn in contenders.items():
            times[name].append(mean_ms(fn, CALLS))
    floor_ms, floor_form = st.copy_floor(10)
    strips = {
        "predict_odometry": lambda: st.predict_odometry([0.2, 0.0, 0.001], Q3),
        "slam_ekf_predict": lambda: st.predict(8.0, 0.01, 4.0, Q, 0.025),
    }
    for fn in strips.values():
        for _ in range(WARM):
            fn()
    st.sync()
    stimes = {name: [] for name in strips}
    for _ in range(REPEATS):
        for name, fn in strips.items():
            stimes[name].append(mean_ms(fn, 200, st.sync))

    def row(name, ts):
        return f"  {name:<24s} {statistics.median(ts):9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})"

    lines = [f"caller-supplied models at the C3 shape: fp32, {N} landmarks (n = {3 + 2 * N}), after {STEPS} bench steps "
             f"({matched[-1]} of {NZ} observations matched in the last)",
             f"ms per call, wall clock around synchronising calls: median of {REPEATS} repeats of {CALLS} calls after {WARM} warm-up calls, "
             "the contenders visited in turn in every repeat"]
    lines += [row(name, ts) for name, ts in times.items()]
    lines.append(f"  slam_ekf_copy_floor      {floor_ms:9.4f} ms per pass ({floor_form}, 10 passes)")
    for k, m in ((2, 1), (16, 8)):
        lin, ref = times[f"update_linear k = {k}"], times[f"slam_ekf_update m = {m}"]
        diff, margin = statistics.median(lin) - statistics.median(ref), max(ref) - min(ref)
        verdict = "inside the yardstick's own spread" if diff <= margin else "SLOWER than the yardstick by more than its spread"
        lines.append(f"  k = {k}: update_linear - slam_ekf_update = {diff:+.4f} ms; spread of the yardstick's five repeats {margin:.4f} ms: {verdict}")
    lines.append("ms per call, 200 calls and one slam_ekf_sync (the predicts do not synchronise):")
    lines += [row(name, ts) for name, ts in stimes.items()]
    # per-launch times from the library's event timers: one more round
    lines.append("mean ms per bracketed launch (slam_ekf_timing, an event pair around every launch; launches in brackets):")
    st.timing(True)
    for name, fn in contenders.items():
        st.timing_reset()
        for _ in range(CALLS):
            fn()
        st.sync()
        rd = st.timing_read()
        parts = ", ".join(f"{kn} {ms / cnt:.4f} [{cnt}]" for kn, (ms, cnt) in rd.items() if cnt)
        lines.append(f"  {name:<24s} {parts}")
    st.timing(False)
    st.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    N = int(opt("--landmarks", 10000))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "linear_bench.txt"))
    if "--measure" in sys.argv:
        measure(N, out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", "--landmarks", str(N), "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
