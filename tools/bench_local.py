#!/usr/bin/env python3
"""Times of the compressed local-area updates (libslamhip_local.so, csrc/ekf_local.hip) at the C3 shape of bench.py: fp32, 10 000
landmarks, after 20 bench steps.  In ONE process, for an area of the 256 landmarks nearest the vehicle, then of 64 and of 1024:
  (a) one LOCAL step -- area.predict + area.update with the step's matched observations that lie in the area -- beside the GLOBAL
      step, slam_ekf_predict + slam_ekf_update with the same observations on a clone (slam_ekf_copy) of the same state;
  (b) close, beside slam_ekf_copy_floor (the bare read + rewrite of the stored tiles) and beside the global update of (a);
  (c) the break-even: close / (global step - local step), the number of steps an area must live to pay for its close.
Protocol: both contenders of (a) are warmed up (WARM calls), then REPEATS repeats; a repeat visits them in turn and times CALLS
calls of each, wall clock around calls that end in a device synchronise (slam_ekf_update reads its status back); the median of
the repeat means is reported with (min, max).  close is timed alone, wall clock around the call (it synchronises), REPEATS times,
each after a fresh open and one local step, the global stream drained before the clock starts; its first call (which allocates
the scratch) is the warm-up and is not counted.  The repeated updates shrink P; the times do not depend on its values.
The measuring process runs under `timeout -k 10`.
  python tools/bench_local.py [--landmarks N] [--out FILE]      (FILE: default profiles/local_bench.txt)"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 540
STEPS, NZ = 20, 64
WARM, REPEATS, CALLS = 5, 5, 20
AREAS = (256, 64, 1024)


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def mean_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(N, out_path):
    sys.path.insert(0, ROOT)
    import bench as B
    from __graft_entry__ import load_package
    pkg = load_package()
    st, zs = B.make_workload_on_device(pkg, N, NZ, STEPS, B.SEED, "f32", 0)
    matched = [B.gpu_step(st, z) for z in zs]
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * np.pi / 180) ** 2]])
    a = st.associate_vector(zs[0], B.R, B.GATE1, B.GATE2)
    gid, zall = a[a > 0], zs[0][:, a > 0]
    x = np.asarray(st.download("x"), dtype=np.float64)
    dist = np.hypot(x[3::2] - x[0], x[4::2] - x[1])
    order = np.argsort(dist, kind="stable")
    clone = st.copy()

    def row(name, ts):
        return f"  {name:<34s} {statistics.median(ts):9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})"

    lines = [f"compressed local-area updates at the C3 shape: fp32, {N} landmarks (n = {3 + 2 * N}), after {STEPS} bench steps "
             f"({matched[-1]} of {NZ} observations matched in the last)",
             f"(a) ms per step = predict + update, wall clock, median of {REPEATS} repeats of {CALLS} steps after {WARM} warm-up steps, the two "
             f"contenders visited in turn;  (b) ms per close, wall clock, {REPEATS} closes after one uncounted"]
    floor_ms, floor_form = st.copy_floor(10)
    lines.append(f"  slam_ekf_copy_floor                {floor_ms:9.4f} ms per pass ({floor_form}, 10 passes)")
    for K in AREAS:
        if K > N:
            continue
        ids = (order[:K] + 1).astype(np.int32)
        local_of = {int(g): i + 1 for i, g in enumerate(ids)}
        inside = np.array([int(g) in local_of for g in gid], dtype=bool)
        zin, gin = np.ascontiguousarray(zall[:, inside]), gid[inside]
        lin = np.array([local_of[int(g)] for g in gin], dtype=np.int32)
        area = pkg.LocalArea(st, ids, max_local=K)
        contenders = {
            "local step": lambda: (area.predict(8.0, 0.01, 4.0, Q, 0.025), area.update(zin, B.R, lin)),
            "global step (on a clone)": lambda: (clone.predict(8.0, 0.01, 4.0, Q, 0.025), clone.update(zin, B.R, gin)),
            "global update alone (on the clone)": lambda: clone.update(zin, B.R, gin),
        }
        for fn in contenders.values():
            for _ in range(WARM):
                fn()
        times = {name: [] for name in contenders}
        for _ in range(REPEATS):
            for name, fn in contenders.items():
                times[name].append(mean_ms(fn, CALLS))
        area.close()                                                        # the uncounted first close: allocates the scratch
        closes = []
        for _ in range(REPEATS):
            area.open(ids)
            contenders["local step"]()
            area.state.sync()
            st.sync()
            t0 = time.perf_counter()
            area.close()
            closes.append((time.perf_counter() - t0) * 1e3)
        area.destroy()
        n0 = 3 + 2 * K
        lines.append(f"area of the {K} nearest landmarks (n0 = {n0}), {lin.size} of the step's {gid.size} matched observations lie in it:")
        lines += [row(name, ts) for name, ts in times.items()]
        lines.append(row("close", closes))
        loc, glo, upd = (statistics.median(times[k]) for k in contenders)
        cl = statistics.median(closes)
        gain = glo - loc
        macs = (3 + 2 * N) ** 2 / 2 * n0
        lines.append(f"  close = {cl / floor_ms:.1f} copy floors = {cl / upd:.1f} global updates;  trailing product {macs / 1e9:.1f} G multiply-adds "
                     f"-> {macs / (cl * 1e-3) / 1e12:.2f} T multiply-adds/s if close were that alone")
        if gain > 0:
            lines.append(f"  a step saves {gain:.4f} ms (spread of the global step {max(times['global step (on a clone)']) - min(times['global step (on a clone)']):.4f} ms): "
                         f"break-even after {cl / gain:.0f} steps in the area")
        else:
            lines.append(f"  a local step is NOT faster than the global one ({gain:+.4f} ms): the area never pays")
    clone.close()
    st.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    N = int(opt("--landmarks", 10000))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "local_bench.txt"))
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
