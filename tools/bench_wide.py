#!/usr/bin/env python3
"""Times of the joint update of libslamhip_wide.so (csrc/ekf_wide.hip) at the C3 shape of bench.py -- fp32, 10 000 landmarks,
after 20 bench steps.  GPU only; nothing is asserted.  In ONE process, every contender on a clone of its own of the state the bench
steps left (slam_ekf_copy), alternating, on the step's matched observations and on 8 of them:
  (1) FirstEstimates.update_joint: one wide front half, one down-date;
  (2) FirstEstimates.update: the batched form, one 16-column down-date per 8 observations;
  (3) slam_ekf_update: the product's call on the same observations;
  (4) slam_ekf_copy_floor: the bare read + rewrite of the stored tiles, the memory side of any down-date.
Protocol (tools/bench_fej.py's): every contender is warmed up (WARM calls), then REPEATS = 5 repeats; a repeat visits the contenders
in turn and times CALLS calls of each, wall clock; per contender the median of its five repeat means is reported with (min, max).
Then, with the library's event timers on, the mean time of every bracketed launch of one more round: the wide chain brackets its model
and S kernels as `pht`, its factor kernel as `factor`, its panel kernel as `w1` and the down-date as `syrk`.
Not measured: fp64, other map sizes.  The measuring process runs under `timeout -k 10`.
  python tools/bench_wide.py [--out FILE]      (FILE: default profiles/wide_bench.txt)"""
import ctypes
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 560
STEPS, NZ, N = 20, 64, 10000
WARM, REPEATS, CALLS = 5, 5, 20


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def mean_ms(fn, calls, sync):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure_calls(pkg, B):
    st, zs = B.make_workload_on_device(pkg, N, NZ, STEPS, B.SEED, "f32", 0)
    matched = [B.gpu_step(st, z) for z in zs]
    a = st.associate_vector(zs[0], B.R, B.GATE1, B.GATE2)
    ids_all = a[a > 0]
    z_all = zs[0][:, a > 0]
    assert ids_all.size >= 8, "the bench scene matches fewer than 8 observations"
    L = pkg._lib
    dp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    rr = np.ascontiguousarray(B.R.T).reshape(4)
    clones = []

    def clone(fej):
        c = st.copy()
        clones.append(c)
        return (c, c.fej()) if fej else (c, None)

    def joint(z, ids):
        c, f = clone(True)
        return lambda: f.update_joint(z, B.R, ids)

    def batched(z, ids):
        c, f = clone(True)
        return lambda: f.update(z, B.R, ids)

    def update(z, ids):
        c = clone(False)[0]
        zz, ii = np.ascontiguousarray(z.T), np.ascontiguousarray(ids, dtype=np.int32)
        args = (c._h, dp(zz), ip(ii), int(ii.size), dp(rr), L.SLAM_FORM_CHOLESKY)
        keep.append((zz, ii))
        return lambda: L.check(L.lib.slam_ekf_update(*args))

    keep = []
    m_all = int(ids_all.size)
    contenders = {}
    for m in (m_all, 8):
        z, ids = z_all[:, :m], ids_all[:m]
        contenders[f"update_joint m = {m}"] = joint(z, ids)
        contenders[f"fej.update m = {m} ({(m + 7) // 8} batches)"] = batched(z, ids)
        contenders[f"slam_ekf_update m = {m}"] = update(z, ids)
    syncs = {name: c.sync for name, c in zip(contenders, clones)}
    for name, fn in contenders.items():
        for _ in range(WARM):
            fn()
        syncs[name]()
    times = {name: [] for name in contenders}
    for _ in range(REPEATS):
        for name, fn in contenders.items():
            times[name].append(mean_ms(fn, CALLS, syncs[name]))
    floor_ms, floor_form = st.copy_floor(10)
    width = max(len(name) for name in contenders) + 2
    med = {name: statistics.median(ts) for name, ts in times.items()}
    lines = [f"the joint update of libslamhip_wide.so, fp32, {N} landmarks (n = {3 + 2 * N}), on clones of the state after {STEPS} bench steps "
             f"({matched[-1]} of {NZ} observations matched in the last)",
             f"ms per call, wall clock: median of {REPEATS} repeats of {CALLS} calls (and one synchronise) after {WARM} warm-up calls, the "
             "contenders visited in turn in every repeat"]
    lines += [f"  {name:<{width}s} {med[name]:9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})" for name, ts in times.items()]
    lines.append(f"  {'slam_ekf_copy_floor':<{width}s} {floor_ms:9.4f} ms per pass ({floor_form}, 10 passes)")
    names = list(contenders)
    for q, m in ((0, m_all), (3, 8)):
        j, b, p = med[names[q]], med[names[q + 1]], med[names[q + 2]]
        lines.append(f"  m = {m}: the batched form takes {b / j:.2f} x the joint update; the joint update takes {j / p:.2f} x slam_ekf_update")
    lines.append("mean ms per bracketed launch (slam_ekf_timing, an event pair around every launch; launches in brackets):")
    for (name, fn), c in zip(contenders.items(), clones):
        c.timing(True)
        c.timing_reset()
        for _ in range(CALLS):
            fn()
        c.sync()
        rd = c.timing_read()
        lines.append(f"  {name:<{width}s} " + ", ".join(f"{kn} {ms / cnt:.4f} [{cnt}]" for kn, (ms, cnt) in rd.items() if cnt))
        c.timing(False)
    lines.append("not measured: fp64, other map sizes")
    for c in clones:
        c.close()
    st.close()
    return lines


def measure(out_path):
    sys.path.insert(0, ROOT)
    import bench as B
    from __graft_entry__ import load_package
    pkg = load_package()
    lines = measure_calls(pkg, B) + [""]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))


def main():
    out_path = opt("--out", os.path.join(ROOT, "profiles", "wide_bench.txt"))
    if "--measure" in sys.argv:
        measure(out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
