#!/usr/bin/env python3
"""Times of the iterated update (libslamhip_iterated.so, csrc/ekf_iterated.hip) at the C3 shape of bench.py -- fp32, 10 000 landmarks,
after 20 bench steps -- and again at 1 000 landmarks.  GPU only; nothing is asserted.  In ONE process per shape, every contender on a
clone of its own of the state the bench steps left (slam_ekf_copy), with the SAME 8 matched observations:
  (1) slam_ekf_update_iterated with max_iter = 1, 5 and 20 and tol = 0: that many iterations unless an iterate repeats bit for
      bit first (the step is then exactly 0), which a state that has already taken the same observations does after a few; the
      iterations actually RUN (out[0]) are recorded beside every time.  And slam_ekf_iterated_nis, the solve kernel alone on a
      state it does not change, with the same three limits: every call of it repeats the same iteration;
  (2) slam_ekf_update (Cholesky form) and slam_ekf_update_linear in innovation mode (the 16 rows and innovations taken from
      slam_ekf_predict_observation): the two one-shot updates the library had;
  (3) slam_ekf_copy_floor: the bare read + rewrite of the stored tiles, the memory side of any down-date.
The quantity of interest is the time per EXTRA iteration, (t(k) - t(1)) / (iterations run - 1), and whether it depends on N.
Protocol: every contender is warmed up (WARM calls), then REPEATS = 5 repeats; a repeat visits the contenders in turn (alternating,
so that drift of the machine hits all alike) and times CALLS calls of each, wall clock around calls that end in a device
synchronise; per contender the median of its five repeat means is reported with (min, max).  Then, with the library's event timers
on, the mean time of every bracketed launch of one more round: the solve kernel is bracketed as `factor`, the panel kernel as `w1`.
The measuring process runs under `timeout -k 10`.
  python tools/bench_iterated.py [--out FILE]      (FILE: default profiles/iterated_bench.txt)"""
import ctypes
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
SHAPES = (10000, 1000)
ITERS = (1, 5, 20)


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def mean_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure_shape(pkg, B, O, N):
    st, zs = B.make_workload_on_device(pkg, N, NZ, STEPS, B.SEED, "f32", 0)
    matched = [B.gpu_step(st, z) for z in zs]
    a = st.associate_vector(zs[0], B.R, B.GATE1, B.GATE2)
    ids = a[a > 0][:8]
    z = zs[0][:, a > 0][:, :8]
    assert ids.size == 8, "the bench scene matches fewer than 8 observations"
    L = pkg._lib
    keep, clones = [], []
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    zz = np.ascontiguousarray(z.T)
    ii = np.ascontiguousarray(ids, dtype=np.int32)
    rr = np.ascontiguousarray(B.R.T).reshape(4)

    def clone():
        clones.append(st.copy())
        return clones[-1]

    ran = {}                                                              # contender -> out[0] of every call: the iterations RUN

    def iterated(k, commit):
        c, out = clone(), np.zeros(10)
        fn = L.iterated_lib().slam_ekf_update_iterated if commit else L.iterated_lib().slam_ekf_iterated_nis
        args = (c._h, dp(zz), ip(ii), 8, dp(rr), k, 0.0, dp(out))
        log = ran.setdefault(f"{'update_iterated' if commit else 'iterated_nis'} max_iter = {k}", [])

        def call():
            L.check(fn(*args))
            log.append(out[0])
        return call

    def update():
        c = clone()
        args = (c._h, dp(zz), ip(ii), 8, dp(rr), L.SLAM_FORM_CHOLESKY)
        return lambda: L.check(L.lib.slam_ekf_update(*args))

    def linear():
        c = clone()
        Hs, v = [], []
        for i in range(8):
            zp, H = c.predict_observation(int(ids[i]))
            nz = np.flatnonzero(H.any(axis=0))
            Hs += [{int(q): float(H[r, q]) for q in nz if H[r, q] != 0.0} for r in range(2)]
            v += [z[0, i] - zp[0], O.mpi_to_pi(z[1, i] - zp[1])]
        ptr, idx, val = pkg.ekf.linear_rows(Hs, c.n)
        vv, RR, out = np.array(v), np.ascontiguousarray(np.kron(np.eye(8), B.R)), np.zeros(4)
        args = (c._h, 16, ip(ptr), ip(idx), dp(val), dp(vv), dp(RR), L.SLAM_LINEAR_INNOVATION, 0, dp(out))
        keep.append((ptr, idx, val, vv, RR, out))
        fn = L.linear_lib().slam_ekf_update_linear
        return lambda: L.check(fn(*args))

    contenders = {f"update_iterated max_iter = {k}": iterated(k, True) for k in ITERS}
    contenders.update({f"iterated_nis max_iter = {k}": iterated(k, False) for k in ITERS})
    contenders["slam_ekf_update m = 8"] = update()
    contenders["update_linear k = 16"] = linear()
    for fn in contenders.values():
        for _ in range(WARM):
            fn()
    times = {name: [] for name in contenders}
    for log in ran.values():
        del log[:]
    for _ in range(REPEATS):
        for name, fn in contenders.items():
            times[name].append(mean_ms(fn, CALLS))
    floor_ms, floor_form = st.copy_floor(10)

    def row(name, ts):
        return f"  {name:<30s} {statistics.median(ts):9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})"

    lines = [f"the iterated update, fp32, {N} landmarks (n = {3 + 2 * N}), on clones of the state after {STEPS} bench steps "
             f"({matched[-1]} of {NZ} observations matched in the last); 8 matched observations, tol = 0",
             f"ms per call, wall clock around synchronising calls: median of {REPEATS} repeats of {CALLS} calls after {WARM} warm-up calls, "
             "the contenders visited in turn in every repeat"]
    lines += [row(name, ts) for name, ts in times.items()]
    lines.append(f"  {'slam_ekf_copy_floor':<30s} {floor_ms:9.4f} ms per pass ({floor_form}, 10 passes)")
    med = {k: statistics.median(times[f"update_iterated max_iter = {k}"]) for k in ITERS}
    lines.append("iterations RUN per call in the timed repeats (tol = 0 stops an iteration early only where an iterate repeats bit for bit):")
    its = {name: statistics.mean(log) for name, log in ran.items()}
    lines += [f"  {name:<30s} mean {its[name]:6.2f}  (min {min(log):.0f}, max {max(log):.0f})" for name, log in ran.items()]
    for what in ("iterated_nis", "update_iterated"):
        t = {k: statistics.median(times[f"{what} max_iter = {k}"]) for k in ITERS}
        n = {k: its[f"{what} max_iter = {k}"] for k in ITERS}
        spread = max(times[f"{what} max_iter = 1"]) - min(times[f"{what} max_iter = 1"])
        per = ", ".join(f"(t({k}) - t(1)) / ({n[k]:.2f} - 1) = {(t[k] - t[1]) / (n[k] - 1) * 1e3:.2f} us" for k in ITERS[1:] if n[k] > 1)
        lines.append(f"  {what}, per extra iteration RUN: {per}; spread of max_iter = 1 over its five repeats {spread * 1e3:.2f} us")
    lines.append(f"  update_iterated max_iter = 1 - slam_ekf_update = {(med[1] - statistics.median(times['slam_ekf_update m = 8'])) * 1e3:+.2f} us, "
                 f"- update_linear = {(med[1] - statistics.median(times['update_linear k = 16'])) * 1e3:+.2f} us")
    lines.append("mean ms per bracketed launch (slam_ekf_timing, an event pair around every launch; launches in brackets):")
    for (name, fn), c in zip(contenders.items(), clones):
        c.timing(True)
        c.timing_reset()
        if name in ran:
            del ran[name][:]
        for _ in range(CALLS):
            fn()
        c.sync()
        rd = c.timing_read()
        parts = ", ".join(f"{kn} {ms / cnt:.4f} [{cnt}]" for kn, (ms, cnt) in rd.items() if cnt)
        if name in ran:
            parts += f"; iterations run: mean {statistics.mean(ran[name]):.2f}"
        lines.append(f"  {name:<30s} {parts}")
        c.timing(False)
    for c in clones:
        c.close()
    st.close()
    return lines


def measure(out_path):
    sys.path.insert(0, ROOT)
    import bench as B
    from __graft_entry__ import load_package
    pkg = load_package()
    O = __import__("oracle.ekf_ref", fromlist=["ekf_ref"])
    lines = []
    for N in SHAPES:
        part = measure_shape(pkg, B, O, N) + [""]
        print("\n".join(part), flush=True)
        lines += part
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    out_path = opt("--out", os.path.join(ROOT, "profiles", "iterated_bench.txt"))
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
