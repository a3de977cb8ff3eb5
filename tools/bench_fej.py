#!/usr/bin/env python3
"""Times of the first-estimates Jacobian calls (libslamhip_fej.so, csrc/ekf_fej.hip) at the C3 shape of bench.py -- fp32, 10 000
landmarks, after 20 bench steps -- and a record of the pose NEES of sim(fej=True) beside the plain sim.  GPU only; nothing is
asserted.  In ONE process, every contender on a clone of its own of the state the bench steps left (slam_ekf_copy, with room for
the landmarks the augment contenders add), alternating:
  (1) fej.predict beside slam_ekf_predict: both are enqueued, so a repeat times CALLS calls and one synchronise after them;
  (2) fej.update with 8 matched observations beside slam_ekf_update_iterated(max_iter = 1) and slam_ekf_update with the same 8;
      and with ALL the step's matched observations: fej.update in batches of 8, one down-date each, beside slam_ekf_update's one
      wide down-date -- what the 16-column panel costs a full step;
  (3) fej.add_features of one landmark beside slam_ekf_augment;
  (4) slam_ekf_copy_floor: the bare read + rewrite of the stored tiles, the memory side of any down-date.
Protocol: every contender is warmed up (WARM calls), then REPEATS = 5 repeats; a repeat visits the contenders in turn (alternating,
so that drift of the machine hits all alike) and times CALLS calls of each, wall clock; per contender the median of its five repeat
means is reported with (min, max).  Then, with the library's event timers on, the mean time of every bracketed launch of one more
round (the front half is bracketed as `factor`, the panel kernel as `w1`, the strip kernel as `predict`).
The NEES record: SEEDS seeds of the golden course, NEES_STEPS steps each, fp64, the pose NEES e' inv(P_vv) e (3 degrees of freedom;
filt.nees(pose, ids=[])) taken every NEES_EVERY steps from the monitor hook of sim(), and the whole-map NEES per degree of freedom
from sim(nees_every=...).  It is a RECORD, not a claim: no figure of it is promised or tested.
The measuring process runs under `timeout -k 10`.
  python tools/bench_fej.py [--out FILE]      (FILE: default profiles/fej_bench.txt)"""
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
ROOM = 512                                                                # landmarks the augment contenders may add to their clones
SEEDS, NEES_STEPS, NEES_EVERY = 20, 3000, 50


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
    Q = np.array([[0.25, 0.0], [0.0, (3 * np.pi / 180) ** 2]])
    zz8, ii8 = np.ascontiguousarray(z_all[:, :8].T), np.ascontiguousarray(ids_all[:8], dtype=np.int32)
    zza, iia = np.ascontiguousarray(z_all.T), np.ascontiguousarray(ids_all, dtype=np.int32)
    zn = np.array([[35.0], [0.4]])
    clones = []

    def clone(fej):
        c = st.copy(max_landmarks=N + ROOM)
        clones.append(c)
        return (c, c.fej()) if fej else (c, None)

    def fej_predict():
        c, f = clone(True)
        return lambda: f.predict(7.5, 0.05, 4.0, Q, 0.025)

    def predict():
        c, _ = clone(False)
        return lambda: c.predict(7.5, 0.05, 4.0, Q, 0.025)

    def fej_update8():                                                    # the C call, like its two neighbours
        (c, f), out = clone(True), np.zeros(4)
        args = (f._f, dp(zz8), ip(ii8), 8, dp(rr), dp(out))
        fn = L.fej_lib().slam_ekf_fej_update
        return lambda: L.check(fn(*args))

    def fej_update(z, ids):
        c, f = clone(True)
        return lambda: f.update(z, B.R, ids)

    def iterated():
        c, out = clone(False)[0], np.zeros(10)
        args = (c._h, dp(zz8), ip(ii8), 8, dp(rr), 1, 0.0, dp(out))
        fn = L.iterated_lib().slam_ekf_update_iterated
        return lambda: L.check(fn(*args))

    def update(zz, ii):
        c = clone(False)[0]
        args = (c._h, dp(zz), ip(ii), int(ii.size), dp(rr), L.SLAM_FORM_CHOLESKY)
        return lambda: L.check(L.lib.slam_ekf_update(*args))

    def fej_augment():
        c, f = clone(True)
        return lambda: f.add_features(zn, B.R)

    def augment():
        c = clone(False)[0]
        return lambda: c.add_features(zn, B.R)

    m_all = int(ids_all.size)
    contenders = {
        "fej.predict": fej_predict(), "slam_ekf_predict": predict(),
        "fej.update m = 8": fej_update8(), "update_iterated max_iter = 1": iterated(),
        "slam_ekf_update m = 8": update(zz8, ii8),
        f"fej.update m = {m_all} ({(m_all + 7) // 8} batches)": fej_update(z_all, ids_all), f"slam_ekf_update m = {m_all}": update(zza, iia),
        "fej.add_features 1": fej_augment(), "slam_ekf_augment 1": augment(),
    }
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
    lines = [f"first-estimates Jacobian calls, fp32, {N} landmarks (n = {3 + 2 * N}), on clones of the state after {STEPS} bench steps "
             f"({matched[-1]} of {NZ} observations matched in the last)",
             f"ms per call, wall clock: median of {REPEATS} repeats of {CALLS} calls (and one synchronise) after {WARM} warm-up calls, the "
             "contenders visited in turn in every repeat"]
    lines += [f"  {name:<{width}s} {statistics.median(ts):9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})" for name, ts in times.items()]
    lines.append(f"  {'slam_ekf_copy_floor':<{width}s} {floor_ms:9.4f} ms per pass ({floor_form}, 10 passes)")
    lines.append(f"  more than 8 observations per down-date are not in this library (the 16-column panel is its siblings' limit): a step of "
                 f"{m_all} matched observations costs {(m_all + 7) // 8} down-dates, as the two rows above show; 64 would cost eight")
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
    for c in clones:
        c.close()
    st.close()
    return lines


def measure_nees(pkg):
    Sm = pkg.sim
    golden = os.path.join(ROOT, "tests", "golden")
    wp = Sm.get_waypoints(os.path.join(golden, "course1.txt"))
    cfg = np.load(os.path.join(golden, "config1.npz"))
    pose = {False: [], True: []}
    whole = {False: [], True: []}
    for seed in range(SEEDS):
        for fej in (False, True):
            st = pkg.EKFSlamState(Sm.initial_pose(wp), np.zeros((3, 3)), dtype="f64", max_landmarks=64, grow=True)
            mine = []

            def monitor(vehicle, filt, nsteps):
                if nsteps % NEES_EVERY == 0 and filt.N:
                    try:
                        mine.append(float(filt.nees(np.asarray(vehicle.pose, dtype=float), ids=[])))
                    except pkg.NotPositiveDefinite:
                        mine.append(float("nan"))

            try:
                log = Sm.sim(st, wp, cfg["landmarks"], seed=seed, nlaps=2, max_steps=NEES_STEPS, fej=fej, nees_every=NEES_EVERY,
                             monitor=monitor)
            finally:
                st.close()
            pose[fej].append(float(np.nanmean(mine)))
            whole[fej].append(float(np.nanmean([v / dof for _, v, dof in log.nees if dof > 3])))
    lines = [f"NEES of sim(fej=True) beside the plain sim: {SEEDS} seeds of the golden course, {NEES_STEPS} steps each, fp64, taken every "
             f"{NEES_EVERY} steps and averaged over a run.  A RECORD, not a claim: no figure here is promised or tested.",
             "  pose NEES e' inv(P_vv) e (ideal: 3), per-run means over the seeds:"]
    for fej, name in ((False, "standard"), (True, "FEJ")):
        v = pose[fej]
        lines.append(f"    {name:<9s} mean {statistics.mean(v):8.3f}  median {statistics.median(v):8.3f}  (min {min(v):.3f}, max {max(v):.3f})")
    lines.append("  whole-map NEES per degree of freedom (ideal: 1), per-run means over the seeds:")
    for fej, name in ((False, "standard"), (True, "FEJ")):
        v = whole[fej]
        lines.append(f"    {name:<9s} mean {statistics.mean(v):8.3f}  median {statistics.median(v):8.3f}  (min {min(v):.3f}, max {max(v):.3f})")
    return lines


def measure(out_path):
    sys.path.insert(0, ROOT)
    import bench as B
    from __graft_entry__ import load_package
    pkg = load_package()
    lines = []
    for part in (lambda: measure_calls(pkg, B), lambda: measure_nees(pkg)):
        got = part() + [""]
        print("\n".join(got), flush=True)
        lines += got
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))


def main():
    out_path = opt("--out", os.path.join(ROOT, "profiles", "fej_bench.txt"))
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
