#!/usr/bin/env python3
"""Time of the per-particle trajectory history (libslamhip_path.so) beside the step it follows, on one GPU at the C4 shape:
fp32, 262144 particles x 512 landmarks, 16 known-id observations per step.  In ONE process:
  (1) slam_pf_step_normalized alone, and followed by slam_pf_path_record: per step over runs of 20 steps behind one final
      synchronisation (the step itself synchronises; the record is enqueued behind it), the two forms ALTERNATING, seven runs
      each, medians;
  (2) the same step followed by slam_pf_resample_local, and by slam_pf_path_resample, every step: alternating likewise;
  (3) the record alone: 50 enqueued back to back behind one synchronisation, per record -- with nothing pending (3 n values)
      and with a resampling pending (n int32 more) -- beside hipMemcpyAsync (device to device, the filter's stream) of the
      SAME bytes, 50 back to back likewise;
  (4) the read-outs slam_pf_path_mean / _survivors / _best on a ring of L = 64 and L = 256 records filled by the filter itself
      under the Neff rule (0.75 n): wall time around the synchronising call, median of 15 after 2 warm-up calls, the bytes the
      algorithm needs and their rate.
      mean       12 B per (particle, record) gathered + 4 B per (particle, record with ancestors) + 4 n (log-weights)
      survivors  per record with ancestors: n mark bytes read, n cleared, 4 B per marked particle's ancestor, 1 B per mark set
      best       4 n (log-weights) + 16 L
The measuring process runs under `timeout -k 10`.
  python tools/bench_pf_path.py [n] [nl] [--out FILE]      (FILE: default profiles/pf_path_bench.txt)"""
import ctypes as C
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12
TIMEOUT_S = 420
M = 16
RUN = 20
ROUNDS = 7
B2B = 50


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


def hip_runtime():
    """The HIP runtime this process already runs on (the one libslamhip.so was resolved against), by its path."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if len(paths) != 1:
        raise RuntimeError(f"expected one loaded HIP runtime, found {sorted(paths)}")
    rt = C.CDLL(paths.pop())
    rt.hipMemcpyAsync.restype = C.c_int
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return rt


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def alternating(forms, rounds=ROUNDS):
    """Median, min and max (us per step) of each form, the forms taking turns; one untimed turn of each first."""
    for fn in forms:
        fn()
    ts = [[] for _ in forms]
    for _ in range(rounds):
        for k, fn in enumerate(forms):
            ts[k].append(wall(fn) / RUN * 1e6)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def median_us(fn, reps=15, warm=2, per=1):
    for _ in range(warm):
        fn()
    ts = [wall(fn) / per * 1e6 for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def measure(n, nl, out_path):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    import torch
    Q = np.array([[0.5 ** 2, 0.0], [0.0, (3 * math.pi / 180) ** 2]])
    R = np.array([[0.1 ** 2, 0.0], [0.0, (math.pi / 180) ** 2]])
    rng = np.random.default_rng(20240602)
    lm = rng.uniform(-200, 200, (nl, 2))
    pf = pkg.PFSlamState(n, nl, seed=20240602, dtype="f32", distributed=False)
    sh = pf.shard
    sh.set_pose([0.0, 0.0, 0.3])
    sh.init_landmarks(lm, 0.01, 0.1)
    state = dict(pose=np.array([0.0, 0.0, 0.3]), t=0, resamples=0)

    def step():
        """One step_fused_normalized along the nominal path: (Neff, largest normalised log-weight)."""
        p = state["pose"]
        p = np.array([p[0] + 0.2 * math.cos(p[2]), p[1] + 0.2 * math.sin(p[2]), p[2]])
        ids = (np.arange(M) + M * state["t"]) % nl + 1
        dx, dy = lm[ids - 1, 0] - p[0], lm[ids - 1, 1] - p[1]
        z = np.vstack([np.hypot(dx, dy), np.arctan2(dy, dx) - p[2]]) + rng.normal(0, [[0.1], [math.pi / 180]], (2, M))
        state["pose"], state["t"] = p, state["t"] + 1
        return sh.step_fused_normalized(8.0, 0.0, 4.0, Q, 0.025, z, ids, R)

    def u0():
        state["resamples"] += 1
        return pkg.philox_uniform(state["resamples"], 2, sh.seed)

    ph = pkg.PathHistory(sh, 256)
    lines = [f"per-particle trajectory history beside the step it follows: fp32, n = {n}, nl = {nl}, m = {M} known-id observations",
             f"(1), (2): us per step over runs of {RUN} steps behind one synchronisation, the forms alternating, median of {ROUNDS} runs "
             f"(min, max)"]

    # (1) the step alone / with a record
    def run_plain():
        for _ in range(RUN):
            step()
        sh.sync()

    def run_record():
        for _ in range(RUN):
            step()
            ph.record()
        sh.sync()

    t_plain, t_rec = alternating([run_plain, run_record])
    lines += [f"slam_pf_step_normalized alone                    {t_plain[0]:9.1f} us  (min {t_plain[1]:.1f}, max {t_plain[2]:.1f})",
              f"slam_pf_step_normalized + slam_pf_path_record    {t_rec[0]:9.1f} us  (min {t_rec[1]:.1f}, max {t_rec[2]:.1f})   "
              f"record: {t_rec[0] - t_plain[0]:+.1f} us per step"]

    # (2) a resampling at every step, without and through the path object
    def run_local():
        for _ in range(RUN):
            _neff, gmax = step()
            sh.resample_local(gmax, u0())
        sh.sync()

    def run_path():
        for _ in range(RUN):
            _neff, gmax = step()
            ph.resample(gmax, u0())
        sh.sync()

    t_loc, t_pth = alternating([run_local, run_path])
    lines += [f"step + slam_pf_resample_local every step         {t_loc[0]:9.1f} us  (min {t_loc[1]:.1f}, max {t_loc[2]:.1f})",
              f"step + slam_pf_path_resample every step          {t_pth[0]:9.1f} us  (min {t_pth[1]:.1f}, max {t_pth[2]:.1f})   "
              f"compose: {t_pth[0] - t_loc[0]:+.1f} us per step"]

    # (3) the record alone beside hipMemcpyAsync of the same bytes
    rt = hip_runtime()
    stream = C.c_void_p()
    pkg._lib.check(pkg._lib.lib.slam_pf_stream(sh._h, C.byref(stream)))
    src = torch.zeros(4 * n, dtype=torch.float32, device=sh.device)
    dst = torch.empty_like(src)
    torch.cuda.synchronize(sh.device)

    def records():
        for _ in range(B2B):
            ph.record()
        sh.sync()

    def copies(nbytes):
        def go():
            for _ in range(B2B):
                if rt.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream):
                    raise RuntimeError("hipMemcpyAsync failed")
            sh.sync()
        return go

    lines.append(f"(3): us per call, {B2B} enqueued back to back behind one synchronisation, median of 15 (min, max)")
    for label, nbytes, pending in (("nothing pending", 12 * n, False), ("a resampling pending", 16 * n, True)):
        if pending:
            def go():
                for _ in range(B2B):
                    ph.resample(gmax_now[0], 0.5)      # uniform weights after the first one: the identity, n int32 pending
                    ph.record()
                sh.sync()

            def go_without():
                for _ in range(B2B):
                    ph.resample(gmax_now[0], 0.5)
                sh.sync()
            gmax_now = [float(sh.download(landmarks=False)[1].max())]
            t_both = median_us(go, per=B2B)
            t_res = median_us(go_without, per=B2B)
            t_r = tuple(a - b for a, b in zip(t_both, t_res))
            note = f"(resample + record {t_both[0]:.1f} us less resample alone {t_res[0]:.1f} us)"
        else:
            t_r = median_us(records, per=B2B)
            note = ""
        t_c = median_us(copies(nbytes), per=B2B)
        rate = lambda us: f"{2 * nbytes / (us * 1e-6) / 1e9:7.1f} GB/s read + written"
        lines += [f"slam_pf_path_record, {label:22s} {t_r[0]:9.1f} us  (min {t_r[1]:.1f}, max {t_r[2]:.1f})   {nbytes / 1e6:.2f} MB  "
                  f"{rate(t_r[0])} {note}",
                  f"hipMemcpyAsync of the same bytes             {t_c[0]:9.1f} us  (min {t_c[1]:.1f}, max {t_c[2]:.1f})   {nbytes / 1e6:.2f} MB  "
                  f"{rate(t_c[0])}"]
    ph.close()

    # (4) the read-outs on a ring the filter filled under the Neff rule
    lines.append("(4): wall time around the synchronising call, median of 15 after 2 warm-up calls (min, max); the ring was filled by the "
                 "filter under the Neff rule (0.75 n)")
    ph = pkg.PathHistory(sh, 256)
    made = 0
    for L in (64, 256):
        while made < L:
            neff, gmax = step()
            if neff < 0.75 * n:
                ph.resample(gmax, u0())
            ph.record()
            made += 1
        flagged = sum(1 for k in range(L - 1) if ph.get(k)[2])        # records whose ancestors a walk applies (all but the oldest)
        sv = ph.survivors()
        marked = int(sum(int(sv[t]) for t in range(1, L) if ph.get(L - 1 - t)[2]))
        b_mean = 12 * n * L + 4 * n * flagged + 4 * n
        b_surv = 2 * n * flagged + n + 4 * marked + int(sv[:-1].sum())
        b_best = 4 * n + 16 * L
        lines.append(f"L = {L}: {flagged} of {L - 1} steps back go through ancestors; survivors oldest {int(sv[0])}, middle "
                     f"{int(sv[L // 2])}, newest {int(sv[-1])}")
        for name, fn, byts in (("slam_pf_path_mean", ph.mean, b_mean), ("slam_pf_path_survivors", ph.survivors, b_surv),
                               ("slam_pf_path_best", ph.best, b_best)):
            t = median_us(fn)
            lines.append(f"  {name:24s} {t[0]:9.1f} us  (min {t[1]:.1f}, max {t[2]:.1f})   {byts / 1e6:9.2f} MB  "
                         f"{byts / (t[0] * 1e-6) / 1e9:7.1f} GB/s = {100 * byts / (t[0] * 1e-6) / HBM:4.1f} % of 6.3 TB/s")
        a, b = ph.mean(), ph.mean()
        lines.append(f"  two mean calls bit-identical: {bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))}; "
                     f"mean resultant length of the headings {float(a[:, 3].min()):.4f} .. {float(a[:, 3].max()):.4f}")
    ph.close()
    pf.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def main():
    pos = positional()
    n = int(pos[0]) if len(pos) > 0 else 262144
    nl = int(pos[1]) if len(pos) > 1 else 512
    out_path = opt("--out", os.path.join(ROOT, "profiles", "pf_path_bench.txt"))
    if "--measure" in sys.argv:
        measure(n, nl, out_path)
        return 0
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure", str(n), str(nl),
           "--out", out_path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
