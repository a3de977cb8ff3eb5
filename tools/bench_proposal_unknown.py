#!/usr/bin/env python3
"""The FastSLAM-2.0 step with unknown correspondences (slam_pf_step_proposal_unknown, libslamhip_proposal.so) beside
slam_pf_step_unknown with the same observations, in one run on clones of one particle set.

    python tools/bench_proposal_unknown.py [--n 262144] [--slots 64] [--reps 30] [--warmup 5]

fp32, 262 144 particles x 64 slots, half the slots in use (32 landmarks on a ring, entered by two calls of 16 new ones).  Each
timed call is synchronous (it returns the weight statistics), so the time is the host's clock around the call: launch, kernel,
fold and the poll of the pinned result.  Every repetition observes the same m landmarks from the truth's pose (all matched), and
the filter is normalised after each call, as a driver would.  Printed per m: the median and the best time of both calls, their
ratio, the bytes the three passes of the new kernel move per call against its time, and the time of pass A alone
(slam_pf_associate_proposal with the same observations)."""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

V, DT, WB = 3.0, 0.02, 4.0
Q = np.diag([0.5 ** 2, math.radians(3.0) ** 2])
R = np.diag([0.05 ** 2, math.radians(0.5) ** 2])
G1, G2 = 9.2, 25.0


def observe(lm, pose, rng):
    dx, dy = lm[:, 0] - pose[0], lm[:, 1] - pose[1]
    return np.vstack([np.hypot(dx, dy) + 0.05 * rng.standard_normal(len(lm)),
                      np.arctan2(dy, dx) - pose[2] + math.radians(0.5) * rng.standard_normal(len(lm))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pkg = load_package()
    import torch
    from slam_jl_amd.ekf import _obs, _ptr, _small
    n, nl, used = a.n, a.slots, a.slots // 2
    ang = 2 * math.pi * np.arange(used) / used
    lm = np.stack([(14.0 + 3.0 * (np.arange(used) % 3)) * np.cos(ang), (14.0 + 3.0 * (np.arange(used) % 3)) * np.sin(ang)], axis=1)
    rng = np.random.default_rng(1)
    base = pkg.PFShard(n, nl, 7, dtype="f32")
    base.set_pose([0.0, 0.0, 0.1])
    base.clear_landmarks()
    pose = np.array([0.0, 0.0, 0.1])
    for k in range(0, used, 16):                                            # enter the landmarks: all new
        pose = np.array([pose[0] + V * DT * math.cos(pose[2]), pose[1] + V * DT * math.sin(pose[2]), pose[2]])
        s = base.step_unknown_fused(V, 0.0, WB, Q, DT, observe(lm[k:k + 16], pose, rng), R, G1, G2)
        base.normalize(s[0], s[1])
    in_use = int((base.download()[2][:, 2, :] >= 0).sum(axis=0).max())
    print(f"fp32, {n} particles x {nl} slots, {in_use} slots in use; {a.reps} timed calls after {a.warmup}")
    esz = 4
    for m in (8, 16):
        sel = (np.arange(m) * (used // m)) % used
        res = {}
        for name in ("proposal", "yardstick"):
            sh = pkg.PFShard(n, nl, 7, dtype="f32")
            sh.copy_from(base)
            p, r = pose.copy(), np.random.default_rng(2)
            times, matched = [], 0
            for it in range(a.warmup + a.reps):
                p = np.array([p[0] + V * DT * math.cos(p[2]), p[1] + V * DT * math.sin(p[2]), p[2]])
                z = observe(lm[sel], p, r)
                call = sh.step_proposal_unknown if name == "proposal" else sh.step_unknown_fused
                last = it == a.warmup + a.reps - 1
                t0 = time.perf_counter()
                out = call(V, 0.0, WB, Q, DT, z, R, G1, G2, want_assoc=last)
                t1 = time.perf_counter()
                s = out[0] if last else out
                if last:
                    matched = float((out[1] >= 0).sum().item()) / (m * n)
                sh.normalize(s[0], s[1])
                if it >= a.warmup:
                    times.append((t1 - t0) * 1e6)
            res[name] = (float(np.median(times)), float(np.min(times)), matched)
            sh.close()
        # pass A alone: slam_pf_associate_proposal on a clone of the starting state (enqueued; timed to the stream's end)
        sh = pkg.PFShard(n, nl, 7, dtype="f32")
        sh.copy_from(base)
        dec = torch.empty((m, n), dtype=torch.int32, device=sh.device)
        zp, q4, r4 = _obs(observe(lm[sel], pose, np.random.default_rng(3))), _small(Q), _small(R)
        lib = pkg._lib.proposal_lib()
        ta = []
        for it in range(a.warmup + a.reps):
            sh.sync()
            t0 = time.perf_counter()
            pkg._lib.check(lib.slam_pf_associate_proposal(sh._h, V, 0.0, WB, _ptr(q4), DT, _ptr(zp), m, _ptr(r4), G1, G2,
                                                          C.c_void_p(dec.data_ptr()), None))
            sh.sync()
            if it >= a.warmup:
                ta.append((time.perf_counter() - t0) * 1e6)
        sh.close()
        print(f"m = {m:2d}: slam_pf_associate_proposal (pass A alone, {m * n * 4 / 1e6:.1f} MB of decisions written, launch to stream "
              f"sync) median {float(np.median(ta)):7.1f} us (best {float(np.min(ta)):7.1f})")
        # bytes per particle: pass A Pxx of every slot + four rows of the slots in use; pass B the matched records; pass C the
        # matched records read and written; pose and log-weight read and written.  The yardstick: the same without pass B.
        mm = res["proposal"][2] * m
        pass_a = nl * esz + in_use * 4 * esz
        pass_b = mm * 5 * esz
        pass_c = mm * 10 * esz
        rest = 8 * esz
        total = (pass_a + pass_b + pass_c + rest) * n
        med_p, min_p, _ = res["proposal"]
        med_y, min_y, my = res["yardstick"]
        print(f"m = {m:2d}: slam_pf_step_proposal_unknown median {med_p:7.1f} us (best {min_p:7.1f}), matched {res['proposal'][2]:.3f}; "
              f"slam_pf_step_unknown median {med_y:7.1f} us (best {min_y:7.1f}), matched {my:.3f}; ratio {med_p / med_y:.3f}")
        print(f"        bytes per call: pass A {pass_a * n / 1e6:.1f} MB, pass B {pass_b * n / 1e6:.1f} MB, pass C {pass_c * n / 1e6:.1f} MB, "
              f"pose and weight {rest * n / 1e6:.1f} MB: {total / 1e6:.1f} MB in {med_p:.1f} us = {total / med_p / 1e6:.2f} TB/s; "
              f"yardstick plus one more read of the matched records at its own rate: "
              f"{med_y * (1 + pass_b / (pass_a + pass_c + rest)):.1f} us")
    base.close()


if __name__ == "__main__":
    main()
