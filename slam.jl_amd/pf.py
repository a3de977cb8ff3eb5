"""FastSLAM-1.0 (known correspondences) on the GPU: ``PFSlamState`` and its sharded driver.

The reference only declares the types ``Particle`` / ``PFSlamState`` (src/common.jl:14-20,31-34)
and no particle-filter code (README.md:6); the algorithm is SURVEY.md 8a rows F1-F4.

Two layers:

* :class:`PFShard` -- one process's slice of the particles, a thin wrapper of the ``slam_pf_*``
  C ABI (HIP kernels, SoA state resident in HBM).  No CPU fallback.
* :class:`FastSLAM` -- the host logic that is the same for 1 and for G GPUs: per step an
  all-reduce of three scalars (max log-weight, sum w, sum w^2) for normalisation and Neff; on a
  resampling step an all-gather of the log-weights (the RCCL collective BASELINE.json names),
  the same global systematic-resampling table on every rank, and an exchange of the particle
  records whose ancestor lives on another rank.  It talks to the shard through a small protocol
  (the methods of :class:`PFShard`) and to the other ranks through ``torch.distributed``
  (``nccl`` = RCCL on the GPUs; the multi-process CPU tests drive the same logic over ``gloo``
  with a NumPy shard that lives in the test-suite, never here).

Random numbers are Philox4x32-10 keyed by (seed, step, global particle id): a run gives the same
particles whatever the number of ranks.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys

import numpy as np

from ._lib import SLAM_F32, SLAM_F64, SLAM_PF_HALTED, SLAM_PF_PEER_BLOB_BYTES, check, evidence_lib, frame_lib, handover_lib, lib, path_lib, pfcopy_lib, proposal_lib
from .ekf import EKFSlamState, _obs, _small, _ptr, rigid_fit

__all__ = ["PFShard", "PFSlamState", "FastSLAM", "LandmarkEvidence", "PathHistory", "philox_uniform", "small", "shared_page", "attach_local_peers",
           "finalise_map", "ellipse_axes", "MapSnapshot", "particles_to_ekf", "ekf_to_particles", "save_particles", "load_particles",
           "kld_particle_count"]

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_RESAMPLE = 2
STREAM_HANDOVER = 3                 # slam_ekf_to_pf's three normals per particle (include/slamhip_handover.h)


def philox_uniform(step: int, stream: int, seed: int) -> float:
    """One U(0,1) from Philox4x32-10 with counter (0, 0, step, stream): the systematic-resampling
    offset every rank derives for itself (host scalar; same generator as the kernels)."""
    c = [0, 0, step & 0xFFFFFFFF, stream & 0xFFFFFFFF]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return ((c[0] >> 8) + 0.5) / 16777216.0


def finalise_map(sums):
    """The map from the (summed) rows of ``PFShard.map_sums``: ``sums`` [1 + cnt, 10] (row 0 the pose row) ->
    [cnt, 8] = {mass W_l / W, mean x, mean y, Cxx, Cxy, Cyy, count, 0} per landmark with
    C = sum w P / W_l + (sum w m m' / W_l - mean mean'), the moment-matched Gaussian of the particles' mixture; a
    landmark without mass is a row of zeros.  The same arithmetic as ``slam_pf_get_map``, for one rank and for the sum
    over many."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 10)
    W, r = s[0, 0], s[1:]
    out = np.zeros((r.shape[0], 8))
    ok = (r[:, 0] > 0.0) & (W > 0.0)
    Wl = r[ok, 0]
    mx, my = r[ok, 1] / Wl, r[ok, 2] / Wl
    out[ok, 0] = Wl / W
    out[ok, 1], out[ok, 2] = mx, my
    out[ok, 3] = r[ok, 6] / Wl + (r[ok, 3] / Wl - mx * mx)
    out[ok, 4] = r[ok, 7] / Wl + (r[ok, 4] / Wl - mx * my)
    out[ok, 5] = r[ok, 8] / Wl + (r[ok, 5] / Wl - my * my)
    out[ok, 6] = r[ok, 9]
    return out


def ellipse_axes(cxx, cxy, cyy):
    """(rx, ry, phi) of the covariance ellipses [[cxx, cxy], [cxy, cyy]] (arrays) with the convention ``slam_ekf_ellipses``
    documents: rx <= ry the square roots of the ascending eigenvalues, phi the direction of the FIRST (smaller
    eigenvalue's) eigenvector in [-pi/2, pi/2]."""
    cxx, cxy, cyy = (np.asarray(v, dtype=np.float64) for v in (cxx, cxy, cyy))
    half, mean = 0.5 * (cxx - cyy), 0.5 * (cxx + cyy)
    rad = np.hypot(half, cxy)
    l1, l2 = np.maximum(mean - rad, 0.0), np.maximum(mean + rad, 0.0)
    # eigenvector of the smaller eigenvalue l1: (cxy, l1 - cxx) or, where that one vanishes, (l1 - cyy, cxy)
    vx = np.where(np.abs(l1 - cxx) >= np.abs(l1 - cyy), cxy, l1 - cyy)
    vy = np.where(np.abs(l1 - cxx) >= np.abs(l1 - cyy), l1 - cxx, cxy)
    iso = (vx == 0.0) & (vy == 0.0)                         # a circle (or a diagonal matrix with cxx <= cyy): the x axis
    vx = np.where(iso, 1.0, vx)
    flip = (vx < 0.0) | ((vx == 0.0) & (vy < 0.0))
    phi = np.arctan2(np.where(flip, -vy, vy), np.where(flip, -vx, vx))
    return np.sqrt(l1), np.sqrt(l2), phi


class MapSnapshot:
    """The read-outs of a particle filter from one set of map sums ([1 + nl, 10], ``FastSLAM.map_sums``): host arithmetic only."""

    def __init__(self, sums):
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, 10)
        self.map = finalise_map(self.sums)

    def pose(self):
        s = self.sums[0]
        return np.array([s[1] / s[0], s[2] / s[0], math.atan2(s[6], s[7])])

    @property
    def N(self):
        return int(np.count_nonzero(self.map[:, 0] > 0.0))

    def feature_ellipses(self):
        m = self.map[self.map[:, 0] > 0.0]
        rx, ry, phi = ellipse_axes(m[:, 3], m[:, 4], m[:, 5])
        return np.vstack([m[:, 1], m[:, 2], rx, ry, phi])

    def vehicle_ellipse(self):
        s = self.sums[0]
        mx, my = s[1] / s[0], s[2] / s[0]
        rx, ry, phi = ellipse_axes(s[3] / s[0] - mx * mx, s[4] / s[0] - mx * my, s[5] / s[0] - my * my)
        return np.array([mx, my, math.atan2(s[6], s[7]), float(rx), float(ry), float(phi)])


class _Small:
    """A 2 x 2 matrix already in the library's column-major double[4] form, with its pointer (see :func:`small`)."""
    __slots__ = ("a", "ptr")

    def __init__(self, M):
        self.a = _small(M)
        self.ptr = _ptr(self.a)


def small(M):
    """Convert a 2 x 2 matrix once for repeated ``step_auto`` calls."""
    return M if isinstance(M, _Small) else _Small(M)


class PFShard:
    """Global particle ids [first, first + n) of an n_global-particle filter on one GPU."""

    def __init__(self, n_local, max_landmarks, seed, dtype="f32", first=0, n_global=None, device=0):
        import torch
        self.n = int(n_local)
        self.first = int(first)
        self.n_global = int(n_global if n_global is not None else n_local)
        self.nl = int(max_landmarks)
        self.seed = int(seed)
        self.np_dtype = np.float32 if dtype == "f32" else np.float64
        self.torch_dtype = torch.float32 if dtype == "f32" else torch.float64
        self.device = torch.device("cuda", int(device))
        self._h = C.c_void_p()
        check(lib.slam_pf_create(C.byref(self._h), SLAM_F32 if dtype == "f32" else SLAM_F64, self.n, self.n_global,
                                 self.first, self.nl, int(device), C.c_uint64(self.seed)))
        rows = C.c_int()
        check(lib.slam_pf_record_rows(self._h, C.byref(rows)))
        self.rows = rows.value
        self._borrowers = 0                          # LandmarkEvidence / PathHistory objects that follow this shard's particles

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib.slam_pf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- filter operations ---------------------------------------------------------------------
    def set_pose(self, pose):
        p = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(3))
        check(lib.slam_pf_set_pose(self._h, _ptr(p)))

    def init_landmarks(self, lm_xy, var, jitter_sigma):
        xy = np.ascontiguousarray(np.asarray(lm_xy, dtype=np.float64).reshape(-1, 2))
        check(lib.slam_pf_init_landmarks(self._h, _ptr(xy), xy.shape[0], float(var), float(jitter_sigma)))

    def predict(self, V, G, wheelbase, Q, dt):
        q = _small(Q)
        check(lib.slam_pf_predict(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt)))

    def update_known(self, z, ids, R):
        zp = _obs(z)
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if idv.shape[0] != zp.shape[0]:
            raise ValueError("ids and z disagree on the number of observations")
        if zp.shape[0] == 0:
            return
        r = _small(R)
        check(lib.slam_pf_update_known(self._h, _ptr(zp), _ptr(idv, C.c_int32), zp.shape[0], _ptr(r)))

    def clear_landmarks(self):
        """Every landmark slot of every particle unused (the start of an unknown-correspondence run)."""
        check(lib.slam_pf_clear_landmarks(self._h))

    def update_unknown(self, z, R, gate1, gate2, want_assoc=False):
        """Unknown correspondences: per-particle gated nearest-neighbour association against the
        particle's own landmarks, then updates / new landmarks.  ``want_assoc``: return the decisions as an
        int32 torch tensor [m, n] on the device (slot >= 0 matched, -1 new, -2 dropped)."""
        zp = _obs(z)
        m = zp.shape[0]
        if m == 0:
            return None
        r = _small(R)
        assoc = None
        ptr = None
        if want_assoc:
            import torch
            assoc = torch.empty((m, self.n), dtype=torch.int32, device=self.device)
            ptr = C.c_void_p(assoc.data_ptr())
        check(lib.slam_pf_update_unknown(self._h, _ptr(zp), m, _ptr(r), float(gate1), float(gate2), ptr))
        if want_assoc:
            self.sync()
        return assoc

    def step_unknown_fused(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, want_assoc=False):
        """predict + update_unknown + weight_stats as ONE sweep over the particles (slam_pf_step_unknown), for up to 64
        observations; with at most 16 the same particles, decisions and statistics bit for bit.  Returns
        (gmax, s1, s2), or ((gmax, s1, s2), assoc) with ``want_assoc`` (int32 torch tensor [m, n] on the device: slot >= 0
        matched, -1 new, -2 dropped)."""
        zp = _obs(z)
        m = zp.shape[0]
        q, r = _small(Q), _small(R)
        assoc = None
        ptr = None
        if want_assoc:
            import torch
            assoc = torch.empty((m, self.n), dtype=torch.int32, device=self.device)
            ptr = C.c_void_p(assoc.data_ptr()) if m else None
        out = np.empty(3)
        check(lib.slam_pf_step_unknown(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt), _ptr(zp), m, _ptr(r),
                                       float(gate1), float(gate2), ptr, _ptr(out)))
        stats = (float(out[0]), float(out[1]), float(out[2]))      # (the call synchronises: assoc is complete)
        return (stats, assoc) if want_assoc else stats

    def step_proposal_unknown(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, want_assoc=False):
        """FastSLAM 2.0 with unknown correspondences (slam_pf_step_proposal_unknown, include/ext/slamhip_proposal.h): every
        particle associates the at most 16 observations with its own landmarks under the prior proposal, draws its pose from
        the proposal that knows the matched ones, and updates its map from the sampled pose.  Whole filter on this shard.
        Returns (gmax, s1, s2), or ((gmax, s1, s2), assoc) with ``want_assoc`` (int32 torch tensor [m, n] on the device:
        slot >= 0 matched, -1 new, -2 dropped)."""
        zp = _obs(z)
        m = zp.shape[0]
        q, r = _small(Q), _small(R)
        assoc = None
        ptr = None
        if want_assoc:
            import torch
            assoc = torch.empty((m, self.n), dtype=torch.int32, device=self.device)
            ptr = C.c_void_p(assoc.data_ptr()) if m else None
        out = np.empty(3)
        check(proposal_lib().slam_pf_step_proposal_unknown(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt),
                                                           _ptr(zp), m, _ptr(r), float(gate1), float(gate2), ptr, _ptr(out)))
        stats = (float(out[0]), float(out[1]), float(out[2]))      # (the call synchronises: assoc is complete)
        return (stats, assoc) if want_assoc else stats

    def associate_proposal(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, want_nis=False):
        """The association of ``step_proposal_unknown`` alone (slam_pf_associate_proposal): the state is only read.  Returns
        the decisions (int32 torch tensor [m, n] on the device), or (decisions, nis) with ``want_nis``: the nis of the winning
        slot in the shard's dtype, NaN where nothing matched."""
        import torch
        zp = _obs(z)
        m = zp.shape[0]
        q, r = _small(Q), _small(R)
        assoc = torch.empty((m, self.n), dtype=torch.int32, device=self.device)
        nis = torch.empty((m, self.n), dtype=self.torch_dtype, device=self.device) if want_nis else None
        check(proposal_lib().slam_pf_associate_proposal(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt),
                                                        _ptr(zp), m, _ptr(r), float(gate1), float(gate2),
                                                        C.c_void_p(assoc.data_ptr()) if m else None,
                                                        C.c_void_p(nis.data_ptr()) if (want_nis and m) else None))
        self.sync()
        return (assoc, nis) if want_nis else assoc

    def weight_stats(self):
        out = np.empty(3)
        check(lib.slam_pf_weight_stats(self._h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def step_fused(self, V, G, wheelbase, Q, dt, z, ids, R):
        """predict + update_known + weight_stats as ONE sweep over the particles (slam_pf_step): the same
        particles bit for bit, the same three statistics."""
        zp = _obs(z)
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if idv.shape[0] != zp.shape[0]:
            raise ValueError("ids and z disagree on the number of observations")
        q, r = _small(Q), _small(R)
        out = np.empty(3)
        check(lib.slam_pf_step(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt), _ptr(zp),
                               _ptr(idv, C.c_int32), zp.shape[0], _ptr(r), _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def step_proposal(self, V, G, wheelbase, Q, dt, z, ids, R):
        """The FastSLAM-2.0 step (slam_pf_step_proposal): as step_fused, but the pose is drawn from the
        proposal that already knows this step's observations.  Returns the same three statistics."""
        zp = _obs(z)
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if idv.shape[0] != zp.shape[0]:
            raise ValueError("ids and z disagree on the number of observations")
        q, r = _small(Q), _small(R)
        out = np.empty(3)
        check(lib.slam_pf_step_proposal(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt), _ptr(zp),
                                        _ptr(idv, C.c_int32), zp.shape[0], _ptr(r), _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def step_fused_normalized(self, V, G, wheelbase, Q, dt, z, ids, R):
        """step_fused + normalize with this shard's own statistics (the whole filter lives here): returns
        (Neff, max normalised log-weight)."""
        zp = _obs(z)
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if idv.shape[0] != zp.shape[0]:
            raise ValueError("ids and z disagree on the number of observations")
        q, r = _small(Q), _small(R)
        out = np.empty(4)
        check(lib.slam_pf_step_normalized(self._h, float(V), float(G), float(wheelbase), _ptr(q), float(dt), _ptr(zp),
                                          _ptr(idv, C.c_int32), zp.shape[0], _ptr(r), _ptr(out)))
        T = self.np_dtype                          # (neff, largest log-weight after the shift, exactly as stored)
        return float(out[3]), float(T(out[0]) - T(out[0] + math.log(out[1])))

    def normalize(self, gmax, gsum):
        check(lib.slam_pf_normalize(self._h, float(gmax), float(gsum)))

    def mean_pose_sums(self):
        out = np.empty(4)
        check(lib.slam_pf_mean_pose_sums(self._h, _ptr(out)))
        return out

    # -- the step without the host in the loop (slam_pf_step_auto) -----------------------------------
    @staticmethod
    def prepare_obs(z, ids):
        """Observations in the layout the library takes, converted once, with their ctypes pointers (a timed loop calls
        step_auto with these: a step is then one foreign call)."""
        zp = _obs(z)
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if idv.shape[0] != zp.shape[0]:
            raise ValueError("ids and z disagree on the number of observations")
        return zp, idv, _ptr(zp), _ptr(idv, C.c_int32)

    def step_auto(self, V, G, wheelbase, Q, dt, z, ids, R, neff_frac=0.75, force=None, proposal=False, prepared=None):
        """One whole filter step ENQUEUED (slam_pf_step_auto): statistics, normalisation, Neff, the decision to resample
        and -- filter wholly on this shard -- the resampling itself stay on the device.  ``force``: None = Neff rule,
        False / True = never / always.  Returns False, or True when the library reports SLAM_PF_HALTED (a queued step
        of a sharded filter wants a resampling; nothing was enqueued by this call)."""
        zp, _idv, pz, pi = prepared if prepared is not None else self.prepare_obs(z, ids)
        pq = Q.ptr if isinstance(Q, _Small) else _ptr(_small(Q))
        pr = R.ptr if isinstance(R, _Small) else _ptr(_small(R))
        rc = lib.slam_pf_step_auto(self._h, V, G, wheelbase, pq, dt, pz, pi, zp.shape[0], pr, neff_frac,
                                   -1 if force is None else int(bool(force)), 1 if proposal else 0)
        if rc == SLAM_PF_HALTED:
            return True
        if rc:
            check(rc)
        return False

    @staticmethod
    def prepare_batch(controls, obs, force=None):
        """K steps in the layout slam_pf_step_auto_batch takes, converted once: ``controls`` K x (V, G); ``obs`` K pairs
        (z 2 x m_k, ids m_k); ``force`` None (the Neff rule at every step), one value for all steps or K values (None / False /
        True each).  Returns an opaque tuple for ``step_auto_batch``."""
        K = len(obs)
        vg = np.ascontiguousarray(np.asarray(controls, dtype=np.float64).reshape(K, 2))
        ms = np.array([np.asarray(i).reshape(-1).shape[0] for _, i in obs], dtype=np.int32)
        stride = max(1, int(ms.max()) if K else 1)
        zz = np.zeros((K, stride, 2))
        ii = np.zeros((K, stride), dtype=np.int32)
        for k, (z, ids) in enumerate(obs):
            if ms[k]:
                zz[k, :ms[k]] = _obs(z)
                ii[k, :ms[k]] = np.asarray(ids, dtype=np.int32).reshape(-1)
        if force is None or isinstance(force, (bool, np.bool_)):
            force = [force] * K
        ff = np.array([-1 if f is None else int(bool(f)) for f in force], dtype=np.int32)
        if ff.shape[0] != K:
            raise ValueError("force: one value per step")
        return K, vg, zz, ii, ms, stride, ff

    def step_auto_batch(self, batch, wheelbase, Q, dt, R, neff_frac=0.75, proposal=False, persistent=False, start=0):
        """K filter steps ENQUEUED by one call (slam_pf_step_auto_batch; ``batch`` from prepare_batch): the same filter as
        K step_auto calls, bit for bit.  ``persistent=True``: runs of steps that cannot resample may go as persistent launches of
        up to 16 steps -- the caller vouches that nothing else keeps the device's compute units busy meanwhile (the grid takes them
        whole and its workgroups wait for each other).  Returns the number of steps taken from ``start`` on: all of them, or fewer when the library reports SLAM_PF_HALTED (sharded
        halting flow: resolve the halt and call again with ``start`` advanced)."""
        K, vg, zz, ii, ms, stride, ff = batch
        pq = Q.ptr if isinstance(Q, _Small) else _ptr(_small(Q))
        pr = R.ptr if isinstance(R, _Small) else _ptr(_small(R))
        took = C.c_int(0)
        rc = lib.slam_pf_step_auto_batch(self._h, K - start, _ptr(vg[start:]), wheelbase, pq, dt, _ptr(zz[start:]),
                                         _ptr(ii[start:], C.c_int32), _ptr(ms[start:], C.c_int32), stride, pr, neff_frac,
                                         _ptr(ff[start:], C.c_int32), 1 if proposal else 0, 2 if persistent else 0, C.byref(took))
        if rc and rc != SLAM_PF_HALTED:
            check(rc)
        return int(took.value)

    def flush(self):
        """Wait for the queued steps: (Neff of the last step, it resampled?, resamplings so far, steps so far), or None
        when the library reports SLAM_PF_HALTED."""
        out = np.empty(4)
        rc = lib.slam_pf_flush(self._h, _ptr(out))
        if rc == SLAM_PF_HALTED:
            return None
        check(rc)
        return float(out[0]), bool(out[1]), int(out[2]), int(out[3])

    def debug_stamps(self):
        """100 MHz stamps of the last auto step (slam_pf_debug_stamps), as microseconds since the kernel's start."""
        out = (C.c_uint64 * 8)()
        check(lib.slam_pf_debug_stamps(self._h, out))
        return [(int(v) - int(out[0])) / 100.0 for v in out[:8]]

    def halt_info(self):
        out = np.empty(2)
        check(lib.slam_pf_halt_info(self._h, _ptr(out)))
        return float(out[0]), int(out[1])

    def resume(self, resamplings):
        check(lib.slam_pf_resume(self._h, int(resamplings)))

    def resample_count(self):
        out = C.c_int64()
        check(lib.slam_pf_resample_count(self._h, C.byref(out)))
        return int(out.value)

    def set_resample_count(self, count):
        check(lib.slam_pf_set_resample_count(self._h, int(count)))

    def attach_exchange(self, rank, world, page):
        """``page``: a float64 NumPy array over host memory that every rank has mapped (>= 2 * world * 8 values)."""
        assert page.dtype == np.float64 and page.flags.c_contiguous and page.size >= 2 * world * 8
        self._xchg_page = page                       # keeps the mapping alive
        check(lib.slam_pf_attach_exchange(self._h, int(rank), int(world), C.c_void_p(page.ctypes.data), page.nbytes))

    # -- sharding behind the C ABI: peers (slam_pf_export_peer / slam_pf_attach_peers) ------------------------
    def export_peer(self):
        """This shard's peer blob (bytes): IPC handles of its buffers and inbox; every rank attaches all ranks' blobs."""
        buf = C.create_string_buffer(SLAM_PF_PEER_BLOB_BYTES)
        check(lib.slam_pf_export_peer(self._h, buf))
        return bytes(buf.raw)

    def attach_peers(self, rank, world, blobs):
        """``blobs``: the ``world`` peer blobs in rank order.  From here on step_auto resamples the sharded filter on
        the device (no SLAM_PF_HALTED); calls that need plain maps (download with landmarks, pack, legacy sweeps) are
        collective."""
        assert len(blobs) == world and all(len(b) == SLAM_PF_PEER_BLOB_BYTES for b in blobs)
        check(lib.slam_pf_attach_peers(self._h, int(rank), int(world), C.c_char_p(b"".join(blobs))))

    def detach_peers(self):
        check(lib.slam_pf_detach_peers(self._h))

    def peer_selftest(self, timeout_ms=3000):
        """Collective: True when every attached peer's inbox write arrived here within the time-out."""
        return lib.slam_pf_peer_selftest(self._h, int(timeout_ms)) == 0

    def comm_info(self):
        """{world, peers attached?, SLAM_PF_HALTED returns so far, resamplings so far}."""
        out = (C.c_int64 * 4)()
        check(lib.slam_pf_comm_info(self._h, out))
        return dict(world=int(out[0]), peers=bool(out[1]), halts=int(out[2]), resamples=int(out[3]))

    def resample_if_needed(self, neff_frac=0.75):
        """slam_pf_resample: normalise and resample if Neff < neff_frac * n (filter wholly on this shard)."""
        out = C.c_int()
        check(lib.slam_pf_resample(self._h, float(neff_frac), C.byref(out)))
        return bool(out.value)

    def mean_pose(self):
        out = np.empty(3)
        check(lib.slam_pf_get_mean_pose(self._h, _ptr(out)))
        return out

    def weights(self):
        out = np.empty(self.n)
        check(lib.slam_pf_get_weights(self._h, _ptr(out)))
        return out

    def transform(self, tx, ty, theta):
        """Express this shard's particles in another frame (slam_pf_transform): every pose and every landmark record in
        use through p <- R(theta) p + (tx, ty), Pf <- R Pf R'; log-weights and the RNG step are untouched.  Enqueued;
        collective with peers attached."""
        check(frame_lib().slam_pf_transform(self._h, float(tx), float(ty), float(theta)))

    # -- the map without downloading the particles (slam_pf_map_sums / slam_pf_get_map / slam_pf_get_particle) ---
    @staticmethod
    def _ids(ids):
        if ids is None:
            return None, None, 0
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        cnt = idv.shape[0]
        if cnt == 0:
            idv = np.zeros(1, dtype=np.int32)        # (a NULL pointer would mean "all landmarks")
        return idv, _ptr(idv, C.c_int32), cnt

    def map_sums(self, ids=None):
        """This shard's sums of the weighted map, [1 + cnt, 10] float64: row 0 the pose row {W, sum w x, w y, w x^2,
        w x y, w y^2, w sin(phi), w cos(phi), 0, n_local}, row 1 + i landmark ``ids[i]`` (1-based; None: all)
        {W_l, sum w mx, w my, w mx^2, w mx my, w my^2, w Pxx, w Pxy, w Pyy, count_l}.  One pass over the records where
        they are; a filter wholly on this shard is not changed (collective with peers attached)."""
        _idv, ptr, cnt = self._ids(ids)
        out = np.empty((1 + (self.nl if ids is None else cnt), 10))
        check(lib.slam_pf_map_sums(self._h, ptr, cnt, _ptr(out)))
        return out

    def get_map(self, ids=None):
        """slam_pf_get_map (whole filter on this shard): [cnt, 8] = {mass, mean x, mean y, Cxx, Cxy, Cyy, count, 0}."""
        _idv, ptr, cnt = self._ids(ids)
        out = np.empty((self.nl if ids is None else cnt, 8))
        check(lib.slam_pf_get_map(self._h, ptr, cnt, _ptr(out)))
        return out

    def particle(self, idx=-1, landmarks=True):
        """Local particle ``idx`` (-1: the one with the largest log-weight, lowest index on a tie):
        (global id, log-weight, pose [3], records [nl, 5] or None), float64."""
        gid, lw = C.c_int64(), C.c_double()
        pose = np.empty(3)
        lm = np.empty((self.nl, 5)) if landmarks else None
        check(lib.slam_pf_get_particle(self._h, int(idx), C.byref(gid), C.byref(lw), _ptr(pose),
                                       _ptr(lm) if landmarks else None))
        return int(gid.value), float(lw.value), pose, lm

    # -- hand-over between the two filters on the device (include/slamhip_handover.h) ------------------------
    def to_ekf_into(self, state, ids=None):
        """``state`` (an EKFSlamState of this dtype on this device) becomes the moment-matched joint Gaussian of this filter's
        particles over the pose and the landmarks ``ids`` (1-based, distinct, any order; None: every landmark seen so far,
        ascending) -- slam_pf_to_ekf: full covariance, cross terms included.  Every chosen landmark must be in use in every
        particle.  Returns ``{"W", "neff", "n", "N"}``.  The particle set is unchanged.  Synchronises."""
        if not isinstance(state, EKFSlamState):
            raise TypeError("to_ekf_into needs an EKFSlamState")
        _idv, ptr, cnt = self._ids(ids)
        info = np.zeros(4)
        check(handover_lib().slam_pf_to_ekf(state._h, self._h, ptr, cnt, _ptr(info)))
        return {"W": float(info[0]), "neff": float(info[1]), "n": int(info[2]), "N": int(info[3])}

    def from_ekf(self, state, ids=None):
        """This filter's particles are drawn from the EKF state ``state`` (slam_ekf_to_pf): poses from the vehicle marginal,
        every landmark ``ids`` (1-based, distinct; None: all) the conditional given the pose, uniform weights; one RNG step is
        consumed.  NotPositiveDefinite when the vehicle block or a conditional block is not positive definite.  Synchronises."""
        if not isinstance(state, EKFSlamState):
            raise TypeError("from_ekf needs an EKFSlamState")
        _idv, ptr, cnt = self._ids(ids)
        check(handover_lib().slam_ekf_to_pf(self._h, state._h, ptr, cnt))

    # -- the particle set moved on the device (include/slamhip_pfcopy.h) ------------------------------------
    def meta(self):
        """slam_pf_get_meta: ``{"n", "n_global", "first", "max_landmarks", "dtype", "step", "resamples", "seed", "seen"}`` with
        ``seen`` the per-landmark flags as a uint8 array.  Waits for the queue of an auto-mode filter."""
        out = np.zeros(8, dtype=np.int64)
        seen = np.zeros(self.nl, dtype=np.uint8)
        check(pfcopy_lib().slam_pf_get_meta(self._h, _ptr(out, C.c_int64), seen.ctypes.data))
        return {"n": int(out[0]), "n_global": int(out[1]), "first": int(out[2]), "max_landmarks": int(out[3]),
                "dtype": "f32" if int(out[4]) == SLAM_F32 else "f64", "step": int(out[5]), "resamples": int(out[6]),
                "seed": int(out[7]) & 0xFFFFFFFFFFFFFFFF, "seen": seen}

    def set_rng(self, seed, step):
        """The Philox key and the step counter (slam_pf_set_rng)."""
        check(pfcopy_lib().slam_pf_set_rng(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(step))))
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def upload(self, pose=None, logw=None, lm=None, seen=None):
        """The inverse of :meth:`download` (slam_pf_upload): ``pose`` [3, n], ``logw`` [n], ``lm`` [nl, 5, n] in the shard's dtype
        and ``seen`` [nl] flags; ``pose`` and ``logw`` may each be None (that part stays), ``lm`` and ``seen`` go together.  The
        values are stored as given; with ``lm`` the maps are plain afterwards.  Synchronises."""
        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=self.np_dtype)
            if a.shape != shape:
                raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
            return a
        if (lm is None) != (seen is None):
            raise ValueError("lm and seen are given together or not at all")
        pose, logw, lm = arr(pose, (3, self.n)), arr(logw, (self.n,)), arr(lm, (self.nl, 5, self.n))
        sn = None
        if seen is not None:
            sn = np.ascontiguousarray(np.asarray(seen).reshape(-1) != 0, dtype=np.uint8)
            if sn.shape != (self.nl,):
                raise ValueError(f"expected {self.nl} seen flags")
        check(pfcopy_lib().slam_pf_upload(self._h, None if pose is None else pose.ctypes.data, None if logw is None else logw.ctypes.data,
                                          None if lm is None else lm.ctypes.data, None if sn is None else sn.ctypes.data))

    def copy_from(self, src, fill=0):
        """This shard becomes a copy of ``src`` (slam_pf_copy): poses, log-weights as ``src.download()`` returns them, every
        record bit for bit -- read where lazy resampling left it, ``src`` is only read --, the RNG state and the resample
        count.  Slots beyond ``src.nl`` follow ``fill`` (0: as created, 1: unused, for unknown correspondences)."""
        check(pfcopy_lib().slam_pf_copy(self._h, src._h, int(fill)))
        self.seed = src.seed

    def select_from(self, src, ids, fill=0):
        """As :meth:`copy_from` with landmark k of this shard = slot ``ids[k - 1]`` of ``src`` (1-based, distinct, any order;
        None: all) -- slam_pf_select."""
        _idv, ptr, cnt = self._ids(ids)
        check(pfcopy_lib().slam_pf_select(self._h, src._h, ptr, cnt, int(fill)))
        self.seed = src.seed

    def resize_from(self, src, gmax, u0, fill=0):
        """This shard's n particles are drawn from ``src``'s by systematic resampling into n slots (slam_pf_resize; the counts
        may differ): uniform weights, the resample count is ``src``'s plus one.  ``gmax``: the largest (normalised) log-weight
        of ``src``.  Returns the ancestor table, int32 [n]."""
        anc = np.empty(self.n, dtype=np.int32)
        check(pfcopy_lib().slam_pf_resize(self._h, src._h, float(gmax), float(u0), int(fill), _ptr(anc, C.c_int32)))
        self.seed = src.seed
        return anc

    def pose_bins(self, cell_xy, cell_phi):
        """The number of distinct occupied cells of the pose histogram (slam_pf_pose_bins): the k of KLD-sampling."""
        out = C.c_int64()
        check(pfcopy_lib().slam_pf_pose_bins(self._h, float(cell_xy), float(cell_phi), C.byref(out)))
        return int(out.value)

    # -- resampling pieces (torch tensors on this shard's device) ---------------------------------
    def logw_tensor(self):
        import torch
        t = torch.empty(self.n, dtype=self.torch_dtype, device=self.device)
        check(lib.slam_pf_copy_logw(self._h, C.c_void_p(t.data_ptr())))
        return t

    def ancestors(self, logw_all, gmax, u0):
        import torch
        assert logw_all.is_cuda and logw_all.dtype == self.torch_dtype and logw_all.numel() == self.n_global
        torch.cuda.synchronize(self.device)            # logw_all was produced on torch's stream
        anc = torch.empty(self.n, dtype=torch.int32, device=self.device)
        check(lib.slam_pf_ancestors(self._h, C.c_void_p(logw_all.data_ptr()), float(gmax), float(u0),
                                    C.c_void_p(anc.data_ptr())))
        return anc

    def resample_local(self, gmax, u0):
        """Resampling of a filter that lives wholly on this shard, one library call (slam_pf_resample_local)."""
        check(lib.slam_pf_resample_local(self._h, float(gmax), float(u0)))

    def ancestors_all(self, logw_all, gmax, u0):
        """Global ancestor id of EVERY slot of the filter (n_global int32): identical on every rank."""
        import torch
        assert logw_all.is_cuda and logw_all.dtype == self.torch_dtype and logw_all.numel() == self.n_global
        torch.cuda.synchronize(self.device)            # logw_all was produced on torch's stream
        anc = torch.empty(self.n_global, dtype=torch.int32, device=self.device)
        check(lib.slam_pf_ancestors_all(self._h, C.c_void_p(logw_all.data_ptr()), float(gmax), float(u0),
                                        C.c_void_p(anc.data_ptr())))
        return anc

    def pack(self, local_idx):
        import torch
        idx = local_idx.to(device=self.device, dtype=torch.int32).contiguous()
        rec = torch.empty((self.rows, idx.numel()), dtype=self.torch_dtype, device=self.device)
        if idx.numel():
            torch.cuda.synchronize(self.device)
            check(lib.slam_pf_pack(self._h, C.c_void_p(idx.data_ptr()), idx.numel(), C.c_void_p(rec.data_ptr())))
        return rec

    def resample_apply(self, anc, remote_ids, remote_records):
        import torch
        torch.cuda.synchronize(self.device)
        nrem = 0 if remote_ids is None else int(remote_ids.numel())
        if nrem:
            ids = remote_ids.to(device=self.device, dtype=torch.int32).contiguous()
            rec = remote_records.to(device=self.device, dtype=self.torch_dtype).contiguous()
            assert rec.shape == (self.rows, nrem)
            check(lib.slam_pf_resample_apply(self._h, C.c_void_p(anc.data_ptr()), C.c_void_p(ids.data_ptr()), nrem,
                                             C.c_void_p(rec.data_ptr())))
        else:
            check(lib.slam_pf_resample_apply(self._h, C.c_void_p(anc.data_ptr()), None, 0, None))

    # -- inspection ---------------------------------------------------------------------------------
    def download(self, landmarks=True):
        """(pose [3, n], logw [n], lm [nl, 5, n] or None) as NumPy arrays in the shard's dtype."""
        pose = np.empty((3, self.n), dtype=self.np_dtype)
        logw = np.empty(self.n, dtype=self.np_dtype)
        lm = np.empty((self.nl, 5, self.n), dtype=self.np_dtype) if landmarks else None
        check(lib.slam_pf_download(self._h, pose.ctypes.data, logw.ctypes.data, lm.ctypes.data if landmarks else None))
        return pose, logw, lm

    def sync(self):
        check(lib.slam_pf_sync(self._h))


class LandmarkEvidence:
    """Landmark evidence of an unknown-correspondence filter (include/slamhip_evidence.h): one int8 existence counter per
    (slot, particle) on the device, raised by ``inc`` (up to ``cap``) when the step matched the slot, lowered by ``dec`` when the
    landmark lies within ``r_max`` and +-``half_fov`` of the particle's pose and was not observed; below zero the record is
    discarded and its slot is free again.  A record made since the last pass starts at ``init``.

    ``shard`` is a :class:`PFShard` that holds the WHOLE filter (no peers; sharded filters are not supported).  The object
    borrows the shard: close it before the shard.  A filter with an evidence object is resampled through :meth:`resample`
    (``FastSLAM.step_unknown_pruned`` does) and through nothing else -- otherwise the counters no longer belong to their
    particles."""
    EMPTY = -128

    def __init__(self, shard, r_max, half_fov, inc=1, dec=1, init=1, cap=5):
        self.shard = shard
        self.r_max, self.half_fov = float(r_max), float(half_fov)
        self.inc, self.dec, self.init, self.cap = int(inc), int(dec), int(init), int(cap)
        self._e = C.c_void_p()
        self._lib = evidence_lib()
        check(self._lib.slam_pf_evidence_create(C.byref(self._e), shard._h))
        shard._borrowers = getattr(shard, "_borrowers", 0) + 1

    def close(self):
        if getattr(self, "_e", None) is not None and self._e:
            if self.shard._h:                       # (a shard closed first took the stream along: nothing left to free on)
                self._lib.slam_pf_evidence_destroy(self._e)
            self._e = C.c_void_p()
            self.shard._borrowers = getattr(self.shard, "_borrowers", 1) - 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rule(self):
        return self.r_max, self.half_fov, self.inc, self.dec, self.init, self.cap

    def update(self, assoc, want_counts=True, assume_ready=False):
        """One pass of the rule with the decisions ``assoc`` of the step just made: the int32 torch tensor [m, n] on the
        shard's device that ``update_unknown`` / ``step_unknown_fused`` returned (None: no observation).  Returns the counts
        [records in use, created, decremented, pruned] as int64 (the call then synchronises), or None.  ``assume_ready``: the
        tensor is known to be complete (it came from a call that synchronises), so the device is not synchronised first."""
        m, ptr = 0, None
        if assoc is not None and assoc.numel():
            import torch
            assert assoc.is_cuda and assoc.dtype == torch.int32 and assoc.is_contiguous() and assoc.shape[1] == self.shard.n
            if not assume_ready:
                torch.cuda.synchronize(self.shard.device)    # assoc may have been produced on torch's stream
            m, ptr = int(assoc.shape[0]), C.c_void_p(assoc.data_ptr())
        counts = np.zeros(4, dtype=np.int64) if want_counts else None
        check(self._lib.slam_pf_evidence_update(self._e, ptr, m, *self._rule(), _ptr(counts, C.c_int64) if want_counts else None))
        return counts

    def step(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, want_counts=True):
        """``PFShard.step_unknown_fused`` followed by :meth:`update` with its decisions, as one library call
        (slam_pf_step_unknown_evidence).  Returns ((gmax, s1, s2), counts)."""
        zp = _obs(z)
        q, r = _small(Q), _small(R)
        out = np.empty(3)
        counts = np.zeros(4, dtype=np.int64) if want_counts else None
        check(self._lib.slam_pf_step_unknown_evidence(self._e, float(V), float(G), float(wheelbase), _ptr(q), float(dt), _ptr(zp),
                                                      zp.shape[0], _ptr(r), float(gate1), float(gate2), *self._rule(), _ptr(out),
                                                      _ptr(counts, C.c_int64) if want_counts else None))
        return (float(out[0]), float(out[1]), float(out[2])), counts

    def resample(self, gmax, u0):
        """``PFShard.resample_local`` with the counters following their particles (slam_pf_evidence_resample)."""
        check(self._lib.slam_pf_evidence_resample(self._e, float(gmax), float(u0)))

    def counters(self):
        """The counters, int8 [nl, n] (EMPTY = -128: no landmark in that slot of that particle)."""
        out = np.empty((self.shard.nl, self.shard.n), dtype=np.int8)
        check(self._lib.slam_pf_evidence_get(self._e, out.ctypes.data))
        return out


class PathHistory:
    """Per-particle trajectory history of a filter (include/slamhip_path.h): a ring of ``cap`` records on the device, each a
    snapshot of the poses and the ancestors back to the record before, and the read-outs that follow the CURRENT particles
    back through it -- ``trace`` (the paths of named particles), ``best`` (of the particle with the largest log-weight),
    ``mean`` (the weighted mean path) and ``survivors`` (distinct ancestors still alive at each record, the depletion
    diagnostic).  Device memory: cap * (3 * itemsize + 4) * n + 8 n bytes.

    ``shard`` is a :class:`PFShard` that holds the WHOLE filter (no peers; sharded filters are not supported).  The object
    borrows the shard: close it before the shard.  A filter with a path object is resampled through :meth:`resample`
    (``FastSLAM.resample`` does once ``FastSLAM.track_path`` has been called) and through nothing else -- otherwise the history
    no longer belongs to the particles.  Records are held oldest first: index 0 of every read-out is the oldest held record."""

    def __init__(self, shard, cap):
        self.shard = shard
        self.cap = int(cap)
        self._p = C.c_void_p()
        self._lib = path_lib()
        check(self._lib.slam_pf_path_create(C.byref(self._p), shard._h, self.cap))
        shard._borrowers = getattr(shard, "_borrowers", 0) + 1

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            if self.shard._h:                       # (a shard closed first took the stream along: nothing left to free on)
                self._lib.slam_pf_path_destroy(self._p)
            self._p = C.c_void_p()
            self.shard._borrowers = getattr(self.shard, "_borrowers", 1) - 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def record(self):
        """The live poses into the next slot, with the composed ancestors of the resamplings since the last record
        (slam_pf_path_record).  Enqueued."""
        check(self._lib.slam_pf_path_record(self._p))

    def resample(self, gmax, u0):
        """``PFShard.resample_local`` with the history following the particles (slam_pf_path_resample)."""
        check(self._lib.slam_pf_path_resample(self._p, float(gmax), float(u0)))

    def info(self):
        """{L: records held, records: records ever made, cap, resamples: resamplings seen}."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.slam_pf_path_info(self._p, _ptr(out, C.c_int64)))
        return dict(L=int(out[0]), records=int(out[1]), cap=int(out[2]), resamples=int(out[3]))

    def _rows(self):
        return max(1, self.info()["L"])              # (L == 0: the library refuses the read-out; the buffer is never written)

    def get(self, k=0):
        """The record ``k`` back (0: the newest): (pose [3, n] float64, ancestors [n] int32 -- the identity where none were
        stored --, ancestors stored?)."""
        pose = np.empty((3, self.shard.n))
        anc = np.empty(self.shard.n, dtype=np.int32)
        has = C.c_int()
        check(self._lib.slam_pf_path_get(self._p, int(k), _ptr(pose), _ptr(anc, C.c_int32), C.byref(has)))
        return pose, anc, bool(has.value)

    def trace(self, ids):
        """The paths of the current particles ``ids`` (at most 4096): [len(ids), L, 3] float64 = (x, y, phi), oldest first."""
        idv = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        out = np.empty((max(1, idv.shape[0]), self._rows(), 3))
        check(self._lib.slam_pf_path_trace(self._p, _ptr(idv, C.c_int64), idv.shape[0], _ptr(out)))
        return out

    def best(self):
        """(index, path [L, 3]) of the particle with the largest log-weight (lowest index on a tie)."""
        idx = C.c_int64()
        out = np.empty((self._rows(), 3))
        check(self._lib.slam_pf_path_best(self._p, C.byref(idx), _ptr(out)))
        return int(idx.value), out

    def mean(self):
        """The mean path under the current weights: [L, 4] = (x, y, phi, R), R the mean resultant length of the headings."""
        out = np.empty((self._rows(), 4))
        check(self._lib.slam_pf_path_mean(self._p, _ptr(out)))
        return out

    def survivors(self):
        """int64 [L]: distinct particles at each record that have a descendant among the current particles."""
        out = np.empty(self._rows(), dtype=np.int64)
        check(self._lib.slam_pf_path_survivors(self._p, _ptr(out, C.c_int64)))
        return out


class _SingleProcess:
    """The world of one rank."""
    rank, world = 0, 1

    def allreduce_max(self, v):
        return v

    def allreduce_sum(self, vec):
        return vec

    def all_gather(self, t, n_global):
        return t

    def all_gather_scalars(self, vec):
        return [list(vec)]

    def all_to_all_v(self, send, send_counts, recv_counts):
        return send


class ShmScalars:
    """All-gather of a few float64 per rank through a shared-memory page, for ranks of ONE node.

    The per-step exchange of a sharded filter is three scalars per rank that the HOST needs (Neff decides about
    resampling): through a device collective that is a host-to-device copy, a collective launch and a read-back,
    ~50 us, against a few microseconds here.  Layout [parity][rank][8 float64], entry 7 = the sequence number of the
    call, written last; a call spins until every rank's entry shows its number.  Two parities: a rank can be at most
    one call ahead of the slowest one (it needs everybody's entry of call s before it can write call s + 1), so
    the page of call s is not overwritten while anybody still reads it."""
    WIDTH = 8

    def __init__(self, dist, rank, world):
        import socket
        import uuid
        hosts = [None] * world
        dist.all_gather_object(hosts, socket.gethostname())
        if len(set(hosts)) != 1 or not os.path.isdir("/dev/shm"):
            raise RuntimeError("ranks are not on one node")
        name = [f"/dev/shm/slamhip-{uuid.uuid4().hex}" if rank == 0 else None]
        dist.broadcast_object_list(name, src=0)
        self.rank, self.world, self.seq = rank, world, 0
        shape = (2, world, self.WIDTH)
        if rank == 0:
            np.zeros(shape, dtype=np.float64).tofile(name[0])
        dist.barrier()
        self.mem = np.memmap(name[0], dtype=np.float64, mode="r+", shape=shape)
        dist.barrier()
        if rank == 0:
            os.unlink(name[0])                       # the mappings keep the page alive; nothing is left behind in /dev/shm

    def all_gather(self, vec):
        assert len(vec) < self.WIDTH
        self.seq += 1
        page = self.mem[self.seq & 1]
        mine = page[self.rank]
        mine[:len(vec)] = vec
        mine[self.WIDTH - 1] = self.seq              # published last (x86 keeps the order of the stores)
        flags = page[:, self.WIDTH - 1]
        spins = 0
        while not (flags == self.seq).all():
            spins += 1
            if spins > 50_000_000:
                raise RuntimeError("shared-memory exchange: a rank did not arrive")
        return page[:, :len(vec)].tolist()


class TorchComm:
    """torch.distributed (nccl = RCCL over xGMI on the GPUs, gloo in the CPU tests).

    With the gloo backend device tensors are staged through the host (gloo's CUDA support is partial): that
    is how several ranks can rehearse the real GPU shards on ONE card; RCCL runs never take that path.
    The per-step scalar exchange goes through shared memory when all ranks share a node (ShmScalars)."""

    def __init__(self, device, shm_scalars=True):
        import torch.distributed as dist
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.device = device
        self.stage = dist.get_backend() == "gloo"
        self.shm = None
        if shm_scalars and self.world > 1 and os.environ.get("SLAMHIP_SHM_SCALARS", "1") != "0":
            try:
                self.shm = ShmScalars(dist, self.rank, self.world)
            except RuntimeError:
                self.shm = None                      # several nodes: the collective below

    def _in(self, t):
        return t.cpu() if self.stage and t.is_cuda else t

    def _out(self, t, like):
        return t.to(like.device) if self.stage and like.is_cuda else t

    def allreduce_max(self, v):
        import torch
        t = torch.tensor([v], dtype=torch.float64, device="cpu" if self.stage else self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def allreduce_sum(self, vec):
        import torch
        t = torch.tensor(list(vec), dtype=torch.float64, device="cpu" if self.stage else self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [float(x) for x in t.tolist()]

    def all_gather_scalars(self, vec):
        """[world][len(vec)] float64 table, rows in rank order."""
        if self.shm is not None:
            return self.shm.all_gather([float(v) for v in vec])
        import torch
        t = torch.tensor(list(vec), dtype=torch.float64, device="cpu" if self.stage else self.device)
        out = torch.empty(self.world * t.numel(), dtype=torch.float64, device=t.device)
        self.dist.all_gather_into_tensor(out, t)
        return out.reshape(self.world, -1).tolist()

    def all_gather(self, t, n_global):
        import torch
        src = self._in(t.contiguous())
        out = torch.empty(n_global, dtype=src.dtype, device=src.device)
        self.dist.all_gather_into_tensor(out, src)       # equal slices: rank r owns [r*n, (r+1)*n)
        return self._out(out, t)

    def all_to_all_v(self, send, send_counts, recv_counts):
        """Rows of `send` (dim 0) are grouped by destination rank; returns the rows received, grouped by source."""
        import torch
        src = self._in(send.contiguous())
        out = torch.empty((int(sum(recv_counts)),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        self.dist.all_to_all_single(out, src, [int(c) for c in recv_counts], [int(c) for c in send_counts])
        return self._out(out, send)


class FastSLAM:
    """Host logic of the particle filter, identical for one and for many ranks.

    ``shard`` follows the :class:`PFShard` protocol; ``comm`` is ``None`` (single process) or a
    :class:`TorchComm`.  Equal slices are assumed: rank r owns [r * n, (r + 1) * n).
    """

    def __init__(self, shard, comm=None, neff_frac=0.75):
        self.shard = shard
        self.comm = comm if comm is not None else _SingleProcess()
        self.neff_frac = float(neff_frac)
        self.fused = True                           # use shard.step_fused when the shard offers it
        self.force_exchange = False                 # measurement only: take the multi-rank resampling flow on one rank
        self._gmax_norm = None                      # max log-weight after the last normalize() (None: unknown)
        self.resamples = 0
        self.path_history = None                    # a PathHistory once track_path() has been called
        self.last_neff = float(shard.n_global)
        assert shard.n * self.comm.world == shard.n_global and shard.first == self.comm.rank * shard.n, (
            "ranks must own equal, contiguous slices in rank order")

    def track_path(self, cap):
        """Keep the particles' trajectories from here on: a :class:`PathHistory` of ``cap`` records (returned, and kept as
        ``self.path_history``).  From then on ``resample()`` goes through it, the synchronous ``step`` / ``step_unknown`` /
        ``step_unknown_fused`` make one record at their end, and the enqueued steps (``step_async*``: their resampling stays on
        the device) and ``step_unknown_pruned`` (its resampling goes through the evidence object) raise.  Whole filter on one
        rank only."""
        if self.comm.world != 1 or self.shard.n != self.shard.n_global:
            raise ValueError("the path history supports only a filter that lives wholly on one rank")
        if self.path_history is not None:
            self.path_history.close()
        self.path_history = PathHistory(self.shard, cap)
        return self.path_history

    def _record_path(self):
        if self.path_history is not None:
            self.path_history.record()

    def _no_path(self, what):
        if self.path_history is not None:
            raise RuntimeError(f"{what} cannot be used while the filter tracks its path (FastSLAM.track_path): its resampling "
                               "does not go through the path history")

    def predict(self, V, G, wheelbase, Q, dt):
        self.shard.predict(V, G, wheelbase, Q, dt)

    def update_known(self, z, ids, R):
        self._gmax_norm = None
        self.shard.update_known(z, ids, R)

    def global_stats(self, local=None):
        """(gmax, sum w, sum w^2) with w = exp(logw - gmax): one all-gather of three scalars per rank.
        ``local``: this shard's (max, sum, sum2) if a fused step has already produced them."""
        lmax, s1, s2 = self.shard.weight_stats() if local is None else local
        # ONE small all-gather of (max, sum, sum2) per rank; every rank then folds the same table in rank order
        # (two dependent all-reduces -- MAX, then SUM of the rescaled sums -- cost two collective latencies per step)
        table = self.comm.all_gather_scalars([lmax, s1, s2])
        gmax = max(row[0] for row in table)
        gs1 = gs2 = 0.0
        for m_r, s1_r, s2_r in table:
            f = math.exp(m_r - gmax)
            gs1 += s1_r * f
            gs2 += s2_r * f * f
        return gmax, gs1, gs2

    def normalize(self, local=None):
        """Normalise the weights, return Neff = 1 / sum(w_normalised^2)."""
        gmax, gs1, gs2 = self.global_stats(local)
        self.shard.normalize(gmax, gs1)
        self.last_neff = gs1 * gs1 / gs2
        # the largest log-weight AFTER the shift, exactly as stored (subtracting one constant in the storage type is
        # monotone, so it is the image of the old maximum): spares resample() a reduction over all weights + a sync
        T = getattr(self.shard, "np_dtype", np.float64)
        self._gmax_norm = float(T(gmax) - T(gmax + math.log(gs1)))
        return self.last_neff

    def resample(self):
        """Systematic resampling over the global weights (call after normalize())."""
        import torch
        sh, comm = self.shard, self.comm
        u0 = philox_uniform(self.resamples, STREAM_RESAMPLE, sh.seed)
        local = getattr(sh, "resample_local", None)
        if self.path_history is not None:
            if self.force_exchange or self._gmax_norm is None:
                raise RuntimeError("a filter that tracks its path resamples after normalize(), through the path history only")
            local = self.path_history.resample                          # the same call, the history follows the particles
        if comm.world == 1 and not self.force_exchange and local is not None and self._gmax_norm is not None:
            local(self._gmax_norm, u0)                                  # the whole filter on one GPU: one library call
            self._gmax_norm = None
            self._count_resampling()
            return 0
        logw_all = comm.all_gather(sh.logw_tensor(), sh.n_global)      # the all-gather of log-weights
        gmax = self._gmax_norm if self._gmax_norm is not None else float(logw_all.max().item())
        self._gmax_norm = None
        if comm.world == 1 and not self.force_exchange:                 # every ancestor is local: nothing to exchange
            sh.resample_apply(sh.ancestors(logw_all, gmax, u0), None, None)
            self._count_resampling()
            return 0
        # Every rank computes the ancestor of EVERY slot from the same all-gathered weights, so each knows which of its
        # particles every other rank needs: no request round, ONE all-to-all of records.  The table is ascending
        # (systematic resampling), and so is the owner of each slot: the (destination rank, ancestor) pairs come out
        # sorted, unique_consecutive removes the duplicates, and both the send list (my particles, grouped by
        # destination) and the receive list (ascending ids = grouped by source) are slices of that one list.
        n, me, world = sh.n, comm.rank, comm.world
        anc_all = sh.ancestors_all(logw_all, gmax, u0).to(torch.int64)
        slot_rank = torch.arange(sh.n_global, device=anc_all.device, dtype=torch.int64) // n
        # (boolean-mask indexing synchronises: each mask is turned into an index list once)
        remote = torch.nonzero(torch.div(anc_all, n, rounding_mode="floor") != slot_rank).reshape(-1)
        pairs = torch.unique_consecutive(slot_rank[remote] * sh.n_global + anc_all[remote])
        dst, aid = torch.div(pairs, sh.n_global, rounding_mode="floor"), pairs % sh.n_global
        src = torch.div(aid, n, rounding_mode="floor")
        out_idx, in_idx = torch.nonzero(src == me).reshape(-1), torch.nonzero(dst == me).reshape(-1)
        send_ids, need_ids = aid[out_idx], aid[in_idx]
        counts = torch.stack([torch.bincount(dst[out_idx], minlength=world),
                              torch.bincount(src[in_idx], minlength=world)]).tolist()      # split sizes of the all-to-all
        rec = sh.pack((send_ids - sh.first).to(torch.int32))                                # [rows, n_send]
        got = comm.all_to_all_v(rec.t().contiguous(), counts[0], counts[1])                 # [n_need, rows], ascending ids
        anc = anc_all[sh.first:sh.first + n].to(torch.int32).contiguous()
        sh.resample_apply(anc, need_ids.to(torch.int32), got.t().contiguous())
        self._count_resampling()
        return int(need_ids.numel())

    def _count_resampling(self):
        # the count is part of the filter state (it keys the systematic-resampling offset): the library's copy follows
        self.resamples += 1
        setter = getattr(self.shard, "set_resample_count", None)
        if setter is not None:
            setter(self.resamples)

    def step(self, V, G, wheelbase, Q, dt, z, ids, R, force_resample=None, proposal=False):
        """predict + known-id updates + normalise + (Neff-triggered) resample.  Returns (Neff, resampled?).
        ``proposal``: the FastSLAM-2.0 step -- the pose is drawn from the proposal that knows this step's
        observations (shard.step_proposal) instead of from the motion model alone."""
        fused = getattr(self.shard, "step_fused", None) if self.fused else None
        local = getattr(self.shard, "step_fused_normalized", None) if (self.fused and self.comm.world == 1) else None
        self._gmax_norm = None
        if proposal:
            neff = self.normalize(self.shard.step_proposal(V, G, wheelbase, Q, dt, z, ids, R))
        elif local is not None:                       # the whole filter on one GPU: one library call per step
            neff, self._gmax_norm = local(V, G, wheelbase, Q, dt, z, ids, R)
            self.last_neff = neff
        elif fused is not None:                     # one sweep over the particles instead of five launches
            neff = self.normalize(fused(V, G, wheelbase, Q, dt, z, ids, R))
        else:
            self.predict(V, G, wheelbase, Q, dt)
            self.update_known(z, ids, R)
            neff = self.normalize()
        do = force_resample if force_resample is not None else (neff < self.neff_frac * self.shard.n_global)
        if do:
            self.resample()
        self._record_path()
        return neff, bool(do)

    # -- the same step without the host in the loop --------------------------------------------------------------------
    def step_async(self, V, G, wheelbase, Q, dt, z, ids, R, force_resample=None, proposal=False, prepared=None):
        """``step`` ENQUEUED (shard.step_auto): returns nothing; Neff and the resampling decision stay on the device,
        steps queue back to back, ``flush()`` waits and reports.  On one rank the resampling itself happens on the
        device too.  A sharded filter resamples through the host (all-gather of the log-weights + record exchange): the
        library halts at such a step, skips what was queued behind it, and this method resolves the halt the moment
        the library reports it -- resample(), resume (the skipped steps are enqueued again), carry on."""
        self._no_path("step_async")
        self._gmax_norm = None
        sh = self.shard
        while sh.step_auto(V, G, wheelbase, Q, dt, z, ids, R, neff_frac=self.neff_frac, force=force_resample,
                           proposal=proposal, prepared=prepared):
            self._resolve_halt()

    def step_async_batch(self, batch, wheelbase, Q, dt, R, proposal=False, persistent=False):
        """K ``step_async`` calls as one (shard.step_auto_batch, ``batch`` from PFShard.prepare_batch); ``persistent=True`` allows
        persistent launches of up to 16 steps (see there).  Halts of the sharded halting flow are resolved on the way."""
        self._no_path("step_async_batch")
        self._gmax_norm = None
        sh = self.shard
        k, K = 0, batch[0]
        while k < K:
            took = sh.step_auto_batch(batch, wheelbase, Q, dt, R, neff_frac=self.neff_frac, proposal=proposal,
                                      persistent=persistent, start=k)
            k += took
            if k < K:
                self._resolve_halt()

    def flush(self):
        """Wait for the steps queued by step_async.  Returns (Neff of the last step, it resampled?)."""
        while True:
            r = self.shard.flush()
            if r is None:
                self._resolve_halt()
                continue
            self.last_neff, did, self.resamples = r[0], r[1], r[2]
            return self.last_neff, did

    def _resolve_halt(self):
        sh = self.shard
        self._gmax_norm, self.resamples = sh.halt_info()
        self.resample()                                   # the legacy path: collectives issued from here
        sh.resume(self.resamples)

    def step_unknown(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, force_resample=None, proposal=False):
        """The filter step with UNKNOWN correspondences: predict, per-particle gated nearest-neighbour
        association + updates / new landmarks, normalise, (Neff-triggered) resample.  Returns (Neff, resampled?).
        Resampling copies whole particle records, unused landmark slots included, so it needs no change.
        ``proposal``: the FastSLAM-2.0 form (shard.step_proposal_unknown: association under the proposal, the pose drawn
        from the proposal that knows the matched observations); at most 16 observations, whole filter on one rank."""
        self._gmax_norm = None
        if proposal:
            assert self.comm.world == 1, "the proposal step with unknown correspondences needs the whole filter on one rank"
            neff = self.normalize(self.shard.step_proposal_unknown(V, G, wheelbase, Q, dt, z, R, gate1, gate2))
        else:
            self.predict(V, G, wheelbase, Q, dt)
            self.shard.update_unknown(z, R, gate1, gate2)
            neff = self.normalize()
        do = force_resample if force_resample is not None else (neff < self.neff_frac * self.shard.n_global)
        if do:
            self.resample()
        self._record_path()
        return neff, bool(do)

    def step_unknown_fused(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, force_resample=None):
        """``step_unknown`` with predict, association + updates and the weight statistics as ONE sweep over the particles
        (shard.step_unknown_fused), for up to 64 observations per step.  Returns (Neff, resampled?)."""
        self._gmax_norm = None
        neff = self.normalize(self.shard.step_unknown_fused(V, G, wheelbase, Q, dt, z, R, gate1, gate2))
        do = force_resample if force_resample is not None else (neff < self.neff_frac * self.shard.n_global)
        if do:
            self.resample()
        self._record_path()
        return neff, bool(do)

    def step_unknown_pruned(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2, evidence, force_resample=None, proposal=False):
        """``step_unknown_fused`` with landmark evidence: the step is taken through ``evidence.step`` (a
        :class:`LandmarkEvidence` of this filter's shard: association + updates / new landmarks, then the counters and the
        pruning), and a resampling goes through ``evidence.resample`` so that the counters follow their particles.  Pruning
        touches no weight.  Whole filter on one rank only.  Returns (Neff, resampled?, counts) with counts = [records in
        use, created, decremented, pruned] of this step.  ``proposal``: the step is shard.step_proposal_unknown (FastSLAM 2.0,
        at most 16 observations), followed by ``evidence.update`` on its decisions."""
        assert self.comm.world == 1, "landmark evidence supports only a filter that lives wholly on one rank"
        self._no_path("step_unknown_pruned")
        self._gmax_norm = None
        if proposal:
            stats, assoc = self.shard.step_proposal_unknown(V, G, wheelbase, Q, dt, z, R, gate1, gate2, want_assoc=True)
            counts = evidence.update(assoc, assume_ready=True)
        else:
            stats, counts = evidence.step(V, G, wheelbase, Q, dt, z, R, gate1, gate2)
        neff = self.normalize(stats)
        do = force_resample if force_resample is not None else (neff < self.neff_frac * self.shard.n_global)
        if do:
            u0 = philox_uniform(self.resamples, STREAM_RESAMPLE, self.shard.seed)
            evidence.resample(self._gmax_norm, u0)
            self._gmax_norm = None
            self._count_resampling()
        return neff, bool(do), counts

    def mean_pose(self):
        s = self.comm.allreduce_sum(list(self.shard.mean_pose_sums()))
        return np.array([s[0], s[1], math.atan2(s[2], s[3])])       # weights are normalised: sums are means

    # -- hand-over to the EKF (include/slamhip_handover.h) --------------------------------------------------------------------
    def to_ekf(self, ids=None, max_landmarks=None):
        """The filter collapsed into a new :class:`EKFSlamState` on the same device and of the same dtype: the moment-matched
        joint Gaussian of the particles over the pose and the landmarks ``ids`` (None: every landmark seen so far), with the
        pose-landmark and landmark-landmark cross-covariances the per-landmark read-out (``map``) does not have
        (PFShard.to_ekf_into).  ``max_landmarks`` as in EKFSlamState (default max(64, 2 N)).  ``state.handover_info`` holds
        ``{"W", "neff", "n", "N"}``.  Whole filter on one rank only."""
        if self.comm.world != 1 or self.shard.n != self.shard.n_global:
            raise ValueError("the hand-over supports only a filter that lives wholly on one rank")
        sh = self.shard
        if max_landmarks is None:
            cnt = sh.nl if ids is None else int(np.asarray(ids).size)
            max_landmarks = max(64, 2 * cnt)
        st = EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype="f32" if sh.np_dtype == np.float32 else "f64",
                          max_landmarks=int(max_landmarks), device=sh.device.index)
        try:
            st.handover_info = sh.to_ekf_into(st, ids)
        except Exception:
            st.close()
            raise
        return st

    # -- clone, more landmark slots, another particle count (include/slamhip_pfcopy.h) ------------------------------------------
    def _movable(self, what):
        sh = self.shard
        if self.comm.world != 1 or not isinstance(self.comm, _SingleProcess):
            raise ValueError(f"{what} supports only a filter without a comm, wholly on one rank")
        if sh.n != sh.n_global or sh.first != 0 or getattr(self, "peers", False):
            raise ValueError(f"{what} supports only a filter that lives wholly on one shard, without peers")
        if self.path_history is not None or getattr(sh, "_borrowers", 0):
            raise ValueError(f"{what}: a PathHistory or LandmarkEvidence object follows this filter's particles; such histories "
                             "are not copied -- close it first")

    def _new_shard(self, n, max_landmarks):
        sh = self.shard
        return PFShard(int(n), int(max_landmarks), sh.seed, dtype="f32" if sh.np_dtype == np.float32 else "f64", device=sh.device.index)

    def _adopt(self, shard):
        old, self.shard = self.shard, shard
        old.close()
        if hasattr(self, "n"):
            self.n = shard.n

    def clone(self):
        """A second filter equal to this one bit for bit -- particles, RNG state, resample count -- on the same device
        (PFShard.copy_from: this filter is only read).  Driven like the original it stays equal to it."""
        self._movable("clone")
        new = object.__new__(type(self))
        FastSLAM.__init__(new, self._new_shard(self.shard.n, self.shard.nl), None, self.neff_frac)
        for name in ("n", "peers", "selftest_ok"):
            if hasattr(self, name):
                setattr(new, name, getattr(self, name))
        try:
            new.shard.copy_from(self.shard)
        except Exception:
            new.shard.close()
            raise
        new.fused, new.resamples, new.last_neff, new._gmax_norm = self.fused, self.resamples, self.last_neff, self._gmax_norm
        return new

    def reserve(self, max_landmarks, unknown=False):
        """Give the filter ``max_landmarks`` >= the current landmark slots, in place: the particles move to a new shard on the
        device (PFShard.copy_from) and the old one is closed.  ``unknown``: the new slots are unused records, as a filter
        with unknown correspondences needs them; otherwise they are as a new filter has them."""
        self._movable("reserve")
        if int(max_landmarks) < self.shard.nl:
            raise ValueError("reserve cannot drop landmark slots (PFShard.select_from chooses landmarks)")
        new = self._new_shard(self.shard.n, max_landmarks)
        try:
            new.copy_from(self.shard, fill=1 if unknown else 0)
        except Exception:
            new.close()
            raise
        self._adopt(new)

    def resize(self, n):
        """The filter continues with ``n`` particles, in place: drawn from the current ones by systematic resampling into n
        slots (PFShard.resize_from), uniform weights, counted as a resampling; the offset is the one an ordinary resampling
        would take now.  Normalises first when the weights are not.  Returns the ancestor table."""
        self._movable("resize")
        if self._gmax_norm is None:
            self.normalize()
        new = self._new_shard(n, self.shard.nl)
        try:
            anc = new.resize_from(self.shard, self._gmax_norm, philox_uniform(self.resamples, STREAM_RESAMPLE, self.shard.seed))
        except Exception:
            new.close()
            raise
        self._adopt(new)
        self._gmax_norm = None
        self.resamples += 1
        self.last_neff = float(n)
        return anc

    def adapt(self, cell_xy, cell_phi, eps=0.05, z=2.326, n_min=64, n_max=1 << 22):
        """KLD-sampling (Fox 2003) between steps: count the occupied cells of the pose histogram (PFShard.pose_bins), take
        the particle count they ask for (:func:`kld_particle_count`) and :meth:`resize` when it differs from the current
        one.  Returns the count the filter continues with."""
        self._movable("adapt")
        want = kld_particle_count(self.shard.pose_bins(cell_xy, cell_phi), eps=eps, z=z, n_min=n_min, n_max=n_max)
        if want != self.shard.n:
            self.resize(want)
        return want

    # -- the map ---------------------------------------------------------------------------------------------------------
    def map_sums(self, ids=None):
        """The filter's sums of the weighted map (PFShard.map_sums added over the ranks), [1 + cnt, 10]."""
        local = self.shard.map_sums(ids)
        return np.asarray(self.comm.allreduce_sum(local.reshape(-1).tolist()), dtype=np.float64).reshape(local.shape)

    def map(self, ids=None):
        """The map: [cnt, 8] = {mass, mean x, mean y, Cxx, Cxy, Cyy, count, 0} per landmark (``ids`` 1-based, None: all),
        the moment-matched Gaussian of the particles' mixture (see finalise_map).  Collective for a sharded filter."""
        return finalise_map(self.map_sums(ids))

    def transform(self, tx, ty, theta):
        """Express the filter in another frame: every rank calls it on its shard (PFShard.transform)."""
        self.shard.transform(tx, ty, theta)

    def align(self, ids, xy, apply=True):
        """Fit the rigid transform (no scale) that carries the map() means of the landmarks ``ids`` (1-based) onto the
        surveyed positions ``xy`` ([2, k] or [k, 2]; 2 x 2 is read as [2, k]) in the least-squares sense and, unless ``apply`` is False, move the
        filter into that frame.  Returns ``(tx, ty, theta)``.  Collective for a sharded filter."""
        m = self.map(np.asarray(ids, dtype=np.int32).reshape(-1))
        if m.shape[0] and not np.all(m[:, 0] > 0.0):
            raise ValueError("a named landmark has no particle that holds it")
        tx, ty, theta = rigid_fit(m[:, 1:3].T, xy)
        if apply:
            self.transform(tx, ty, theta)
        return tx, ty, theta

    def best_particle(self):
        """The particle with the largest log-weight of the whole filter (lowest global id on a tie):
        (global id, log-weight, pose [3], records [nl, 5]), the same on every rank.  Collective for a sharded filter."""
        gid, lw, pose, lm = self.shard.particle(-1)
        if self.comm.world == 1:
            return gid, lw, pose, lm
        table = self.comm.all_gather_scalars([lw, float(gid)])
        best = max(range(len(table)), key=lambda r: (table[r][0], -table[r][1]))
        rec = np.concatenate([pose, lm.reshape(-1)]) if best == self.comm.rank else np.zeros(3 + lm.size)
        rec = np.asarray(self.comm.allreduce_sum(rec.tolist()), dtype=np.float64)       # (the owner's record + zeros)
        return int(table[best][1]), float(table[best][0]), rec[:3], rec[3:].reshape(lm.shape)


def socket_host():
    import socket
    return socket.gethostname()


def shared_page(dist, rank, world, doubles):
    """A zero-filled float64 page in /dev/shm that every rank of ONE node maps (the ranks' scalar page of a sharded
    filter: slam_pf_attach_exchange).  The file is unlinked once every rank has mapped it."""
    import uuid
    name = [f"/dev/shm/slamhip-x-{uuid.uuid4().hex}" if rank == 0 else None]
    dist.broadcast_object_list(name, src=0)
    if rank == 0:
        fd = os.open(name[0], os.O_CREAT | os.O_EXCL | os.O_WRONLY, 0o600)
        with os.fdopen(fd, "wb") as f:
            f.write(np.zeros(doubles, dtype=np.float64).tobytes())
    dist.barrier()
    mem = np.memmap(name[0], dtype=np.float64, mode="r+", shape=(doubles,))
    dist.barrier()
    if rank == 0:
        os.unlink(name[0])
    return mem


class PFSlamState(FastSLAM):
    """``PFSlamState{T}`` (src/common.jl:31-34) as a device-resident, optionally sharded filter.

    ``n`` particles in total; under ``torch.distributed`` every rank constructs it with the same
    arguments and owns n / world of them on its own GPU.
    """

    def __init__(self, n, max_landmarks, seed=0, dtype="f32", device=0, neff_frac=0.75, distributed=None, peers=None):
        """``peers`` (sharded filter): None = the device-side exchange where it can be had (one node, at most 8 ranks, the
        self-test passes; SLAMHIP_PF_PEERS=0 says no), False = the halting flow through ``torch.distributed`` (RCCL on the
        GPUs) whatever the node could do.  ``self.peers`` says which one runs, ``self.selftest_ok`` what the self-test of
        the GPUs' view of each other's inboxes said (None: not tried)."""
        import torch.distributed as dist
        use_dist = dist.is_available() and dist.is_initialized() if distributed is None else distributed
        if use_dist:
            import torch
            rank, world = dist.get_rank(), dist.get_world_size()
            trace = os.environ.get("SLAMHIP_TRACE_CLOSE") == "1"

            def say(msg):
                if trace:
                    print(f"[create rank {rank}] {msg}", file=sys.stderr, flush=True)
            if n % world:
                raise ValueError("n must be divisible by the number of ranks")
            per = n // world
            shard = PFShard(per, max_landmarks, seed, dtype=dtype, first=rank * per, n_global=n, device=device)
            comm = TorchComm(torch.device("cuda", int(device)))
            self.peers = False
            self.selftest_ok = None
            want_peers = (os.environ.get("SLAMHIP_PF_PEERS", "1") != "0") if peers is None else bool(peers)
            if world > 1:
                # the ranks' GPUs address each other's buffers (IPC handles, moved here by an object all-gather): the
                # per-step scalars travel GPU to GPU and a resampling step stays on the device.  SLAMHIP_PF_PEERS=0, more
                # than 8 ranks or ranks on several nodes: the legacy flow -- scalars through a shared pinned page, a
                # resampling step halts and the host resamples through the collectives
                blobs = [None] * world
                say("shard created; exporting")
                mine = shard.export_peer()
                say("exported; all-gather of the blobs")
                dist.all_gather_object(blobs, (socket_host(), mine))
                say("blobs gathered")
                one_node = len({h for h, _ in blobs}) == 1
                if one_node and world <= 8 and want_peers:
                    # attach, then prove that the GPUs see each other's inbox writes; any rank failing either step sends
                    # every rank to the fallback (the decision must be the same everywhere)
                    # one rank at a time (a precaution: with dmabuf IPC the importer asks the EXPORTER's process for the
                    # buffer, so two processes inside an open of each other's memory depend on each other's runtime).
                    # A landmark buffer above 2 GiB makes attach_peers refuse (hipIpcOpenMemHandle hangs above that size
                    # on ROCm 7.2: tools/ipc_gen_test.py) and every rank takes the fallback below
                    ok = True
                    for turn in range(world):
                        if turn == rank:
                            try:
                                shard.attach_peers(rank, world, [b for _, b in blobs])
                            except Exception:  # noqa: BLE001 -- e.g. hipIpcOpenMemHandle refused
                                ok = False
                        dist.barrier()
                    say(f"attached ({ok}); self-test")
                    try:
                        ok = ok and shard.peer_selftest()
                    except Exception:  # noqa: BLE001
                        ok = False
                    say(f"self-test {ok}")
                    oks = [None] * world
                    dist.all_gather_object(oks, bool(ok))
                    self.selftest_ok = bool(all(oks))
                    if all(oks):
                        self.peers = True
                    else:
                        try:
                            shard.detach_peers()
                        except Exception:  # noqa: BLE001
                            pass
                if one_node and not self.peers:
                    shard.attach_exchange(rank, world, shared_page(dist, rank, world, 2 * world * 8))
        else:
            shard = PFShard(n, max_landmarks, seed, dtype=dtype, device=device)
            comm = None
            self.peers = False
            self.selftest_ok = None
        super().__init__(shard, comm, neff_frac)
        self.n = n

    # -- the read-outs telemetry.monitor_messages asks a state for (as EKFSlamState has them) ---------------------------
    def snapshot(self):
        """The map and the pose of this moment from ONE query (one pass over the records, one all-reduce on a sharded
        filter): a :class:`MapSnapshot` with ``pose()``, ``N``, ``feature_ellipses()``, ``vehicle_ellipse()`` -- what
        ``telemetry.monitor_messages`` asks a state for.  The methods below are each a query of their own (``pose`` and
        ``vehicle_ellipse`` of the pose row alone); a caller that wants all of them takes a snapshot."""
        return MapSnapshot(self.map_sums())

    def pose(self):
        """The weighted mean pose [x, y, phi]."""
        return MapSnapshot(self.map_sums([])).pose()

    @property
    def N(self):
        """Landmarks the filter has a map of (weight mass > 0)."""
        return self.snapshot().N

    def feature_ellipses(self):
        """5 x N: cx, cy, rx, ry, phi of the landmarks with mass (in landmark order), the convention of
        ``EKFSlamState.feature_ellipses`` (rx <= ry, phi of the first eigenvector in [-pi/2, pi/2])."""
        return self.snapshot().feature_ellipses()

    def vehicle_ellipse(self):
        """[cx, cy, vehicle_phi, rx, ry, phi] of the particles' pose cloud."""
        return MapSnapshot(self.map_sums([])).vehicle_ellipse()

    def path(self):
        """The path of the particle with the largest log-weight, [L, 3] = (x, y, phi), oldest held record first
        (``track_path`` first; PathHistory.best)."""
        if self.path_history is None:
            raise RuntimeError("the filter does not track its path: call track_path(cap) first")
        return self.path_history.best()[1]

    def mean_path(self):
        """The mean path under the current weights, [L, 4] = (x, y, phi, R) (``track_path`` first; PathHistory.mean)."""
        if self.path_history is None:
            raise RuntimeError("the filter does not track its path: call track_path(cap) first")
        return self.path_history.mean()

    def close(self):
        """Collective for a sharded filter with peers: remote records are brought home, the peers are detached, then a
        barrier -- nobody frees buffers a peer may still read."""
        if getattr(self, "path_history", None) is not None:
            self.path_history.close()
            self.path_history = None
        if getattr(self, "peers", False):
            import torch.distributed as dist
            trace = os.environ.get("SLAMHIP_TRACE_CLOSE") == "1"
            if trace:
                print(f"[close rank {dist.get_rank()}] detach", file=sys.stderr, flush=True)
            self.shard.detach_peers()
            self.shard.sync()
            if trace:
                print(f"[close rank {dist.get_rank()}] barrier", file=sys.stderr, flush=True)
            dist.barrier()
            if trace:
                print(f"[close rank {dist.get_rank()}] destroy", file=sys.stderr, flush=True)
            self.peers = False
        self.shard.close()


def particles_to_ekf(pf, ids=None, max_landmarks=None):
    """``pf.to_ekf(ids, max_landmarks)`` as a free function (the reference's style)."""
    return pf.to_ekf(ids, max_landmarks)


def ekf_to_particles(state, n, seed=0, ids=None, max_landmarks=None, neff_frac=0.75):
    """``state.to_particles(n, ...)`` as a free function: a :class:`PFSlamState` of ``n`` particles drawn from the EKF state
    (vehicle marginal, landmark conditionals), on its device and of its dtype."""
    cnt = state.N if ids is None else int(np.asarray(ids).size)
    pf = PFSlamState(int(n), int(max_landmarks) if max_landmarks is not None else max(cnt, 1), seed=seed,
                     dtype="f32" if state.np_dtype == np.float32 else "f64", device=state.device, neff_frac=neff_frac, distributed=False)
    try:
        pf.shard.from_ekf(state, ids)
    except Exception:
        pf.close()
        raise
    return pf


def save_particles(shard):
    """A checkpoint of a :class:`PFShard` as a dict of NumPy arrays and scalars: ``pose``, ``logw``, ``lm`` (what ``download``
    returns), ``seen`` and the meta (sizes, dtype, seed, RNG step, resample count).  :func:`load_particles` restores it."""
    pose, logw, lm = shard.download()
    d = shard.meta()                                # (after the download: an auto-mode filter has been left by then)
    d.update(pose=pose, logw=logw, lm=lm)
    return d


def load_particles(d, device=0):
    """A new :class:`PFShard` from a :func:`save_particles` dict: same particles, RNG state and resample count, so that the
    restored filter continues bit for bit like the saved one."""
    sh = PFShard(d["n"], d["max_landmarks"], d["seed"], dtype=d["dtype"], first=d["first"], n_global=d["n_global"], device=device)
    try:
        sh.upload(d["pose"], d["logw"], d["lm"], d["seen"])
        sh.set_rng(d["seed"], d["step"])
        sh.set_resample_count(d["resamples"])
    except Exception:
        sh.close()
        raise
    return sh


def kld_particle_count(k, eps=0.05, z=2.326, n_min=64, n_max=1 << 22):
    """The particle count KLD-sampling (Fox 2003) asks for when the pose histogram has ``k`` occupied cells: with a = 2 / (9 (k - 1)),
    ceil((k - 1) / (2 eps) * (1 - a + sqrt(a) z)^3), clamped to [n_min, n_max]; ``n_min`` for k < 2.  ``eps``: the bound on the
    K-L distance, ``z``: the upper 1 - delta quantile of the standard normal (2.326: delta = 0.01).  Host arithmetic."""
    k = int(k)
    if k < 2:
        return int(n_min)
    a = 2.0 / (9.0 * (k - 1))
    n = math.ceil((k - 1) / (2.0 * float(eps)) * (1.0 - a + math.sqrt(a) * float(z)) ** 3)
    return int(min(max(n, int(n_min)), int(n_max)))


def attach_local_peers(shards):
    """Several shards of ONE process (one host thread per shard; several GPUs, or -- the tests -- several shards on one
    card) become the ranks of one sharded filter: every shard attaches every shard's blob (raw pointers, no IPC).
    Shards on ONE card wait for each other inside their kernels, so each shard's stream needs a hardware queue of its own:
    set ``GPU_MAX_HW_QUEUES`` (default 4 per device) to at least ``len(shards) + 2`` before the first HIP call."""
    blobs = [sh.export_peer() for sh in shards]
    for r, sh in enumerate(shards):
        sh.attach_peers(r, len(shards), blobs)
