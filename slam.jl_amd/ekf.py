"""Host-side mirror of SLAM.jl's EKF surface (src/SLAM.jl:5-30) over libslamhip.

Same names, argument meaning and error behaviour as the reference functions --
``predict``, ``update``, ``add_features``, ``associate``, ``compute_association``,
``predict_observation``, ``mpi_to_pi`` and the types ``SlamState`` /
``EKFSlamState`` -- so a caller written like ``sim!`` (sim/ekfslam-sim.jl:100-120)

    state.x, state.cov = predict(state, vehicle, Q, dt)
    zf, idf, zn = associate(state, z, R, 4.0, 25.0)
    state.x, state.cov = update(state, zf, R, idf)
    state.x, state.cov = add_features(state, zn, R)

runs unchanged.  The state lives on the GPU: ``state.x`` / ``state.cov`` are lazy
references (:class:`DeviceRef`) that download only when turned into an array, and
re-assigning a state's own references back to it is free.  The in-place names of
BASELINE.json's north star are provided as ``ekf_predict_`` / ``ekf_update_`` /
``augment_`` (Julia: ``ekf_predict!`` / ``ekf_update!`` / ``augment!``).

Every numeric operation is a HIP kernel behind the C ABI; nothing here computes
filter quantities on the CPU, and nothing imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import SLAM_F32, SLAM_F64, SLAM_FORM_CHOLESKY, SLAM_FORM_JOSEPH, check, lib

__all__ = [
    "observe",
    "SlamState", "EKFSlamState", "DeviceRef", "predict", "update", "add_features", "associate",
    "compute_association", "predict_observation", "mpi_to_pi", "ekf_predict_", "ekf_update_", "augment_",
    "remove_features", "remove_features_", "removal_maps",
    "find_duplicates", "merge_features", "merge_features_", "merge_in_batches",
    "chi2_table", "associate_joint", "observe_joint",
    "copy_state", "select_features", "select_map", "grown_capacity",
    "CovarianceFactor", "linear_rows", "LocalArea", "IteratedResult", "FirstEstimates",
]

_DTYPES = {"f32": (SLAM_F32, np.float32), "f64": (SLAM_F64, np.float64),
           np.float32: (SLAM_F32, np.float32), np.float64: (SLAM_F64, np.float64),
           "float32": (SLAM_F32, np.float32), "float64": (SLAM_F64, np.float64)}


def _dbl(a, n=None):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} values, got {arr.size}")
    return arr


def _small(M):
    """2 x 2 matrix -> column-major double[4]."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (2, 2):
        raise ValueError("expected a 2 x 2 matrix")
    return np.ascontiguousarray(M.T).reshape(4)          # [m11, m21, m12, m22]


def _ptr(a, ctype=C.c_double):
    return a.ctypes.data_as(C.POINTER(ctype))


def _mat3(M):
    """3 x 3 matrix -> column-major double[9]."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (3, 3):
        raise ValueError("expected a 3 x 3 matrix")
    return np.ascontiguousarray(M.T).reshape(9)


def linear_rows(H, n):
    """The CSR arrays ``(ptr int32 [k + 1], idx int32, val float64)`` of a linear measurement over n states, as
    slam_ekf_update_linear takes them.  ``H``: a dense (k, n) array (its non-zeros, in column order) or a list of
    ``{state index: value}`` rows (in the dict's order).  The library checks the row and index limits."""
    rows = []
    if isinstance(H, np.ndarray) or (len(H) and not isinstance(H[0], dict)):
        D = np.atleast_2d(np.asarray(H, dtype=np.float64))
        if D.shape[1] != n:
            raise ValueError(f"H has {D.shape[1]} columns, the state has {n} entries")
        for r in D:
            nz = np.flatnonzero(r)
            rows.append((nz, r[nz]))
    else:
        for r in H:
            rows.append((np.fromiter(r.keys(), dtype=np.int64, count=len(r)), np.fromiter(r.values(), dtype=np.float64, count=len(r))))
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(i) for i, _ in rows])
    idx = np.ascontiguousarray(np.concatenate([i for i, _ in rows]) if rows else np.zeros(0), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate([v for _, v in rows]) if rows else np.zeros(0), dtype=np.float64)
    return ptr, idx, val


def _obs(z):
    """Reference layout z: 2 x nz (rows range, bearing) -> contiguous (range, bearing) pairs."""
    z = np.asarray(z, dtype=np.float64)
    if z.size == 0:
        return np.zeros((0, 2))
    if z.ndim == 1:
        z = z.reshape(2, 1)
    if z.shape[0] != 2:
        raise ValueError("z must be 2 x nz")
    return np.ascontiguousarray(z.T)


def removal_maps(N, ids):
    """The two index maps of a landmark removal, as slam_ekf_remove_landmarks builds them on the host (restated here
    for callers that renumber their own per-landmark tables, and for the CPU tests): ``keep`` (int32, 3 + 2 (N - cnt)
    surviving 0-based state indices, ascending -- x[keep], P[keep][:, keep] is the reduced state) and ``new_index``
    (int32, N entries: the new 1-based id of old landmark j at [j - 1], 0 if removed).  ``ids``: 1-based, any order;
    ValueError for an id outside 1..N or a duplicate (the library: SLAM_E_BADARG)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 1 or ids.max() > N):
        raise ValueError("landmark id out of range")
    gone = np.zeros(N, dtype=bool)
    gone[ids - 1] = True
    if int(gone.sum()) != ids.size:
        raise ValueError("duplicate landmark id")
    left = np.flatnonzero(~gone)
    keep = np.concatenate([np.arange(3), np.stack([3 + 2 * left, 4 + 2 * left], axis=1).reshape(-1)]).astype(np.int32)
    new_index = np.zeros(N, dtype=np.int32)
    new_index[left] = np.arange(1, left.size + 1, dtype=np.int32)
    return keep, new_index


def select_map(N, ids):
    """The index map of a selection, as slam_ekf_select forms it on the device (restated here for callers that carry their own
    per-landmark tables, and for the CPU tests): ``s`` (int32, 3 + 2 len(ids) 0-based state indices of the source, the vehicle
    first, then the two rows of landmark ids[k] for every k in the order given) -- x[s], P[s][:, s] is the selected state.
    ``ids``: 1-based, distinct, any order; ValueError for an id outside 1..N or a repeated one (the library: SLAM_E_BADARG)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 1 or ids.max() > N):
        raise ValueError("landmark id out of range")
    if np.unique(ids).size != ids.size:
        raise ValueError("duplicate landmark id")
    f = 3 + 2 * (ids - 1)
    return np.concatenate([np.arange(3), np.stack([f, f + 1], axis=1).reshape(-1)]).astype(np.int32)


def grown_capacity(capacity, needed):
    """The capacity a growing state (``grow=True``) reserves when ``needed`` landmarks do not fit ``capacity``: twice the
    capacity, or what is needed if that is more -- the amortised doubling of the reference's re-allocation."""
    capacity, needed = int(capacity), int(needed)
    if capacity < 0 or needed < 0:
        raise ValueError("capacity and needed must not be negative")
    return max(2 * capacity, needed)


def merge_in_batches(N, pairs, merge_call, batch_max=_lib.SLAM_MERGE_MAX):
    """Host side of EKFSlamState.merge_landmarks: any number of pairs (1-based ids of the map as it is now, N landmarks)
    through calls of at most ``batch_max`` DISJOINT pairs each (slam_ekf_merge_landmarks takes no landmark twice in one call).
    ``merge_call(batch)`` merges ``batch`` (int32 [m, 2], ids valid at that moment, the second of a pair leaves) and returns that
    call's new_index; the ids of the pairs still waiting are carried through it.  A pair whose landmarks appear in no other
    pair goes down as given (the one named second leaves, as in the C call); where pairs share a landmark (a chain a-b, b-c,
    or the three pairs of a triple) the lowest id survives, and a pair whose landmarks have become one by then is dropped.
    Returns new_index for the N original landmarks: the final id of the landmark each one is now part of.
    ValueError: an id outside 1..N, or a pair that names one landmark twice."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 1 or pairs.max() > N):
        raise ValueError("landmark id out of range")
    if np.any(pairs[:, 0] == pairs[:, 1]):
        raise ValueError("a pair names one landmark twice")
    uses = np.bincount(pairs.reshape(-1), minlength=N + 1)
    cur = np.arange(1, N + 1, dtype=np.int64)               # current id of the landmark that original j is part of
    waiting = [(int(a), int(b)) for a, b in pairs]
    while waiting:
        batch, busy, later = [], set(), []
        for a, b in waiting:
            ca, cb = int(cur[a - 1]), int(cur[b - 1])
            if ca == cb:
                continue                                    # already one landmark
            if len(batch) == batch_max or ca in busy or cb in busy:
                later.append((a, b))
                continue
            if (uses[a] > 1 or uses[b] > 1) and cb < ca:
                ca, cb = cb, ca                             # shared landmarks: the lowest id survives
            batch.append((ca, cb))
            busy.update((ca, cb))
        if not batch:
            break
        new_index = np.asarray(merge_call(np.asarray(batch, dtype=np.int32)), dtype=np.int64)
        cur = new_index[cur - 1]
        waiting = later
    return cur.astype(np.int32)


def mpi_to_pi(phi):
    """src/common.jl:102-110 (host scalar helper: one conditional wrap)."""
    if phi > math.pi:
        return phi - 2 * math.pi
    if phi < -math.pi:
        return phi + 2 * math.pi
    return phi


def rigid_fit(src, dst):
    """The closed-form 2-D least-squares rigid fit (rotation and translation, no scale) of the points ``src`` onto ``dst``
    ([2, k] or [k, 2] each, k >= 2; a 2 x 2 array is ALWAYS read as [2, k], one point per column):
    theta = atan2(sum cross, sum dot) of the two centred point sets, t = the centroid of
    dst minus the rotated centroid of src.  Returns ``(tx, ty, theta)`` with dst ~ R(theta) src + t.  Fewer than two
    points, or all points of either set coincident: ValueError."""
    def pts(a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2 or 2 not in a.shape:
            raise ValueError("points must be [2, k] or [k, 2]")
        return a if a.shape[0] == 2 else a.T                 # (a 2 x 2 array is read as [2, k])
    a, b = pts(src), pts(dst)
    if a.shape != b.shape:
        raise ValueError("src and dst disagree on the number of points")
    if a.shape[1] < 2:
        raise ValueError("a rigid fit needs at least two points")
    ca, cb = a.mean(axis=1, keepdims=True), b.mean(axis=1, keepdims=True)
    da, db = a - ca, b - cb
    if not (np.sum(da * da) > 0.0 and np.sum(db * db) > 0.0):
        raise ValueError("coincident points do not determine a rotation")
    theta = math.atan2(float(np.sum(da[0] * db[1] - da[1] * db[0])), float(np.sum(da[0] * db[0] + da[1] * db[1])))
    c, s = math.cos(theta), math.sin(theta)
    return float(cb[0, 0] - (c * ca[0, 0] - s * ca[1, 0])), float(cb[1, 0] - (s * ca[0, 0] + c * ca[1, 0])), theta


def chi2_table(m, confidence=0.95):
    """The thresholds of the joint-compatibility search: entry k - 1 is the chi-square quantile at ``confidence`` with 2k degrees of
    freedom, k = 1 .. m.  For even degrees of freedom the distribution function has the closed form
    1 - exp(-x / 2) sum_{i < k} (x / 2)^i / i!; the quantile is found by bisection (no scipy)."""
    confidence = float(confidence)
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must lie strictly between 0 and 1")
    m = int(m)
    have = _CHI2_CACHE.get(confidence)
    if have is not None and have.size >= m:
        return have[:m].copy()

    def cdf(x, k):
        h, term, acc = 0.5 * x, 1.0, 0.0
        for i in range(k):
            acc += term
            term *= h / (i + 1)
        return 1.0 - math.exp(-h) * acc

    out = np.empty(int(m))
    for k in range(1, int(m) + 1):
        lo, hi = 0.0, 4.0 * k + 16.0
        while cdf(hi, k) < confidence:
            hi *= 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if cdf(mid, k) < confidence:
                lo = mid
            else:
                hi = mid
        out[k - 1] = 0.5 * (lo + hi)
    _CHI2_CACHE[confidence] = out.copy()
    return out


_CHI2_CACHE = {}                    # confidence -> the longest table computed so far (a filter asks for the same one every step)


JC_INFO_KEYS = ("pairings", "d2", "tests", "exhausted", "truncated", "candidates", "deepest")


class IteratedResult:
    """What an iterated update reports (slam_ekf_update_iterated, include/ext/slamhip_iterated.h): ``iterations`` run, ``converged``
    (the last step was <= tol), the last ``step``, ``nis`` = v' inv(S) v and ``log_det`` of S at the last iteration, the MAP cost after
    the first iteration (``cost_first``) and after the last (``cost_last``), and ``out``, the ten numbers as the library wrote them.
    ``batches``: the results of every batch of a call that took more than 8 observations, this one last."""

    def __init__(self, out):
        self.out = np.array(out, dtype=np.float64)
        self.iterations = int(self.out[0])
        self.converged = bool(self.out[1])
        self.step = float(self.out[2])
        self.nis = float(self.out[3])
        self.log_det = float(self.out[4])
        self.cost_first = float(self.out[8])
        self.cost_last = float(self.out[9])
        self.batches = (self,)

    def __repr__(self):
        return (f"IteratedResult(iterations={self.iterations}, converged={self.converged}, step={self.step:.3g}, nis={self.nis:.6g}, "
                f"cost_first={self.cost_first:.6g}, cost_last={self.cost_last:.6g})")


class SlamState:
    """``abstract SlamState`` (src/common.jl:22)."""


class DeviceRef:
    """Lazy reference to ``x`` or ``cov`` of a device-resident state."""

    __slots__ = ("state", "which")

    def __init__(self, state, which):
        self.state = state
        self.which = which

    def __array__(self, dtype=None, copy=None):
        a = self.state.download(self.which)
        return a.astype(dtype) if dtype is not None else a

    def numpy(self):
        return self.state.download(self.which)

    def __len__(self):
        return self.state.n

    @property
    def shape(self):
        n = self.state.n
        return (n,) if self.which == "x" else (n, n)

    def __getitem__(self, idx):
        return self.numpy()[idx]

    def __repr__(self):
        return f"<DeviceRef {self.which} of {self.state!r}>"


class EKFSlamState(SlamState):
    """``EKFSlamState{T}(x, cov)`` (src/common.jl:25-28), device resident.

    ``max_landmarks`` fixes the capacity (the reference grows P by reallocating,
    src/ekf.jl:108-109); ``dtype`` is "f32" or "f64" (reference: Float64).
    With ``grow=True`` the capacity follows the map instead: where add_features, observe, observe_joint or join would stop with
    SLAM_E_CAPACITY the state moves into a larger handle on the device (:meth:`reserve`) and the step is finished there.
    """

    def __init__(self, x, cov, dtype="f64", max_landmarks=None, device=0, grow=False):
        code, npdt = _DTYPES[dtype]
        self.grow = bool(grow)
        self._gate_mode = None                   # what the caller set through this object: re-applied by reserve()
        self._async = None
        x = np.asarray(x)
        n = int(x.shape[0])
        if n < 3 or (n - 3) % 2:
            raise ValueError("length(x) must be 3 + 2*N")
        N = (n - 3) // 2
        if max_landmarks is None:
            max_landmarks = max(64, 2 * N)
        self.np_dtype = npdt
        self.max_landmarks = int(max_landmarks)
        self.device = int(device)
        self._h = C.c_void_p()
        check(lib.slam_ekf_create(C.byref(self._h), code, self.max_landmarks, int(device)))
        try:
            self.set_state(x, cov)
        except Exception:
            self.close()
            raise

    # -- lifetime ----------------------------------------------------------------
    def close(self):
        for obj in list(getattr(self, "_fej", ())):                       # they borrow the handle: they go first
            obj.close()
        if getattr(self, "_jc", None):
            _lib.jc_lib().slam_ekf_jc_destroy(self._jc)               # the search workspace borrows the handle: it goes first
            self._jc = None
        if getattr(self, "_borrowed", False):                            # the local handle of a LocalArea: its library owns it
            self._h = C.c_void_p()
            return
        if getattr(self, "_h", None) is not None and self._h:
            lib.slam_ekf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return f"EKFSlamState(N={self.N}, dtype={np.dtype(self.np_dtype).name}, max_landmarks={self.max_landmarks})"

    # -- sizes ----------------------------------------------------------------------
    @property
    def N(self):
        out = C.c_int()
        check(lib.slam_ekf_num_landmarks(self._h, C.byref(out)))
        return out.value

    @property
    def n(self):
        return 3 + 2 * self.N

    @property
    def capacity(self):
        """The landmark capacity of the handle (slam_ekf_capacity)."""
        out = C.c_int()
        check(_lib.copy_lib().slam_ekf_capacity(self._h, C.byref(out)))
        return out.value

    # -- a state moved between two handles on the device (include/slamhip_copy.h) --------------
    def copy_from(self, other):
        """This state becomes ``other``'s (slam_ekf_copy): N, x and every entry of cov, bit for bit, on the device.  The
        capacities may differ in either direction as long as other.N fits this one.  ``other`` is only read and may be updated
        or closed right away; gate mode, async flag and timing of this object stay its own.  Enqueued, does not synchronise."""
        if not isinstance(other, EKFSlamState):
            raise TypeError("copy_from needs another EKFSlamState")
        check(_lib.copy_lib().slam_ekf_copy(self._h, other._h))

    def select_from(self, other, ids):
        """This state becomes the marginal of ``other`` over the vehicle and the landmarks ``ids`` (1-based, distinct, any order;
        none: the vehicle alone), on the device (slam_ekf_select): landmark k here is ``other``'s landmark ids[k - 1], x = x[s],
        cov = cov[s][:, s] with s = select_map(other.N, ids), bit for bit."""
        if not isinstance(other, EKFSlamState):
            raise TypeError("select_from needs another EKFSlamState")
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        check(_lib.copy_lib().slam_ekf_select(self._h, other._h, _ptr(ids, C.c_int32) if ids.size else None, int(ids.size)))

    def _blank(self, max_landmarks):
        return EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype=self.np_dtype, max_landmarks=int(max_landmarks),
                            device=self.device, grow=self.grow)

    def copy(self, max_landmarks=None):
        """A new state on the same device that holds this one (copy_from), with this one's capacity or ``max_landmarks``: a fork
        to try a hypothesis on."""
        new = self._blank(self.capacity if max_landmarks is None else max_landmarks)
        try:
            new.copy_from(self)
        except Exception:
            new.close()
            raise
        return new

    def select(self, ids, max_landmarks=None):
        """A new state on the same device that holds the sub-map ``ids`` of this one with its full marginal covariance
        (select_from); ``max_landmarks`` as in the constructor (default max(64, 2 len(ids)))."""
        cnt = int(np.asarray(ids).size)
        new = self._blank(max(64, 2 * cnt) if max_landmarks is None else max_landmarks)
        try:
            new.select_from(self, ids)
        except Exception:
            new.close()
            raise
        return new

    # -- the Cholesky factor of cov on the device (include/ext/slamhip_factor.h) ---------------------
    def factor(self, dtype=None, out=None, panel_tiles=0):
        """cov = L L' on the device (slam_ekf_factor_compute): a :class:`CovarianceFactor`.  ``dtype``: the arithmetic and storage
        type of L, default this state's; "f64" over an fp32 state is the trustworthy check of it (an fp32 factor of an fp64 state is
        refused).  ``out``: an existing factor to compute into (its dtype, capacity and panel width are kept).  ``panel_tiles``:
        1, 2 or 4 tile columns per panel, 0 = the default for the dtype.  NotPositiveDefinite when a pivot fails (the factor
        passed as ``out`` then holds the failing index in ``.info``).  This state is only read.  Synchronises."""
        if out is None:
            new = CovarianceFactor(self.np_dtype if dtype is None else dtype, self.capacity, device=self.device,
                                   panel_tiles=panel_tiles)
            try:
                new.compute(self)
            except Exception:
                new.close()
                raise
            return new
        out.compute(self)
        return out

    def is_positive_definite(self, dtype="f64"):
        """``(ok, index, landmark)``: whether cov has a Cholesky factor in ``dtype`` arithmetic; if not, the first failing state
        index (0-based) and the landmark it belongs to (1-based; 0: the vehicle), else (True, -1, -1).  A failing pivot raises
        nothing."""
        f = CovarianceFactor(dtype, self.capacity, device=self.device)
        try:
            try:
                f.compute(self)
            except _lib.NotPositiveDefinite:
                i = int(f.info[2])
                return False, i, (0 if i < 3 else (i - 3) // 2 + 1)
            return True, -1, -1
        finally:
            f.close()

    def nees(self, x_true, ids=None):
        """The normalised estimation error squared e' cov^-1 e against the true state ``x_true`` (3 + 2 N values, or 3 + 2 len(ids)
        with ``ids``), e = x - x_true with the heading wrapped: over the whole map, or over the vehicle and the landmarks ``ids``
        (1-based) through select() -- the marginal -- and its factor.  In fp64 arithmetic whatever the state's dtype."""
        sub = self.select(ids) if ids is not None else None
        try:
            f = (sub if sub is not None else self).factor(dtype="f64")
            try:
                return f.nees(x_true)
            finally:
                f.close()
        finally:
            if sub is not None:
                sub.close()

    # -- hand-over to the particle filter (include/slamhip_handover.h) -------------------------------
    def to_particles(self, n, seed=0, ids=None, max_landmarks=None, neff_frac=0.75):
        """A new :class:`PFSlamState` of ``n`` particles drawn from this state on the device (slam_ekf_to_pf): poses from the
        vehicle marginal N(x_v, P_vv), every landmark ``ids`` (1-based, distinct; None: all) as its conditional given that pose
        -- the Rao-Blackwell factorisation FastSLAM rests on --, uniform weights.  ``max_landmarks`` is the filter's slot count
        (default: the landmarks handed over).  NotPositiveDefinite when P_vv or a conditional block is not positive definite
        (a vehicle known exactly: use PFShard.set_pose and init_landmarks)."""
        from .pf import ekf_to_particles
        return ekf_to_particles(self, n, seed=seed, ids=ids, max_landmarks=max_landmarks, neff_frac=neff_frac)

    def reserve(self, max_landmarks):
        """Make room for ``max_landmarks`` landmarks (nothing happens if the capacity is already that large): a new handle of
        that capacity is created, the state is copied into it on the device (slam_ekf_copy), the new handle takes the old
        one's place inside this object and the old one is destroyed.  The gate mode and the async flag set through this object
        are applied to the new handle; kernel timing starts switched off, and the joint-association workspace is dropped and
        made again at the next joint call.  Raw device pointers (:meth:`device_ptrs`) obtained before are DEAD afterwards;
        ``DeviceRef``s stay valid because they go through this object.  Old and new matrix exist side by side during the call."""
        max_landmarks = int(max_landmarks)
        if max_landmarks <= self.capacity:
            return
        code = _DTYPES[self.np_dtype][0]
        moved = [(obj, obj.get()) for obj in getattr(self, "_fej", ())]   # FirstEstimates objects follow the state: get ...
        if any(count != self.N for _obj, (_lin, _first, count) in moved):
            raise ValueError("a FirstEstimates object does not follow the map (remap it) and cannot move into a larger handle")
        new = C.c_void_p()
        check(lib.slam_ekf_create(C.byref(new), code, max_landmarks, self.device))
        try:
            check(_lib.copy_lib().slam_ekf_copy(new, self._h))
            if self._gate_mode is not None:
                check(lib.slam_ekf_set_gate_mode(new, self.GATE_MODES[self._gate_mode]))
            if self._async is not None:
                check(lib.slam_ekf_set_async(new, 1 if self._async else 0))
        except Exception:
            lib.slam_ekf_destroy(new)
            raise
        if getattr(self, "_jc", None):
            _lib.jc_lib().slam_ekf_jc_destroy(self._jc)               # it borrows the old handle
            self._jc = None
        for obj, _saved in moved:
            obj._release()                                                # (it borrows the old handle)
        old, self._h = self._h, new
        self.max_landmarks = max_landmarks
        lib.slam_ekf_destroy(old)                                     # (waits for the copy's last read of it)
        for obj, (lin, first, _count) in moved:                           # ... / set, on the new handle
            obj._attach()
            obj.set(lin, first)

    def _grow_for(self, needed):
        self.reserve(grown_capacity(self.capacity, needed))

    # -- state I/O --------------------------------------------------------------------
    def set_state(self, x, cov):
        x = np.ascontiguousarray(np.asarray(x, dtype=self.np_dtype))
        n = x.shape[0]
        cov = np.asarray(cov, dtype=self.np_dtype)
        if cov.shape != (n, n):
            raise ValueError("cov must be n x n")
        covf = np.asfortranarray(cov)
        check(lib.slam_ekf_set_state(self._h, x.ctypes.data, covf.ctypes.data, n, n))

    def set_state_device(self, d_x_ptr, d_P_ptr, n, ldP):
        """Upload from device pointers (e.g. ``tensor.data_ptr()``); column-major P."""
        check(lib.slam_ekf_set_state_device(self._h, C.c_void_p(d_x_ptr), C.c_void_p(d_P_ptr), int(n), int(ldP)))

    def download(self, which="both"):
        n = self.n
        x = np.empty(n, dtype=self.np_dtype) if which in ("x", "both") else None
        P = np.empty((n, n), dtype=self.np_dtype, order="F") if which in ("cov", "both") else None
        check(lib.slam_ekf_get_state(self._h, x.ctypes.data if x is not None else None,
                                     P.ctypes.data if P is not None else None, n, n))
        if which == "x":
            return x
        if which == "cov":
            return P
        return x, P

    def get_block(self, r0, c0, nr, nc):
        """cov[r0:r0+nr, c0:c0+nc] (0-based) without downloading the matrix (slam_ekf_get_block)."""
        out = np.empty((int(nr), int(nc)), dtype=self.np_dtype, order="F")
        check(lib.slam_ekf_get_block(self._h, int(r0), int(c0), int(nr), int(nc), out.ctypes.data, max(int(nr), 1)))
        return out

    def diag(self):
        """diag(cov) (slam_ekf_get_diag)."""
        out = np.empty(self.n, dtype=self.np_dtype)
        check(lib.slam_ekf_get_diag(self._h, out.ctypes.data))
        return out

    def landmark_blocks(self):
        """[3, N]: P[f, f], P[f+1, f], P[f+1, f+1] of every landmark (slam_ekf_get_landmark_blocks: the packed side array
        the gating sweep streams)."""
        out = np.empty((3, self.N), dtype=self.np_dtype)
        check(lib.slam_ekf_get_landmark_blocks(self._h, out.ctypes.data))
        return out

    GATE_MODES = {"auto": 0, "sweep": 1, "grid": 2}

    def set_gate_mode(self, mode):
        """How associate / observe search the map (slam_ekf_set_gate_mode; the reference's TODO, src/data-association.jl:18-20):
        "sweep" = every landmark, "grid" = the uniform grid over the landmark means (O(candidates)), "auto" = the grid
        from 16384 landmarks on.  Decisions are identical in every mode."""
        check(lib.slam_ekf_set_gate_mode(self._h, self.GATE_MODES[mode]))
        self._gate_mode = mode

    def gate_info(self):
        """slam_ekf_gate_info as a dict: which form the last gating used, the grid's size, and what the grid queries have
        visited / fully evaluated so far."""
        out = (C.c_int64 * 8)()
        check(lib.slam_ekf_gate_info(self._h, out))
        keys = ("form", "cells_per_axis", "in_grid", "tail", "rebuilds", "queries", "visited", "evaluated")
        d = dict(zip(keys, (int(v) for v in out)))
        d["form"] = {0: None, 1: "sweep", 2: "grid"}[d["form"]]
        return d

    def device_ptrs(self):
        """(x_ptr, P_ptr, ld, stream_ptr) raw device addresses for zero-copy interop."""
        dx, dP, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ld = C.c_int()
        check(lib.slam_ekf_device_ptrs(self._h, C.byref(dx), C.byref(dP), C.byref(ld), C.byref(st)))
        return dx.value, dP.value, ld.value, st.value

    @property
    def x(self):
        return DeviceRef(self, "x")

    @x.setter
    def x(self, value):
        if isinstance(value, DeviceRef) and value.state is self:
            return                                   # state.x, state.cov = predict(state, ...)
        self._pending_x = np.asarray(value, dtype=self.np_dtype)
        self._flush_pending()

    @property
    def cov(self):
        return DeviceRef(self, "cov")

    @cov.setter
    def cov(self, value):
        if isinstance(value, DeviceRef) and value.state is self:
            return
        self._pending_cov = np.asarray(value, dtype=self.np_dtype)
        self._flush_pending()

    def _flush_pending(self):
        # x and cov change size together (reset: sim/browser/wsserver.jl:161-174); upload once both agree
        px = getattr(self, "_pending_x", None)
        pc = getattr(self, "_pending_cov", None)
        if px is None:
            px = self.download("x")
        if pc is None:
            pc = self.download("cov")
        if pc.shape == (px.shape[0], px.shape[0]):
            self.set_state(px, pc)
            self._pending_x = None
            self._pending_cov = None

    def pose(self):
        out = np.empty(3)
        check(lib.slam_ekf_get_pose(self._h, _ptr(out)))
        return out

    def feature_ellipses(self):
        """feature_ellipses(x, cov) (sim/browser/wsserver.jl:72-85): 5 x N array [cx; cy; rx; ry; phi], computed
        on the device from the 2 x 2 diagonal blocks -- P is not downloaded."""
        N = self.N
        out = np.empty((5, N), dtype=np.float64, order="F")
        check(lib.slam_ekf_ellipses(self._h, _ptr(out) if N else None, None))
        return out

    def vehicle_ellipse(self):
        """[cx, cy, vehicle_phi, rx, ry, phi] of monitor() (sim/browser/wsserver.jl:60-65)."""
        out = np.empty(6)
        check(lib.slam_ekf_ellipses(self._h, None, _ptr(out)))
        return out

    # -- in-place operations (ekf_predict!, ekf_update!, augment!) ---------------------
    def predict(self, v, g, wheelbase, Q, dt):
        q = _small(Q)
        check(lib.slam_ekf_predict(self._h, float(v), float(g), float(wheelbase), _ptr(q), float(dt)))

    def associate_vector(self, z, R, gate1, gate2):
        """int32 assoc[nz]: j >= 1 matched landmark, 0 dropped, -1 new feature."""
        zp = _obs(z)
        nz = zp.shape[0]
        assoc = np.zeros(nz, dtype=np.int32)
        if nz:
            r = _small(R)
            check(lib.slam_ekf_associate(self._h, _ptr(zp), nz, _ptr(r), float(gate1), float(gate2),
                                         _ptr(assoc, C.c_int32)))
        return assoc

    def associate(self, z, R, gate1, gate2):
        """(zf 2 x nf, idf 1 x nf Int, zn 2 x nn), observation order preserved
        (src/data-association.jl:11-13,43-47)."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc = self.associate_vector(z, R, gate1, gate2)
        zf = z[:, assoc > 0]
        idf = assoc[assoc > 0].astype(np.int64).reshape(1, -1)
        zn = z[:, assoc < 0]
        return zf, idf, zn

    def update(self, zf, R, idf, form="cholesky"):
        zp = _obs(zf)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        if zp.shape[0] == 0:
            return
        r = _small(R)
        code = SLAM_FORM_JOSEPH if form == "joseph" else SLAM_FORM_CHOLESKY
        check(lib.slam_ekf_update(self._h, _ptr(zp), _ptr(ids, C.c_int32), zp.shape[0], _ptr(r), code))

    def add_features(self, zn, R):
        zp = _obs(zn)
        if zp.shape[0] == 0:
            return
        r = _small(R)
        rc = lib.slam_ekf_augment(self._h, _ptr(zp), zp.shape[0], _ptr(r))
        if rc == _lib.SLAM_E_CAPACITY and self.grow:                  # decided before anything was enqueued: grow, then again
            self._grow_for(self.N + zp.shape[0])
            rc = lib.slam_ekf_augment(self._h, _ptr(zp), zp.shape[0], _ptr(r))
        check(rc)

    def remove_landmarks(self, ids):
        """Take the landmarks ``ids`` (1-based, as idf; any order) out of the map, in place on the device
        (slam_ekf_remove_landmarks): x <- x[keep], P <- P[keep, keep] bit for bit, the others keep their order and are
        renumbered 1..N - len(ids).  Returns ``new_index`` (int32, length N_old): the new id of old landmark j at
        [j - 1], 0 if it was removed."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        new_index = np.zeros(self.N, dtype=np.int32)
        check(lib.slam_ekf_remove_landmarks(self._h, _ptr(ids, C.c_int32) if ids.size else None, int(ids.size),
                                            _ptr(new_index, C.c_int32) if new_index.size else None))
        return new_index

    def find_duplicates(self, gate, cap=1024):
        """Pairs of landmarks that are one feature entered twice (slam_ekf_find_duplicates): (a, b), a < b, 1-based, whose
        difference has a Mahalanobis distance below ``gate`` under the joint covariance, D = P_aa + P_bb - P_ab - P_ab'.
        Returns ``(pairs, count)``: int32 [min(count, cap), 2] in ascending order and the number of pairs in the whole
        map.  The state is not changed; P is read only for the pairs the means and diagonal blocks cannot rule out."""
        cap = int(cap)
        pairs = np.zeros((max(cap, 0), 2), dtype=np.int32)
        count = C.c_int()
        check(lib.slam_ekf_find_duplicates(self._h, float(gate), _ptr(pairs, C.c_int32) if cap > 0 else None, cap,
                                           C.byref(count)))
        return pairs[:min(count.value, max(cap, 0))], count.value

    def merge_landmarks(self, pairs, Rc=None):
        """Fuse the landmarks of every pair (1-based ids) into one, in place on the device (slam_ekf_merge_landmarks): the
        constraint m_a - m_b = 0 with noise ``Rc`` (2 x 2, None = exact) as one Cholesky-form update per call of at most
        SLAM_MERGE_MAX pairs, then the second landmark of each pair leaves the map as remove_landmarks removes it.  More
        pairs, or pairs that share a landmark, are split into several calls (merge_in_batches: chains end at their lowest
        id).  Returns ``new_index`` (int32, length N_old): the new id of old landmark j at [j - 1]; a landmark that was
        merged away carries the new id of the one it became part of."""
        rc = None if Rc is None else _small(Rc)

        def call(batch):
            batch = np.ascontiguousarray(batch, dtype=np.int32)
            new_index = np.zeros(self.N, dtype=np.int32)
            check(lib.slam_ekf_merge_landmarks(self._h, _ptr(batch, C.c_int32), int(batch.shape[0]),
                                               _ptr(rc) if rc is not None else None, _ptr(new_index, C.c_int32)))
            return new_index

        return merge_in_batches(self.N, pairs, call)

    # -- caller-supplied models (libslamhip_linear.so, include/ext/slamhip_linear.h) ------------------------------------
    def _linear(self, fn, H, z, R, wrap, innovation):
        ptr, idx, val = linear_rows(H, self.n)
        k = ptr.size - 1
        zz = _dbl(z, k)
        Rm = np.asarray(R, dtype=np.float64)
        if Rm.ndim < 2:                                                   # a scalar (k = 1) or the diagonal
            Rm = np.diag(np.broadcast_to(Rm.reshape(-1), (k,)).astype(np.float64))
        if Rm.shape != (k, k):
            raise ValueError(f"R must be {k} x {k}")
        rr = np.ascontiguousarray(Rm.T).reshape(-1)                       # column-major
        mask = 0
        for i in wrap:
            if not 0 <= int(i) < k:
                raise ValueError("wrap names a row that does not exist")
            mask |= 1 << int(i)
        out = np.zeros(4)
        mode = _lib.SLAM_LINEAR_INNOVATION if innovation else _lib.SLAM_LINEAR_MEASURED
        check(fn(self._h, k, _ptr(ptr, C.c_int32), _ptr(idx, C.c_int32), _ptr(val), _ptr(zz), _ptr(rr), mode, mask, _ptr(out)))
        return out

    def update_linear(self, H, z, R, wrap=(), innovation=False):
        """The Kalman update from a linear measurement z = H x + noise(R), in place on the device (slam_ekf_update_linear): the
        Cholesky form of ``update`` with the caller's H.  ``H``: a dense (k, n) array or a list of ``{state index: value}`` rows,
        k <= 16 rows of at most 8 non-zeros; state indices are 0-based (0, 1, 2 the vehicle; landmark j at 3 + 2 (j - 1)).
        ``R``: k x k, the diagonal, or a scalar.  ``wrap``: the rows whose innovation is an angle (wrapped to [-pi, pi]).
        ``innovation=True``: ``z`` already IS the innovation of a model the caller linearised.  Returns
        ``[v' inv(S) v, log det S, smallest pivot, -1]``; raises NotPositiveDefinite with the state unchanged."""
        return self._linear(_lib.linear_lib().slam_ekf_update_linear, H, z, R, wrap, innovation)

    def linear_nis(self, H, z, R, wrap=(), innovation=False):
        """What ``update_linear`` would return, with the state only read (slam_ekf_linear_nis): the chi-square gate to apply
        before committing a fix."""
        return self._linear(_lib.linear_lib().slam_ekf_linear_nis, H, z, R, wrap, innovation)

    def predict_linear(self, xv, Gv, Qv):
        """Predict with a caller's motion model (slam_ekf_predict_linear): x[0:3] = xv, P_vv = Gv P_vv Gv' + Qv,
        P_vm = Gv P_vm.  Of Qv the lower triangle is read."""
        a, g, q = _dbl(xv, 3), _mat3(Gv), _mat3(Qv)
        check(_lib.linear_lib().slam_ekf_predict_linear(self._h, _ptr(a), _ptr(g), _ptr(q)))

    def predict_odometry(self, d, Q3):
        """Compose the pose with a vehicle-frame increment d = (dx, dy, dtheta) of covariance Q3, wholly on the device
        (slam_ekf_predict_odometry): wheel odometry of any drive."""
        a, q = _dbl(d, 3), _mat3(Q3)
        check(_lib.linear_lib().slam_ekf_predict_odometry(self._h, _ptr(a), _ptr(q)))

    def fix_position(self, xy, R):
        """A position fix (a GPS receiver): the vehicle is at ``xy`` with covariance ``R``."""
        return self.update_linear([{0: 1.0}, {1: 1.0}], xy, R)

    def fix_heading(self, phi, var):
        """A heading fix (a compass): the heading is ``phi`` with variance ``var``; the innovation is wrapped."""
        return self.update_linear([{2: 1.0}], [phi], var, wrap=(0,))

    def fix_landmark(self, j, xy, R):
        """Landmark ``j`` (1-based) was surveyed at ``xy`` with covariance ``R``."""
        f = 3 + 2 * (int(j) - 1)
        return self.update_linear([{f: 1.0}, {f + 1: 1.0}], xy, R)

    def constrain_landmarks(self, a, b, dxy, R):
        """Landmark ``b`` lies ``dxy`` from landmark ``a`` (1-based), with covariance ``R`` (0: exactly)."""
        fa, fb = 3 + 2 * (int(a) - 1), 3 + 2 * (int(b) - 1)
        return self.update_linear([{fb: 1.0, fa: -1.0}, {fb + 1: 1.0, fa + 1: -1.0}], dxy, R)

    # -- the iterated update (libslamhip_iterated.so, include/ext/slamhip_iterated.h) -------------------------------------
    def _iterated(self, fn, zp, ids, r, max_iter, tol):
        out = np.zeros(10)
        check(fn(self._h, _ptr(zp), _ptr(ids, C.c_int32), zp.shape[0], _ptr(r), int(max_iter), float(tol), _ptr(out)))
        return IteratedResult(out)

    def update_iterated(self, zf, R, idf, max_iter=10, tol=1e-9):
        """The iterated EKF update (slam_ekf_update_iterated): ``update`` in its Cholesky form with the range-bearing model
        relinearised at every iterate -- Gauss-Newton on the MAP cost, WITHOUT a line search -- until the largest change of an
        iterate is at most ``tol`` or ``max_iter`` (1 .. 64) iterations have run; every iteration runs on the device and the map is
        touched once, at the end.  ``max_iter=1`` is ``update``.  Returns an :class:`IteratedResult` (iterations, converged, step,
        nis, cost_first, cost_last); raises NotPositiveDefinite with the state unchanged.
        A call takes at most 8 observations.  More are applied as consecutive batches of 8 in the order given, each iterated on the
        state the batch before it left: that is SEQUENTIAL and is not the joint update of all of them.  The result is then the
        last batch's, and its ``batches`` lists every batch's.  No observation: nothing is done and None is returned."""
        zp = _obs(zf)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        if zp.shape[0] == 0:
            return None
        r = _small(R)
        fn = _lib.iterated_lib().slam_ekf_update_iterated
        B = _lib.SLAM_ITERATED_MAXOBS
        done = []
        for s in range(0, zp.shape[0], B):
            done.append(self._iterated(fn, np.ascontiguousarray(zp[s:s + B]), np.ascontiguousarray(ids[s:s + B]), r, max_iter, tol))
        done[-1].batches = tuple(done)
        return done[-1]

    def iterated_nis(self, zf, R, idf, max_iter=10, tol=1e-9):
        """What ``update_iterated`` would return, with the state only read (slam_ekf_iterated_nis): the dry run that tells whether
        the iteration converges and lowers the cost (``cost_last`` against ``cost_first``) before it is committed.  At most 8
        observations: a second batch would have to start from the state the first one leaves."""
        zp = _obs(zf)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        if zp.shape[0] > _lib.SLAM_ITERATED_MAXOBS:
            raise ValueError("iterated_nis takes at most 8 observations")
        res = self._iterated(_lib.iterated_lib().slam_ekf_iterated_nis, zp, ids, _small(R), max_iter, tol)
        res.batches = (res,)
        return res

    def observe_iterated(self, z, R, gate1, gate2, max_iter=10, tol=1e-9):
        """associate -> update_iterated -> add_features (sim/ekfslam-sim.jl:114-120 with the iterated update), the three calls in
        sequence from the host.  Returns ``(assoc, result)``: the association vector (see associate_vector) and what
        ``update_iterated`` returned (None when nothing was matched)."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc = self.associate_vector(z, R, gate1, gate2)
        res = self.update_iterated(z[:, assoc > 0], R, assoc[assoc > 0], max_iter=max_iter, tol=tol)
        self.add_features(z[:, assoc < 0], R)
        return assoc, res

    # -- first-estimates Jacobians (libslamhip_fej.so, include/ext/slamhip_fej.h) -----------------------------------------
    def fej(self):
        """A :class:`FirstEstimates` object attached to this state: predict, update and add_features whose Jacobians are evaluated
        at every landmark's first estimate and at the vehicle's predicted pose, so that the filter gains no information along the
        three unobservable directions of the map.  It starts from the current estimates and is closed with the state."""
        return FirstEstimates(self)

    def update_joint_at_estimates(self, zf, R, idf):
        """``update`` (Cholesky form) of up to 64 observations per call through the wide front half of libslamhip_wide.so with the
        Jacobians at the stored state (slam_ekf_wide_update without a first-estimates object): the same estimator as ``update``,
        by other kernels -- the cross-check of :meth:`FirstEstimates.update_joint`.  Returns one row of ``out`` per batch of 64."""
        return _wide_batches(_lib.wide_lib().slam_ekf_wide_update, self._h, None, zf, R, idf)

    def transform(self, tx, ty, theta):
        """Express the whole state in another frame, in place on the device (slam_ekf_transform): every position becomes
        R(theta) p + (tx, ty), the heading mpi_to_pi(phi + theta), cov becomes T cov T' with T = blockdiag(R, 1, R, R, ...).
        Enqueued on the state's stream; nothing is downloaded."""
        check(_lib.frame_lib().slam_ekf_transform(self._h, float(tx), float(ty), float(theta)))

    def submap(self, max_landmarks):
        """A fresh local map for :meth:`join`: a state of the same dtype on the same device with pose (0, 0, 0), no landmark
        and cov = 0 -- its frame is this state's vehicle pose for as long as this state neither moves nor observes."""
        return EKFSlamState(np.zeros(3), np.zeros((3, 3)), dtype=self.np_dtype, max_landmarks=int(max_landmarks),
                            device=self.device)

    def join(self, other, merge_gate=None, Rc=None):
        """Map joining on the device (slam_ekf_join): the local map ``other``, whose frame is this state's vehicle pose (see
        :meth:`submap`), is appended to this one: the vehicle is composed with ``other``'s, ``other``'s landmark j becomes landmark
        N + j, cov becomes F cov F' + G cov_other G'.  ``other`` is only read and may be closed right away.  Returns
        ``first_new``, the 1-based id of ``other``'s first landmark in this map.
        With ``merge_gate`` set the overlap is fused afterwards: find_duplicates(merge_gate), then merge_landmarks(.., Rc) on at
        most SLAM_MERGE_MAX disjoint pairs, round after round until no pair is found; returns ``(first_new, new_index)`` with
        new_index (int32, one entry per landmark of the joined map) composed over the rounds."""
        if not isinstance(other, EKFSlamState):
            raise TypeError("join needs another EKFSlamState")
        first = C.c_int32()
        rc = _lib.join_lib().slam_ekf_join(self._h, other._h, C.byref(first))
        if rc == _lib.SLAM_E_CAPACITY and self.grow:                  # decided before anything was enqueued: grow, then again
            self._grow_for(self.N + other.N)
            rc = _lib.join_lib().slam_ekf_join(self._h, other._h, C.byref(first))
        check(rc)
        if merge_gate is None:
            return first.value
        cur = np.arange(1, self.N + 1, dtype=np.int64)
        while True:
            pairs, count = self.find_duplicates(float(merge_gate))
            if count == 0:
                break
            batch, busy = [], set()
            for a, b in pairs:
                if len(batch) == _lib.SLAM_MERGE_MAX:
                    break
                if int(a) in busy or int(b) in busy:
                    continue
                batch.append((int(a), int(b)))
                busy.update((int(a), int(b)))
            new_index = np.asarray(self.merge_landmarks(np.asarray(batch, dtype=np.int32), Rc), dtype=np.int64)
            cur = new_index[cur - 1]
        return first.value, cur.astype(np.int32)

    def align(self, ids, xy, apply=True):
        """Fit the rigid transform (no scale) that carries the means of the landmarks ``ids`` (1-based) onto the surveyed
        positions ``xy`` ([2, k] or [k, 2]; for two landmarks a 2 x 2 array is read as [2, k]: one point per column) in the
        least-squares sense (rigid_fit) and, unless ``apply`` is False, move
        the state into that frame (transform).  Only x is downloaded.  Returns ``(tx, ty, theta)``."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        x = np.asarray(self.download("x"), dtype=np.float64)
        f = 3 + 2 * (ids - 1)
        if ids.size and (ids.min() < 1 or ids.max() > self.N):
            raise ValueError("landmark id out of range")
        tx, ty, theta = rigid_fit(np.stack([x[f], x[f + 1]]), xy)
        if apply:
            self.transform(tx, ty, theta)
        return tx, ty, theta

    def observe(self, z, R, gate1, gate2, form="cholesky"):
        """associate -> update -> add_features (sim/ekfslam-sim.jl:114-120) in one library call with no host
        round trip between the gating and the update.  Returns the association vector
        (see associate_vector); the state afterwards equals the three calls in sequence."""
        zp = _obs(z)
        nz = zp.shape[0]
        assoc = np.zeros(nz, dtype=np.int32)
        if nz:
            r = _small(R)
            code = SLAM_FORM_JOSEPH if form == "joseph" else SLAM_FORM_CHOLESKY
            rc = lib.slam_ekf_observe(self._h, _ptr(zp), nz, _ptr(r), float(gate1), float(gate2), code, _ptr(assoc, C.c_int32))
            if rc == _lib.SLAM_E_CAPACITY and self.grow:
                # the association vector is complete and the update has been applied (slam_ekf_observe reports the capacity
                # behind the update's own status); only the new features are missing: grow, then append them
                new = np.ascontiguousarray(zp[assoc < 0])
                self._grow_for(self.N + new.shape[0])
                rc = lib.slam_ekf_augment(self._h, _ptr(new), new.shape[0], _ptr(r))
            check(rc)
        return assoc

    # -- compressed local-area updates (include/ext/slamhip_local.h) ---------------------------
    def landmarks_within(self, cx, cy, r):
        """The ids (1-based, ascending, int32) of the landmarks whose mean lies within ``r`` of (cx, cy): a host choice from the
        downloaded mean."""
        x = np.asarray(self.download("x"), dtype=np.float64)
        lm = x[3:].reshape(-1, 2)
        near = np.hypot(lm[:, 0] - float(cx), lm[:, 1] - float(cy)) <= float(r)
        return (np.flatnonzero(near) + 1).astype(np.int32)

    def local(self, ids, max_local=None):
        """A :class:`LocalArea` over the vehicle and the landmarks ``ids`` of this state, opened: a context manager that closes
        the area on a clean exit and aborts it on an exception.  While it is open this state must not be written."""
        return LocalArea(self, ids, max_local=max_local)

    # -- joint-compatibility data association (include/slamhip_jc.h) ---------------------------
    def _jc_handle(self):
        """The search workspace (slam_ekf_jc_create), made at the first joint call and destroyed by close()."""
        if getattr(self, "_jc", None) is None:
            jc = C.c_void_p()
            check(_lib.jc_lib().slam_ekf_jc_create(C.byref(jc), self._h))
            self._jc = jc
        return self._jc

    def associate_joint_vector(self, z, R, gate1, gate2, confidence=0.95, max_nodes=20000, chi2=None):
        """(assoc, info): the association vector of associate_vector (j >= 1 matched, 0 dropped, -1 new) from the
        joint-compatibility search (slam_ekf_associate_joint: at most 64 observations, each landmark used at most once, the stacked
        innovation of the result inside the chi-square gate of ``confidence``), and ``info``: pairings, d2, tests, exhausted,
        truncated, candidates, deepest.  ``chi2`` overrides the thresholds of chi2_table(nz, confidence).  The state is not changed."""
        zp = _obs(z)
        nz = zp.shape[0]
        assoc = np.zeros(nz, dtype=np.int32)
        info = np.zeros(8)
        table = np.ascontiguousarray(chi2_table(nz, confidence) if chi2 is None else np.asarray(chi2, dtype=np.float64))
        if table.size < nz:
            raise ValueError("chi2 needs one threshold per observation")
        r = _small(R)
        check(_lib.jc_lib().slam_ekf_associate_joint(self._jc_handle(), _ptr(zp) if nz else None, nz, _ptr(r), float(gate1),
                                                     float(gate2), _ptr(table) if nz else None, int(max_nodes),
                                                     _ptr(assoc, C.c_int32) if nz else None, _ptr(info)))
        d = dict(zip(JC_INFO_KEYS, (float(v) for v in info[:7])))
        for key in JC_INFO_KEYS:
            if key != "d2":
                d[key] = int(d[key])
        return assoc, d

    def associate_joint(self, z, R, gate1, gate2, confidence=0.95, max_nodes=20000):
        """(zf, idf, zn, info) in associate()'s shapes, from the joint-compatibility search (associate_joint_vector)."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc, info = self.associate_joint_vector(z, R, gate1, gate2, confidence, max_nodes)
        return z[:, assoc > 0], assoc[assoc > 0].astype(np.int64).reshape(1, -1), z[:, assoc < 0], info

    def joint_nis(self, z, idf, R):
        """d2 = v' inv(S_H) v of the hypothesis "observation i is landmark idf[i]" (1-based, distinct) under the JOINT innovation
        covariance H P H' + blockdiag(R) (slam_ekf_joint_nis).  NotPositiveDefinite if that matrix has a pivot that is not positive."""
        zp = _obs(z)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        r = _small(R)
        out = C.c_double()
        check(_lib.jc_lib().slam_ekf_joint_nis(self._jc_handle(), _ptr(zp), _ptr(ids, C.c_int32), int(ids.shape[0]), _ptr(r),
                                               C.byref(out)))
        return out.value

    def observe_joint(self, z, R, gate1, gate2, confidence=0.95, max_nodes=20000, form="cholesky"):
        """associate_joint -> update -> add_features.  Returns ``(assoc, info)``; the state afterwards equals the three calls made
        by hand."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc, info = self.associate_joint_vector(z, R, gate1, gate2, confidence, max_nodes)
        self.update(z[:, assoc > 0], R, assoc[assoc > 0], form=form)
        self.add_features(z[:, assoc < 0], R)
        return assoc, info

    def compute_association(self, z, R, idf):
        zz = _dbl(z, 2)
        r = _small(R)
        out = np.empty(2)
        check(lib.slam_ekf_nis(self._h, _ptr(zz), int(idf), _ptr(r), _ptr(out)))
        return float(out[0]), float(out[1])

    def predict_observation(self, idf):
        """(z (2,), H (2, n) dense with 5 non-zero columns) -- src/common.jl:139-165."""
        zp, Hv, Hf = np.empty(2), np.empty(6), np.empty(4)
        check(lib.slam_ekf_predict_observation(self._h, int(idf), _ptr(zp), _ptr(Hv), _ptr(Hf)))
        n = self.n
        H = np.zeros((2, n))
        H[:, 0:3] = Hv.reshape(3, 2).T
        f = 3 + 2 * (int(idf) - 1)
        H[:, f:f + 2] = Hf.reshape(2, 2).T
        return zp, H

    # -- stream / timing ----------------------------------------------------------------
    def set_async(self, flag=True):
        check(lib.slam_ekf_set_async(self._h, 1 if flag else 0))
        self._async = bool(flag)

    def sync(self):
        check(lib.slam_ekf_sync(self._h))

    def timing(self, enable=True, kernels=None):
        """Bracket kernel launches with HIP events; ``kernels``: names from ``_lib.KERNEL_IDS`` to restrict
        it to (each event pair costs ~10 us of stream time)."""
        mask = 1 if enable else 0
        if enable and kernels:
            mask = 0
            for name in kernels:
                mask |= 2 << _lib.KERNEL_IDS[name]
        check(lib.slam_ekf_timing(self._h, mask))

    def state_written(self):
        """Tell the library that landmark entries of x / P were written through the raw device views
        (:meth:`device_ptrs`): the gating's side array, variance bound and grid are refreshed on the device."""
        check(lib.slam_ekf_state_written(self._h))

    def copy_floor(self, reps=10):
        """Bare read + rewrite of the stored covariance tiles (the memory side of the down-date, nothing else), timed on
        this handle's own matrix: ``(milliseconds per pass, launch form)``.  The state is unchanged."""
        out = (C.c_double * 2)()
        check(lib.slam_ekf_copy_floor(self._h, int(reps), out))
        return float(out[0]), ("one workgroup per tile", "persistent grid")[int(out[1])]

    def debug_stamps(self, enable=True):
        """Diagnostics: 100 MHz wall-clock stamps of the factorisation kernel's phases (last update): [0..7] the workgroup that
        factors S, [8..15] the first of the workgroups that form W1 in the same launch."""
        out = (C.c_uint64 * 16)()
        check(lib.slam_ekf_debug_stamps(self._h, 1 if enable else 0, out))
        return [int(v) for v in out]

    def timing_reset(self):
        check(lib.slam_ekf_timing_reset(self._h))

    def timing_read(self):
        """{kernel: (total_ms, launches)} accumulated since the last reset."""
        out = {}
        for name, kid in _lib.KERNEL_IDS.items():
            ms, cnt = C.c_double(), C.c_int64()
            check(lib.slam_ekf_timing_read(self._h, kid, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def timing_min(self, kernel):
        """Milliseconds of the fastest bracketed launch of `kernel` since the last reset (0.0: none)."""
        ms = C.c_double()
        check(lib.slam_ekf_timing_min(self._h, _lib.KERNEL_IDS[kernel], C.byref(ms)))
        return ms.value

    def timing_stats(self, kernel):
        """(launches, mean_ms, stdev_ms, min_ms) of the bracketed launches of `kernel` since the last reset."""
        out = np.zeros(4)
        check(lib.slam_ekf_timing_stats(self._h, _lib.KERNEL_IDS[kernel], _ptr(out)))
        return int(out[0]), float(out[1]), float(out[2]), float(out[3])


# ---- the reference's function surface ---------------------------------------------------

class CovarianceFactor:
    """The Cholesky factor L of an EKF state's covariance, on the device (include/ext/slamhip_factor.h): L L' = cov, in the
    state's own tile-major layout, with the snapshot of x that ``compute`` took.  ``dtype`` is the arithmetic and storage type of
    L; ``max_landmarks`` the capacity; ``panel_tiles`` 1, 2, 4 or 0 (the default for the dtype)."""

    def __init__(self, dtype="f64", max_landmarks=64, device=0, panel_tiles=0):
        code, npdt = _DTYPES[dtype]
        self.np_dtype = npdt
        self.max_landmarks = int(max_landmarks)
        self.device = int(device)
        self._h = C.c_void_p()
        self._flib = _lib.factor_lib()
        check(self._flib.slam_ekf_factor_create(C.byref(self._h), code, self.max_landmarks, self.device, int(panel_tiles)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._flib.slam_ekf_factor_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute(self, state):
        """Factor ``state``'s covariance into this object; NotPositiveDefinite when a pivot fails (``info`` then names it and
        every read-out is refused until a compute succeeds).  Synchronises."""
        if not isinstance(state, EKFSlamState):
            raise TypeError("compute needs an EKFSlamState")
        info = np.zeros(8)
        check(self._flib.slam_ekf_factor_compute(self._h, state._h, _ptr(info)))
        return info

    @property
    def info(self):
        """[n, status, first failing index or -1, failing pivot, min l_ii, max l_ii, log det, panel_tiles] of the last compute."""
        info = np.zeros(8)
        check(self._flib.slam_ekf_factor_info(self._h, _ptr(info)))
        return info

    n = property(lambda self: int(self.info[0]))
    min_pivot = property(lambda self: float(self.info[4]), doc="the smallest l_ii")
    max_pivot = property(lambda self: float(self.info[5]), doc="the largest l_ii")
    logdet = property(lambda self: float(self.info[6]), doc="log det cov = 2 sum log l_ii")
    panel_tiles = property(lambda self: int(self.info[7]))

    def L(self, r0=0, c0=0, nr=None, nc=None):
        """L[r0 : r0 + nr, c0 : c0 + nc] (0-based; default: to the end), zeros above the diagonal, in the factor's dtype."""
        n = self.n
        nr = n - int(r0) if nr is None else int(nr)
        nc = n - int(c0) if nc is None else int(nc)
        out = np.empty((nr, nc), dtype=self.np_dtype, order="F")
        check(self._flib.slam_ekf_factor_get(self._h, int(r0), int(c0), nr, nc, out.ctypes.data, max(nr, 1)))
        return out

    def mean(self):
        """x as ``compute`` found it, as float64."""
        out = np.empty(max(self.n, 1))
        check(self._flib.slam_ekf_factor_mean(self._h, _ptr(out)))
        return out[:self.n]

    def _rhs(self, A):
        A = np.asarray(A, dtype=np.float64)
        vec = A.ndim == 1
        A = np.asfortranarray(A.reshape(-1, 1) if vec else A)
        if A.ndim != 2 or A.shape[0] != self.n:
            raise ValueError(f"expected {self.n} rows")
        return A, vec

    def whiten(self, E, return_d2=False):
        """``L^-1 E`` for an n-vector or an n x r matrix of error vectors (any r: in slices of 64 columns), fp64 arithmetic; with
        ``return_d2`` also the squared norms of the result's columns."""
        E, vec = self._rhs(E)
        n, r = E.shape
        Y = np.empty((n, r), order="F")
        d2 = np.empty(r)
        for c in range(0, r, _lib.SLAM_FACTOR_MAXRHS):
            w = min(_lib.SLAM_FACTOR_MAXRHS, r - c)
            Bc, Yc, dc = np.asfortranarray(E[:, c:c + w]), np.empty((n, w), order="F"), np.empty(w)
            check(self._flib.slam_ekf_factor_solve(self._h, _ptr(Bc), w, n, _ptr(Yc), _ptr(dc)))
            Y[:, c:c + w], d2[c:c + w] = Yc, dc
        Y = Y[:, 0] if vec else Y
        return (Y, (float(d2[0]) if vec else d2)) if return_d2 else Y

    def colour(self, Z):
        """``L Z`` for an n-vector or an n x r matrix (any r: in slices of 64 columns), fp64 arithmetic."""
        Z, vec = self._rhs(Z)
        n, r = Z.shape
        out = np.empty((n, r), order="F")
        for c in range(0, r, _lib.SLAM_FACTOR_MAXRHS):
            w = min(_lib.SLAM_FACTOR_MAXRHS, r - c)
            Zc, Oc = np.asfortranarray(Z[:, c:c + w]), np.empty((n, w), order="F")
            check(self._flib.slam_ekf_factor_multiply(self._h, _ptr(Zc), w, n, _ptr(Oc)))
            out[:, c:c + w] = Oc
        return out[:, 0] if vec else out

    def nees(self, x_true):
        """e' cov^-1 e with e = mean - x_true, the heading difference wrapped by mpi_to_pi."""
        e = self.mean() - _dbl(x_true, self.n)
        e[2] = mpi_to_pi(e[2])
        return self.whiten(e, return_d2=True)[1]

    def sample(self, count, rng):
        """``count`` joint samples of the state as the columns of an n x count array: mean + L Z with Z = rng.standard_normal((n,
        count)) from the caller's ``numpy.random.Generator``, so the draw is the caller's to reproduce."""
        Z = rng.standard_normal((self.n, int(count)))
        return self.mean()[:, None] + self.colour(Z)


def _wide_batches(fn, h, f, zf, R, idf):
    """One call of libslamhip_wide.so per 64 observations; f: the first-estimates object's handle, or None (the stored state)."""
    zp = _obs(zf)
    ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
    if ids.shape[0] != zp.shape[0]:
        raise ValueError("idf and z disagree on the number of observations")
    if zp.shape[0] == 0:
        return None
    r = _small(R)
    B = _lib.SLAM_WIDE_MAXOBS
    outs = np.zeros(((zp.shape[0] + B - 1) // B, 4))
    for b, s in enumerate(range(0, zp.shape[0], B)):
        zb, ib = np.ascontiguousarray(zp[s:s + B]), np.ascontiguousarray(ids[s:s + B])
        check(fn(h, f, _ptr(zb), _ptr(ib, C.c_int32), zb.shape[0], _ptr(r), _ptr(outs[b])))
    return outs


class FirstEstimates:
    """The linearisation points of a first-estimates Jacobian (FEJ) filter over ``state`` (include/ext/slamhip_fej.h), on the device
    beside the state: ``lin``, the pose the vehicle's Jacobians are evaluated at (the predicted pose, never an updated one), and
    ``first``, every landmark's first estimate.  :meth:`predict`, :meth:`update` and :meth:`add_features` are the state's own with
    the Jacobians evaluated there; no formula changes.  While the object is in use, move the state through it: a call of the
    state's own predict / update leaves ``lin`` behind (:meth:`reset` re-anchors it), and after the map was renumbered
    (remove_landmarks, merge_landmarks, select_from, join) the object refuses to work until :meth:`remap` was told how.  With
    ``grow=True`` on the state the object follows it into a larger handle."""

    def __init__(self, state):
        if not isinstance(state, EKFSlamState):
            raise TypeError("FirstEstimates needs an EKFSlamState")
        self._lib = _lib.fej_lib()
        self.state = state
        self._f = C.c_void_p()
        self._attach()
        if getattr(state, "_fej", None) is None:
            state._fej = []
        state._fej.append(self)

    def _attach(self):
        check(self._lib.slam_ekf_fej_create(C.byref(self._f), self.state._h))

    def _release(self):
        if getattr(self, "_f", None) is not None and self._f:
            self._lib.slam_ekf_fej_destroy(self._f)
            self._f = C.c_void_p()

    # -- lifetime ----------------------------------------------------------------
    def close(self):
        self._release()
        held = getattr(getattr(self, "state", None), "_fej", None)
        if held and self in held:
            held.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the linearisation points ---------------------------------------------------
    def get(self):
        """``(lin [3], first [2 count], count)`` as float64 from the device (slam_ekf_fej_get); first holds (x, y) pairs in landmark
        order, like x[3:]."""
        count = C.c_int32()
        check(self._lib.slam_ekf_fej_get(self._f, None, None, C.byref(count)))
        lin, first = np.zeros(3), np.zeros(2 * count.value)
        check(self._lib.slam_ekf_fej_get(self._f, _ptr(lin), _ptr(first) if count.value else None, None))
        return lin, first, count.value

    def set(self, lin=None, first=None):
        """Write ``lin`` (3 values) and / or ``first`` (2 state.N values) to the device (slam_ekf_fej_set): a checkpoint restored,
        or designed linearisation points.  With ``first`` the object's count becomes the state's."""
        a = None if lin is None else _dbl(lin, 3)
        b = None if first is None else _dbl(np.asarray(first, dtype=np.float64).reshape(-1), 2 * self.state.N)
        if b is not None and not b.size:
            b = np.zeros(1)                                               # an empty map: a pointer that is not null, nothing is read
        check(self._lib.slam_ekf_fej_set(self._f, _ptr(a) if a is not None else None, _ptr(b) if b is not None else None))

    def reset(self, ids=None, pose=False):
        """``first`` of the landmarks ``ids`` (1-based; None: all) becomes their current mean, and with ``pose`` ``lin`` becomes
        the current pose (slam_ekf_fej_reset): the linearisation points re-anchored, e.g. after a loop was closed."""
        if ids is None:
            check(self._lib.slam_ekf_fej_reset(self._f, None, -1, 1 if pose else 0))
            return
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        check(self._lib.slam_ekf_fej_reset(self._f, _ptr(ids, C.c_int32) if ids.size else None, int(ids.size), 1 if pose else 0))

    def remap(self, ids):
        """After the map was renumbered outside the object: new landmark j takes the first estimate of old landmark ``ids[j - 1]``
        (1-based), or its current mean where ``ids[j - 1]`` is 0 (slam_ekf_fej_remap).  One entry per landmark of the state.  For
        ``new_index = state.remove_landmarks(gone)`` the map is ``np.flatnonzero(new_index) + 1``."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        check(self._lib.slam_ekf_fej_remap(self._f, _ptr(ids, C.c_int32) if ids.size else None, int(ids.size)))

    def transform(self, tx, ty, theta):
        """``lin`` and every first estimate expressed in another frame (slam_ekf_fej_transform): call it beside
        ``state.transform(tx, ty, theta)``, which this does NOT do."""
        check(self._lib.slam_ekf_fej_transform(self._f, float(tx), float(ty), float(theta)))

    # -- the steps --------------------------------------------------------------------
    def predict(self, v, g, wheelbase, Q, dt):
        """``state.predict`` with the vehicle Jacobian taken between ``lin`` and the new pose; ``lin`` becomes the new pose.
        Enqueued."""
        q = _small(Q)
        check(self._lib.slam_ekf_fej_predict(self._f, float(v), float(g), float(wheelbase), _ptr(q), float(dt)))

    def update(self, zf, R, idf):
        """``state.update`` (Cholesky form) with the residuals at the current mean and the Jacobians at ``lin`` and the first
        estimates (slam_ekf_fej_update).  More than 8 observations go as consecutive batches of 8 in the order given: the Jacobians do
        not move between the batches, the residuals of a batch are taken at the mean the batch before left.  Returns one row
        ``[v' inv(S) v, log det S, smallest pivot, -1]`` per batch (None without an observation); raises NotPositiveDefinite with the
        state unchanged by the failing batch."""
        zp = _obs(zf)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        if zp.shape[0] == 0:
            return None
        r = _small(R)
        B = _lib.SLAM_FEJ_MAXOBS
        outs = np.zeros(((zp.shape[0] + B - 1) // B, 4))
        for b, s in enumerate(range(0, zp.shape[0], B)):
            zb, ib = np.ascontiguousarray(zp[s:s + B]), np.ascontiguousarray(ids[s:s + B])
            check(self._lib.slam_ekf_fej_update(self._f, _ptr(zb), _ptr(ib, C.c_int32), zb.shape[0], _ptr(r), _ptr(outs[b])))
        return outs

    def _wide(self, fn, zf, R, idf):
        return _wide_batches(fn, self.state._h, self._f, zf, R, idf)

    def update_joint(self, zf, R, idf):
        """:meth:`update` of up to 64 observations JOINTLY, in one pass over the covariance (slam_ekf_wide_update): every residual
        is taken at the mean before the call, every Jacobian at ``lin`` and the first estimates.  This is the filter's own update
        of the whole batch; ``update`` with more than 8 observations is a chain of 8-observation updates and a different
        estimator.  More than 64 go as consecutive batches of 64.  Returns one row ``[v' inv(S) v, log det S, smallest pivot, -1]``
        per batch (None without an observation); raises NotPositiveDefinite with the state unchanged by the failing batch."""
        return self._wide(_lib.wide_lib().slam_ekf_wide_update, zf, R, idf)

    def joint_nis(self, zf, R, idf):
        """What :meth:`update_joint` would return, with the state only read (slam_ekf_wide_nis): the joint chi-square gate of a
        whole batch at the linearisation points before it is committed.  At most 64 observations: a second batch would have to
        start from the state the first one leaves."""
        if _obs(zf).shape[0] > _lib.SLAM_WIDE_MAXOBS:
            raise ValueError("joint_nis takes at most 64 observations")
        return self._wide(_lib.wide_lib().slam_ekf_wide_nis, zf, R, idf)

    def add_features(self, zn, R):
        """``state.add_features`` with the new landmarks' Jacobians taken between ``lin`` and their new means, which become their
        first estimates (slam_ekf_fej_augment).  With ``grow=True`` on the state both move into a larger handle when needed."""
        zp = _obs(zn)
        if zp.shape[0] == 0:
            return
        r = _small(R)
        rc = self._lib.slam_ekf_fej_augment(self._f, _ptr(zp), zp.shape[0], _ptr(r))
        if rc == _lib.SLAM_E_CAPACITY and self.state.grow:               # decided before anything was enqueued: grow, then again
            self.state._grow_for(self.state.N + zp.shape[0])
            rc = self._lib.slam_ekf_fej_augment(self._f, _ptr(zp), zp.shape[0], _ptr(r))
        check(rc)

    def observe(self, z, R, gate1, gate2, joint=False):
        """The product's association at the current estimates (``state.associate_vector``), then this update -- with ``joint``
        :meth:`update_joint` -- and this add_features.  Returns the association vector."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc = self.state.associate_vector(z, R, gate1, gate2)
        (self.update_joint if joint else self.update)(z[:, assoc > 0], R, assoc[assoc > 0])
        self.add_features(z[:, assoc < 0], R)
        return assoc


class LocalArea:
    """The compressed EKF over a local area (include/ext/slamhip_local.h): predict, update and add_features run on a small state
    -- the vehicle plus the landmarks ``ids`` of ``state`` (local landmark j is ids[j - 1]; landmarks added here follow) -- and
    :meth:`close` brings the rest of the map up to date in one pass.  Up to rounding the result is the full filter's.  While the
    area is open ``state`` must not be written, and observations of landmarks outside the area cannot be used.  ``max_local``: the
    local landmark capacity (default len(ids) + 64, at most 1024).  ``area.state`` is the local state as an EKFSlamState whose
    handle this object owns: read it freely (download, associate, ellipses), write it only through this object."""

    def __init__(self, state, ids=None, max_local=None):
        if not isinstance(state, EKFSlamState):
            raise TypeError("LocalArea needs an EKFSlamState")
        self._lib = _lib.local_lib()
        self.parent = state
        self._L = C.c_void_p()
        ids_arr = np.zeros(0, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32).reshape(-1)
        if max_local is None:
            max_local = min(_lib.SLAM_LOCAL_MAXLM, max(1, ids_arr.size + 64))
        self.max_local = int(max_local)
        check(self._lib.slam_ekf_local_create(C.byref(self._L), state._h, self.max_local))
        h = C.c_void_p()
        check(self._lib.slam_ekf_local_state(self._L, C.byref(h)))
        st = EKFSlamState.__new__(EKFSlamState)
        st.grow = False
        st._gate_mode = None
        st._async = None
        st.np_dtype = state.np_dtype
        st.max_landmarks = self.max_local
        st.device = state.device
        st._h = h
        st._borrowed = True
        self.state = st
        if ids is not None:
            try:
                self.open(ids_arr)
            except Exception:
                self.destroy()
                raise

    # -- lifetime ----------------------------------------------------------------
    def destroy(self):
        """Release the local handle and the accumulators; an open area is discarded."""
        if getattr(self, "state", None) is not None:
            self.state.close()
        if getattr(self, "_L", None) is not None and self._L:
            self._lib.slam_ekf_local_destroy(self._L)
            self._L = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.is_open:
            if exc_type is None:
                self.close()
            else:
                self.abort()
        return False

    # -- the area ------------------------------------------------------------------
    def open(self, ids):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        check(self._lib.slam_ekf_local_open(self._L, _ptr(ids, C.c_int32) if ids.size else None, int(ids.size)))
        self.ids = ids.copy()

    def info(self):
        out = (C.c_int64 * 8)()
        check(self._lib.slam_ekf_local_info(self._L, out))
        keys = ("open", "n0", "n_a", "added", "steps", "N_open", "max_local")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    @property
    def is_open(self):
        return bool(self._L) and bool(self.info()["open"])

    def global_ids(self):
        """Global id of every local landmark, in local order: ``ids``, then the landmarks added here (N at open + 1 ...)."""
        i = self.info()
        return np.concatenate([self.ids, i["N_open"] + 1 + np.arange(i["added"], dtype=np.int32)]).astype(np.int32)

    def accumulators(self):
        """(phi n_a x n0, psi n0 x n0, theta n0) as float64 arrays (slam_ekf_local_get): for tests and diagnostics."""
        i = self.info()
        phi = np.zeros((i["n_a"], i["n0"]))
        psi = np.zeros((i["n0"], i["n0"]))
        theta = np.zeros(i["n0"])
        check(self._lib.slam_ekf_local_get(self._L, _ptr(phi), _ptr(psi), _ptr(theta)))
        return phi, psi, theta

    def close(self):
        """Bring the global state up to date (slam_ekf_local_close); returns the global id of the first landmark appended."""
        first = C.c_int()
        check(self._lib.slam_ekf_local_close(self._L, C.byref(first)))
        return first.value

    def abort(self):
        """Discard the area: the global state is untouched."""
        check(self._lib.slam_ekf_local_abort(self._L))

    # -- the steps, on the local state ----------------------------------------------
    def predict(self, v, g, wheelbase, Q, dt):
        q = _small(Q)
        check(self._lib.slam_ekf_local_predict(self._L, float(v), float(g), float(wheelbase), _ptr(q), float(dt)))

    def update(self, zf, R, idf, form="cholesky"):
        """``idf``: LOCAL landmark ids.  Cholesky form only."""
        zp = _obs(zf)
        ids = np.ascontiguousarray(np.asarray(idf, dtype=np.int32).reshape(-1))
        if ids.shape[0] != zp.shape[0]:
            raise ValueError("idf and z disagree on the number of observations")
        r = _small(R)
        code = SLAM_FORM_JOSEPH if form == "joseph" else SLAM_FORM_CHOLESKY
        check(self._lib.slam_ekf_local_update(self._L, _ptr(zp), _ptr(ids, C.c_int32), zp.shape[0], _ptr(r), code))

    def add_features(self, zn, R):
        zp = _obs(zn)
        if zp.shape[0] == 0:
            return
        r = _small(R)
        check(self._lib.slam_ekf_local_augment(self._L, _ptr(zp), zp.shape[0], _ptr(r)))

    def associate(self, z, R, gate1, gate2):
        """(zf, idf, zn) against the LOCAL map: idf are local ids."""
        return self.state.associate(z, R, gate1, gate2)

    def observe(self, z, R, gate1, gate2):
        """associate on the local state, then update, then add_features; returns the association vector (local ids)."""
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        assoc = self.state.associate_vector(z, R, gate1, gate2)
        self.update(z[:, assoc > 0], R, assoc[assoc > 0])
        self.add_features(z[:, assoc < 0], R)
        return assoc


def _state_of(ref_or_state):
    if isinstance(ref_or_state, EKFSlamState):
        return ref_or_state
    if isinstance(ref_or_state, DeviceRef):
        return ref_or_state.state
    return None


def predict(state: EKFSlamState, vehicle, Q, dt):
    """predict(state, vehicle, Q, dt) -> (x, P)   src/ekf.jl:8-43.
    ``vehicle`` needs ``measured_speed``, ``measured_gamma``, ``wheelbase`` (:14-16)."""
    state.predict(vehicle.measured_speed, vehicle.measured_gamma, vehicle.wheelbase, Q, dt)
    return state.x, state.cov


def update(state: EKFSlamState, z, R, idf):
    """update(state, z, R, idf) -> (x, P)   src/ekf.jl:46-77 (here: in place on the device)."""
    state.update(z, R, idf)
    return state.x, state.cov


def add_features(state: EKFSlamState, z, R):
    """add_features(state, z, R) -> (x, P)   src/ekf.jl:84-122."""
    state.add_features(z, R)
    return state.x, state.cov


def associate(state: SlamState, z, R, gate1, gate2):
    """associate(state, z, R, gate1, gate2) -> (zf, idf, zn)   src/data-association.jl:1-51."""
    return state.associate(z, R, gate1, gate2)


def observe(state: EKFSlamState, z, R, gate1, gate2, form="cholesky"):
    """associate + update + add_features (sim/ekfslam-sim.jl:114-120) in one call -> association vector."""
    return _state_of(state).observe(z, R, gate1, gate2, form=form)


def associate_joint(state: EKFSlamState, z, R, gate1, gate2, confidence=0.95, max_nodes=20000):
    """Joint-compatibility association -> (zf, idf, zn, info) (see EKFSlamState.associate_joint)."""
    return _state_of(state).associate_joint(z, R, gate1, gate2, confidence, max_nodes)


def observe_joint(state: EKFSlamState, z, R, gate1, gate2, confidence=0.95, max_nodes=20000, form="cholesky"):
    """associate_joint + update + add_features -> (association vector, info)."""
    return _state_of(state).observe_joint(z, R, gate1, gate2, confidence, max_nodes, form=form)


def _temp_state(x, P=None):
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if P is None:
        P = np.zeros((n, n))
    return EKFSlamState(x, P, dtype="f64", max_landmarks=max(1, (n - 3) // 2))


def compute_association(x, P, z, R, idf):
    """compute_association(x, P, z, R, idf) -> (nis, nd)   src/data-association.jl:53-63.
    ``x`` / ``P`` may be a state's references (no transfer) or host arrays (uploaded to a
    temporary device state)."""
    st = _state_of(x)
    if st is not None:
        return st.compute_association(z, R, idf)
    tmp = _temp_state(x, P)
    try:
        return tmp.compute_association(z, R, idf)
    finally:
        tmp.close()


def predict_observation(x, idf):
    """predict_observation(x, idf) -> (z, H)   src/common.jl:139-165."""
    st = _state_of(x)
    if st is not None:
        return st.predict_observation(idf)
    tmp = _temp_state(x)
    try:
        return tmp.predict_observation(idf)
    finally:
        tmp.close()


# in-place names of BASELINE.json's north star (Julia: ekf_predict!, ekf_update!, augment!)
def ekf_predict_(state, v, g, wheelbase, Q, dt):
    state.predict(v, g, wheelbase, Q, dt)
    return state


def ekf_update_(state, z, R, idf, form="cholesky"):
    state.update(z, R, idf, form=form)
    return state


def augment_(state, z, R):
    state.add_features(z, R)
    return state


# map management: no counterpart in the reference (its map only grows)
def remove_features(state: EKFSlamState, ids):
    """Remove the landmarks ``ids`` (1-based) from the map -> ``new_index`` (see EKFSlamState.remove_landmarks)."""
    return _state_of(state).remove_landmarks(ids)


def remove_features_(state, ids):
    """In-place name (Julia: ``remove_features!``); returns the index map as well."""
    return _state_of(state).remove_landmarks(ids)


def transform_features(state: EKFSlamState, tx, ty, theta):
    """Express the state in another frame -> (x, P) (see EKFSlamState.transform)."""
    st = _state_of(state)
    st.transform(tx, ty, theta)
    return st.x, st.cov


def transform_features_(state, tx, ty, theta):
    """In-place name (Julia: ``transform!``); returns the state."""
    st = _state_of(state)
    st.transform(tx, ty, theta)
    return st


def copy_state(state: EKFSlamState, max_landmarks=None):
    """A copy of the state on the device -> a new EKFSlamState (see EKFSlamState.copy)."""
    return _state_of(state).copy(max_landmarks)


def select_features(state: EKFSlamState, ids, max_landmarks=None):
    """The sub-map ``ids`` with its marginal covariance -> a new EKFSlamState (see EKFSlamState.select)."""
    return _state_of(state).select(ids, max_landmarks)


def find_duplicates(state: EKFSlamState, gate, cap=1024):
    """Duplicate landmark pairs -> ``(pairs, count)`` (see EKFSlamState.find_duplicates)."""
    return _state_of(state).find_duplicates(gate, cap)


def merge_features(state: EKFSlamState, pairs, Rc=None):
    """Merge the landmarks of every pair -> ``new_index`` (see EKFSlamState.merge_landmarks)."""
    return _state_of(state).merge_landmarks(pairs, Rc)


def merge_features_(state, pairs, Rc=None):
    """In-place name (Julia: ``merge_landmarks!``); returns the index map as well."""
    return _state_of(state).merge_landmarks(pairs, Rc)
