"""ctypes binding of libslamhip.so (include/slamhip.h).

There is NO fallback: if the shared library is missing or cannot be loaded the
import fails loudly, and if no HIP device is usable ``slam_ekf_create`` returns
SLAM_E_HIP which is raised as :class:`SlamHipError`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libslamhip.so")
# measurement tooling only (tools/gpu_exp.sh): the experiments build of the SAME sources, `make -C csrc exp`
if os.environ.get("SLAMHIP_LIBRARY"):
    LIB_PATH = os.path.abspath(os.environ["SLAMHIP_LIBRARY"])

SLAM_OK = 0
SLAM_E_BADARG = -1
SLAM_E_CAPACITY = -2
SLAM_E_NOTPD = -3
SLAM_E_HIP = -4
SLAM_E_NOMEM = -5
SLAM_PF_HALTED = 1
SLAM_PF_PEER_BLOB_BYTES = 4096
SLAM_F32, SLAM_F64 = 0, 1
SLAM_FORM_CHOLESKY, SLAM_FORM_JOSEPH = 0, 1
SLAM_MERGE_MAX = 8
KERNEL_IDS = {"gate": 0, "gate_final": 1, "predict": 2, "augment": 3, "pht": 4, "factor": 5, "w1": 6, "syrk": 7}

_ERRNAMES = {SLAM_E_BADARG: "SLAM_E_BADARG", SLAM_E_CAPACITY: "SLAM_E_CAPACITY", SLAM_E_NOTPD: "SLAM_E_NOTPD",
             SLAM_E_HIP: "SLAM_E_HIP", SLAM_E_NOMEM: "SLAM_E_NOMEM"}


class SlamHipError(RuntimeError):
    """A non-zero status from libslamhip (Julia wrapper: ``error(...)``)."""

    def __init__(self, code, message):
        super().__init__(f"{_ERRNAMES.get(code, code)}: {message}")
        self.code = code


class NotPositiveDefinite(SlamHipError):
    """SLAM_E_NOTPD -- the reference's ``chol`` would throw PosDefException (src/ekf.jl:70)."""


def _load():
    # libslamhip.so itself does not depend on torch.  But when torch is used in the same process (the
    # FastSLAM collectives, bench.py) both must share ONE HIP runtime: torch's wheel bundles its own
    # libamdhip64, and if the system runtime gets loaded first torch later reports "No HIP GPUs are
    # available".  So torch, if installed, is imported before the library is opened.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        return C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e


lib = _load()

_h = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

#: every symbol include/slamhip.h and include/slamhip_diag.h declare: name -> (restype, argtypes)
SIGNATURES = {
    "slam_last_error": (C.c_char_p, []),
    "slam_device_count": (C.c_int, []),
    "slam_ekf_create": (C.c_int, [C.POINTER(_h), C.c_int, C.c_int, C.c_int]),
    "slam_ekf_destroy": (C.c_int, [_h]),
    "slam_ekf_set_state": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "slam_ekf_set_state_device": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "slam_ekf_get_state": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "slam_ekf_get_block": (C.c_int, [_h, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "slam_ekf_get_diag": (C.c_int, [_h, C.c_void_p]),
    "slam_ekf_get_landmark_blocks": (C.c_int, [_h, C.c_void_p]),
    "slam_ekf_set_gate_mode": (C.c_int, [_h, C.c_int]),
    "slam_ekf_gate_info": (C.c_int, [_h, C.POINTER(C.c_int64)]),
    "slam_ekf_get_pose": (C.c_int, [_h, _dp]),
    "slam_ekf_num_landmarks": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_ekf_dtype": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_ekf_device_ptrs": (C.c_int, [_h, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                       C.POINTER(C.c_void_p)]),
    "slam_ekf_predict": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double]),
    "slam_ekf_associate": (C.c_int, [_h, _dp, C.c_int, _dp, C.c_double, C.c_double, _ip]),
    "slam_ekf_nis": (C.c_int, [_h, _dp, C.c_int, _dp, _dp]),
    "slam_ekf_predict_observation": (C.c_int, [_h, C.c_int, _dp, _dp, _dp]),
    "slam_ekf_update": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, C.c_int]),
    "slam_ekf_augment": (C.c_int, [_h, _dp, C.c_int, _dp]),
    "slam_ekf_ellipses": (C.c_int, [_h, _dp, _dp]),
    "slam_ekf_observe": (C.c_int, [_h, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _ip]),
    "slam_ekf_set_async": (C.c_int, [_h, C.c_int]),
    "slam_ekf_sync": (C.c_int, [_h]),
    "slam_ekf_timing": (C.c_int, [_h, C.c_int]),
    "slam_ekf_timing_read": (C.c_int, [_h, C.c_int, _dp, C.POINTER(C.c_int64)]),
    "slam_ekf_timing_reset": (C.c_int, [_h]),
    "slam_ekf_timing_min": (C.c_int, [_h, C.c_int, _dp]),
    "slam_ekf_timing_stats": (C.c_int, [_h, C.c_int, _dp]),
    "slam_ekf_debug_stamps": (C.c_int, [_h, C.c_int, C.POINTER(C.c_uint64)]),
    "slam_ekf_state_written": (C.c_int, [_h]),
    "slam_ekf_copy_floor": (C.c_int, [_h, C.c_int, _dp]),
    "slam_ekf_remove_landmarks": (C.c_int, [_h, _ip, C.c_int, _ip]),
    "slam_ekf_find_duplicates": (C.c_int, [_h, C.c_double, _ip, C.c_int, C.POINTER(C.c_int)]),
    "slam_ekf_merge_landmarks": (C.c_int, [_h, _ip, C.c_int, _dp, _ip]),
    "slam_pf_create": (C.c_int, [C.POINTER(_h), C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint64]),
    "slam_pf_destroy": (C.c_int, [_h]),
    "slam_pf_set_pose": (C.c_int, [_h, _dp]),
    "slam_pf_init_landmarks": (C.c_int, [_h, _dp, C.c_int, C.c_double, C.c_double]),
    "slam_pf_predict": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double]),
    "slam_pf_update_known": (C.c_int, [_h, _dp, _ip, C.c_int, _dp]),
    "slam_pf_clear_landmarks": (C.c_int, [_h]),
    "slam_pf_update_unknown": (C.c_int, [_h, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_void_p]),
    "slam_pf_step": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, _ip, C.c_int, _dp, _dp]),
    "slam_pf_step_proposal": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, _ip, C.c_int, _dp, _dp]),
    "slam_pf_step_normalized": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, _ip, C.c_int, _dp,
                                          _dp]),
    "slam_pf_weight_stats": (C.c_int, [_h, _dp]),
    "slam_pf_normalize": (C.c_int, [_h, C.c_double, C.c_double]),
    "slam_pf_copy_logw": (C.c_int, [_h, C.c_void_p]),
    "slam_pf_resample_local": (C.c_int, [_h, C.c_double, C.c_double]),
    "slam_pf_ancestors_all": (C.c_int, [_h, C.c_void_p, C.c_double, C.c_double, C.c_void_p]),
    "slam_pf_ancestors": (C.c_int, [_h, C.c_void_p, C.c_double, C.c_double, C.c_void_p]),
    "slam_pf_record_rows": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_pf_pack": (C.c_int, [_h, C.c_void_p, C.c_int, C.c_void_p]),
    "slam_pf_resample_apply": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "slam_pf_mean_pose_sums": (C.c_int, [_h, _dp]),
    "slam_pf_download": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_void_p]),
    "slam_pf_sync": (C.c_int, [_h]),
    "slam_pf_stream": (C.c_int, [_h, C.POINTER(C.c_void_p)]),
    "slam_pf_step_auto": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, _ip, C.c_int, _dp, C.c_double,
                                    C.c_int, C.c_int]),
    "slam_pf_step_auto_batch": (C.c_int, [_h, C.c_int, _dp, C.c_double, _dp, C.c_double, _dp, _ip, _ip, C.c_int, _dp, C.c_double,
                                          _ip, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "slam_pf_flush": (C.c_int, [_h, _dp]),
    "slam_pf_halt_info": (C.c_int, [_h, _dp]),
    "slam_pf_resume": (C.c_int, [_h, C.c_int64]),
    "slam_pf_resample_count": (C.c_int, [_h, C.POINTER(C.c_int64)]),
    "slam_pf_set_resample_count": (C.c_int, [_h, C.c_int64]),
    "slam_pf_attach_exchange": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "slam_pf_export_peer": (C.c_int, [_h, C.c_void_p]),
    "slam_pf_attach_peers": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p]),
    "slam_pf_detach_peers": (C.c_int, [_h]),
    "slam_pf_peer_selftest": (C.c_int, [_h, C.c_int]),
    "slam_pf_comm_info": (C.c_int, [_h, C.POINTER(C.c_int64)]),
    "slam_pf_debug_stamps": (C.c_int, [_h, C.POINTER(C.c_uint64)]),
    "slam_pf_resample": (C.c_int, [_h, C.c_double, C.POINTER(C.c_int)]),
    "slam_pf_get_mean_pose": (C.c_int, [_h, _dp]),
    "slam_pf_get_weights": (C.c_int, [_h, _dp]),
    "slam_pf_map_sums": (C.c_int, [_h, _ip, C.c_int, _dp]),
    "slam_pf_get_map": (C.c_int, [_h, _ip, C.c_int, _dp]),
    "slam_pf_get_particle": (C.c_int, [_h, C.c_int64, C.POINTER(C.c_int64), _dp, _dp, _dp]),
    "slam_pf_step_unknown": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, C.c_int, _dp, C.c_double,
                                       C.c_double, C.c_void_p, _dp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)          # AttributeError here = the library lacks a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


# ---- the side libraries -----------------------------------------------------------------------------------------------------
# libslamhip.so exports exactly what its two headers declare; every later feature lives beside it in a side library
# libslamhip_<name>.so, which links against libslamhip.so (run path $ORIGIN), works on its handles and exports what its header
# declares: include/slamhip_<name>.h for a companion, include/ext/slamhip_<name>.h for an extension (ext=True).  Each is one
# Companion below and one row of LIBRARIES at the end of this section.  A side library is opened at its first use, not at
# import: a tree with only libslamhip.so built imports and runs as before.
class Companion:
    """libslamhip_<name>.so beside the package and its signature table; calling it returns the library, opened on first use.
    `header` is its public header relative to the repository (under include/ext/ when `ext`), `libs` the other side libraries it
    is linked against (<name>_LIBS in csrc/Makefile).
    No fallback: missing or unloadable is an ImportError.  With SLAMHIP_LIBRARY pointing elsewhere the handles belong to THAT
    library while the companion is linked against libslamhip.so, whose copy of the helpers it would run on them: refused."""

    def __init__(self, name, signatures, ext=False, libs=()):
        self.name = name
        self.path = os.path.join(_HERE, f"libslamhip_{name}.so")
        self.signatures = signatures
        self.ext = ext
        self.libs = tuple(libs)
        self.header = f"include/ext/slamhip_{name}.h" if ext else f"include/slamhip_{name}.h"
        self._lib = None

    def __call__(self):
        if self._lib is not None:
            return self._lib
        soname = os.path.basename(self.path)
        if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
            raise ImportError(f"{soname} is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                              f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
        if not os.path.exists(self.path):
            raise ImportError(f"{self.path} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
        try:
            cl = C.CDLL(self.path)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise ImportError(f"cannot load {self.path}: {e}.  slam.jl_amd has no CPU fallback.") from e
        for name, (res, args) in self.signatures.items():
            fn = getattr(cl, name)
            fn.restype = res
            fn.argtypes = args
        self._lib = cl
        return cl


# ---- frame: the rigid frame change, opened at the first transform -----------------------------------------------------------
#: every symbol include/slamhip_frame.h declares
FRAME_SIGNATURES = {
    "slam_ekf_transform": (C.c_int, [_h, C.c_double, C.c_double, C.c_double]),
    "slam_pf_transform": (C.c_int, [_h, C.c_double, C.c_double, C.c_double]),
}
frame_lib = Companion("frame", FRAME_SIGNATURES)
FRAME_LIB_PATH = frame_lib.path

# ---- join: map joining, opened at the first join ------------------------------------------------------------------------------
#: every symbol include/slamhip_join.h declares
JOIN_SIGNATURES = {
    "slam_ekf_join": (C.c_int, [_h, _h, _ip]),
}
join_lib = Companion("join", JOIN_SIGNATURES)
JOIN_LIB_PATH = join_lib.path

# ---- evidence: landmark evidence and pruning, opened when the first evidence object is made ----------------------------------
SLAM_PF_EVIDENCE_EMPTY = -128
SLAM_PF_EVIDENCE_MAXOBS = 64
_i64p = C.POINTER(C.c_int64)

#: every symbol include/slamhip_evidence.h declares
EVIDENCE_SIGNATURES = {
    "slam_pf_evidence_create": (C.c_int, [C.POINTER(_h), _h]),
    "slam_pf_evidence_destroy": (C.c_int, [_h]),
    "slam_pf_evidence_update": (C.c_int, [_h, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _i64p]),
    "slam_pf_step_unknown_evidence": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, C.c_int, _dp,
                                                C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                                C.c_int, _dp, _i64p]),
    "slam_pf_evidence_resample": (C.c_int, [_h, C.c_double, C.c_double]),
    "slam_pf_evidence_get": (C.c_int, [_h, C.c_void_p]),
}

evidence_lib = Companion("evidence", EVIDENCE_SIGNATURES)
EVIDENCE_LIB_PATH = evidence_lib.path

# ---- jc: joint-compatibility data association, opened when the first search workspace is made -------------------------------
SLAM_JC_MAXOBS = 64
SLAM_JC_MAXCAND = 8
SLAM_JC_NODE_CAP = 40000

#: every symbol include/slamhip_jc.h declares
JC_SIGNATURES = {
    "slam_ekf_jc_create": (C.c_int, [C.POINTER(_h), _h]),
    "slam_ekf_jc_destroy": (C.c_int, [_h]),
    "slam_ekf_associate_joint": (C.c_int, [_h, _dp, C.c_int, _dp, C.c_double, C.c_double, _dp, C.c_int64, _ip, _dp]),
    "slam_ekf_joint_nis": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, _dp]),
}

jc_lib = Companion("jc", JC_SIGNATURES)
JC_LIB_PATH = jc_lib.path

# ---- path: per-particle trajectory history for FastSLAM, opened when the first path object is made --------------------------
SLAM_PF_PATH_MAXTRACE = 4096

#: every symbol include/slamhip_path.h declares
PATH_SIGNATURES = {
    "slam_pf_path_create": (C.c_int, [C.POINTER(_h), _h, C.c_int]),
    "slam_pf_path_destroy": (C.c_int, [_h]),
    "slam_pf_path_record": (C.c_int, [_h]),
    "slam_pf_path_resample": (C.c_int, [_h, C.c_double, C.c_double]),
    "slam_pf_path_info": (C.c_int, [_h, _i64p]),
    "slam_pf_path_get": (C.c_int, [_h, C.c_int, _dp, _ip, C.POINTER(C.c_int)]),
    "slam_pf_path_trace": (C.c_int, [_h, _i64p, C.c_int, _dp]),
    "slam_pf_path_best": (C.c_int, [_h, _i64p, _dp]),
    "slam_pf_path_mean": (C.c_int, [_h, _dp]),
    "slam_pf_path_survivors": (C.c_int, [_h, _i64p]),
}

path_lib = Companion("path", PATH_SIGNATURES)
PATH_LIB_PATH = path_lib.path

# ---- copy: an EKF state copied, grown or extracted between two handles, opened at the first copy ----------------------------
#: every symbol include/slamhip_copy.h declares
COPY_SIGNATURES = {
    "slam_ekf_capacity": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_ekf_copy": (C.c_int, [_h, _h]),
    "slam_ekf_select": (C.c_int, [_h, _h, _ip, C.c_int]),
}

copy_lib = Companion("copy", COPY_SIGNATURES)
COPY_LIB_PATH = copy_lib.path

# ---- handover: a state handed between FastSLAM and the EKF (handles of both kinds), opened at the first hand-over -----------
#: every symbol include/slamhip_handover.h declares
HANDOVER_SIGNATURES = {
    "slam_pf_to_ekf": (C.c_int, [_h, _h, _ip, C.c_int, _dp]),
    "slam_ekf_to_pf": (C.c_int, [_h, _h, _ip, C.c_int]),
}

handover_lib = Companion("handover", HANDOVER_SIGNATURES)
HANDOVER_LIB_PATH = handover_lib.path

# ---- pfcopy: a particle set uploaded, copied, selected and resized between handles, opened at the first call ----------------
#: every symbol include/slamhip_pfcopy.h declares
PFCOPY_SIGNATURES = {
    "slam_pf_get_meta": (C.c_int, [_h, _i64p, C.c_void_p]),
    "slam_pf_set_rng": (C.c_int, [_h, C.c_uint64, C.c_uint32]),
    "slam_pf_upload": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "slam_pf_select": (C.c_int, [_h, _h, _ip, C.c_int, C.c_int]),
    "slam_pf_copy": (C.c_int, [_h, _h, C.c_int]),
    "slam_pf_resize": (C.c_int, [_h, _h, C.c_double, C.c_double, C.c_int, _ip]),
    "slam_pf_pose_bins": (C.c_int, [_h, C.c_double, C.c_double, _i64p]),
}

pfcopy_lib = Companion("pfcopy", PFCOPY_SIGNATURES)
PFCOPY_LIB_PATH = pfcopy_lib.path

# ---- the extensions: libraries wired like a companion whose header lives in include/ext/ ------------------------------------
# ---- factor: the Cholesky factor of an EKF state's covariance, opened when the first factor object is made --------------------
SLAM_FACTOR_MAXRHS = 64

#: every symbol include/ext/slamhip_factor.h declares
FACTOR_SIGNATURES = {
    "slam_ekf_factor_create": (C.c_int, [C.POINTER(_h), C.c_int, C.c_int, C.c_int, C.c_int]),
    "slam_ekf_factor_destroy": (C.c_int, [_h]),
    "slam_ekf_factor_compute": (C.c_int, [_h, _h, _dp]),
    "slam_ekf_factor_info": (C.c_int, [_h, _dp]),
    "slam_ekf_factor_get": (C.c_int, [_h, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "slam_ekf_factor_mean": (C.c_int, [_h, _dp]),
    "slam_ekf_factor_solve": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp, _dp]),
    "slam_ekf_factor_multiply": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp]),
}

factor_lib = Companion("factor", FACTOR_SIGNATURES, ext=True)
FACTOR_LIB_PATH = factor_lib.path

# ---- linear: caller-supplied motion and measurement models for the EKF, opened at the first such call --------------------------
SLAM_LINEAR_MAXROWS = 16
SLAM_LINEAR_MAXNNZ = 8
SLAM_LINEAR_MEASURED, SLAM_LINEAR_INNOVATION = 0, 1

#: every symbol include/ext/slamhip_linear.h declares
LINEAR_SIGNATURES = {
    "slam_ekf_update_linear": (C.c_int, [_h, C.c_int, _ip, _ip, _dp, _dp, _dp, C.c_int, C.c_uint32, _dp]),
    "slam_ekf_linear_nis": (C.c_int, [_h, C.c_int, _ip, _ip, _dp, _dp, _dp, C.c_int, C.c_uint32, _dp]),
    "slam_ekf_predict_linear": (C.c_int, [_h, _dp, _dp, _dp]),
    "slam_ekf_predict_odometry": (C.c_int, [_h, _dp, _dp]),
}

linear_lib = Companion("linear", LINEAR_SIGNATURES, ext=True)
LINEAR_LIB_PATH = linear_lib.path

# ---- proposal: FastSLAM 2.0 with unknown correspondences, opened at the first such step -------------------------------------------
#: every symbol include/ext/slamhip_proposal.h declares
PROPOSAL_SIGNATURES = {
    "slam_pf_step_proposal_unknown": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, C.c_int, _dp,
                                                C.c_double, C.c_double, C.c_void_p, _dp]),
    "slam_pf_associate_proposal": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double, _dp, C.c_int, _dp,
                                             C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "slam_pf_proposal_limits": (C.c_int, [C.POINTER(C.c_int)]),
}

proposal_lib = Companion("proposal", PROPOSAL_SIGNATURES, ext=True)
PROPOSAL_LIB_PATH = proposal_lib.path


# ---- local: compressed local-area updates for the EKF, opened when the first area object is made ----------------------------------
SLAM_LOCAL_MAXLM = 1024

#: every symbol include/ext/slamhip_local.h declares
LOCAL_SIGNATURES = {
    "slam_ekf_local_create": (C.c_int, [C.POINTER(_h), _h, C.c_int]),
    "slam_ekf_local_destroy": (C.c_int, [_h]),
    "slam_ekf_local_open": (C.c_int, [_h, _ip, C.c_int]),
    "slam_ekf_local_state": (C.c_int, [_h, C.POINTER(_h)]),
    "slam_ekf_local_predict": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double]),
    "slam_ekf_local_update": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, C.c_int]),
    "slam_ekf_local_augment": (C.c_int, [_h, _dp, C.c_int, _dp]),
    "slam_ekf_local_close": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_ekf_local_abort": (C.c_int, [_h]),
    "slam_ekf_local_info": (C.c_int, [_h, _i64p]),
    "slam_ekf_local_get": (C.c_int, [_h, _dp, _dp, _dp]),
}

local_lib = Companion("local", LOCAL_SIGNATURES, ext=True, libs=("copy",))
LOCAL_LIB_PATH = local_lib.path


# ---- iterated: the iterated EKF update, relinearised on the device, opened at the first such call ----------------------------------
SLAM_ITERATED_MAXOBS = 8
SLAM_ITERATED_MAXITER = 64

#: every symbol include/ext/slamhip_iterated.h declares
ITERATED_SIGNATURES = {
    "slam_ekf_update_iterated": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, C.c_int, C.c_double, _dp]),
    "slam_ekf_iterated_nis": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, C.c_int, C.c_double, _dp]),
    "slam_ekf_iterated_limits": (C.c_int, [_ip]),
}

iterated_lib = Companion("iterated", ITERATED_SIGNATURES, ext=True)
ITERATED_LIB_PATH = iterated_lib.path


# ---- fej: first-estimates Jacobian predict, update and augment for the EKF, opened when the first such object is made ---------------
SLAM_FEJ_MAXOBS = 8

#: every symbol include/ext/slamhip_fej.h declares
FEJ_SIGNATURES = {
    "slam_ekf_fej_create": (C.c_int, [C.POINTER(_h), _h]),
    "slam_ekf_fej_destroy": (C.c_int, [_h]),
    "slam_ekf_fej_predict": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_double]),
    "slam_ekf_fej_update": (C.c_int, [_h, _dp, _ip, C.c_int, _dp, _dp]),
    "slam_ekf_fej_augment": (C.c_int, [_h, _dp, C.c_int, _dp]),
    "slam_ekf_fej_reset": (C.c_int, [_h, _ip, C.c_int, C.c_int]),
    "slam_ekf_fej_remap": (C.c_int, [_h, _ip, C.c_int]),
    "slam_ekf_fej_transform": (C.c_int, [_h, C.c_double, C.c_double, C.c_double]),
    "slam_ekf_fej_get": (C.c_int, [_h, _dp, _dp, _ip]),
    "slam_ekf_fej_set": (C.c_int, [_h, _dp, _dp]),
    "slam_ekf_fej_limits": (C.c_int, [_ip]),
}

fej_lib = Companion("fej", FEJ_SIGNATURES, ext=True)
FEJ_LIB_PATH = fej_lib.path


# ---- wide: the joint update of up to 64 observations in one down-date, opened at the first such call --------------------------------
SLAM_WIDE_MAXOBS = 64

#: every symbol include/ext/slamhip_wide.h declares
WIDE_SIGNATURES = {
    "slam_ekf_wide_update": (C.c_int, [_h, _h, _dp, _ip, C.c_int, _dp, _dp]),
    "slam_ekf_wide_nis": (C.c_int, [_h, _h, _dp, _ip, C.c_int, _dp, _dp]),
    "slam_ekf_wide_limits": (C.c_int, [_ip]),
}

wide_lib = Companion("wide", WIDE_SIGNATURES, ext=True)
WIDE_LIB_PATH = wide_lib.path

#: side library name -> its loader, all fifteen in the order they were added.  A new library is one row here.
LIBRARIES = {c.name: c for c in (frame_lib, join_lib, evidence_lib, jc_lib, path_lib, copy_lib, handover_lib, pfcopy_lib,
                                 factor_lib, linear_lib, proposal_lib, local_lib, iterated_lib, fej_lib, wide_lib)}
#: the rows whose header lies in include/
COMPANIONS = {name: c for name, c in LIBRARIES.items() if not c.ext}
#: the rows whose header lies in include/ext/
EXTENSIONS = {name: c for name, c in LIBRARIES.items() if c.ext}


def proposal_max_obs() -> int:
    """Observations per call of the proposal step with unknown correspondences, as the library reports it."""
    out = (C.c_int * 4)()
    check(proposal_lib().slam_pf_proposal_limits(out))
    return int(out[0])


def last_error() -> str:
    msg = lib.slam_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int) -> None:
    if rc == SLAM_OK:
        return
    if rc == SLAM_E_NOTPD:
        raise NotPositiveDefinite(rc, last_error())
    raise SlamHipError(rc, last_error())


def device_count() -> int:
    return int(lib.slam_device_count())
