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


# ---- the companion library: the rigid frame change (include/slamhip_frame.h) -----------------------------------------------
# libslamhip.so exports exactly what its two headers declare; the frame change lives beside it in libslamhip_frame.so, which
# links against libslamhip.so (run path $ORIGIN) and works on its handles.  It is opened at the first transform, not at
# import: a tree with only libslamhip.so built imports and runs as before.
FRAME_LIB_PATH = os.path.join(_HERE, "libslamhip_frame.so")

#: every symbol include/slamhip_frame.h declares
FRAME_SIGNATURES = {
    "slam_ekf_transform": (C.c_int, [_h, C.c_double, C.c_double, C.c_double]),
    "slam_pf_transform": (C.c_int, [_h, C.c_double, C.c_double, C.c_double]),
}

_frame = None


def frame_lib():
    """libslamhip_frame.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  With SLAMHIP_LIBRARY
    pointing elsewhere the handles belong to THAT library while the companion is linked against libslamhip.so, whose copy
    of the helpers it would run on them: refused."""
    global _frame
    if _frame is not None:
        return _frame
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_frame.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(FRAME_LIB_PATH):
        raise ImportError(f"{FRAME_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        fl = C.CDLL(FRAME_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {FRAME_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in FRAME_SIGNATURES.items():
        fn = getattr(fl, name)
        fn.restype = res
        fn.argtypes = args
    _frame = fl
    return fl


# ---- the second companion library: map joining (include/slamhip_join.h) ------------------------------------------------------
# Same arrangement as the frame change: libslamhip_join.so links against libslamhip.so (run path $ORIGIN), works on its handles
# and is opened at the first join, not at import.
JOIN_LIB_PATH = os.path.join(_HERE, "libslamhip_join.so")

#: every symbol include/slamhip_join.h declares
JOIN_SIGNATURES = {
    "slam_ekf_join": (C.c_int, [_h, _h, _ip]),
}

_join = None


def join_lib():
    """libslamhip_join.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _join
    if _join is not None:
        return _join
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_join.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(JOIN_LIB_PATH):
        raise ImportError(f"{JOIN_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        jl = C.CDLL(JOIN_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {JOIN_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in JOIN_SIGNATURES.items():
        fn = getattr(jl, name)
        fn.restype = res
        fn.argtypes = args
    _join = jl
    return jl


# ---- the third companion library: landmark evidence and pruning (include/slamhip_evidence.h) --------------------------------
# Same arrangement again: libslamhip_evidence.so links against libslamhip.so (run path $ORIGIN), works on its particle-filter
# handles and is opened when the first evidence object is made, not at import.
EVIDENCE_LIB_PATH = os.path.join(_HERE, "libslamhip_evidence.so")
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

_evidence = None


def evidence_lib():
    """libslamhip_evidence.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses
    SLAMHIP_LIBRARY for the reason frame_lib() gives: the handles would belong to another library than the one the companion is
    linked against."""
    global _evidence
    if _evidence is not None:
        return _evidence
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_evidence.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(EVIDENCE_LIB_PATH):
        raise ImportError(f"{EVIDENCE_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        el = C.CDLL(EVIDENCE_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {EVIDENCE_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in EVIDENCE_SIGNATURES.items():
        fn = getattr(el, name)
        fn.restype = res
        fn.argtypes = args
    _evidence = el
    return el


# ---- the fourth companion library: joint-compatibility data association (include/slamhip_jc.h) -------------------------------
# Same arrangement again: libslamhip_jc.so links against libslamhip.so (run path $ORIGIN), works on its EKF handles and is
# opened when the first search workspace is made, not at import.
JC_LIB_PATH = os.path.join(_HERE, "libslamhip_jc.so")
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

_jc = None


def jc_lib():
    """libslamhip_jc.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _jc
    if _jc is not None:
        return _jc
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_jc.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(JC_LIB_PATH):
        raise ImportError(f"{JC_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        cl = C.CDLL(JC_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {JC_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in JC_SIGNATURES.items():
        fn = getattr(cl, name)
        fn.restype = res
        fn.argtypes = args
    _jc = cl
    return cl


# ---- the fifth companion library: per-particle trajectory history for FastSLAM (include/slamhip_path.h) ----------------------
# Same arrangement again: libslamhip_path.so links against libslamhip.so (run path $ORIGIN), works on its particle-filter
# handles and is opened when the first path object is made, not at import.
PATH_LIB_PATH = os.path.join(_HERE, "libslamhip_path.so")
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

_path = None


def path_lib():
    """libslamhip_path.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _path
    if _path is not None:
        return _path
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_path.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(PATH_LIB_PATH):
        raise ImportError(f"{PATH_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        pl = C.CDLL(PATH_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {PATH_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in PATH_SIGNATURES.items():
        fn = getattr(pl, name)
        fn.restype = res
        fn.argtypes = args
    _path = pl
    return pl


# ---- the sixth companion library: an EKF state copied, grown or extracted between two handles (include/slamhip_copy.h) --------
# Same arrangement again: libslamhip_copy.so links against libslamhip.so (run path $ORIGIN), works on its EKF handles and is
# opened at the first copy, not at import.
COPY_LIB_PATH = os.path.join(_HERE, "libslamhip_copy.so")

#: every symbol include/slamhip_copy.h declares
COPY_SIGNATURES = {
    "slam_ekf_capacity": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "slam_ekf_copy": (C.c_int, [_h, _h]),
    "slam_ekf_select": (C.c_int, [_h, _h, _ip, C.c_int]),
}

_copy = None


def copy_lib():
    """libslamhip_copy.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _copy
    if _copy is not None:
        return _copy
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_copy.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(COPY_LIB_PATH):
        raise ImportError(f"{COPY_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        yl = C.CDLL(COPY_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {COPY_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in COPY_SIGNATURES.items():
        fn = getattr(yl, name)
        fn.restype = res
        fn.argtypes = args
    _copy = yl
    return yl


# ---- the seventh companion library: a state handed between FastSLAM and the EKF (include/slamhip_handover.h) ------------------
# Same arrangement again: libslamhip_handover.so links against libslamhip.so (run path $ORIGIN), works on its handles of both
# kinds and is opened at the first hand-over, not at import.
HANDOVER_LIB_PATH = os.path.join(_HERE, "libslamhip_handover.so")

#: every symbol include/slamhip_handover.h declares
HANDOVER_SIGNATURES = {
    "slam_pf_to_ekf": (C.c_int, [_h, _h, _ip, C.c_int, _dp]),
    "slam_ekf_to_pf": (C.c_int, [_h, _h, _ip, C.c_int]),
}

_handover = None


def handover_lib():
    """libslamhip_handover.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _handover
    if _handover is not None:
        return _handover
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_handover.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(HANDOVER_LIB_PATH):
        raise ImportError(f"{HANDOVER_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        hl = C.CDLL(HANDOVER_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {HANDOVER_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in HANDOVER_SIGNATURES.items():
        fn = getattr(hl, name)
        fn.restype = res
        fn.argtypes = args
    _handover = hl
    return hl


# ---- the eighth companion library: a particle set uploaded, copied, selected and resized (include/slamhip_pfcopy.h) ------------
# Same arrangement again: libslamhip_pfcopy.so links against libslamhip.so (run path $ORIGIN), works on its particle-filter
# handles and is opened at the first call, not at import.
PFCOPY_LIB_PATH = os.path.join(_HERE, "libslamhip_pfcopy.so")

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

_pfcopy = None


def pfcopy_lib():
    """libslamhip_pfcopy.so, opened on first use.  No fallback: missing or unloadable is an ImportError.  Refuses SLAMHIP_LIBRARY
    for the reason frame_lib() gives: the handles would belong to another library than the one the companion is linked against."""
    global _pfcopy
    if _pfcopy is not None:
        return _pfcopy
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libslamhip.so"):
        raise ImportError(f"libslamhip_pfcopy.so is linked against {os.path.join(_HERE, 'libslamhip.so')}; the handles of "
                          f"{LIB_PATH} (SLAMHIP_LIBRARY) cannot be passed to it")
    if not os.path.exists(PFCOPY_LIB_PATH):
        raise ImportError(f"{PFCOPY_LIB_PATH} is missing: build it with `make -C slam.jl_amd/csrc`.  slam.jl_amd has no CPU fallback.")
    try:
        kl = C.CDLL(PFCOPY_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ImportError(f"cannot load {PFCOPY_LIB_PATH}: {e}.  slam.jl_amd has no CPU fallback.") from e
    for name, (res, args) in PFCOPY_SIGNATURES.items():
        fn = getattr(kl, name)
        fn.restype = res
        fn.argtypes = args
    _pfcopy = kl
    return kl


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
