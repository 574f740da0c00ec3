"""ctypes binding of libcdx_host.so, the host build of the per-candidate code (``csrc/host_ref.cpp``).

The CPU tests, the GPU tests that hold the device to the host rule and the host paths of ``tools/`` call it; the
product never does.  Every ``cdxh_*`` entry point has its line in ``_SIGS``; tests/test_abi.py holds the table to the
definitions in host_ref.cpp.
"""
import ctypes as C
import os
import threading

from ._native import (LIB_DIR, CdxChain, CdxCollision, CdxEquilLimits, CdxEquilParams, CdxForceEq, CdxGpis, CdxGpisModeBuffers,
                      CdxGpisModeOpt, CdxGpisModeParams, CdxHand, CdxHandParams, CdxIkParams, CdxProblem, CdxTrajParams, CdxWrenchParams)

_P = C.c_void_p
_I32 = C.c_int32
_I64 = C.c_int64
_U64 = C.c_uint64
_F64 = C.c_double
_CHAIN, _HAND, _HAND_PARAMS = C.POINTER(CdxChain), C.POINTER(CdxHand), C.POINTER(CdxHandParams)
_MODE = [_CHAIN, C.POINTER(CdxGpisModeParams)]
_SIGS = {
    "cdxh_fk_forward": (C.c_int, [_CHAIN, _P, _I64, _P, _P]),
    "cdxh_fk_backward": (C.c_int, [_CHAIN, _P, _I64, _P, _P]),
    "cdxh_fk_jacobian": (C.c_int, [_CHAIN, _P, _I64, _P, _P]),
    "cdxh_ik_solve": (C.c_int, [_CHAIN, C.POINTER(CdxIkParams), _I64, _P, _I32] + [_P] * 8),
    "cdxh_ik_solve_pose": (C.c_int, [_CHAIN, C.POINTER(CdxIkParams), _I64, _P, _I32] + [_P] * 11),
    "cdxh_ik_solve_frames": (C.c_int, [_CHAIN, C.POINTER(CdxIkParams), _I64, _P, _I32] + [_P] * 6 + [_U64] * 2 + [_P] * 5 + [_I32]),
    "cdxh_dyn_inverse": (C.c_int, [_CHAIN, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "cdxh_dyn_inertia": (C.c_int, [_CHAIN, _P, _I64, _P, _I32, _P]),
    "cdxh_dyn_forward": (C.c_int, [_CHAIN, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P]),
    "cdxh_min_wrench": (C.c_int, [C.POINTER(CdxWrenchParams), _I64] + [_P] * 10),
    "cdxh_grasp_equilibrium": (C.c_int, [C.POINTER(CdxEquilParams), _I64, _I64] + [_P] * 6 + [_I32] + [_P] * 10),
    "cdxh_equil_reduce": (C.c_int, [C.POINTER(CdxEquilLimits), _I64, _I64, _I32] + [_P] * 13),
    "cdxh_hand_prepare": (C.c_int, [_I32, _I32, _P, _P, _P, _I32, _P, _P, _HAND]),
    "cdxh_hand_spheres": (C.c_int, [_CHAIN, _HAND, _I64] + [_P] * 5),
    "cdxh_hand_cost": (C.c_int, [_HAND, _HAND_PARAMS, _I64] + [_P] * 7),
    "cdxh_hand_pullback": (C.c_int, [_CHAIN, _HAND, _I64] + [_P] * 6),
    "cdxh_hand_term": (C.c_int, [_CHAIN, _HAND, _HAND_PARAMS, _I64] + [_P] * 5 + [_F64, _I32] + [_P] * 6),
    "cdxh_traj_seed": (C.c_int, [_I64, _I32, _I32, _I32, _P, _P, _F64, _U64, _P]),
    "cdxh_traj_step": (C.c_int, [C.POINTER(CdxTrajParams), _I64, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "cdxh_traj_gradient": (C.c_int, [C.POINTER(CdxTrajParams), _I64, _P, _P, _P]),
    "cdxh_hand_bytes": (C.c_size_t, [_I32, _I32]),
    "cdxh_hand_sincos": (None, [_P, _I64, _P, _P]),
    "cdxh_n_queries": (_I64, [C.POINTER(CdxProblem), _I64]),
    "cdxh_closure_queries": (C.c_int, [C.POINTER(CdxProblem), _I64] + [_P] * 5),
    "cdxh_closure_cost": (C.c_int, [C.POINTER(CdxProblem), _I64] + [_P] * 19),
    "cdxh_collision": (C.c_int, [C.POINTER(CdxCollision), _I64] + [_P] * 7),
    "cdxh_force_eq": (None, [C.POINTER(CdxForceEq), _I64] + [_P] * 14),
    "cdxh_gpis_mode_cost": (C.c_int, _MODE + [C.POINTER(CdxGpisModeBuffers), _I64, _I32, _P, _U64, _I32]),
    "cdxh_gpis_mode_step": (C.c_int, _MODE + [C.POINTER(CdxGpisModeOpt), C.POINTER(CdxGpisModeBuffers), _I64, _I32,
                                              _I32, _I32]),
    "cdxh_gpis_joint": (C.c_int, [C.POINTER(CdxGpis), _P, _I64, _P]),
    "cdxh_gpis_kernel_values": (C.c_int, [_I32, _F64, _F64, _F64, _P]),
    "cdxh_svd3": (None, [_P] * 4),
    "cdxh_sdf_forward": (None, [_P, _I64, _P, _I64] + [_P] * 5),
    "cdxh_face_dist2": (None, [_P, _P, _I64, _P, _P]),
    "cdxh_surface_extract": (_I64, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P, _P, _P]),
    "cdxh_mesh_extract": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _I64, _I64, _P, _P, _P, _P]),
    "cdxh_mesh_refine": (C.c_int, [_P, _I32, _P, _I32, _P, _P, _P, _P, _I64, _P, _P]),
    "cdxh_fps": (C.c_int, [_P, _I32, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "cdxh_knn": (C.c_int, [_P, _I32, _I64, _P, _I64, _I64, _F64, _I32, _P, _P, _P]),
    "cdxh_cloud_normals": (C.c_int, [_P, _I32, _I64, _P, _P, _I64, _P, _P, _P, _P]),
    "cdxh_sym3_eig": (None, [_P, _I64, _P, _P]),
    "cdxh_knn_grid": (C.c_int, [_P, _I64] + [_P] * 5),
    "cdxh_knn_ring_bound": (C.c_int, [_P] * 5 + [_I64, _I32] + [_P] * 3),
    "cdxh_ray_cast": (C.c_int, [_P, _I64, _P, _P, _I64, _F64, _F64, _P, _P, _P]),
    "cdxh_pixel_rays": (C.c_int, [_I32, _I32, _P, _P, _P, _P]),
    "cdxh_ray_ball_miss": (None, [_P] * 5 + [_I64, _P, _P]),
    "cdxh_depth_unproject": (_I64, [_P, _I32, _I32, _I32, _I32, _P, _F64, _F64, _F64, _P, _I64, _P]),
    "cdxh_sample_prepare": (C.c_int, [_P, _I32, _I64, _P, _P]),
    "cdxh_sample_draw": (C.c_int, [_P, _I32, _I64, _P, _U64, _U64, _I64, _P, _P, _P, _P]),
    "cdxh_philox4x32_10": (None, [_P] * 3),
}

_lib = None
_lock = threading.Lock()


def lib_path():
    return os.path.join(LIB_DIR, "libcdx_host.so")


def load():
    """Loads libcdx_host.so, building it first if it is missing (g++ alone, a few seconds)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            from .build import build_host
            build_host()
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def ptr(a):
    """Host pointer of a (contiguous) numpy array as c_void_p, or None."""
    if a is None:
        return None
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be contiguous")
    return a.ctypes.data_as(C.c_void_p)
