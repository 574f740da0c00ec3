"""ctypes binding of the C ABI in ``include/cdx.h`` (libcdx.so, gfx950).

There is no CPU fallback: if the library is missing or fails to load, every operator
raises.  Struct layouts are checked against the library's own ``sizeof`` at load time.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

MAX_BODIES, MAX_TIPS, MAX_DOFS, MAX_LEVELS = 32, 8, 32, 4
MAX_DEPTH = 16  # CDX_MAX_DEPTH: bodies on the longest root→tip path
KERNELS = {"tps": 0, "rbf": 1, "joint": 2}
NPAD_ALIGN = 256  # CDX_NPAD_ALIGN
SCREEN_BANDS = 24  # CDX_SCREEN_BANDS
FIELD_MAX_STEPS = 1024  # CDX_FIELD_MAX_STEPS
DTYPE_F32, DTYPE_F64 = 0, 1  # CDX_DTYPE_*
FPS_MODES = {"auto": 0, "block": 1, "rounds": 2}  # cdx_fps mode
SAMPLE_MODES = {"auto": 0, "table": 1, "splitters": 2}  # cdx_sample_draw mode
KNN_MODES = {"auto": 0, "scan": 1, "grid": 2}  # CDX_KNN_*
KNN_MAX_K = 64  # CDX_KNN_MAX_K
PROF_STAGES = 6  # cdx_profile_read array length
SDF_REUSE_ORDER, SDF_MESH_CULLED, SDF_MESH_EXACT = 1, 2, 4  # cdx_sdf_query flags
SDF_SCHED_KEEP = 8  # cdx_sdf_query_batch, first query: keep the schedule's order
RAY_MODES = {"auto": 0, "scan": 1, "walk": 2}  # CDX_RAY_*
DEPTH_U16 = 2  # CDX_DEPTH_U16, next to DTYPE_F32 / DTYPE_F64
ERRORS = {-1: "invalid argument", -2: "unsupported GPIS kernel", -3: "chain exceeds descriptor capacity",
          -10: "HIP launch failed"}


class CdxGpis(C.Structure):
    _fields_ = [("X1", C.c_void_p), ("alpha", C.c_void_p), ("Ainv", C.c_void_p), ("Linv_t", C.c_void_p),
                ("Linv", C.c_void_p), ("N", C.c_int32),
                ("N_pad", C.c_int32), ("kernel", C.c_int32), ("_pad", C.c_int32), ("R", C.c_double),
                ("sigma", C.c_double), ("bias", C.c_double), ("screen", C.c_void_p), ("screen_delta", C.c_double)]


class CdxBody(C.Structure):
    _fields_ = [("F", C.c_float * 9), ("t", C.c_float * 3), ("sign", C.c_float), ("axis", C.c_int8),
                ("parent", C.c_int8), ("dof", C.c_int8), ("_pad", C.c_int8)]


class CdxChain(C.Structure):
    _fields_ = [("n_bodies", C.c_int32), ("n_dofs", C.c_int32), ("n_tips", C.c_int32), ("has_offsets", C.c_int32),
                ("tip_body", C.c_int32 * MAX_TIPS), ("tip_offset", (C.c_float * 3) * MAX_TIPS),
                ("bodies", CdxBody * MAX_BODIES)]


class CdxIkParams(C.Structure):
    _fields_ = [("lower", C.c_double * MAX_DOFS), ("upper", C.c_double * MAX_DOFS), ("ref_q", C.c_double * MAX_DOFS),
                ("rho", C.c_double), ("tol", C.c_double), ("mu0", C.c_double), ("mu_min", C.c_double),
                ("mu_max", C.c_double), ("nu", C.c_double), ("max_iters", C.c_int32), ("_pad", C.c_int32)]


class CdxDyn(C.Structure):
    _fields_ = [("mass", C.c_double * MAX_BODIES), ("mcom", (C.c_double * 3) * MAX_BODIES),
                ("inertia", (C.c_double * 6) * MAX_BODIES), ("damping", C.c_double * MAX_DOFS)]


class CdxEquilParams(C.Structure):
    _fields_ = [("n_tips", C.c_int32), ("max_iters", C.c_int32), ("mu", C.c_double), ("tol", C.c_double),
                ("mu0", C.c_double), ("mu_min", C.c_double), ("mu_max", C.c_double), ("nu", C.c_double)]


class CdxEquilLimits(C.Structure):
    _fields_ = [("margin_min", C.c_double), ("min_normal_force", C.c_double), ("max_shift", C.c_double),
                ("max_chord", C.c_double)]


class CdxWrenchParams(C.Structure):
    _fields_ = [("n_tips", C.c_int32), ("max_iters", C.c_int32), ("check_every", C.c_int32), ("_pad", C.c_int32),
                ("mu", C.c_double), ("min_force", C.c_double), ("reg", C.c_double), ("rho", C.c_double),
                ("tol", C.c_double)]


HAND_MAX_SPHERES, HAND_MAX_PAIRS, HAND_LANES = 256, 32768, 64  # CDX_MAX_SPHERES, CDX_HAND_MAX_PAIRS, CDX_HAND_LANES


class CdxHand(C.Structure):
    _fields_ = [("n_spheres", C.c_int32), ("n_pairs", C.c_int32), ("n_bodies", C.c_int32), ("_pad", C.c_int32),
                ("radius", C.c_void_p), ("local", C.c_void_p), ("body", C.c_void_p), ("len", C.c_void_p),
                ("pairs", C.c_void_p), ("entry", C.c_void_p), ("group_base", C.c_int32 * 4)]


class CdxHandParams(C.Structure):
    _fields_ = [("m_obj", C.c_double), ("m_self", C.c_double), ("m_floor", C.c_double), ("w_obj", C.c_double),
                ("w_self", C.c_double), ("w_floor", C.c_double), ("floor_z", C.c_double), ("floor_on", C.c_int32),
                ("_pad", C.c_int32)]


TRAJ_MAX_T, TRAJ_LANES = 64, 32  # CDX_TRAJ_MAX_T, CDX_TRAJ_LANES


class CdxTrajParams(C.Structure):
    _fields_ = [("lower", C.c_double * MAX_DOFS), ("upper", C.c_double * MAX_DOFS), ("w_smooth", C.c_double),
                ("w_col", C.c_double), ("w_lim", C.c_double), ("m_lim", C.c_double), ("step", C.c_double),
                ("T", C.c_int32), ("n_dofs", C.c_int32)]


class CdxProblem(C.Structure):
    _fields_ = [("chain", CdxChain), ("gpis", CdxGpis), ("n_levels", C.c_int32), ("n_query_levels", C.c_int32),
                ("level_query", C.c_int32 * MAX_LEVELS), ("coeff", (C.c_float * MAX_TIPS) * MAX_LEVELS),
                ("weight", C.c_double * MAX_LEVELS), ("ref_q", C.c_float * MAX_DOFS), ("cos_mu", C.c_float),
                ("gravity", C.c_int32), ("optimize_palm", C.c_int32), ("_pad", C.c_int32), ("com", C.c_float * 3),
                ("dummy_target_z", C.c_float), ("dummy_comp", C.c_float), ("_pad2", C.c_float),
                ("uncertainty", C.c_double), ("loop", C.c_void_p)]


MAX_PAIRS = 28


class CdxCollision(C.Structure):
    _fields_ = [("chain", CdxChain), ("n_pairs", C.c_int32), ("palm_term", C.c_int32),
                ("pairs", (C.c_int8 * 2) * MAX_PAIRS), ("pair_threshold", C.c_double), ("floor_z", C.c_double)]


class CdxForceEq(C.Structure):
    _fields_ = [("cos_mu", C.c_float), ("gravity", C.c_int32), ("com", C.c_float * 3), ("dummy_target_z", C.c_float),
                ("dummy_comp", C.c_float), ("n_tips", C.c_int32)]


class CdxKinParams(C.Structure):
    _fields_ = [("fe", CdxForceEq), ("ref_q", C.c_float * MAX_DOFS)]


class CdxKinOpt(C.Structure):
    _fields_ = [("rule", C.c_int32), ("clamp_box", C.c_int32), ("lr", C.c_double * 3), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("alpha", C.c_double), ("palm_offset", C.c_float * 3),
                ("box_lb", C.c_float * (MAX_TIPS * 3)), ("box_ub", C.c_float * (MAX_TIPS * 3)), ("_pad", C.c_int32)]


KIN_OPT_FIELDS = ["pose", "target", "comp", "g_pose", "g_target", "g_comp", "m_pose", "v_pose", "m_target", "v_target",
                  "m_comp", "v_comp", "loss"]


class CdxKinOptBuffers(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in KIN_OPT_FIELDS] + [("margin", C.c_void_p * 2), ("normal", C.c_void_p * 2)] +
                [(n, C.c_void_p) for n in ("opt_value", "opt_margin", "opt_normal", "opt_pose", "opt_target",
                                            "opt_comp", "any", "tips", "fk_state")])


class CdxGpisModeParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("_pad", C.c_int32), ("fe", CdxForceEq), ("uncertainty", C.c_double),
                ("ref_q", C.c_double * MAX_DOFS), ("palm_offset", C.c_double * 3)]


class CdxGpisModeOpt(C.Structure):
    _fields_ = [("lr", C.c_double * 3), ("alpha", C.c_double), ("eps", C.c_double),
                ("box_lb", C.c_double * (MAX_TIPS * 3)), ("box_ub", C.c_double * (MAX_TIPS * 3)),
                ("comp_min", C.c_double)]


GPIS_MODE_FIELDS = ["pose", "target", "comp", "tips", "mean", "gmean", "normal", "std", "gstd", "tmean", "tgmean",
                    "g_pose", "g_target", "g_comp", "g_tip", "v_pose", "v_target", "v_comp", "loss"]


class CdxGpisModeBuffers(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in GPIS_MODE_FIELDS] +
                [("margin", C.c_void_p * 2), ("normal_slot", C.c_void_p * 2)] +
                [(n, C.c_void_p) for n in ("opt_value", "opt_margin", "opt_normal", "opt_pose", "opt_target",
                                            "opt_comp", "any")])


class CdxSdfBatchQuery(C.Structure):
    _fields_ = [("mesh", C.c_void_p), ("faces", C.c_void_p), ("F", C.c_int64), ("points", C.c_void_p), ("P", C.c_int64),
                ("sqdist", C.c_void_p), ("sign", C.c_void_p), ("normals", C.c_void_p), ("clst", C.c_void_p),
                ("face_idx", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("flags", C.c_int32), ("_pad", C.c_int32)]


class CdxAdam(C.Structure):
    _fields_ = [("lr", C.c_double * 5), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("comp_min", C.c_double), ("target_lb", C.c_double * (MAX_TIPS * 3)),
                ("target_ub", C.c_double * (MAX_TIPS * 3)), ("clamp_target", C.c_int32), ("best_after", C.c_int32)]


OPT_BUFFER_FIELDS = ["q", "comp", "target", "palm_pos", "palm_ori", "g_q", "g_comp", "g_target", "g_palm_pos",
                     "g_palm_ori", "m_q", "v_q", "m_comp", "v_comp", "m_target", "v_target", "m_palm_pos",
                     "v_palm_pos", "m_palm_ori", "v_palm_ori", "total_loss", "total_margin", "opt_value", "opt_margin",
                     "opt_q", "opt_comp", "opt_target", "opt_palm"]


class CdxOptBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OPT_BUFFER_FIELDS] + [("loop", C.c_void_p)]


class CdxScreenReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("screened", "screened_rows", "exact_rows", "audited_rows", "bound_misses",
                                         "audit_misses", "audit_flips", "faults")] + \
               [("max_ratio", C.c_double), ("max_ratio_audit", C.c_double)] + \
               [(n, C.c_int64) for n in ("cum_closures", "cum_audited_rows", "cum_bound_misses", "cum_audit_misses",
                                         "cum_audit_flips", "cum_faults")] + \
               [("cum_max_ratio", C.c_double), ("cum_max_ratio_audit", C.c_double)] + \
               [("repaired", C.c_int32), ("discarded_rows", C.c_int32), ("min_gap", C.c_double),
                ("audit_cut", C.c_double), ("cum_repairs", C.c_int64), ("cum_discarded_rows", C.c_int64),
                ("cum_min_gap", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_P = C.c_void_p
_I64 = C.c_int64
_SIGS = {
    "cdx_gpis_mean": (C.c_int, [C.POINTER(CdxGpis), _P, _I64, _P, _P, _P, _P]),
    "cdx_gpis_std_workspace": (C.c_size_t, [C.POINTER(CdxGpis), _I64]),
    "cdx_gpis_std": (C.c_int, [C.POINTER(CdxGpis), _P, _I64, _P, _P, _P, _P]),
    "cdx_gpis_joint_workspace": (C.c_size_t, [C.POINTER(CdxGpis), _I64]),
    "cdx_gpis_joint": (C.c_int, [C.POINTER(CdxGpis), _P, _I64, _P, _P, _P]),
    "cdx_gpis_screen_bytes": (C.c_size_t, [C.c_int32]),
    "cdx_gpis_screen_prepare": (C.c_int, [C.POINTER(CdxGpis), _P, _P]),
    "cdx_gpis_screen_set_bands": (C.c_int, [C.POINTER(CdxGpis), C.POINTER(C.c_double), _P]),
    "cdx_gpis_screen_info": (C.c_int, [C.POINTER(CdxGpis), C.POINTER(C.c_double), _P]),
    "cdx_gpis_screen_workspace": (C.c_size_t, [C.POINTER(CdxGpis), _I64]),
    "cdx_gpis_screen_var": (C.c_int, [C.POINTER(CdxGpis), _P, _I64, _P, _P, _P]),
    "cdx_gpis_field_workspace": (C.c_size_t, [C.POINTER(CdxGpis), C.c_int32, _I64]),
    "cdx_gpis_field": (C.c_int, [C.POINTER(CdxGpis), _P, _P, _P, C.c_int32, _I64, _P, _P, _P, _P, _P]),
    "cdx_gpis_field_points": (C.c_int, [_P, _P, _P, C.c_int32, _P, _I64, _P, _P]),
    "cdx_gpis_surface_workspace": (C.c_size_t, [C.c_int32]),
    "cdx_gpis_surface_count": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "cdx_gpis_surface_place": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _I64, _P, _P, _P,
                                         _P]),
    "cdx_gpis_mesh_workspace": (C.c_size_t, [C.c_int32]),
    "cdx_gpis_mesh_count": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    "cdx_gpis_mesh_place": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _I64, _I64, _P, _P, _P, _P]),
    "cdx_gpis_mesh_refine_init": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _I64, _P, _P, _P]),
    "cdx_gpis_mesh_refine_step": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _I64, _P, _P, _P]),
    "cdx_fps_capacity": (_I64, []),
    "cdx_fps_workspace": (C.c_size_t, [_I64, _I64, C.c_int32]),
    "cdx_fps": (C.c_int, [_P, C.c_int32, _I64, _I64, _I64, _I64, C.c_int32, _P, _P, _P, _P, _P]),
    "cdx_knn_auto_rows": (_I64, []),
    "cdx_knn_grid_bytes": (C.c_size_t, [_I64]),
    "cdx_knn_prepare": (C.c_int, [_P, C.c_int32, _I64, _P, _P]),
    "cdx_knn_workspace": (C.c_size_t, [_I64, _I64, _I64, C.c_int32]),
    "cdx_knn": (C.c_int, [_P, C.c_int32, _I64, _P, _P, _I64, _I64, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    "cdx_cloud_normals": (C.c_int, [_P, C.c_int32, _I64, _P, _P, _I64, C.POINTER(C.c_double), _P, _P, _P]),
    "cdx_sample_scan_faces": (_I64, []),
    "cdx_sample_table_capacity": (_I64, []),
    "cdx_sample_prepare_workspace": (C.c_size_t, [_I64]),
    "cdx_sample_prepare": (C.c_int, [_P, C.c_int32, _I64, _P, _P, _P, _P]),
    "cdx_sample_draw": (C.c_int, [_P, C.c_int32, _I64, _P, C.c_uint64, C.c_uint64, _I64, C.c_int32, _P, _P, _P, _P,
                                  _P]),
    "cdx_gpis_fit": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_double, _P, _P, _P]),
    "cdx_gpis_factor_workspace": (C.c_size_t, [C.c_int32]),
    "cdx_gpis_factor": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "cdx_fk_forward": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, _P, _P]),
    "cdx_fk_backward": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, _P, _P]),
    "cdx_fk_jacobian": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, _P, _P]),
    "cdx_ik_workspace": (C.c_size_t, [_I64, C.c_int32, C.c_int32]),
    "cdx_ik_rows_per_block": (C.c_int32, [C.c_int32, C.c_int32]),
    "cdx_ik_abi_size": (C.c_size_t, []),
    "cdx_ik_solve": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxIkParams), _I64, _P, C.c_int32, _P, _P,
                               C.POINTER(C.c_double), _P, _P, _P, _P, _P, _P, _P]),
    "cdx_ik_solve_pose": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxIkParams), _I64, _P, C.c_int32, _P, _P, _P,
                                    C.POINTER(C.c_double)] + [_P] * 9),
    "cdx_ik_pose_rows_per_block": (C.c_int32, [C.c_int32, C.c_int32]),
    "cdx_ik_solve_frames": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxIkParams), _I64, _P, C.c_int32, _P, _P, _P,
                                      C.POINTER(C.c_double), _P, _P, C.c_uint64, C.c_uint64] + [_P] * 7),
    "cdx_ik_frames_rows_per_block": (C.c_int32, [C.c_int32, C.c_int32, C.c_uint64]),
    "cdx_dyn_inverse": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, _P, _P] + [C.c_int32] * 3 + [_P, C.c_int32, _P, _P, _P]),
    "cdx_dyn_inertia": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, C.c_int32, _P, _P]),
    "cdx_dyn_forward": (C.c_int, [C.POINTER(CdxChain), _P, _I64, _P, _P, _P] + [C.c_int32] * 3 + [_P, C.c_int32, _P, _P]),
    "cdx_dyn_rows_per_block": (C.c_int32, [C.c_int32] * 3),
    "cdx_dyn_abi_size": (C.c_size_t, []),
    "cdx_min_wrench": (C.c_int, [C.POINTER(CdxWrenchParams), _I64] + [_P] * 11),
    "cdx_wrench_rows_per_block": (C.c_int32, [C.c_int32]),
    "cdx_wrench_abi_size": (C.c_size_t, []),
    "cdx_grasp_equilibrium": (C.c_int, [C.POINTER(CdxEquilParams), _I64, _I64] + [_P] * 6 + [C.c_int32] + [_P] * 11),
    "cdx_equil_reduce": (C.c_int, [C.POINTER(CdxEquilLimits), _I64, _I64, C.c_int32] + [_P] * 14),
    "cdx_equil_abi_sizes": (None, [C.POINTER(C.c_size_t)]),
    "cdx_hand_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cdx_hand_abi_sizes": (None, [C.POINTER(C.c_size_t)]),
    "cdx_hand_prepare": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.POINTER(CdxHand), _P]),
    "cdx_hand_spheres": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxHand), _I64, _P, _P, _P, _P, _P, _P]),
    "cdx_hand_cost": (C.c_int, [C.POINTER(CdxHand), C.POINTER(CdxHandParams), _I64] + [_P] * 8),
    "cdx_hand_pullback": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxHand), _I64] + [_P] * 7),
    "cdx_hand_term": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxHand), C.POINTER(CdxHandParams), _I64] + [_P] * 5 +
                      [C.c_double, C.c_int32] + [_P] * 7),
    "cdx_traj_seed": (C.c_int, [_I64, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_double, C.c_uint64, _P, _P]),
    "cdx_traj_step": (C.c_int, [C.POINTER(CdxTrajParams), _I64, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "cdx_traj_abi_sizes": (None, [C.POINTER(C.c_size_t)]),
    "cdx_force_eq_forward": (C.c_int, [C.POINTER(CdxForceEq), _I64, _P, _P, _P, _P, _P, C.c_uint64, _P, _P, _P, _P,
                                       _P]),
    "cdx_force_eq_backward": (C.c_int, [C.POINTER(CdxForceEq), _I64, _P, _P, _P, _P, _P, C.c_uint64, _P, _P, _P, _P,
                                        _P, _P]),
    "cdx_collision_loss": (C.c_int, [C.POINTER(CdxCollision), _I64, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "cdx_closure_workspace": (C.c_size_t, [C.POINTER(CdxProblem), _I64]),
    "cdx_closure_screen_stats": (C.c_int, [C.POINTER(CdxProblem), _I64, _P, C.POINTER(C.c_int32)]),
    "cdx_closure_screen_report": (C.c_int, [C.POINTER(CdxProblem), _I64, _P, C.POINTER(CdxScreenReport), _P]),
    "cdx_closure_screen_reset": (C.c_int, [C.POINTER(CdxProblem), _I64, _P, _P]),
    "cdx_debug_fail_next_closure": (C.c_int, [C.c_int32]),
    "cdx_closure": (C.c_int, [C.POINTER(CdxProblem), _I64, _P, _P, _P, _P, _P, _P, C.c_uint64, _P,
                              _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cdx_pack_survivors": (C.c_int, [_I64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_double, C.c_double,
                                     _I64, _I64, _P, _P]),
    "cdx_sdf_forward": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "cdx_sdf_backward": (C.c_int, [_P, _P, _P, _I64, _P, _P]),
    "cdx_sdf_forward_f64": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "cdx_sdf_backward_f64": (C.c_int, [_P, _P, _P, _I64, _P, _P]),
    "cdx_sdf_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64), _P]),
    "cdx_sdf_chunk_visits": (C.c_int, [C.POINTER(C.c_uint64), _P]),
    "cdx_kin_cost": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxKinParams), _I64] + [_P] * 14 + [C.c_uint64] +
                     [_P] * 8),
    "cdx_sdf_mesh_bytes": (C.c_size_t, [_I64]),
    "cdx_sdf_mesh_prepare": (C.c_int, [_P, _I64, _P, _P]),
    "cdx_sdf_query_workspace": (C.c_size_t, [_I64]),
    "cdx_sdf_query_order": (C.c_int, [_P, _I64, _P, C.c_size_t, _P]),
    "cdx_sdf_batch_schedule_bytes": (C.c_size_t, [C.c_int32, _P]),
    "cdx_sdf_query_batch": (C.c_int, [C.c_int32, _P, _P, C.c_size_t, _P]),
    "cdx_sdf_query": (C.c_int, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_int32, _P]),
    "cdx_sdf_mesh_flags": (C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    "cdx_ray_mesh_bytes": (C.c_size_t, [_I64]),
    "cdx_ray_mesh_prepare": (C.c_int, [_P, _I64, _P, _P]),
    "cdx_ray_cast": (C.c_int, [_P, _P, _P, _I64, _P, _P, _I64, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P]),
    "cdx_depth_render": (C.c_int, [_P, _P, _P, _I64, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int32, _P, _P, _P]),
    "cdx_depth_workspace": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "cdx_depth_count": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                  _P, _P, _P]),
    "cdx_depth_place": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_double,
                                  C.c_double, C.c_double, C.POINTER(C.c_double), _P, _I64, _P, _P]),
    "cdx_ray_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64), _P]),
    "cdx_version": (C.c_char_p, []),
    "cdx_abi_sizes": (None, [C.POINTER(C.c_size_t)]),
    "cdx_selftest_mfma_f64": (C.c_int, [_P, _P, _P, _P]),
    "cdx_profile_enable": (C.c_int, [C.c_int]),
    "cdx_optimizer_step": (C.c_int, [C.POINTER(CdxAdam), C.POINTER(CdxOptBuffers), _I64, C.c_int32, C.c_int32,
                                     C.c_int32, _P]),
    "cdx_profile_read": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "cdx_kin_step": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxKinOpt), C.POINTER(CdxKinOptBuffers), _I64, C.c_int32,
                               C.c_int32, C.c_int32, _P]),
    "cdx_kin_fk_state_bytes": (_I64, [_I64, C.c_int32]),
    "cdx_kin_iteration": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxKinParams), C.POINTER(CdxKinOpt),
                                    C.POINTER(CdxKinOptBuffers), _I64, C.c_int32] + [_P] * 10 +
                          [C.c_uint64, C.c_int32, _P]),
    "cdx_gpis_mode_cost": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxGpisModeParams), C.POINTER(CdxGpisModeBuffers),
                                     _I64, C.c_int32, _P, C.c_uint64, C.c_int32, _P]),
    "cdx_gpis_mode_step": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxGpisModeParams), C.POINTER(CdxGpisModeOpt),
                                     C.POINTER(CdxGpisModeBuffers), _I64, C.c_int32, C.c_int32, C.c_int32, _P]),
    "cdx_gpis_mode_iteration": (C.c_int, [C.POINTER(CdxChain), C.POINTER(CdxGpisModeParams), C.POINTER(CdxGpisModeOpt),
                                          C.POINTER(CdxGpisModeBuffers), _I64, C.c_int32, _P, C.c_uint64, C.c_int32,
                                          _P]),
    "cdx_gpis_mode_abi_sizes": (None, [C.POINTER(C.c_size_t)]),
}

# (getter, the structs it reports in its order, label of the group): load() holds every layout to the library's sizeof
_ABI_SIZES = [
    ("cdx_abi_sizes", [CdxGpis, CdxBody, CdxChain, CdxProblem, CdxCollision, CdxAdam, CdxOptBuffers, CdxForceEq,
                       CdxScreenReport, CdxKinParams, CdxKinOpt, CdxKinOptBuffers, CdxSdfBatchQuery], "core"),
    ("cdx_gpis_mode_abi_sizes", [CdxGpisModeParams, CdxGpisModeOpt, CdxGpisModeBuffers], "GPIS mode"),
    ("cdx_ik_abi_size", [CdxIkParams], "IK"),
    ("cdx_dyn_abi_size", [CdxDyn], "dynamics"),
    ("cdx_wrench_abi_size", [CdxWrenchParams], "wrench"),
    ("cdx_equil_abi_sizes", [CdxEquilParams, CdxEquilLimits], "equilibrium"),
    ("cdx_hand_abi_sizes", [CdxHand, CdxHandParams], "hand"),
    ("cdx_traj_abi_sizes", [CdxTrajParams], "trajectory"),
]

_lib = None
_lock = threading.Lock()


def lib_path():
    return os.environ.get("CDX_LIB", os.path.join(LIB_DIR, "libcdx.so"))


def load():
    """Loads libcdx.so (raises ImportError if it is missing — there is no fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(f"compliancedex_amd native library not built: {path} "
                              "(run `python -m compliancedex_amd.build`)")
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for getter, structs, label in _ABI_SIZES:
            fn = getattr(lib, getter)
            if fn.argtypes:  # fills an array, one size per struct
                sizes = (C.c_size_t * len(structs))()
                fn(sizes)
                theirs = list(sizes)
            else:  # returns the size of its one struct
                theirs = [fn()]
            mine = [C.sizeof(s) for s in structs]
            if theirs != mine:
                raise ImportError(f"ABI struct size mismatch ({label}): library {theirs} vs binding {mine}")
        info = build_info()
        if not info["matches"] and "CDX_LIB" not in os.environ:
            import warnings
            warnings.warn(f"{path} was not built from this tree's csrc/ (stamp {info['lib_sha16']}, sources "
                          f"{info['src_sha16']}): rebuild with `python -m compliancedex_amd.build`")
        _lib = lib
        return lib


def build_info():
    """Source digest of the tree vs the one libcdx.so was built from (build.stamp_info)."""
    from .build import stamp_info
    return stamp_info(lib_path())


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {ERRORS.get(rc, rc)} (code {rc})")


def ptr(t):
    """Device pointer of a (contiguous) tensor, or None."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def stream_ptr(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream
