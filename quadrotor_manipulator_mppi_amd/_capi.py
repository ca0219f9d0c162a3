"""ctypes binding of ``include/mppi_hip.h`` (libmppi_hip.so).

This is the reference-side binding a maintainer would add: the
structs mirror the header field by field and every prototype is declared so
ctypes checks argument types.  There is NO fallback: if the library is missing
or cannot be loaded, :func:`lib` raises, and nothing in this package computes
the control step on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPPI_HIP_LIB", os.path.join(PKG, "lib", "libmppi_hip.so"))

MAX_ACTION, MAX_JOINTS, MAX_HORIZON, MAX_SAVGOL = 16, 16, 256, 31
MODEL_DRONE, MODEL_ARM, MODEL_WHOLEBODY, MODEL_QUADROTOR, MODEL_AERIAL = 0, 1, 2, 3, 4
NOISE_PHILOX, NOISE_INJECTED = 0, 1
JOINT_FIXED, JOINT_REVOLUTE, JOINT_PRISMATIC, JOINT_FLOATING = 0, 1, 2, 3
OK, ERR_INVALID_ARG, ERR_HIP, ERR_NONFINITE, ERR_STATE, ERR_COMM, ERR_PEER_TIMEOUT = 0, -1, -2, -3, -4, -5, -6
COST_COVAR, COST_CENTER, COST_JOINT_TRACK, COST_ACTION, COST_JOINT_LIMIT = 1, 2, 4, 8, 16
COST_TARGET_TRACK = 32   # the pose target moves along the horizon (mppi_set_target_trajectory)
ABI_VERSION = 10
MAX_PEERS = 8
MAX_ELITES = 64
MAX_OBSTACLES = 16
MAX_BODY_SPHERES = 16
COMM_ID_BYTES = 128
PEER_HANDLE_BYTES = 64


class Joint(C.Structure):
    _fields_ = [("type", C.c_int32), ("q_index", C.c_int32), ("xyz", C.c_float * 3),
                ("rpy", C.c_float * 3), ("axis", C.c_float * 3), ("has_axis", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_vehicles", C.c_int32), ("n_samples", C.c_int32),
                ("n_horizon", C.c_int32), ("n_action", C.c_int32),
                ("dt", C.c_double), ("lambda_", C.c_double),
                ("sigma", C.c_float * (MAX_ACTION * MAX_ACTION)),
                ("w_stage_pos", C.c_float), ("w_stage_ori", C.c_float),
                ("w_term_pos", C.c_float), ("w_term_ori", C.c_float),
                ("n_joints", C.c_int32), ("joints", Joint * MAX_JOINTS),
                ("savgol_window", C.c_int32), ("savgol_order", C.c_int32),
                ("noise_mode", C.c_int32), ("seed", C.c_uint64), ("device", C.c_int32),
                ("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("state_f64", C.c_int32),
                ("store_trajectory", C.c_int32), ("store_noise", C.c_int32),
                ("check_reach", C.c_int32), ("reach_tol", C.c_float),
                ("blocks_per_vehicle", C.c_int32), ("block_threads", C.c_int32),
                ("cost_terms", C.c_int32), ("w_covar", C.c_float), ("cost_alpha", C.c_float),
                ("cost_gamma", C.c_float), ("w_center", C.c_float), ("w_joint_track", C.c_float),
                ("w_action", C.c_float), ("joint_limit_penalty", C.c_float),
                ("q_center", C.c_float * MAX_JOINTS), ("q_lower", C.c_float * MAX_JOINTS),
                ("q_upper", C.c_float * MAX_JOINTS),
                ("quad_mass", C.c_float), ("quad_inertia", C.c_float * 3), ("quad_kd", C.c_float),
                ("quad_gravity", C.c_float), ("quad_literal_jinv", C.c_int32),
                ("vehicle_offset", C.c_int32)]


class BodySphere(C.Structure):
    _fields_ = [("frame", C.c_int32), ("offset", C.c_float * 3), ("radius", C.c_float)]


class Scene(C.Structure):
    _fields_ = [("n_body", C.c_int32), ("body", BodySphere * MAX_BODY_SPHERES),
                ("w_obs", C.c_float), ("margin", C.c_float), ("penalty", C.c_float)]


FIELD_MAX_VOXELS = 1 << 21


class FieldDesc(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("voxel", C.c_float), ("origin", C.c_float * 3), ("reserved", C.c_int32)]


DEPTH_MAX_PIXELS = 1 << 20
DEPTH_MAX_SAMPLES = 16384


class DepthViewC(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("carve", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("z_min", C.c_float), ("z_max", C.c_float), ("pos", C.c_float * 3), ("quat_xyzw", C.c_float * 4),
                ("reserved", C.c_int32 * 3)]


MAX_SELF_PAIRS = 32


class SelfCollision(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("pair", (C.c_int32 * 2) * MAX_SELF_PAIRS),
                ("w_self", C.c_float), ("margin", C.c_float), ("penalty", C.c_float), ("reserved", C.c_int32)]


class Limits(C.Structure):
    _fields_ = [("lo", C.c_float * 4), ("hi", C.c_float * 4)]   # thrust, tau_x, tau_y, tau_z


class Link(C.Structure):
    _fields_ = [("parent", C.c_int32), ("type", C.c_int32), ("xyz", C.c_double * 3), ("rpy", C.c_double * 3),
                ("axis", C.c_double * 3), ("mass", C.c_double), ("com", C.c_double * 3),
                ("inertia", C.c_double * 9)]


class Stats(C.Structure):
    _fields_ = [("rho", C.c_float), ("eta", C.c_float), ("ess", C.c_float),
                ("nonfinite", C.c_int32), ("reach", C.c_int32), ("_pad", C.c_int32)]


_P = C.c_void_p
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_U32 = C.POINTER(C.c_uint32)
_I32 = C.POINTER(C.c_int32)
_I64 = C.POINTER(C.c_int64)
_CFG = C.POINTER(Config)
_ST = C.c_int32

# name -> (restype, argtypes); exactly the functions include/mppi_hip.h declares
PROTOTYPES = {
    "mppi_abi_version": (C.c_int32, []),
    "mppi_last_error": (C.c_char_p, []),
    "mppi_struct_sizes": (None, [_I32, _I32, _I32]),
    "mppi_config_default": (None, [_CFG, C.c_int32]),
    "mppi_state_dim": (C.c_int32, [_CFG]),
    "mppi_output_dim": (C.c_int32, [_CFG]),
    "mppi_traj_channels": (C.c_int32, [_CFG]),
    "mppi_create": (_ST, [_CFG, C.POINTER(_P)]),
    "mppi_destroy": (None, [_P]),
    "mppi_set_stream": (_ST, [_P, _P]),
    "mppi_set_joint_trajectory": (_ST, [_P, C.c_int32, _F]),
    "mppi_set_target": (_ST, [_P, C.c_int32, _F, _F]),
    "mppi_set_target_trajectory": (_ST, [_P, C.c_int32, _F, _F]),
    "mppi_set_u_prev": (_ST, [_P, _F]),
    "mppi_get_u_prev": (_ST, [_P, _F]),
    "mppi_set_state": (_ST, [_P, _D]),
    "mppi_set_step_counter": (_ST, [_P, C.c_uint32]),
    "mppi_get_step_counter": (_ST, [_P, _U32]),
    "mppi_exchange_slot_floats": (_ST, [_P, _I64]),
    "mppi_bind_exchange": (_ST, [_P, _P]),
    "mppi_rollout": (_ST, [_P, _P]),
    "mppi_finalize": (_ST, [_P]),
    "mppi_comm_unique_id": (_ST, [C.POINTER(C.c_uint8)]),
    "mppi_comm_available": (_ST, []),
    "mppi_comm_init": (_ST, [_P, C.POINTER(C.c_uint8)]),
    "mppi_comm_init_ex": (_ST, [_P, C.POINTER(C.c_uint8), C.c_int32]),
    "mppi_peer_open": (_ST, [_P, C.POINTER(C.c_uint8)]),
    "mppi_peer_connect": (_ST, [_P, C.POINTER(C.c_uint8)]),
    "mppi_peer_probe": (_ST, [_P, C.c_int32]),
    "mppi_peer_region": (_ST, [_P, C.POINTER(C.c_uint64)]),
    "mppi_peer_connect_ptrs": (_ST, [_P, C.POINTER(C.c_uint64)]),
    "mppi_peer_status": (_ST, [_P, _U32, C.POINTER(C.c_uint64), _U32]),
    "mppi_peer_reset": (_ST, [_P, C.c_uint32, C.c_uint32]),
    "mppi_peer_info": (_ST, [_P, _I32, _I32, _U32]),
    "mppi_comm_info": (_ST, [_P, _I32, _I32]),
    "mppi_exchange": (_ST, [_P]),
    "mppi_read_outputs": (_ST, [_P, _D, _F, C.POINTER(Stats)]),
    "mppi_step": (_ST, [_P, _D, _F, _D, _F, C.POINTER(Stats)]),
    "mppi_run_steps": (_ST, [_P, C.c_int32]),
    "mppi_dispatch_info": (_ST, [_P, C.c_char_p, C.c_int32]),
    "mppi_kernel_info": (_ST, [_P, C.c_char_p, C.c_int32]),
    "mppi_synchronize": (_ST, [_P]),
    "mppi_set_prewarm": (_ST, [_P, C.c_int32]),
    "mppi_get_prewarm": (_ST, [_P, _I32, C.POINTER(C.c_int64)]),
    "mppi_get_costs": (_ST, [_P, _F]),
    "mppi_get_weights": (_ST, [_P, _F]),
    "mppi_get_noise": (_ST, [_P, _F]),
    "mppi_get_trajectory": (_ST, [_P, _F]),
    "mppi_get_weighted_noise": (_ST, [_P, _F, _F]),
    "mppi_get_plan": (_ST, [_P, _F, _F, _F, _F]),
    "mppi_get_elites": (_ST, [_P, C.c_int32, _I32, _F, _F, _F]),
    "mppi_scene_default": (None, [C.POINTER(Scene), _CFG]),
    "mppi_create_scene": (_ST, [_CFG, C.POINTER(Scene), C.POINTER(_P)]),
    "mppi_set_obstacles": (_ST, [_P, C.c_int32, C.c_int32, _F, _F, _F]),
    "mppi_get_clearances": (_ST, [_P, _F]),
    "mppi_get_plan_clearance": (_ST, [_P, _F]),
    "mppi_create_scene_field": (_ST, [_CFG, C.POINTER(Scene), C.POINTER(FieldDesc), C.POINTER(_P)]),
    "mppi_set_distance_field": (_ST, [_P, _F, _F]),
    "mppi_set_occupancy": (_ST, [_P, _F, C.POINTER(C.c_uint8), C.c_float]),
    "mppi_get_distance_field": (_ST, [_P, _I32, _F, _F]),
    "mppi_occupancy_field": (_ST, [C.POINTER(FieldDesc), C.POINTER(C.c_uint8), C.c_float, _F]),
    "mppi_integrate_depth": (_ST, [_P, C.POINTER(DepthViewC), _F, C.c_float]),
    "mppi_shift_map": (_ST, [_P, _I32, C.c_float]),
    "mppi_get_occupancy": (_ST, [_P, C.POINTER(C.c_uint8)]),
    "mppi_depth_integrate_host": (_ST, [C.POINTER(FieldDesc), C.POINTER(DepthViewC), _F, C.POINTER(C.c_uint8)]),
    "mppi_self_collision_default": (None, [C.POINTER(SelfCollision), _CFG, C.POINTER(Scene)]),
    "mppi_create_scene_self": (_ST, [_CFG, C.POINTER(Scene), C.POINTER(FieldDesc), C.POINTER(SelfCollision), C.POINTER(_P)]),
    "mppi_get_self_clearances": (_ST, [_P, _F]),
    "mppi_get_plan_self_clearance": (_ST, [_P, _F]),
    "mppi_limits_default": (None, [C.POINTER(Limits), _CFG]),
    "mppi_create_limits": (_ST, [_CFG, C.POINTER(Limits), C.POINTER(_P)]),
    "mppi_set_limits": (_ST, [_P, C.POINTER(Limits)]),
    "mppi_get_limits": (_ST, [_P, _I32, C.POINTER(Limits)]),
    "mppi_limits_apply": (_ST, [C.POINTER(Limits), _F, _F, C.c_int32, C.c_int32, _F, _F]),
    "mppi_enable_timing": (_ST, [_P, C.c_int32]),
    "mppi_get_timing": (_ST, [_P, _D, _D, _I64, _I64]),
    "mppi_kernel_timing": (_ST, [_P, C.c_int32, _D, _D]),
    "mppi_kernel_timing_ex": (_ST, [_P, C.c_int32, _D, _D, _D]),
    "mppi_exchange_timing": (_ST, [_P, C.c_int32, _D]),
    "mppi_rollout_bytes": (C.c_int64, [_CFG]),
    "mppi_joint_origin": (None, [C.POINTER(Joint), _F]),
    "mppi_base_transform": (None, [_D, C.c_int32, _F]),
    "mppi_target_rotation": (None, [_F, _F]),
    "mppi_savgol_coefficients": (C.c_int32, [C.c_int32, C.c_int32, _F]),
    "mppi_host_fk": (_ST, [C.POINTER(Joint), C.c_int32, _D, _D, C.c_int32, _F]),
    "mppi_dyn_create": (_ST, [C.POINTER(Link), C.c_int32, C.c_double, C.POINTER(_P)]),
    "mppi_dyn_destroy": (None, [_P]),
    "mppi_dyn_dims": (None, [_P, _I32, _I32, _I32]),
    "mppi_dyn_rnea": (_ST, [_P, _D, _D, _D, _D]),
    "mppi_dyn_terms": (_ST, [_P, _D, _D, _D, _D]),
    "mppi_computed_torque": (_ST, [_P, _D, _D, _D, C.c_double, C.c_double, C.c_int32, _D]),
    "mppi_philox_words": (C.c_int32, [C.c_int32]),
    "mppi_philox_normals": (_ST, [C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, _F, _U32]),
}

# diagnostics entry points that are not in the header (csrc/mppi_debug.cpp); their users bind them
DEBUG_PROTOTYPES = {
    "mppi_debug_step_launches": (C.c_int32, [_CFG, _I32, C.c_char_p, C.c_int32]),
    "mppi_debug_scene_step_launches": (C.c_int32, [_CFG, C.POINTER(Scene), _I32, C.c_char_p, C.c_int32]),
    "mppi_debug_scene_rollout_kernels": (C.c_int32, [_I32, C.c_char_p, C.c_char_p, C.c_int32]),
    "mppi_debug_scene_layout": (C.c_int32, [_CFG, C.POINTER(Scene), _F, _I32]),
    "mppi_debug_obstacles": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F]),
    "mppi_debug_field_layout": (C.c_int32, [_CFG, C.POINTER(FieldDesc), _F, _F, _F]),
    "mppi_debug_field_sample": (C.c_int32, [_F, C.c_int32, _F, _F, _I32]),
    "mppi_debug_field_step_launches": (C.c_int32, [_CFG, C.POINTER(Scene), C.POINTER(FieldDesc), _I32, C.c_char_p,
                                                   C.c_int32, C.POINTER(C.c_uint64)]),
    "mppi_debug_field_rollout_kernels": (C.c_int32, [_I32, C.c_char_p, C.c_char_p, C.c_int32]),
    "mppi_debug_self_layout": (C.c_int32, [_CFG, C.POINTER(Scene), C.POINTER(SelfCollision), _F, _F, _I32]),
    "mppi_debug_self_step_launches": (C.c_int32, [_CFG, C.POINTER(Scene), C.POINTER(FieldDesc), C.POINTER(SelfCollision), _I32,
                                                  C.c_char_p, C.c_int32]),
    "mppi_debug_self_rollout_kernels": (C.c_int32, [_I32, C.c_char_p, C.c_char_p, C.c_int32]),
    "mppi_debug_limits_step_launches": (C.c_int32, [_CFG, C.POINTER(Limits), _I32, C.c_char_p, C.c_int32]),
    "mppi_debug_limits_plan_kernel": (C.c_int32, [_I32, C.c_char_p, C.c_int32]),
    "mppi_debug_limits_set": (C.c_int32, [_CFG, C.c_int32, C.POINTER(Limits)]),
    "mppi_debug_edt_kernels": (C.c_int32, [_I32, C.c_char_p, C.c_int32]),
    "mppi_debug_field_words": (C.c_int32, [_P, _F]),
    "mppi_debug_depth_validate": (C.c_int32, [C.POINTER(FieldDesc), C.POINTER(DepthViewC), C.c_float]),
    "mppi_debug_map_shift": (C.c_int32, [C.POINTER(FieldDesc), _I32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _F]),
}

_lib = None
_lock = threading.Lock()


class MPPIError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"[mppi status {status}] {msg}")
        self.status = status


class PeerTimeout(MPPIError):
    """MPPI_ERR_PEER_TIMEOUT: a peer-exchange step was given up since the last reset (the engine
    still works; every rank holds its warm start until ShardedEngine.resync / mppi_peer_reset)."""


def lib():
    """Load libmppi_hip.so (once).  Raises if it is missing -- no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libmppi_hip.so not found at {LIB_PATH}: build it with "
                               "`python -m quadrotor_manipulator_mppi_amd.build` (hipcc, gfx950). "
                               "There is no CPU fallback for the MPPI control step.")
        try:   # share torch's HIP runtime instance when torch is present
            import torch  # noqa: F401
        except ImportError:
            pass
        h = C.CDLL(LIB_PATH)
        # MPPI_CAPI_LENIENT=1: tolerate entry points an older build lacks (same-box A/B of
        # library builds in tools/ only; the shipped binding requires every one)
        lenient = os.environ.get("MPPI_CAPI_LENIENT") == "1"
        for name, (res, args) in PROTOTYPES.items():
            if lenient and not hasattr(h, name):
                continue
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        sizes = [C.c_int32(), C.c_int32(), C.c_int32()]
        h.mppi_struct_sizes(*[C.byref(s) for s in sizes])
        got = (sizes[0].value, sizes[1].value, sizes[2].value)
        want = (C.sizeof(Config), C.sizeof(Joint), C.sizeof(Stats))
        if got != want:
            raise RuntimeError(f"mppi_hip ABI layout mismatch: library {got} vs binding {want}")
        if h.mppi_abi_version() != ABI_VERSION:
            raise RuntimeError("mppi_hip ABI version mismatch")
        _lib = h
        return h


def check(status: int, what: str = "") -> None:
    if status != OK:
        msg = lib().mppi_last_error().decode(errors="replace")
        raise (PeerTimeout if status == ERR_PEER_TIMEOUT else MPPIError)(status, f"{what}: {msg}" if what else msg)


def fptr(a):
    """float* of a contiguous float32 numpy array (or None)."""
    return None if a is None else a.ctypes.data_as(_F)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_D)
