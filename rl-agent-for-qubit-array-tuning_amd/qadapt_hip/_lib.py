"""ctypes binding of libqdsim.so (include/qdsim.h).  There is NO fallback: if the
library is missing or a call fails, an exception is raised."""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
LIB_PATH = os.environ.get("QDSIM_LIB", os.path.join(CSRC, "libqdsim.so"))   # QDSIM_LIB: diagnostic builds

QD_FLAG_VALIDATE = 1
QD_FLAG_PIXEL_SEARCH = 2
QD_FLAG_GS_GERSHGORIN_ZERO = 8
QD_NOISE_SENSOR = 1
QD_NOISE_RADIAL = 2
QD_NOISE_LATCH = 4
QD_MAP_GLOBAL, QD_MAP_PER_SCAN = 0, 1
QD_POINTS_SLOTS = 64
QD_LINE_SLOTS = 4096
QD_GRID_SLOTS = 4096
QD_LEVELS_MAX = 8
QD_SCAN_VIRTUAL, QD_SCAN_PHYSICAL = 0, 1
QD_ERR_ARG, QD_ERR_HIP, QD_ERR_STATE = 1, 2, 3

EXPORTS = [
    "qd_param_block_doubles", "qd_state_block_doubles", "qd_layout_query", "qd_create", "qd_destroy",
    "qd_last_error", "qd_bind_outputs", "qd_load_episodes", "qd_apply_actions", "qd_observe",
    "qd_update_capacitance", "qd_step", "qd_snapshot", "qd_get_state", "qd_set_state", "qd_get_raw",
    "qd_get_occupations", "qd_get_candidates", "qd_get_eigen", "qd_get_search_stats", "qd_get_solver_stats", "qd_get_rng_state", "qd_set_rng_state",
    "qd_time_ground_kernel", "qd_time_candidates_kernel", "qd_time_kernels", "qd_timed_kernel_name", "qd_chunk_envs",
    "qd_probe", "qd_probe_compose", "qd_time_select", "qd_eval_points", "qd_probe_ex", "qd_scan_affine",
    "qd_scan_grid", "qd_eval_points_closed", "qd_scan_grid_closed", "qd_eval_points_ex",
    "qd_eval_points_thermal", "qd_scan_grid_thermal", "qd_scan_grid_levels", "qd_eval_points_response",
    "qd_scan_grid_response",
]
# exported too, kept apart: names with a digit, which a scan of qdsim.h for `qd_[a-z_]+(` does not find
EXPORTS_WITH_DIGITS = ["qd_scan2d", "qd_scan1d"]

QD_CURVES = {"constant": 0, "polynomial": 1, "exponential": 2, "linear": 3}
QD_UPDATE_KALMAN, QD_UPDATE_DIRECT = 0, 1


class QdConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n_dot", ctypes.c_int32), ("resolution", ctypes.c_int32),
        ("batch", ctypes.c_int32), ("max_steps", ctypes.c_int32), ("env_chunk", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("noise_flags", ctypes.c_int32),
        ("gate_ramp_start", ctypes.c_double), ("gate_quadratic_start", ctypes.c_double),
        ("barrier_ramp_start", ctypes.c_double), ("kalman_prior_mean", ctypes.c_double),
        ("kalman_prior_variance", ctypes.c_double), ("kalman_prior_mean_nnn", ctypes.c_double),
        ("kalman_variance_threshold", ctypes.c_double), ("kalman_process_noise", ctypes.c_double),
        ("rng_seed", ctypes.c_uint64), ("env_id_offset", ctypes.c_int64),
        ("use_deltas", ctypes.c_int32), ("sparse_reward", ctypes.c_int32), ("gate_curve_type", ctypes.c_int32),
        ("update_method", ctypes.c_int32), ("cnn_outputs", ctypes.c_int32), ("num_charge_states", ctypes.c_int32),
        ("delta_max", ctypes.c_double), ("gate_curve_exponent", ctypes.c_double),
        ("plunger_radius", ctypes.c_double), ("outer_plunger_radius", ctypes.c_double),
        ("outer_plunger_reward_max", ctypes.c_double), ("barrier_radius", ctypes.c_double),
    ]


class QdProbeOpts(ctypes.Structure):
    """qd_probe_opts of include/qdsim.h: the stochastic stages, Philox serial and stream base of a qd_probe_ex call and the
    device destination of its occupations."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("noise_flags", ctypes.c_int32), ("serial", ctypes.c_uint64),
        ("stream_base", ctypes.c_int64), ("occ_dst", ctypes.c_void_p),
    ]


class QdScanOpts(ctypes.Structure):
    """qd_scan_opts of include/qdsim.h: frame, stochastic stages, Philox serial and stream base of a qd_scan2d call, the
    per-query virtual gate matrices and peak widths, and the device destination of its occupations."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("frame", ctypes.c_int32), ("noise_flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("serial", ctypes.c_uint64), ("stream_base", ctypes.c_int64),
        ("vgm_dev", ctypes.c_void_p), ("gamma_dev", ctypes.c_void_p), ("occ_dst", ctypes.c_void_p),
    ]


class QdScanAffineOpts(ctypes.Structure):
    """qd_scan_affine_opts of include/qdsim.h: the fields of qd_scan_opts for a qd_scan_affine call."""
    _fields_ = list(QdScanOpts._fields_)


class QdScan1dOpts(ctypes.Structure):
    """qd_scan1d_opts of include/qdsim.h: the fields of qd_scan_opts for a qd_scan1d call (occ_dst is [nq][n][N])."""
    _fields_ = list(QdScanOpts._fields_)


class QdScanGridOpts(ctypes.Structure):
    """qd_scan_grid_opts of include/qdsim.h: the fields of qd_scan_opts for a qd_scan_grid call (occ_dst is [nq][ny][nx][N])."""
    _fields_ = list(QdScanOpts._fields_)


class QdPointsOpts(ctypes.Structure):
    """qd_points_opts of include/qdsim.h: the number of energy levels per point of a qd_eval_points_ex call, the peak widths and
    (closed regime) total charges of its groups on the host, and the device destinations of kept states, levels and norms."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("gamma_host", ctypes.POINTER(ctypes.c_double)),
        ("n_charge_host", ctypes.POINTER(ctypes.c_int32)), ("states_dst", ctypes.c_void_p),
        ("levels_dst", ctypes.c_void_p), ("hnorm_dst", ctypes.c_void_p),
    ]


class QdThermalOpts(ctypes.Structure):
    """qd_thermal_opts of include/qdsim.h: the peak widths and (closed regime) total charges of the groups of a
    qd_eval_points_thermal call on the host, and the device destinations of the occupation variances and the tail weights."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("gamma_host", ctypes.POINTER(ctypes.c_double)),
        ("n_charge_host", ctypes.POINTER(ctypes.c_int32)), ("var_dst", ctypes.c_void_p), ("ztail_dst", ctypes.c_void_p),
    ]


class QdResponseOpts(ctypes.Structure):
    """qd_response_opts of include/qdsim.h: the fields of qd_thermal_opts for a qd_eval_points_response call, and the device
    destinations of chi [points][N][2N-1], the jacobian [points][N][2N] and dS/dv [points][2N]."""
    _fields_ = list(QdThermalOpts._fields_) + [("chi_dst", ctypes.c_void_p), ("jac_dst", ctypes.c_void_p), ("dsignal_dst", ctypes.c_void_p)]


class QdGridThermalOpts(ctypes.Structure):
    """qd_grid_thermal_opts of include/qdsim.h: the (closed regime) total charges of the queries of a qd_scan_grid_thermal call
    and the destinations of the occupation variances and the tail weights, all on the device."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_charge_dev", ctypes.c_void_p),
        ("var_dst", ctypes.c_void_p), ("ztail_dst", ctypes.c_void_p),
    ]


class QdGridResponseOpts(ctypes.Structure):
    """qd_grid_response_opts of include/qdsim.h: the fields of qd_grid_thermal_opts for a qd_scan_grid_response call, and the
    device destinations of chi [nq][ny][nx][N][2N-1], the jacobian [..][N][2N], dS/dv [..][2N] and of the two derivatives along
    the axes of the grid, d<n>/d(sx, sy) [..][N][2] and dS/d(sx, sy) [..][2]."""
    _fields_ = list(QdGridThermalOpts._fields_) + [
        ("chi_dst", ctypes.c_void_p), ("jac_dst", ctypes.c_void_p), ("dsignal_dst", ctypes.c_void_p),
        ("docc_axes_dst", ctypes.c_void_p), ("dsignal_axes_dst", ctypes.c_void_p),
    ]


class QdGridLevelsOpts(ctypes.Structure):
    """qd_grid_levels_opts of include/qdsim.h: the number of energy levels per point of a qd_scan_grid_levels call, the (closed
    regime) total charges of its queries and the destinations of the levels and the norms, all on the device."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("n_charge_dev", ctypes.c_void_p),
        ("levels_dst", ctypes.c_void_p), ("hnorm_dst", ctypes.c_void_p),
    ]


class QdError(RuntimeError):
    pass


def build(force=False):
    """Compile libqdsim.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-s", "-C", CSRC, "libqdsim.so"])
    return LIB_PATH


_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise QdError(
            f"{LIB_PATH} not found: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
            "qadapt_hip has no CPU fallback.")
    # libqdsim.so needs libamdhip64.so.7.  PyTorch-ROCm ships its own copy with that
    # soname; loading torch first makes the dynamic loader reuse it, so device
    # pointers and streams are shared with torch instead of living in a second runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, fp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_void_p
    L.qd_param_block_doubles.argtypes = [ctypes.c_int]; L.qd_param_block_doubles.restype = ctypes.c_int
    L.qd_state_block_doubles.argtypes = [ctypes.c_int]; L.qd_state_block_doubles.restype = ctypes.c_int
    L.qd_layout_query.argtypes = [ctypes.c_int, ip]; L.qd_layout_query.restype = ctypes.c_int
    L.qd_create.argtypes = [ctypes.POINTER(QdConfig), ctypes.c_int, ctypes.POINTER(vp)]
    L.qd_create.restype = ctypes.c_int
    L.qd_destroy.argtypes = [vp]; L.qd_destroy.restype = ctypes.c_int
    L.qd_last_error.argtypes = [vp]; L.qd_last_error.restype = ctypes.c_char_p
    L.qd_bind_outputs.argtypes = [vp, fp, fp, fp, fp]; L.qd_bind_outputs.restype = ctypes.c_int
    L.qd_load_episodes.argtypes = [vp, ip, ctypes.c_int, dp, dp, ctypes.c_int, vp]
    L.qd_load_episodes.restype = ctypes.c_int
    L.qd_apply_actions.argtypes = [vp, fp, dp, vp, vp]; L.qd_apply_actions.restype = ctypes.c_int
    L.qd_observe.argtypes = [vp, vp, ctypes.c_int, vp]; L.qd_observe.restype = ctypes.c_int
    L.qd_update_capacitance.argtypes = [vp, vp, ctypes.c_int, fp, fp, ctypes.c_int, vp]
    L.qd_update_capacitance.restype = ctypes.c_int
    L.qd_step.argtypes = [vp, fp, fp, fp, dp, vp, vp]; L.qd_step.restype = ctypes.c_int
    L.qd_snapshot.argtypes = [vp, vp, ctypes.c_int, fp, fp, fp, fp, dp, dp, vp, vp]; L.qd_snapshot.restype = ctypes.c_int
    L.qd_get_state.argtypes = [vp, dp, vp]; L.qd_get_state.restype = ctypes.c_int
    L.qd_set_state.argtypes = [vp, dp, vp]; L.qd_set_state.restype = ctypes.c_int
    L.qd_get_raw.argtypes = [vp, dp, dp]; L.qd_get_raw.restype = ctypes.c_int
    L.qd_get_occupations.argtypes = [vp, dp]; L.qd_get_occupations.restype = ctypes.c_int
    L.qd_get_candidates.argtypes = [vp, vp]; L.qd_get_candidates.restype = ctypes.c_int
    L.qd_get_eigen.argtypes = [vp, dp]; L.qd_get_eigen.restype = ctypes.c_int
    L.qd_get_search_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]; L.qd_get_search_stats.restype = ctypes.c_int
    L.qd_get_solver_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]; L.qd_get_solver_stats.restype = ctypes.c_int
    L.qd_get_rng_state.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]; L.qd_get_rng_state.restype = ctypes.c_int
    L.qd_set_rng_state.argtypes = [vp, ctypes.c_uint64]; L.qd_set_rng_state.restype = ctypes.c_int
    L.qd_time_ground_kernel.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), vp]
    L.qd_time_ground_kernel.restype = ctypes.c_int
    L.qd_time_candidates_kernel.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), vp]
    L.qd_time_candidates_kernel.restype = ctypes.c_int
    L.qd_time_kernels.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), vp]; L.qd_time_kernels.restype = ctypes.c_int
    L.qd_timed_kernel_name.argtypes = [ctypes.c_int]; L.qd_timed_kernel_name.restype = ctypes.c_char_p
    L.qd_chunk_envs.argtypes = [vp]; L.qd_chunk_envs.restype = ctypes.c_int
    L.qd_probe.argtypes = [vp, vp, ctypes.c_int, dp, dp, dp, dp, dp, fp, dp, vp]; L.qd_probe.restype = ctypes.c_int
    L.qd_probe_ex.argtypes = [vp, vp, ctypes.c_int, dp, dp, dp, dp, dp, fp, dp, ctypes.POINTER(QdProbeOpts), vp]
    L.qd_probe_ex.restype = ctypes.c_int
    L.qd_probe_compose.argtypes = [vp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, dp, vp]
    L.qd_probe_compose.restype = ctypes.c_int
    L.qd_time_select.argtypes = [vp, dp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, dp, ctypes.POINTER(ctypes.c_float), vp]
    L.qd_time_select.restype = ctypes.c_int
    L.qd_eval_points.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_double),
                                 dp, dp, vp]
    L.qd_eval_points.restype = ctypes.c_int
    L.qd_scan2d.argtypes = [vp, vp, ctypes.c_int, vp, dp, dp, dp, dp, dp, fp, dp, ctypes.POINTER(QdScanOpts), vp]
    L.qd_scan2d.restype = ctypes.c_int
    L.qd_scan_affine.argtypes = [vp, vp, ctypes.c_int, dp, dp, dp, dp, dp, dp, fp, dp, ctypes.POINTER(QdScanAffineOpts), vp]
    L.qd_scan_affine.restype = ctypes.c_int
    L.qd_scan1d.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, dp, fp, dp, ctypes.POINTER(QdScan1dOpts), vp]
    L.qd_scan1d.restype = ctypes.c_int
    L.qd_scan_grid.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, dp, fp, dp,
                               ctypes.POINTER(QdScanGridOpts), vp]
    L.qd_scan_grid.restype = ctypes.c_int
    L.qd_eval_points_closed.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_double),
                                        ip, dp, dp, vp, vp]
    L.qd_eval_points_closed.restype = ctypes.c_int
    L.qd_scan_grid_closed.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, vp, dp, fp, dp,
                                      ctypes.POINTER(QdScanGridOpts), vp]
    L.qd_scan_grid_closed.restype = ctypes.c_int
    L.qd_eval_points_ex.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, dp, dp, dp, dp,
                                    ctypes.POINTER(QdPointsOpts), vp]
    L.qd_eval_points_ex.restype = ctypes.c_int
    L.qd_eval_points_thermal.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_double),
                                         dp, dp, ctypes.POINTER(QdThermalOpts), vp]
    L.qd_eval_points_thermal.restype = ctypes.c_int
    L.qd_eval_points_response.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_double),
                                          dp, dp, ctypes.POINTER(QdResponseOpts), vp]
    L.qd_eval_points_response.restype = ctypes.c_int
    L.qd_scan_grid_thermal.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, dp, dp, fp, dp,
                                       ctypes.POINTER(QdScanGridOpts), ctypes.POINTER(QdGridThermalOpts), vp]
    L.qd_scan_grid_thermal.restype = ctypes.c_int
    L.qd_scan_grid_response.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, dp, dp, fp, dp,
                                        ctypes.POINTER(QdScanGridOpts), ctypes.POINTER(QdGridResponseOpts), vp]
    L.qd_scan_grid_response.restype = ctypes.c_int
    L.qd_scan_grid_levels.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp, dp, fp, dp,
                                      ctypes.POINTER(QdScanGridOpts), ctypes.POINTER(QdGridLevelsOpts), vp]
    L.qd_scan_grid_levels.restype = ctypes.c_int
    _LIB = L
    return L


def check(handle, rc, what):
    if rc != 0:
        msg = lib().qd_last_error(handle).decode() if handle else "no handle"
        raise QdError(f"{what} failed (code {rc}): {msg}")
