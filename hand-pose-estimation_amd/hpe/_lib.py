"""ctypes binding of include/hpe.h (libhpe.so, built in-tree by the package Makefile).

The product path has no CPU fallback: if libhpe.so is missing or no gfx950 device is
visible, the calls raise.  The binding only marshals plain pointers and sizes.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent  # hand-pose-estimation_amd/
LIB_PATH = PKG_DIR / "libhpe.so"

PROF_PSO_GEN, PROF_REFINE, PROF_PSO_INIT, PROF_PSO_FINAL, PROF_PREP = 0, 1, 2, 3, 4
PROF_OPT_DESCENT, PROF_OPT_MOVE, PROF_SWARM_BEST, PROF_EXCHANGE = 5, 6, 7, 8
SUBSWARM_ID_BYTES = 128
BATCH_MAX = 16  # HPE_BATCH_MAX
BATCH_FORM_AUTO, BATCH_FORM_WAVE = 0, 1  # HPE_BATCH_FORM_*
WINDOW_OFF, WINDOW_FIXED, WINDOW_FOLLOW = 0, 1, 2  # HPE_WINDOW_*
PACING_LOCKSTEP, PACING_FREE = 0, 1  # HPE_PACING_*
HPE_OK, HPE_E_ARG, HPE_E_HIP, HPE_E_STATE, HPE_E_NOMEM, HPE_E_NODEVICE = 0, -1, -2, -3, -4, -5

dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)


class HandParams(C.Structure):
    _fields_ = [("geo_cm", C.c_double * 20), ("radii_cm", C.c_double * 48),
                ("cmc_deg", C.c_double * 5), ("spacing_cm", C.c_double * 5),
                ("tb_spheres", C.c_int32 * 4), ("fg_spheres", C.c_int32 * 4)]


class Frame(C.Structure):
    _fields_ = [("depth_cm", dp), ("dt", fp), ("cloud", dp), ("n", C.c_int32),
                ("scale", C.c_double), ("dtmax", C.c_double), ("K", C.c_double * 9)]


class Window(C.Structure):
    """hpe_window: 32 bytes, every bound inclusive."""
    _fields_ = [("row_lo", C.c_int32), ("row_hi", C.c_int32), ("col_lo", C.c_int32),
                ("col_hi", C.c_int32), ("z_lo", C.c_double), ("z_hi", C.c_double)]


VIEW_FLIP_COLS = 1  # HPE_VIEW_FLIP_COLS


class View(C.Structure):
    """hpe_view: 32 bytes (hpe/view.py is the rule in numpy)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32),
                ("row0", C.c_int32), ("col0", C.c_int32), ("step", C.c_int32),
                ("flags", C.c_uint32), ("pad", C.c_int32)]


CLEAN_MEDIAN = 1  # HPE_CLEAN_MEDIAN


class CleanPar(C.Structure):
    """hpe_clean: 8 bytes (hpe/clean.py is the rule in numpy)."""
    _fields_ = [("edge", C.c_uint16), ("support", C.c_uint8), ("flags", C.c_uint8),
                ("pad", C.c_uint32)]


REPORT_TRACK, REPORT_INIT = 1, 2  # HPE_REPORT_* kinds
REPORT_F_NAN, REPORT_F_EMPTY, REPORT_F_SUSPECT, REPORT_F_LOST = 1, 2, 4, 8  # HPE_REPORT_F_*


class LaneReport(C.Structure):
    """hpe_lane_report: 1096 bytes, every field naturally aligned."""
    _fields_ = [("seq", C.c_uint64), ("call", C.c_uint64), ("lane", C.c_int32),
                ("kind", C.c_int32), ("n", C.c_int32), ("flags", C.c_int32),
                ("bad_streak", C.c_int32), ("pad", C.c_int32), ("state", C.c_double * 27),
                ("joints", (C.c_double * 3) * 21), ("px", (C.c_double * 2) * 21)]


class ReportWatch(C.Structure):
    """hpe_report_watch: SUSPECT iff !(cost <= cost_max) || n < n_min; LOST after `streak`."""
    _fields_ = [("cost_max", C.c_double), ("n_min", C.c_int32), ("streak", C.c_int32)]


class LocateParams(C.Structure):
    """hpe_locate_params: 72 bytes."""
    _fields_ = [("search", Window), ("bin", C.c_double), ("slab", C.c_double),
                ("half_xy", C.c_double), ("half_z", C.c_double), ("skip", C.c_int32),
                ("min_pixels", C.c_int32)]


class Locate(C.Structure):
    """hpe_locate: 104 bytes, every field naturally aligned."""
    _fields_ = [("seq", C.c_uint64), ("lane", C.c_int32), ("found", C.c_int32),
                ("k_near", C.c_int32), ("m1", C.c_int32), ("m2", C.c_int32), ("pad", C.c_int32),
                ("px", C.c_double * 2), ("centre", C.c_double * 3), ("window", Window)]


# name -> (restype, argtypes); the list IS the exported C ABI (tests check it against
# include/hpe.h)
SIGNATURES = {
    "hpe_abi_version": (C.c_int, []),
    "hpe_last_error": (C.c_char_p, [C.c_void_p]),
    "hpe_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(HandParams)]),
    "hpe_destroy": (C.c_int, [C.c_void_p]),
    "hpe_stream": (C.c_void_p, [C.c_void_p]),
    "hpe_sync": (C.c_int, [C.c_void_p]),
    "hpe_preprocess_depth": (C.c_int, [fp, C.c_int, C.c_int, C.c_double, dp, fp, dp, ip, dp,
                                       dp, dp]),
    "hpe_store_frame": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Frame)]),
    "hpe_select_frame": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_set_frame": (C.c_int, [C.c_void_p, C.POINTER(Frame)]),
    "hpe_prepare_frame": (C.c_int, [C.c_void_p, C.c_int, fp, C.c_int, C.c_int, C.c_double]),
    "hpe_frame_readback": (C.c_int, [C.c_void_p, C.c_int, dp, fp, dp, ip, dp, dp]),
    "hpe_pipeline_begin": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_int, C.c_double]),
    "hpe_track_pipelined": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, fp]),
    "hpe_track_raw_sequence_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                             C.c_int, C.c_void_p]),
    "hpe_pipe_readback": (C.c_int, [C.c_void_p, C.c_int, dp, fp, dp, ip, dp, dp]),
    "hpe_track_raw_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_int, C.c_void_p]),
    "hpe_batch_pipeline_begin": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                           C.c_int, C.c_double]),
    "hpe_track_batch_pipelined": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "hpe_batch_pipeline_begin_u16": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                               C.c_float, C.c_int, C.c_int, C.c_double]),
    "hpe_track_batch_pipelined_u16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.POINTER(C.c_void_p)]),
    "hpe_batch_frame_buffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t)]),
    "hpe_batch_pipeline_begin_view": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                                C.POINTER(View), C.c_float, C.c_int, C.c_int,
                                                C.c_double]),
    "hpe_view_fit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                               C.c_int, C.c_uint32, C.POINTER(View), dp, dp]),
    "hpe_batch_views_readback": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(View)]),
    "hpe_clean_defaults": (C.c_int, [C.c_float, C.POINTER(CleanPar)]),
    "hpe_set_batch_clean": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(CleanPar)]),
    "hpe_clean_depth_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(View),
                                      C.POINTER(CleanPar), C.c_void_p]),
    "hpe_batch_clean_readback": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hpe_set_batch_form": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_batch_wave_wpp": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hpe_set_batch_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Window),
                                       C.c_double, C.c_double]),
    "hpe_window_from_pose": (C.c_int, [C.c_void_p, dp, C.c_double, C.c_double, C.c_double,
                                       C.POINTER(Window)]),
    "hpe_batch_windows_readback": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Window)]),
    "hpe_set_batch_hands": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(HandParams)]),
    "hpe_lane_window_from_pose": (C.c_int, [C.c_void_p, C.c_int, dp, C.c_double, C.c_double,
                                            C.c_double, C.POINTER(Window)]),
    "hpe_set_batch_seeds": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "hpe_set_batch_groups": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ip]),
    "hpe_batch_group_pick": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hpe_batch_group_rows": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "hpe_set_batch_pacing": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_batch_pending": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "hpe_pso_optimise_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, ip,
                                         C.c_void_p]),
    "hpe_batch_pipeline_optimise": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                              C.c_uint32, C.c_void_p]),
    "hpe_lane_report_size": (C.c_size_t, []),
    "hpe_set_batch_report": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ReportWatch)]),
    "hpe_batch_report": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(LaneReport)]),
    "hpe_batch_report_wait": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_int,
                                        C.POINTER(LaneReport)]),
    "hpe_batch_lost": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "hpe_lane_joints_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                      C.c_void_p, C.c_void_p]),
    "hpe_locate_defaults": (C.c_int, [C.POINTER(LocateParams)]),
    "hpe_locate_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                   C.c_double, C.POINTER(LocateParams), C.POINTER(Locate)]),
    "hpe_batch_pipeline_locate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, dp,
                                            C.POINTER(LocateParams)]),
    "hpe_batch_locate_result": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Locate)]),
    "hpe_build_spheres":(C.c_int, [C.c_void_p, dp, C.c_int, dp, dp]),
    "hpe_eval_costs": (C.c_int, [C.c_void_p, dp, C.c_int, C.c_int, dp, ip]),
    "hpe_cal_cost2": (C.c_int, [C.c_void_p, dp, ip, C.c_int, dp, dp]),
    "hpe_eval_spheres": (C.c_int, [C.c_void_p, dp, C.c_int, C.c_int, ip, dp]),
    "hpe_set_pso_params": (C.c_int, [C.c_void_p, dp, dp, dp, C.c_double, C.c_double,
                                     C.c_double, C.c_int, C.c_double, C.c_double]),
    "hpe_set_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "hpe_pso_evolve": (C.c_int, [C.c_void_p, dp, C.c_int, dp, dp]),
    "hpe_pso_optimise": (C.c_int, [C.c_void_p, dp, C.c_int, dp, dp, dp, C.c_int]),
    "hpe_pso_trace": (C.c_int, [C.c_void_p, dp, ip, ip, C.c_int]),
    "hpe_refine_init_pose": (C.c_int, [C.c_void_p, dp, ip]),
    "hpe_set_refine_exact": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_set_refine_spec": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_graph_captures": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "hpe_set_exchange": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_pick_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "hpe_subswarm_unique_id": (C.c_int, [C.c_void_p]),
    "hpe_subswarm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "hpe_subswarm_init_scripted": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp, C.c_int]),
    "hpe_subswarm_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_subswarm_fini": (C.c_int, [C.c_void_p]),
    "hpe_subswarm_info": (C.c_int, [C.c_void_p, ip, ip, ip, ip, dp]),
    "hpe_get_refine_exact": (C.c_int, [C.c_void_p]),
    "hpe_get_refine_spec": (C.c_int, [C.c_void_p]),
    "hpe_track_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp, dp]),
    "hpe_track_frame_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hpe_track_sequence_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p]),
    "hpe_track_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, ip,
                                      C.c_int, C.c_int, C.c_void_p]),
    "hpe_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_profile_read": (C.c_int, [C.c_void_p, ip, dp, dp, dp]),
    "hpe_profile_read_kernel": (C.c_int, [C.c_void_p, C.c_int, ip, dp, dp, dp]),
    "hpe_refine_eval_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "hpe_render_depth": (C.c_int, [C.c_void_p, dp, C.c_double, fp]),
    "hpe_debug_stamps": (C.c_int, [C.POINTER(C.c_uint64)]),
}

# hpe_exchange_fn: int (*)(void *user, double *d_ext, int generation)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)

_lib = None


def load(path: os.PathLike | str | None = None):
    """Load libhpe.so (raises if it is absent: there is no fallback path)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # HPE_LIB_VARIANT=<file in the package dir>: A/B a second in-tree build (tools only)
    variant = os.environ.get("HPE_LIB_VARIANT")
    p = Path(path) if path else (PKG_DIR / variant if variant else LIB_PATH)
    if not p.exists():
        raise RuntimeError(f"{p} not built: run `make -C {PKG_DIR}` (no CPU fallback exists)")
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        if variant and not path and not hasattr(lib, name):
            continue  # an older build under A/B: entry points added since are absent
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = lib
    return lib


class HpeError(RuntimeError):
    pass


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a
