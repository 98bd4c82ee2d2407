"""ctypes binding of libpeleanalysis_amd.so (the C ABI in include/peleanalysis_amd.h).

This is the host-side mirror used by tests/ and bench.py; the C++ tool drivers in
tools/ call the same C ABI directly.  There is NO CPU fallback: if the HIP library is
missing or no GPU is present, constructing a Context raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from .hierarchy import Hierarchy, Level, MultiFab, mf_layout

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpeleanalysis_amd.so")

BC_PERIODIC, BC_NEUMANN, BC_REFLECT_ODD = 0, 1, 2


class PaFab(C.Structure):
    _fields_ = [("p", C.c_void_p), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("ncomp", C.c_int32), ("nstride", C.c_int64)]


class PaBox(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


class PaCurvParams(C.Structure):
    _fields_ = [("prog_min", C.c_double), ("prog_max", C.c_double), ("do_threshold", C.c_int32), ("threshold", C.c_double),
                ("fused", C.c_int32), ("do_gauss_curv", C.c_int32), ("do_strain", C.c_int32), ("get_strain_tensor", C.c_int32),
                ("do_velnormal", C.c_int32), ("vel_comp", C.c_int32), ("do_smooth", C.c_int32), ("smoothing_time", C.c_double),
                ("spacedim", C.c_int32)]


class PaStreamAltParams(C.Structure):
    _fields_ = [("isoComp", C.c_int32), ("altVal", C.c_double), ("ncarry", C.c_int32), ("carry", C.c_int32 * 8), ("thickComp", C.c_int32),
                ("thickLo", C.c_double), ("thickHi", C.c_double), ("TComp", C.c_int32), ("strainComp", C.c_int32), ("TVal", C.c_double),
                ("addAngle", C.c_int32)]


class PaXfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("sendbuf", C.c_void_p), ("nsend", C.c_int64), ("recvbuf", C.c_void_p), ("nrecv", C.c_int64)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PaXfer))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32)


DONE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
DONE2_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)


class PaComm(C.Structure):
    _fields_ = [("user", C.c_void_p), ("rank", C.c_int32), ("nranks", C.c_int32), ("exchange", EXCHANGE_FN), ("allreduce", ALLREDUCE_FN)]


class PaIsoFrag(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("nvert", C.c_int64), ("tris", C.c_void_p), ("ntri", C.c_int64)]


class PaJpdfParams(C.Structure):
    _fields_ = [("nload", C.c_int32), ("do_stoichiometry", C.c_int32), ("hlist", C.c_double * 8), ("olist", C.c_double * 8), ("vmin", C.c_double * 8),
                ("vmax", C.c_double * 8), ("do_conditioning", C.c_int32), ("cvar", C.c_int32), ("norm_cval", C.c_int32), ("cnorm_min", C.c_double),
                ("cnorm_max", C.c_double), ("cmin", C.c_double), ("cmax", C.c_double), ("uncombined", C.c_int32)]


class PaSdfGrid(C.Structure):
    _fields_ = [("ntri", C.c_int64), ("tri", C.c_void_p), ("nvert", C.c_int64), ("x", C.c_void_p), ("origin", C.c_float * 3), ("dx", C.c_float),
                ("n", C.c_int32 * 3), ("phi", C.c_void_p)]


class PaSselCond(C.Structure):
    _fields_ = [("kind", C.c_int32), ("comp", C.c_int32), ("comp2", C.c_int32), ("sgn", C.c_int32), ("val", C.c_double), ("val2", C.c_double)]


_lib = None


def load_library() -> C.CDLL:
    """dlopen the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pi32, pdbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    sig = {
        "pa_version": (C.c_int, []),
        "pa_options_reload": (None, []),
        "pa_ctx_create": (vp, [C.c_int, vp]),
        "pa_ctx_destroy": (None, [vp]),
        "pa_last_error": (C.c_char_p, [vp]),
        "pa_sync": (C.c_int, [vp]),
        "pa_ctx_stream": (vp, [vp]),
        "pa_device_malloc": (vp, [vp, i64]),
        "pa_device_free": (None, [vp, vp]),
        "pa_memcpy_h2d": (C.c_int, [vp, vp, vp, i64]),
        "pa_memcpy_d2h": (C.c_int, [vp, vp, vp, i64]),
        "pa_memcpy_d2d": (C.c_int, [vp, vp, vp, i64]),
        "pa_device_count": (C.c_int, []),
        "pa_profile_enable": (C.c_int, [vp, C.c_int]),
        "pa_sweep_kernel_name": (C.c_char_p, [vp]),
        "pa_sweep_occupancy": (C.c_int, [vp, C.c_int]),
        "pa_profile_read": (C.c_int, [vp, C.c_int, C.POINTER(i64), pdbl, C.c_int]),
        "pa_level_create": (vp, [vp, C.c_int, pi32, pi32, pi32, pi32, pdbl, pdbl]),
        "pa_level_create_sharded": (vp, [vp, C.c_int, pi32, pi32, C.c_int, C.c_int, pi32, pi32, pi32, pdbl, pdbl]),
        "pa_level_global_ids": (C.c_int, [vp, pi32]),
        "pa_ctx_set_comm": (C.c_int, [vp, C.POINTER(PaComm)]),
        "pa_ctx_set_delay_comm": (C.c_int, [vp, C.c_int, C.c_int, dbl, dbl]),
        "pa_delay_comm_stats": (C.c_int, [vp, C.POINTER(i64), pdbl]),
        "pa_rccl_unique_id": (C.c_int, [vp, vp]),
        "pa_ctx_init_rccl": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "pa_ctx_nranks": (C.c_int, [vp]),
        "pa_comm_selftest": (C.c_int, [vp, i64]),
        "pa_allreduce": (C.c_int, [vp, pdbl, C.c_int, C.c_int]),
        "pa_distribution_map": (C.c_int, [C.c_int, pi32, C.c_int, pi32]),
        "pa_plan_fill_boundary": (i64, [C.c_int, pi32, pi32, C.c_int, pi32, pi32, pi32, C.c_int, pi32, i64]),
        "pa_plan_coarse_source": (i64, [C.c_int, pi32, pi32, pi32, pi32, C.c_int, pi32, pi32, pi32, pi32, pi32, C.c_int, C.c_int, C.c_int, C.c_int, pi32,
                                        i64]),
        "pa_plan_restriction": (i64, [C.c_int, pi32, pi32, pi32, pi32, C.c_int, pi32, pi32, pi32, pi32, pi32, C.c_int, C.c_int, C.c_int, pi32, i64]),
        "pa_level_retile": (C.c_int, [C.c_int, pi32, pi32, C.c_int, pi32, C.c_int]),
        "pa_hierarchy_retile_limits": (C.c_int, [C.c_int, pi32, C.POINTER(pi32), C.c_int, pi32]),
        "pa_hierarchy_retile_limits_ranks": (C.c_int, [C.c_int, pi32, C.POINTER(pi32), C.c_int, C.c_int, pi32]),
        "pa_level_destroy": (None, [vp]),
        "pa_level_nboxes": (C.c_int, [vp]),
        "pa_mf_layout": (i64, [C.c_int, pi32, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
        "pa_mf_create": (vp, [vp, vp, C.c_int, C.c_int, vp]),
        "pa_mf_destroy": (None, [vp]),
        "pa_mf_data": (vp, [vp]),
        "pa_mf_size": (i64, [vp]),
        "pa_mf_upload": (C.c_int, [vp, vp, vp]),
        "pa_mf_download": (C.c_int, [vp, vp, vp]),
        "pa_mf_upload_comps": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
        "pa_mf_download_comps": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
        "pa_mf_setval": (C.c_int, [vp, vp, C.c_int, C.c_int, dbl]),
        "pa_mf_copy": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]),
        "pa_fill_boundary": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "pa_apply_bc": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, pi32, C.c_int, C.c_int]),
        "pa_bc_errors": (C.c_int, [vp]),
        "pa_grad_level": (C.c_int, [vp, vp, C.c_int, vp, C.c_int]),
        "pa_minmax_level": (C.c_int, [vp, vp, C.c_int, pdbl, pdbl]),
        "pa_progress_level": (C.c_int, [vp, vp, C.c_int, dbl, dbl, vp, C.c_int, C.c_int]),
        "pa_normal_level": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]),
        "pa_div_level": (C.c_int, [vp, vp, C.c_int, dbl, vp, C.c_int, dbl, vp, C.c_int]),
        "pa_progress_shell_level": (C.c_int, [vp, vp, C.c_int, dbl, dbl, vp, C.c_int, C.c_int, C.c_int]),
        "pa_gradcurv_level": (C.c_int, [vp, vp, C.c_int, dbl, dbl, dbl, vp, C.c_int]),
        "pa_gradcurv_faces_level": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, pi32, C.c_int, dbl, vp, C.c_int, C.c_int]),
        "pa_grad_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.c_int, pdbl, C.POINTER(PaFab), C.c_int]),
        "pa_progress_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.c_int, dbl, dbl, C.POINTER(PaFab), C.c_int]),
        "pa_normal_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.c_int, pdbl, C.POINTER(PaFab), C.c_int, C.POINTER(PaFab), C.c_int,
                                    C.POINTER(PaFab), C.c_int]),
        "pa_div_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.c_int, pdbl, dbl, C.POINTER(PaFab), C.c_int]),
        "pa_gradcurv_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.c_int, dbl, dbl, pdbl, dbl, C.POINTER(PaFab), C.c_int]),
        "pa_boxfilter_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.POINTER(PaFab), C.c_int, C.c_int, C.c_int, pdbl]),
        "pa_box_filter_weights": (C.c_int, [C.c_int, pdbl]),
        "pa_filter_weights": (C.c_int, [C.c_int, C.c_int, pdbl]),
        "pa_boxfilter_level": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, pdbl]),
        "pa_boxfilter_hierarchy": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, pi32, C.POINTER(pdbl)]),
        "pa_boxfilter_level2d": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, pdbl]),
        "pa_filter_last_launch": (C.c_int, [vp, pi32]),
        "pa_foextrap": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "pa_fillpatch_two_levels": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "pa_fill_ghosts_hierarchy": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, C.c_int, pi32, C.c_int, C.c_int, C.c_int]),
        "pa_mc_count_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.POINTER(PaFab), C.c_int, dbl, C.POINTER(i64), C.POINTER(i64)]),
        "pa_mc_emit_fab": (C.c_int, [vp, PaBox, C.POINTER(PaFab), C.POINTER(PaFab), C.c_int, dbl, vp, vp, vp, i64, i64]),
        "pa_iso_mask_level": (C.c_int, [vp, vp, C.c_int, vp, C.c_int]),
        "pa_iso_coords_level": (C.c_int, [vp, vp, C.c_int]),
        "pa_mc_level_fine": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(PaBox), C.c_int, dbl, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                       C.POINTER(vp)]),
        "pa_msq_level_fine": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(PaBox), C.c_int, dbl, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(vp)]),
        "pa_mc_hierarchy_fine": (C.c_int, [vp, C.c_int, C.POINTER(vp), pi32, C.c_int, C.POINTER(C.POINTER(PaBox)), C.c_int, dbl, C.POINTER(C.POINTER(i64)),
                                           C.POINTER(C.POINTER(i64)), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "pa_mc_hierarchy_xyz": (C.c_int, [vp, C.c_int, C.POINTER(vp), pi32, C.c_int, C.POINTER(C.POINTER(PaBox)), C.c_int, dbl, C.POINTER(C.POINTER(i64)),
                                          C.POINTER(C.POINTER(i64)), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "pa_msq_level": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(PaBox), C.c_int, dbl, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                   C.POINTER(vp)]),
        "pa_mc_level": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(PaBox), C.c_int, dbl, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                  C.POINTER(vp)]),
        "pa_iso_merge": (C.c_int, [vp, C.c_int, C.POINTER(PaIsoFrag), C.c_int, C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), C.POINTER(vp)]),
        "pa_mc_edge_table": (C.POINTER(C.c_uint16), []),
        "pa_mc_tri_table": (C.POINTER(C.c_int8), []),
        "pa_sdf_level_set3": (C.c_int, [vp, C.c_int, C.POINTER(PaSdfGrid), C.c_int]),
        "pa_sdf_signed_fab": (C.c_int, [vp, PaBox, vp, C.POINTER(PaFab), C.c_int, dbl, dbl, C.POINTER(PaFab), C.c_int]),
        "pa_smooth_solve": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, dbl, pi32, dbl, C.c_int, C.POINTER(C.c_int), pdbl]),
        "pa_stream_trace": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, i64, pdbl, C.c_int, dbl, vp, pi32]),
        "pa_last_slow_cells": (C.c_int, [vp]),
        "pa_level_irregular_cells": (i64, [vp, vp]),
        "pa_stream_trace_ranks": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, i64, pdbl, C.c_int, dbl, vp, pi32, C.c_int]),
        "pa_vtrace_fab": (C.c_int, [vp, C.POINTER(PaFab), i32, vp, i64, vp, i32, C.POINTER(PaFab), i32, C.POINTER(PaFab), i32, pdbl, pdbl, pdbl, dbl,
                                    pi32]),
        "pa_streamgrad_prepare": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "pa_streamgrad_trace": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, i64, vp, C.POINTER(i64), vp, C.c_int, dbl, vp, pi32]),
        "pa_streamalt_run": (C.c_int, [vp, i32, C.POINTER(i64), vp, vp, i32, i32, i64, C.POINTER(PaStreamAltParams), vp, vp]),
        "pa_interpstream_fab": (C.c_int, [vp, C.POINTER(PaFab), i32, C.POINTER(PaFab), i32, C.POINTER(PaFab), pdbl, pdbl, pi32]),
        "pa_set_distance_fab": (C.c_int, [vp, C.POINTER(PaFab), C.POINTER(PaFab)]),
        "pa_streamsample_run": (C.c_int, [vp, C.c_int, C.POINTER(vp), i32, pdbl, pdbl, pi32, pi32, pi32, pi32, pi32, vp, vp, i32, i32, i32, pi32]),
        "pa_device_mem_info": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "pa_minmax_comps_level": (C.c_int, [vp, vp, C.c_int, pi32, pdbl, pdbl]),
        "pa_jpdf_create": (vp, [vp, C.c_int, C.c_int]),
        "pa_jpdf_begin": (C.c_int, [vp, vp, dbl, pdbl]),
        "pa_jpdf_add_level": (C.c_int, [vp, vp, vp, vp, C.c_int, dbl, C.POINTER(PaJpdfParams), C.POINTER(i64), C.POINTER(i64)]),
        "pa_jpdf_read": (C.c_int, [vp, vp, pdbl, pdbl, pdbl]),
        "pa_condmean_create": (vp, [vp, C.c_int, C.c_int, C.c_int]),
        "pa_condmean_begin": (C.c_int, [vp, vp, i64, pdbl]),
        "pa_condmean_add_level": (C.c_int, [vp, vp, vp, vp, C.c_int, C.POINTER(PaBox), i64, dbl, dbl, C.c_int]),
        "pa_condmean_read": (C.c_int, [vp, vp, C.POINTER(i64), pdbl, pdbl, pdbl, pdbl]),
        "pa_hist_destroy": (None, [vp]),
        "pa_integral_create": (vp, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(PaBox), C.c_int]),
        "pa_integral_begin": (C.c_int, [vp, vp, dbl, pdbl]),
        "pa_integral_add_level": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, dbl, C.c_int, dbl, dbl, C.c_int]),
        "pa_integral_slots": (i64, [vp]),
        "pa_integral_read": (C.c_int, [vp, vp, pdbl]),
        "pa_integral_destroy": (None, [vp]),
        "pa_surfbin_create": (vp, [vp, C.c_int, pi32, pdbl, pdbl, i64]),
        "pa_surfbin_begin": (C.c_int, [vp, vp, dbl]),
        "pa_surfbin_max_area": (dbl, [i64, pdbl, pdbl, pdbl, i64, pi32]),
        "pa_surfbin_add_surface": (C.c_int, [vp, vp, i64, pdbl, pdbl, pdbl, C.POINTER(pdbl), pdbl, i64, pi32, C.c_int, C.c_int, dbl, dbl, C.c_int]),
        "pa_surfbin_read": (C.c_int, [vp, vp, pdbl, C.POINTER(i64), pdbl, pdbl, C.POINTER(i64)]),
        "pa_surfbin_destroy": (None, [vp]),
        "pa_fe_build": (vp, [vp, C.c_int, C.POINTER(vp), pi32, C.POINTER(PaBox), C.c_int, pi32, C.POINTER(i64), C.POINTER(i64)]),
        "pa_fe_connectivity": (C.c_int, [vp, vp, C.POINTER(vp)]),
        "pa_fe_nodes": (C.c_int, [vp, vp, C.POINTER(i64), C.POINTER(vp)]),
        "pa_fe_gather": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), C.c_int, pi32, vp]),
        "pa_fe_stage_times": (C.c_int, [vp, vp, pdbl, C.POINTER(i64)]),
        "pa_fe_destroy": (None, [vp]),
        "pa_tube_create": (vp, [vp, i32, C.POINTER(i64), i64, pi32, i64, pi32]),
        "pa_tube_destroy": (None, [vp]),
        "pa_tube_wedges": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "pa_tube_lines": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
        "pa_tube_peaks": (C.c_int, [vp, vp, vp, i32, i32, i32, pi32, vp, vp]),
        "pa_tube_node_means": (C.c_int, [vp, vp, i32, vp, vp]),
        "pa_tube_node_all": (C.c_int, [vp, vp, vp, vp]),
        "pa_tube_node_avg": (C.c_int, [vp, vp, vp, i32, i32, vp]),
        "pa_tube_smooth": (C.c_int, [vp, vp, vp, vp, i32, vp]),
        "pa_tube_neighbors": (C.c_int, [vp, vp, C.POINTER(i64), C.POINTER(i64), pi32]),
        "pa_ssel_create": (vp, [vp, i32, C.POINTER(i64), i64, pi32]),
        "pa_ssel_destroy": (None, [vp]),
        "pa_ssel_peaks": (C.c_int, [vp, vp, vp, i32, i32, vp, vp]),
        "pa_ssel_scatter": (C.c_int, [vp, vp, vp, i32, i32, pi32, vp, vp, dbl, dbl, i32, i32, vp, C.POINTER(i64)]),
        "pa_ssel_gather_lines": (C.c_int, [vp, vp, vp, i32, i32, pi32, i64, pi32, i32, i32, vp]),
        "pa_ssel_filter": (C.c_int, [vp, vp, i32, i32, i32, i64, i32, C.POINTER(PaSselCond), vp]),
        "pa_ssel_arclength": (C.c_int, [vp, vp, i32, i32, i64, i32, dbl]),
        "pa_ssub_select_seedbox": (C.c_int, [vp, vp, vp, i32, i64, i32, vp, pdbl, pdbl, vp, C.POINTER(i64), C.POINTER(i64)]),
        "pa_ssub_plan": (vp, [vp, vp, i64, i32, vp, i64, vp]),
        "pa_ssub_destroy": (None, [vp]),
        "pa_ssub_counts": (C.c_int, [vp, C.POINTER(i64)]),
        "pa_ssub_gather": (C.c_int, [vp, vp, vp, i32, i32, pi32, vp, i32, i32]),
        "pa_ssub_read": (C.c_int, [vp, vp, pi32, C.POINTER(i64), pi32, pi32]),
        "pa_ssub_last_launch": (C.c_int, [vp, C.POINTER(i64)]),
        "pa_smooth_last": (C.c_int, [vp, C.POINTER(C.c_int), pdbl]),
        "pa_curvature_last_path": (C.c_int, [vp]),
        "pa_level_free_scratch": (i64, [vp]),
        "pa_grad_run": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, pi32, C.POINTER(vp), C.c_int]),
        "pa_curvature_run": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, pi32, C.POINTER(PaCurvParams), C.POINTER(vp), C.c_int]),
        "pa_gradcurv_run": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, pi32, C.POINTER(PaCurvParams), C.POINTER(vp), C.POINTER(vp),
                                      C.c_int]),
        "pa_gradcurv_run_comps": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, C.c_int, pi32, C.POINTER(PaCurvParams), C.POINTER(vp), C.POINTER(vp),
                                            C.c_int, DONE_FN, vp]),
        "pa_gradcurv_run_comps2": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.c_int, C.c_int, pi32, C.POINTER(PaCurvParams), C.POINTER(vp), C.POINTER(vp),
                                             C.c_int, C.c_int, DONE2_FN, vp]),
        "pa_resample_create": (vp, [vp]),
        "pa_resample_begin": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), C.c_int]),
        "pa_resample_add_file_level": (C.c_int, [vp, vp, C.c_int, vp, pi32, vp, C.c_int, C.c_int, vp]),
        "pa_resample_finish": (C.c_int, [vp, vp, C.c_int, C.POINTER(i64)]),
        "pa_resample_destroy": (None, [vp]),
        "pa_flatten_level": (C.c_int, [vp, vp, pi32, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(i64)]),
        "pa_flatten_last_launch": (None, [C.POINTER(i64)]),
        "pa_plane_create": (vp, [vp, C.c_int, C.c_int, C.POINTER(PaBox), C.c_int]),
        "pa_plane_run": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), pi32, pi32]),
        "pa_plane_read": (C.c_int, [vp, vp, pdbl, C.POINTER(i64)]),
        "pa_plane_minmax": (C.c_int, [vp, vp, C.c_int, pdbl, pdbl]),
        "pa_plane_pixelize": (C.c_int, [vp, vp, C.c_int, dbl, dbl, C.POINTER(C.c_uint8)]),
        "pa_plane_destroy": (None, [vp]),
        "pa_decimate_create": (vp, [vp, i64, pdbl, i64, pi32, dbl, C.c_int, C.c_int]),
        "pa_decimate_round": (C.c_int, [vp, vp, i64]),
        "pa_decimate_run": (C.c_int, [vp, vp, i64, C.c_int]),
        "pa_decimate_last_round": (C.c_int, [vp, C.POINTER(i64)]),
        "pa_decimate_counts": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "pa_decimate_read": (C.c_int, [vp, vp, pdbl, pi32]),
        "pa_decimate_read_state": (C.c_int, [vp, vp, pdbl, pi32, C.POINTER(C.c_uint8), pdbl]),
        "pa_decimate_destroy": (None, [vp]),
        "pa_surf_create": (vp, [vp, i64, C.c_int, pdbl, i64, pi32]),
        "pa_surf_counts": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int)]),
        "pa_surf_read": (C.c_int, [vp, vp, pdbl, pi32]),
        "pa_surf_slice": (C.c_int, [vp, vp, C.c_int, dbl, C.POINTER(i64), C.POINTER(i64)]),
        "pa_surf_slice_read": (C.c_int, [vp, vp, pdbl, pi32, pi32, pi32, pi32, pi32]),
        "pa_surf_trim": (C.c_int, [vp, vp, C.c_int, pi32, pi32, pdbl, dbl, C.c_int, C.POINTER(i64)]),
        "pa_surf_area": (C.c_int, [vp, vp, pdbl, pdbl, pdbl]),
        "pa_surf_last_launch": (C.c_int, [vp, C.POINTER(i64)]),
        "pa_surf_destroy": (None, [vp]),
        "pa_surfjoin_merge": (C.c_int, [vp, vp, vp, dbl, C.c_int, C.c_int, C.POINTER(C.c_int)]),
        "pa_surfjoin_scale": (C.c_int, [vp, vp, C.c_int, pi32, pdbl]),
        "pa_surfjoin_product": (vp, [vp, vp, C.c_int, pi32]),
        "pa_surfjoin_select": (vp, [vp, vp, vp, C.c_int, pi32, pi32]),
        "pa_surfsmooth_run": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "pa_surfsmooth_read": (C.c_int, [vp, vp, pi32, pi32, pdbl, pdbl]),
    }
    missing = []
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:  # symbol missing from the .so: calling it later raises AttributeError
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    L._pa_signatures = sig
    L._pa_missing = missing  # tests/test_abi.py asserts this is empty
    _lib = L
    return L


def declared_symbols(header: Optional[str] = None) -> List[str]:
    """Names of every function declared in include/peleanalysis_amd.h."""
    import re
    header = header or os.path.join(os.path.dirname(_HERE), "include", "peleanalysis_amd.h")
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pa_[a-z0-9_]+)\s*\(", txt)))


def reload_options() -> None:
    """pa_options_reload: the library reads its PA_* environment switches once (first context); a caller that changes one
    afterwards -- a test, bench.py --ab -- asks for a re-read."""
    load_library().pa_options_reload()


class PaError(RuntimeError):
    pass


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


class Context:
    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = load_library()
        self.h = self.lib.pa_ctx_create(int(device), C.c_void_p(stream) if stream else None)
        if not self.h:
            raise PaError("pa_ctx_create failed: no MI355X/HIP device visible (no CPU fallback)")

    def check(self, rc: int):
        if rc != 0:
            raise PaError(self.lib.pa_last_error(self.h).decode())

    def sync(self):
        self.check(self.lib.pa_sync(self.h))

    def profile_enable(self, on=True):
        """False / True: no / every tag; an int > 1: bit mask (1 << tag) of the tags to time"""
        self.check(self.lib.pa_profile_enable(self.h, int(on)))

    def profile_read(self, tag: int, reset: bool = False):
        n, ms = C.c_int64(0), C.c_double(0.0)
        self.check(self.lib.pa_profile_read(self.h, tag, C.byref(n), C.byref(ms), int(reset)))
        return n.value, ms.value

    def bc_errors(self) -> int:
        return int(self.lib.pa_bc_errors(self.h))

    # ---- multi-GPU transports (include/peleanalysis_amd.h: pa_comm)
    def set_comm(self, comm: "PaComm"):
        """caller-supplied transport; the structure (and its callbacks) must outlive the context"""
        self._comm = comm
        self.check(self.lib.pa_ctx_set_comm(self.h, C.byref(comm) if comm is not None else None))

    def rccl_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self.check(self.lib.pa_rccl_unique_id(self.h, buf))
        return buf.raw

    def init_rccl(self, nranks: int, rank: int, unique_id: bytes):
        """built-in transport: grouped ncclSend / ncclRecv on the context's stream (RCCL over xGMI)"""
        assert len(unique_id) == 128
        self.check(self.lib.pa_ctx_init_rccl(self.h, int(nranks), int(rank), C.create_string_buffer(unique_id, 128)))

    def comm_selftest(self, n: int = 4096):
        self.check(self.lib.pa_comm_selftest(self.h, int(n)))

    def allreduce(self, vals, op: int):
        a = np.ascontiguousarray(vals, dtype=np.float64).copy()
        self.check(self.lib.pa_allreduce(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size, int(op)))
        return a

    def close(self):
        if self.h:
            self.lib.pa_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DevBuf:
    """raw HBM buffer from pa_device_malloc (freed with the object)"""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr = ctx.lib.pa_device_malloc(ctx.h, self.nbytes)
        if not self.ptr:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    @classmethod
    def from_numpy(cls, ctx: Context, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(ctx, a.nbytes)
        ctx.check(ctx.lib.pa_memcpy_h2d(ctx.h, b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return b

    def to_numpy(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx.check(self.ctx.lib.pa_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
                self.ctx.lib.pa_device_free(self.ctx.h, self.ptr)
        except Exception:
            pass


class DevLevel:
    def __init__(self, ctx: Context, level: Level, owner: Optional[Sequence[int]] = None, rank: int = 0, nranks: int = 1):
        """level: the whole BoxArray of the AMR level.  owner (one rank per box) + rank + nranks: this context holds only the
        boxes with owner == rank (pa_level_create_sharded); self.level then describes those boxes, self.gids their indices
        in the BoxArray, self.glob the whole level."""
        self.ctx, self.glob = ctx, level
        b = np.ascontiguousarray(level.boxes, dtype=np.int32)
        if owner is None:
            self.level, self.gids = level, np.arange(level.nboxes)
            self.h = ctx.lib.pa_level_create(ctx.h, level.nboxes, b.ctypes.data_as(C.POINTER(C.c_int32)), _i3(level.domlo), _i3(level.domhi),
                                             _i3(level.is_per), _d3(level.prob_lo), _d3(level.prob_hi))
        else:
            o = np.ascontiguousarray(owner, dtype=np.int32)
            assert len(o) == level.nboxes
            self.gids = np.nonzero(o == rank)[0]
            self.level = Level(level.boxes[self.gids], level.domlo, level.domhi, level.is_per, level.prob_lo, level.prob_hi)
            self.h = ctx.lib.pa_level_create_sharded(ctx.h, level.nboxes, b.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     int(rank), int(nranks), _i3(level.domlo), _i3(level.domhi), _i3(level.is_per),
                                                     _d3(level.prob_lo), _d3(level.prob_hi))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def close(self):
        """pa_level_destroy: the level's device arrays, cached plans and work multifabs.  There is NO finaliser: a level (and a multifab)
        lives until close() -- or the end of a `with` block -- is reached; destroy the multifabs on a level before the level, the levels
        before their context"""
        if self.h:
            self.ctx.lib.pa_level_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DevMF:
    """MultiFab in HBM.  devptr: optional externally owned device pointer (e.g. torch tensor)."""

    def __init__(self, ctx: Context, dlev: DevLevel, ncomp: int, ng: int, devptr: Optional[int] = None):
        self.ctx, self.dlev, self.ncomp, self.ng = ctx, dlev, int(ncomp), int(ng)
        self.h = ctx.lib.pa_mf_create(ctx.h, dlev.h, ncomp, ng, C.c_void_p(devptr) if devptr else None)
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        self.size = int(ctx.lib.pa_mf_size(self.h))
        self.ptr = int(ctx.lib.pa_mf_data(self.h))

    @classmethod
    def from_host(cls, ctx, dlev, mf: MultiFab) -> "DevMF":
        d = cls(ctx, dlev, mf.ncomp, mf.ng)
        d.upload(mf)
        return d

    def upload(self, mf: MultiFab):
        assert mf.total == self.size, (mf.total, self.size)
        self.ctx.check(self.ctx.lib.pa_mf_upload(self.ctx.h, self.h, mf.data.ctypes.data_as(C.c_void_p)))

    def download(self) -> MultiFab:
        mf = MultiFab(self.dlev.level, self.ncomp, self.ng)
        assert mf.total == self.size
        self.ctx.check(self.ctx.lib.pa_mf_download(self.ctx.h, self.h, mf.data.ctypes.data_as(C.c_void_p)))
        return mf

    def setval(self, v: float, comp: int = 0, ncomp: Optional[int] = None):
        """pa_mf_setval: components comp .. comp + ncomp - 1 (default: all) of every FAB, ghost cells included"""
        self.ctx.check(self.ctx.lib.pa_mf_setval(self.ctx.h, self.h, int(comp), self.ncomp - int(comp) if ncomp is None else int(ncomp), float(v)))

    def fab(self, b: int) -> PaFab:
        """pa_fab for box b (device pointer into this multifab)."""
        lv = self.dlev.level
        off, cs, _ = mf_layout(lv.boxes, self.ncomp, self.ng)
        f = PaFab()
        f.nstride = int(cs[b])
        f.p = self.ptr + 8 * int(off[b])
        for d in range(3):
            f.lo[d] = int(lv.boxes[b, d]) - self.ng
            f.hi[d] = int(lv.boxes[b, 3 + d]) + self.ng
        f.ncomp = self.ncomp
        return f

    def close(self):
        if self.h:
            self.ctx.lib.pa_mf_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def box_of(level: Level, b: int, grow: int = 0) -> PaBox:
    bx = PaBox()
    for d in range(3):
        bx.lo[d] = int(level.boxes[b, d]) - grow
        bx.hi[d] = int(level.boxes[b, 3 + d]) + grow
    return bx


def _handles(mfs: Sequence[Optional[DevMF]]):
    return (C.c_void_p * len(mfs))(*[m.h if m is not None else None for m in mfs])


def bc_from_flags(is_per, sym_dir=(0, 0, 0)):
    """grad.cpp:180-193 / curvature.cpp:428-441"""
    return [BC_PERIODIC if p else (BC_REFLECT_ODD if s else BC_NEUMANN) for p, s in zip(is_per, sym_dir)]


def grad_run(ctx: Context, states: Sequence[DevMF], comp: int, bc, outs: Sequence[DevMF], ocomp: int):
    ctx.check(ctx.lib.pa_grad_run(ctx.h, len(states), _handles(states), comp, _i3(bc), _handles(outs), ocomp))


def curv_params(prog_min=None, prog_max=None, threshold=None, fused=True, do_gauss=False, do_strain=False, strain_tensor=False,
                do_velnormal=False, vel_comp=0, do_smooth=False, smoothing_time=1e-7, spacedim=3) -> PaCurvParams:
    p = PaCurvParams()
    p.spacedim = int(spacedim)
    p.do_smooth, p.smoothing_time = int(do_smooth), float(smoothing_time)
    p.do_gauss_curv, p.do_strain, p.get_strain_tensor, p.do_velnormal, p.vel_comp = int(do_gauss), int(do_strain), int(strain_tensor), int(do_velnormal), int(vel_comp)
    p.prog_min = 1e20 if prog_min is None else prog_min
    p.prog_max = -1e20 if prog_max is None else prog_max
    p.do_threshold = 0 if threshold is None else 1
    p.threshold = 0.0 if threshold is None else float(threshold)
    p.fused = 1 if fused else 0
    return p


def curvature_run(ctx, states, comp, bc, params: PaCurvParams, outs, ocomp):
    ctx.check(ctx.lib.pa_curvature_run(ctx.h, len(states), _handles(states), comp, _i3(bc), C.byref(params), _handles(outs), ocomp))


def gradcurv_run(ctx, states, comp, bc, params: PaCurvParams, works, outs, ocomp):
    ctx.check(ctx.lib.pa_gradcurv_run(ctx.h, len(states), _handles(states), comp, _i3(bc), C.byref(params), _handles(works),
                                      _handles(outs), ocomp))


def gradcurv_run_comps(ctx, states, comp0, ncomps, bc, params: PaCurvParams, works, outs, ocomp, done=None):
    """pa_gradcurv_run_comps; done(comp) is called when a component's results are complete in outs (sync before reading)"""
    err = []

    def _cb(user, comp):
        try:
            done(comp)
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            err.append(e)
            return 1
    cb = DONE_FN(_cb) if done is not None else C.cast(None, DONE_FN)
    rc = ctx.lib.pa_gradcurv_run_comps(ctx.h, len(states), _handles(states), int(comp0), int(ncomps), _i3(bc), C.byref(params), _handles(works),
                                       _handles(outs), int(ocomp), cb, None)
    if err:
        raise err[0]
    ctx.check(rc)


def gradcurv_run_comps2(ctx, states, comp0, ncomps, bc, params: PaCurvParams, works, outs, ocomp, nbatch, done=None):
    """pa_gradcurv_run_comps2: batches of nbatch components, outs hold nbatch slots of 8 components from ocomp;
    done(comp, ocomp_of_its_slot) is called for every component of a batch once the batch is complete (sync before reading)"""
    err = []

    def _cb(user, comp, oc):
        try:
            done(comp, oc)
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            err.append(e)
            return 1
    cb = DONE2_FN(_cb) if done is not None else C.cast(None, DONE2_FN)
    rc = ctx.lib.pa_gradcurv_run_comps2(ctx.h, len(states), _handles(states), int(comp0), int(ncomps), _i3(bc), C.byref(params), _handles(works),
                                        _handles(outs), int(ocomp), int(nbatch), cb, None)
    if err:
        raise err[0]
    ctx.check(rc)


def mc_hierarchy(ctx: Context, states, fine_mask, loops_per_level, isocomp: int, isoval: float, download: bool = True, ratio: int = 2, xyz: bool = False):
    """pa_mc_hierarchy_fine: marching cubes on every level in one call.  states: DevMF per level; fine_mask: flag per level
    (mask by the next finer level); loops_per_level: (nboxes, 6) arrays.  Returns per level the per-box list
    [(verts, vkeys, tris)] (download=False: only the per-box counts [(nv, nt)]).
    xyz=True: pa_mc_hierarchy_xyz -- the states hold the fields only (isocomp among them), vertex coordinates come from cell indices"""
    nlev = len(states)
    arrs, nvs, nts = [], [], []
    for l in range(nlev):
        lp = np.asarray(loops_per_level[l], dtype=np.int64).reshape(-1, 6)
        nb = len(lp)
        arr = (PaBox * max(nb, 1))()
        for b in range(nb):
            for d in range(3):
                arr[b].lo[d], arr[b].hi[d] = int(lp[b, d]), int(lp[b, 3 + d])
        arrs.append(arr)
        nvs.append((C.c_int64 * max(nb, 1))())
        nts.append((C.c_int64 * max(nb, 1))())
    parr = (C.POINTER(PaBox) * nlev)(*[C.cast(a, C.POINTER(PaBox)) for a in arrs])
    pnv = (C.POINTER(C.c_int64) * nlev)(*[C.cast(a, C.POINTER(C.c_int64)) for a in nvs])
    pnt = (C.POINTER(C.c_int64) * nlev)(*[C.cast(a, C.POINTER(C.c_int64)) for a in nts])
    fm = (C.c_int32 * nlev)(*[int(bool(f)) for f in fine_mask])
    pv, pk, pt = (C.c_void_p * nlev)(), (C.c_void_p * nlev)(), (C.c_void_p * nlev)()
    block = C.c_void_p()
    fn = ctx.lib.pa_mc_hierarchy_xyz if xyz else ctx.lib.pa_mc_hierarchy_fine
    ctx.check(fn(ctx.h, nlev, _handles(states), fm, int(ratio), parr, int(isocomp), float(isoval), pnv, pnt, pv, pk, pt, C.byref(block)))
    out = []
    try:
        for l in range(nlev):
            nb = len(np.asarray(loops_per_level[l]).reshape(-1, 6))
            nv, nt = nvs[l], nts[l]
            if not download:
                out.append([(int(nv[b]), int(nt[b])) for b in range(nb)])
                continue
            nc = states[l].ncomp + (3 if xyz else 0)
            tv, tt = int(sum(nv[:nb])), int(sum(nt[:nb]))
            V = np.empty((tv, nc)); K = np.empty((tv, 6), np.int32); T = np.empty((tt, 3), np.int32)
            if tv:
                ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, V.ctypes.data_as(C.c_void_p), pv[l], V.nbytes))
                ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, K.ctypes.data_as(C.c_void_p), pk[l], K.nbytes))
            if tt:
                ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, T.ctypes.data_as(C.c_void_p), pt[l], T.nbytes))
            lev, ov, ot = [], 0, 0
            for b in range(nb):
                lev.append((V[ov:ov + nv[b]], K[ov:ov + nv[b]], T[ot:ot + nt[b]]))
                ov += nv[b]; ot += nt[b]
            out.append(lev)
    finally:
        if block.value:
            ctx.lib.pa_device_free(ctx.h, block)
    return out


def sdf_level_set(ctx: Context, meshes, exact_band: int = 1):
    """pa_sdf_level_set3 on a batch: meshes = list of (tris (nt,3) uint32, verts (nv,3) float32, origin, dx, (ni,nj,nk));
    returns the list of phi arrays, float32 (nk, nj, ni)."""
    grids = (PaSdfGrid * len(meshes))()
    keep, outs = [], []
    for g, (tris, verts, origin, dx, n) in zip(grids, meshes):
        tris = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        dt = DevBuf.from_numpy(ctx, tris) if len(tris) else None
        dv = DevBuf.from_numpy(ctx, verts) if len(verts) else None
        ni, nj, nk = (int(v) for v in n)
        dp = DevBuf(ctx, 4 * ni * nj * nk)
        keep += [dt, dv]
        outs.append((dp, (nk, nj, ni)))
        g.ntri, g.tri, g.nvert, g.x = len(tris), (dt.ptr if dt else None), len(verts), (dv.ptr if dv else None)
        for d in range(3):
            g.origin[d] = np.float32(origin[d])
            g.n[d] = (ni, nj, nk)[d]
        g.dx = np.float32(dx)
        g.phi = dp.ptr
    ctx.check(ctx.lib.pa_sdf_level_set3(ctx.h, len(meshes), grids, int(exact_band)))
    ctx.sync()
    return [dp.to_numpy(np.float32, shape) for dp, shape in outs]


def smooth_solve(ctx, rhs, rcomp, sol, scomp, dt, bc, tol=1e-12, maxiter=100):
    """pa_smooth_solve; returns (iterations, relative residual)"""
    it, res = C.c_int(0), C.c_double(0.0)
    ctx.check(ctx.lib.pa_smooth_solve(ctx.h, len(rhs), _handles(rhs), rcomp, _handles(sol), scomp, float(dt), _i3(bc), float(tol), int(maxiter),
                                      C.byref(it), C.byref(res)))
    return it.value, res.value


def stream_trace(ctx, vfield, vcomp, seeds, nsteps, dt):
    """pa_stream_trace -> (pos float64 [2*nseed][nsteps][3], number of redistributions)"""
    seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    n = len(seeds)
    buf = DevBuf(ctx, max(8 * 2 * n * nsteps * 3, 8))
    nred = C.c_int32(0)
    ctx.check(ctx.lib.pa_stream_trace(ctx.h, len(vfield), _handles(vfield), int(vcomp), n, seeds.ctypes.data_as(C.POINTER(C.c_double)), int(nsteps),
                                      float(dt), C.c_void_p(buf.ptr), C.byref(nred)))
    if n == 0:  # nothing to copy back
        return np.zeros((0, nsteps, 3)), nred.value
    return buf.to_numpy(np.float64, (2 * n, nsteps, 3)), nred.value


def _dev_fab(buf: "DevBuf", lo, shape_zyx, ncomp: int, comp0: int = 0) -> PaFab:
    """PaFab over a dense FAB [ncomp][nz][ny][nx] in buf whose cell lo..lo+shape-1 (component comp0 first)"""
    f = PaFab()
    n = int(np.prod(shape_zyx))
    f.p = buf.ptr + 8 * comp0 * n
    for d in range(3):
        f.lo[d] = int(lo[d])
        f.hi[d] = int(lo[d]) + int(shape_zyx[2 - d]) - 1
    f.ncomp = int(ncomp) - int(comp0)
    f.nstride = n
    return f


def vtrace_fab(ctx: Context, T: np.ndarray, T_lo, loc: np.ndarray, ids, nRKsteps: int, dx, plo, phi, hRK: float, g_lo=None, g_hi=None, vcomp=None):
    """pa_vtrace_fab: vtrace of stream_nd.f90 on one FAB.  T [nT][nz][ny][nx] on T_lo..; loc [3][N] node coordinates; ids 1-based.
    vcomp None: computeVec = 1 with g over g_lo..g_hi (default: T's box grown by -1); else the vector field is T's components
    vcomp..vcomp+2 over T's box (traceAlongV).  -> (strm [3+nT][nRKsteps][n_ids], g [3][..] or None, errFlag)"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    loc = np.ascontiguousarray(loc, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    nT, n = T.shape[0], len(ids)
    nRKh = (nRKsteps - 1) // 2
    tb = DevBuf.from_numpy(ctx, T)
    tf = _dev_fab(tb, T_lo, T.shape[1:], nT)
    if vcomp is None:
        glo = np.asarray(T_lo if g_lo is None else g_lo) + (1 if g_lo is None else 0)
        ghi = (np.asarray(T_lo) + np.array(T.shape[:0:-1]) - 2) if g_hi is None else np.asarray(g_hi)
        gshape = tuple(int(v) for v in (ghi - glo + 1)[::-1])
        gb = DevBuf(ctx, 8 * 3 * int(np.prod(gshape)))
        gf = _dev_fab(gb, glo, gshape, 3)
    else:
        gb, gshape = None, None
        gf = _dev_fab(tb, T_lo, T.shape[1:], nT, vcomp)
    lb = DevBuf.from_numpy(ctx, loc)
    ib = DevBuf.from_numpy(ctx, ids if n else np.zeros(1, np.int32))
    sb = DevBuf(ctx, max(8, 8 * (3 + nT) * nRKsteps * n))
    sf = _dev_fab(sb, (0, -nRKh, 0), (1, nRKsteps, max(n, 1)), 3 + nT)
    sf.hi[0] = n - 1
    err = C.c_int32(0)
    ctx.check(ctx.lib.pa_vtrace_fab(ctx.h, C.byref(tf), nT, C.c_void_p(lb.ptr), loc.shape[1], C.c_void_p(ib.ptr), n, C.byref(gf), 1 if vcomp is None else 0,
                                    C.byref(sf), 3 + nT, _d3(dx), _d3(plo), _d3(phi), float(hRK), C.byref(err)))
    strm = sb.to_numpy(np.float64, (3 + nT, nRKsteps, n))
    g = gb.to_numpy(np.float64, (3,) + gshape) if gb is not None else None
    return strm, g, err.value


def streamgrad_prepare(ctx: Context, states: Sequence[DevMF]):
    """pa_streamgrad_prepare: the ghost cells of stream.cpp:796-884 on every level, in place"""
    ctx.check(ctx.lib.pa_streamgrad_prepare(ctx.h, len(states), _handles(states)))


def streamgrad_trace(ctx: Context, states: Sequence[DevMF], nodes: np.ndarray, ins, nRKsteps: int, hRK: float, vcomp=None):
    """pa_streamgrad_trace.  nodes [3][N]; ins[l][b] = 1-based node ids of (level l, box b).  -> (per level per box: strm
    [3+nT][nRKsteps][n] or None, per level per box errFlag)"""
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    counts = [len(ids) for per in ins for ids in per]
    start = np.zeros(len(counts) + 1, dtype=np.int64)
    start[1:] = np.cumsum(counts)
    nlines = int(start[-1])
    ncs = 3 + states[0].ncomp
    allids = np.concatenate([np.asarray(ids, np.int32) for per in ins for ids in per] + [np.zeros(0, np.int32)])
    nb = DevBuf.from_numpy(ctx, nodes)
    ib = DevBuf.from_numpy(ctx, allids if nlines else np.zeros(1, np.int32))
    sb = DevBuf(ctx, max(8, 8 * nlines * nRKsteps * ncs))
    flags = np.zeros(len(counts), dtype=np.int32)
    ctx.check(ctx.lib.pa_streamgrad_trace(ctx.h, len(states), _handles(states), -1 if vcomp is None else int(vcomp), nodes.shape[1], C.c_void_p(nb.ptr),
                                          start.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(ib.ptr), int(nRKsteps), float(hRK), C.c_void_p(sb.ptr),
                                          flags.ctypes.data_as(C.POINTER(C.c_int32))))
    flat = sb.to_numpy(np.float64, (max(nlines, 1) * nRKsteps * ncs,))
    out, fl, g = [], [], 0
    for per in ins:
        o, f = [], []
        for ids in per:
            n = len(ids)
            if n == 0:
                o.append(None)
            else:
                s0 = int(start[g]) * nRKsteps * ncs
                o.append(flat[s0:s0 + n * nRKsteps * ncs].reshape(ncs, nRKsteps, n).copy())
            f.append(int(flags[g]))
            g += 1
        out.append(o)
        fl.append(f)
    return out, fl


def streamalt_nout(carry=(), thickComp=-1, TComp=-1, addAngle=False):
    """components and queries of pa_streamalt_run for these options -> (nout, nquery)"""
    return 3 + len(carry) + 1 + (thickComp >= 0) + (TComp >= 0) + bool(addAngle), 1 + 2 * (thickComp >= 0) + (TComp >= 0)


def streamalt_run(ctx: Context, lines, ins, nRKsteps: int, nNodes: int, isoComp: int, altVal: float, carry=(), thickComp: int = -1, thickLo: float = 0.0,
                  thickHi: float = 0.0, TComp: int = -1, TVal: float = 0.0, strainComp: int = -1, addAngle: bool = False, with_branch: bool = True,
                  out_fill=None, ncs: Optional[int] = None):
    """pa_streamalt_run on lines in streamgrad_trace's form: lines[l][b] = [ncs][nRKsteps][n] or None, ins[l][b] = the 1-based node ids
    of those lines; or lines = (DevBuf of the trace's flat buffer, ncs).  out_fill: the uint64 bit pattern every output double
    starts with (the int8 branch codes start as -1).  -> (out [nout][nNodes] -- the angle column holds the COSINE --, branch int8
    [nquery][nNodes] or None)"""
    counts = [len(ids) for per in ins for ids in per]
    start = np.zeros(len(counts) + 1, dtype=np.int64)
    start[1:] = np.cumsum(counts)
    nlines = int(start[-1])
    allids = np.concatenate([np.asarray(ids, np.int32) for per in ins for ids in per] + [np.zeros(0, np.int32)])
    if isinstance(lines, tuple):
        sb, ncs = lines
    else:
        live = [np.ascontiguousarray(x, dtype=np.float64) for per in lines for x in per if x is not None]
        if ncs is None:
            ncs = live[0].shape[0]
        sb = _dev(ctx, np.concatenate([x.ravel() for x in live] + [np.zeros(0)]))
    ib = _dev(ctx, allids)
    nout, nq = streamalt_nout(carry, thickComp, TComp, addAngle)
    fill = np.full(nout * max(nNodes, 1), np.nan) if out_fill is None else np.full(nout * max(nNodes, 1), out_fill, dtype=np.uint64).view(np.float64)
    ob = DevBuf.from_numpy(ctx, fill)
    bb = DevBuf.from_numpy(ctx, np.full(max(nq * nNodes, 8), -1, dtype=np.int8)) if with_branch else None
    P = PaStreamAltParams()
    P.isoComp, P.altVal, P.ncarry = int(isoComp), float(altVal), len(carry)
    if len(carry) > 8:
        raise PaError("pa_streamalt_run: more than 8 carried components")
    for k, c in enumerate(carry):
        P.carry[k] = int(c)
    P.thickComp, P.thickLo, P.thickHi = int(thickComp), float(thickLo), float(thickHi)
    P.TComp, P.strainComp, P.TVal, P.addAngle = int(TComp), int(strainComp), float(TVal), int(bool(addAngle))
    ctx.check(ctx.lib.pa_streamalt_run(ctx.h, len(counts), start.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(ib.ptr), C.c_void_p(sb.ptr), int(ncs),
                                       int(nRKsteps), int(nNodes), C.byref(P), C.c_void_p(ob.ptr), C.c_void_p(bb.ptr) if bb is not None else None))
    out = ob.to_numpy(np.float64, (nout, nNodes))
    return out, (bb.to_numpy(np.int8, (nq, nNodes)) if bb is not None else None)


def interpstream_fab(ctx: Context, loc: np.ndarray, loc_lo, fab: np.ndarray, fab_lo, dx, plo):
    """pa_interpstream_fab: interpstream of sampleStreamlines_nd.f90 on one FAB.  loc [nl][nz][ny][nx] on loc_lo.. (X / Y / Z
    first); fab [np][..] on fab_lo...  -> (strm [np][nz][ny][nx] -- NaN where nothing was written --, status 0 / 1 / 2)"""
    loc = np.ascontiguousarray(loc, dtype=np.float64)
    fab = np.ascontiguousarray(fab, dtype=np.float64)
    lb, fb = DevBuf.from_numpy(ctx, loc), DevBuf.from_numpy(ctx, fab)
    sb = DevBuf.from_numpy(ctx, np.full((fab.shape[0],) + loc.shape[1:], np.nan))
    lf, ff, sf = _dev_fab(lb, loc_lo, loc.shape[1:], loc.shape[0]), _dev_fab(fb, fab_lo, fab.shape[1:], fab.shape[0]), _dev_fab(sb, loc_lo, loc.shape[1:], fab.shape[0])
    st = C.c_int32(0)
    ctx.check(ctx.lib.pa_interpstream_fab(ctx.h, C.byref(lf), loc.shape[0], C.byref(ff), fab.shape[0], C.byref(sf), _d3(dx), _d3(plo), C.byref(st)))
    return sb.to_numpy(np.float64, (fab.shape[0],) + loc.shape[1:]), st.value


def set_distance_fab(ctx: Context, loc: np.ndarray, loc_lo):
    """pa_set_distance_fab: set_distance of sampleStreamlines_nd.f90.  loc [>= 3][nz][ny][nx] on loc_lo..  -> res [nz][ny][nx]"""
    loc = np.ascontiguousarray(loc, dtype=np.float64)
    lb = DevBuf.from_numpy(ctx, loc)
    rb = DevBuf.from_numpy(ctx, np.full(loc.shape[1:], np.nan))
    lf, rf = _dev_fab(lb, loc_lo, loc.shape[1:], loc.shape[0]), _dev_fab(rb, loc_lo, loc.shape[1:], 1)
    ctx.check(ctx.lib.pa_set_distance_fab(ctx.h, C.byref(lf), C.byref(rf)))
    return rb.to_numpy(np.float64, loc.shape[1:])


def streamsample_run(ctx: Context, data: Sequence[DevMF], K: int, file_dx, plo, is_per, str_boxes, has_lines, bbox, xyz, ncout: int, dcomp: int = 4,
                     with_xyzd: bool = True, out: Optional["DevBuf"] = None):
    """pa_streamsample_run.  str_boxes[l] = [nb][6] Str boxes of level l; has_lines / bbox per level per box; xyz[l][b] = [3][nj][ni] path
    coordinates.  out: the device result of an earlier pass (the next pass writes its components into it).  -> (out DevBuf,
    per level per box [ncout][nj][ni] arrays, per level per box status)"""
    nbox = np.array([len(b) for b in str_boxes], dtype=np.int32)
    sb = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32).reshape(-1, 6) for b in str_boxes]), dtype=np.int32)
    hl = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32).ravel() for h in has_lines]), dtype=np.int32)
    bb = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32).reshape(-1, 6) for b in bbox]), dtype=np.int32)
    flat = [np.asarray(x, np.float64) for per in xyz for x in per]
    npts = [int(x[0].size) for x in flat]
    xs = np.concatenate([x.reshape(3, -1).ravel() for x in flat])
    xb = DevBuf.from_numpy(ctx, xs)
    if out is None:
        out = DevBuf.from_numpy(ctx, np.full(ncout * sum(npts), np.nan))
    fdx = np.ascontiguousarray(np.asarray(file_dx, np.float64).reshape(-1, 3)[:len(data)])
    fail = np.zeros(len(hl), dtype=np.int32)
    ctx.check(ctx.lib.pa_streamsample_run(ctx.h, len(data), _handles(data), int(K), fdx.ctypes.data_as(C.POINTER(C.c_double)), _d3(plo), _i3(is_per),
                                          nbox.ctypes.data_as(C.POINTER(C.c_int32)), sb.ctypes.data_as(C.POINTER(C.c_int32)),
                                          hl.ctypes.data_as(C.POINTER(C.c_int32)), bb.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(xb.ptr),
                                          C.c_void_p(out.ptr), int(ncout), int(dcomp), int(bool(with_xyzd)), fail.ctypes.data_as(C.POINTER(C.c_int32))))
    allv = out.to_numpy(np.float64, (ncout * sum(npts),))
    res, st, g, o = [], [], 0, 0
    for per in xyz:
        r, s = [], []
        for x in per:
            n = int(np.asarray(x)[0].size)
            r.append(allv[o:o + ncout * n].reshape((ncout,) + np.asarray(x).shape[1:]).copy())
            s.append(int(fail[g]))
            o += ncout * n
            g += 1
        res.append(r)
        st.append(s)
    return out, res, st


def _dev(ctx: Context, a) -> "DevBuf":
    """a DevBuf as it is, a host array uploaded (at least 8 bytes, so that an empty array still has an address)"""
    if isinstance(a, DevBuf):
        return a
    a = np.ascontiguousarray(a)
    return DevBuf.from_numpy(ctx, a) if a.nbytes else DevBuf(ctx, 8)


class Tube:
    """pa_tube (streamTubeStats.cpp): the tables of one stream directory and the calls on them.  box_desc [nbt][4] = (ni, nj, jlo,
    offset in points) of every Str box of every level, node_table [nNodes][2] = (box, line) of node id n + 1, face = the 1-based
    connectivity.  xyz / data arguments: flat buffers in the layout of Tube.flat, host arrays (uploaded) or DevBufs."""

    def __init__(self, ctx: Context, box_desc, node_table, face):
        self.ctx = ctx
        self.box = np.ascontiguousarray(box_desc, dtype=np.int64).reshape(-1, 4)
        self.node = np.ascontiguousarray(node_table, dtype=np.int32).reshape(-1, 2)
        self.face = np.ascontiguousarray(face, dtype=np.int32).reshape(-1, 3)
        self.nNodes, self.nElts = len(self.node), len(self.face)
        self.h = ctx.lib.pa_tube_create(ctx.h, len(self.box), self.box.ctypes.data_as(C.POINTER(C.c_int64)), self.nNodes,
                                        self.node.ctypes.data_as(C.POINTER(C.c_int32)), self.nElts, self.face.ctypes.data_as(C.POINTER(C.c_int32)))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    @staticmethod
    def flat(fabs) -> np.ndarray:
        """fabs[g] = [ncomp][nj][ni] of every box -> box g at ncomp * off_g doubles, component-major, i fastest, then j"""
        return np.concatenate([np.asarray(a, np.float64).ravel() for a in fabs]) if len(fabs) else np.zeros(0)

    def _out(self, n):
        return DevBuf(self.ctx, max(8, 8 * int(n)))

    def wedges(self, xyz, data, K: int, jlo: int, nPtsOnStr: int, with_geom: bool = True):
        """pa_tube_wedges -> (vol, area, wa [nElts] or None without with_geom, ints_raw [K][nElts], ints_per_area [K][nElts])"""
        E = self.nElts
        x, d = _dev(self.ctx, xyz), _dev(self.ctx, data)
        vol, area, wa, raw, per = self._out(E), self._out(E), self._out(E), self._out(K * E), self._out(K * E)
        self.ctx.check(self.ctx.lib.pa_tube_wedges(self.ctx.h, self.h, x.ptr, d.ptr, int(K), int(jlo), int(nPtsOnStr), int(bool(with_geom)), vol.ptr, area.ptr,
                                                   wa.ptr, raw.ptr, per.ptr))
        g = tuple(b.to_numpy(np.float64, (E,)) for b in (vol, area, wa)) if with_geom else (None, None, None)
        return g + (raw.to_numpy(np.float64, (K, E)), per.to_numpy(np.float64, (K, E)))

    def lines(self, xyz, data, ncomp: int, comp: int, use_eps: bool = False) -> np.ndarray:
        """pa_tube_lines -> gradmax [nNodes]"""
        x, d, o = _dev(self.ctx, xyz), _dev(self.ctx, data), self._out(self.nNodes)
        self.ctx.check(self.ctx.lib.pa_tube_lines(self.ctx.h, self.h, x.ptr, d.ptr, int(ncomp), int(comp), int(bool(use_eps)), o.ptr))
        return o.to_numpy(np.float64, (self.nNodes,))

    def peaks(self, data, ncomp: int, pcomp: int, sample_comps=()):
        """pa_tube_peaks -> (peak_samples [nsample][nNodes], ok [nNodes] bool)"""
        sc = np.ascontiguousarray(sample_comps, dtype=np.int32)
        d, o, k = _dev(self.ctx, data), self._out(len(sc) * self.nNodes), self._out(self.nNodes)
        self.ctx.check(self.ctx.lib.pa_tube_peaks(self.ctx.h, self.h, d.ptr, int(ncomp), int(pcomp), len(sc), sc.ctypes.data_as(C.POINTER(C.c_int32)), o.ptr, k.ptr))
        return o.to_numpy(np.float64, (len(sc), self.nNodes)), k.to_numpy(np.int32, (self.nNodes,)) != 0

    def node_means(self, vals) -> np.ndarray:
        """pa_tube_node_means: vals [nv][nNodes] -> [nv][nElts]"""
        vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, self.nNodes)
        v, o = _dev(self.ctx, vals), self._out(len(vals) * self.nElts)
        self.ctx.check(self.ctx.lib.pa_tube_node_means(self.ctx.h, self.h, len(vals), v.ptr, o.ptr))
        return o.to_numpy(np.float64, (len(vals), self.nElts))

    def node_all(self, ok) -> np.ndarray:
        """pa_tube_node_all: ok [nNodes] -> [nElts] 1.0 / 0.0"""
        k, o = _dev(self.ctx, np.ascontiguousarray(ok, dtype=np.int32)), self._out(self.nElts)
        self.ctx.check(self.ctx.lib.pa_tube_node_all(self.ctx.h, self.h, k.ptr, o.ptr))
        return o.to_numpy(np.float64, (self.nElts,))

    def node_avg(self, data, ncomp: int, comp: int) -> np.ndarray:
        """pa_tube_node_avg -> [nElts]"""
        d, o = _dev(self.ctx, data), self._out(self.nElts)
        self.ctx.check(self.ctx.lib.pa_tube_node_avg(self.ctx.h, self.h, d.ptr, int(ncomp), int(comp), o.ptr))
        return o.to_numpy(np.float64, (self.nElts,))

    def smooth(self, vals, area, nSmooth: int) -> np.ndarray:
        """pa_tube_smooth -> [nElts]"""
        v, a, o = _dev(self.ctx, np.asarray(vals, np.float64)), _dev(self.ctx, np.asarray(area, np.float64)), self._out(self.nElts)
        self.ctx.check(self.ctx.lib.pa_tube_smooth(self.ctx.h, self.h, v.ptr, a.ptr, int(nSmooth), o.ptr))
        return o.to_numpy(np.float64, (self.nElts,))

    def neighbors(self):
        """pa_tube_neighbors -> (rowptr [nElts + 1] int64, cols [nnz] int32)"""
        nnz = C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_tube_neighbors(self.ctx.h, self.h, C.byref(nnz), None, None))
        rp, cols = np.zeros(self.nElts + 1, np.int64), np.zeros(max(nnz.value, 1), np.int32)
        self.ctx.check(self.ctx.lib.pa_tube_neighbors(self.ctx.h, self.h, C.byref(nnz), rp.ctypes.data_as(C.POINTER(C.c_int64)), cols.ctypes.data_as(C.POINTER(C.c_int32))))
        return rp, cols[:nnz.value]

    def close(self):
        if self.h:
            self.ctx.lib.pa_tube_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.close()
        except Exception:
            pass


SSEL_MAX, SSEL_MIN, SSEL_RXY, SSEL_AT = 0, 1, 2, 3
SSEL_SIGNS = {"ge": 0, "gt": 1, "lt": 2, "le": 3, "eq": 4, "ne": 5}  # do_test (stream2plt.cpp:732-751); any other string tests false (-1)


class StreamSel:
    """pa_ssel (streamScatter.cpp, stream2plt.cpp): the tables of one stream directory -- box_desc and node_table as for Tube -- and
    the selection calls on them.  data arguments: flat buffers in the layout of Tube.flat, host arrays (uploaded) or DevBufs."""

    def __init__(self, ctx: Context, box_desc, node_table=(), out_fill=None, int_fill=None):
        """out_fill / int_fill: the uint64 / int32 bit pattern every output double / int starts from (tests: a sentinel no call may
        leave behind); None: whatever the allocation holds (zeros for the dense array of gather_lines)"""
        self.ctx, self.out_fill, self.int_fill = ctx, out_fill, int_fill
        self.box = np.ascontiguousarray(box_desc, dtype=np.int64).reshape(-1, 4)
        self.node = np.ascontiguousarray(node_table, dtype=np.int32).reshape(-1, 2)
        self.nNodes = len(self.node)
        self.h = ctx.lib.pa_ssel_create(ctx.h, len(self.box), self.box.ctypes.data_as(C.POINTER(C.c_int64)), self.nNodes,
                                        self.node.ctypes.data_as(C.POINTER(C.c_int32)))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def _f64(self, n) -> "DevBuf":
        n = max(1, int(n))
        return DevBuf(self.ctx, 8 * n) if self.out_fill is None else DevBuf.from_numpy(self.ctx, np.full(n, self.out_fill, dtype=np.uint64))

    def _i32(self, n) -> "DevBuf":
        n = max(2, int(n))
        return DevBuf(self.ctx, 4 * n) if self.int_fill is None else DevBuf.from_numpy(self.ctx, np.full(n, self.int_fill, dtype=np.int32))

    def peaks(self, data, ncomp: int, comp: int, on_device: bool = False):
        """pa_ssel_peaks -> (jpeak [nNodes] int32, hival [nNodes]); on_device: the two DevBufs"""
        N = self.nNodes
        d, j, h = _dev(self.ctx, data), self._i32(N), self._f64(N)
        self.ctx.check(self.ctx.lib.pa_ssel_peaks(self.ctx.h, self.h, d.ptr, int(ncomp), int(comp), j.ptr, h.ptr))
        return (j, h) if on_device else (j.to_numpy(np.int32, (N,)), h.to_numpy(np.float64, (N,)))

    def scatter(self, data, ncomp: int, comps, jpeak, hival, more_than: float, less_than: float, group: Optional[int] = None) -> np.ndarray:
        """pa_ssel_scatter -> [nkept][len(comps)], the kept nodes in node-id order; group: variables per call (the same rows)"""
        comps = np.ascontiguousarray(comps, dtype=np.int32)
        d = _dev(self.ctx, data)
        j = jpeak if isinstance(jpeak, DevBuf) else _dev(self.ctx, np.asarray(jpeak, np.int32))
        h = hival if isinstance(hival, DevBuf) else _dev(self.ctx, np.asarray(hival, np.float64))
        n = C.c_int64(-1)
        self.ctx.check(self.ctx.lib.pa_ssel_scatter(self.ctx.h, self.h, None, int(ncomp), 0, None, None, h.ptr, float(more_than), float(less_than), 0, 0, None,
                                                    C.byref(n)))
        nv = len(comps)
        out = self._f64(n.value * nv)
        group = group or 64
        for c0 in range(0, nv, group):
            part, m = comps[c0:c0 + group], C.c_int64(-1)
            self.ctx.check(self.ctx.lib.pa_ssel_scatter(self.ctx.h, self.h, d.ptr, int(ncomp), len(part), part.ctypes.data_as(C.POINTER(C.c_int32)), j.ptr, h.ptr,
                                                        float(more_than), float(less_than), nv, c0, out.ptr, C.byref(m)))
            assert m.value == n.value
        return out.to_numpy(np.float64, (n.value, nv))

    def gather_lines(self, data, ncomp: int, comps, sel, slo: int, shi: int, extra: int = 0, on_device: bool = False):
        """pa_ssel_gather_lines -> final [len(comps) + extra][shi - slo + 1][nSel]; the extra components are zero (out_fill: the whole array starts as the pattern)"""
        comps = np.ascontiguousarray(comps, dtype=np.int32)
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1, 2)
        shape = (len(comps) + extra, shi - slo + 1, len(sel))
        d, f = _dev(self.ctx, data), (self._f64(np.prod(shape)) if self.out_fill is not None else DevBuf.from_numpy(self.ctx, np.zeros(max(1, int(np.prod(shape))))))
        self.ctx.check(self.ctx.lib.pa_ssel_gather_lines(self.ctx.h, self.h, d.ptr, int(ncomp), len(comps), comps.ctypes.data_as(C.POINTER(C.c_int32)), len(sel),
                                                         sel.ctypes.data_as(C.POINTER(C.c_int32)), int(slo), int(shi), f.ptr))
        return f if on_device else f.to_numpy(np.float64, shape)

    def filter(self, final, ncompSel: int, slo: int, shi: int, nSel: int, conds) -> np.ndarray:
        """pa_ssel_filter -> write_lines [nSel] int32.  conds: (kind, comp, comp2, sgn string or code, val, val2)"""
        arr = (PaSselCond * max(1, len(conds)))()
        for q, (kind, comp, comp2, sgn, val, val2) in zip(arr, conds):
            q.kind, q.comp, q.comp2, q.val, q.val2 = int(kind), int(comp), int(comp2), float(val), float(val2)
            q.sgn = SSEL_SIGNS.get(sgn, -1) if isinstance(sgn, str) else int(sgn)
        f, w = _dev(self.ctx, final), self._i32(nSel)
        self.ctx.check(self.ctx.lib.pa_ssel_filter(self.ctx.h, f.ptr, int(ncompSel), int(slo), int(shi), int(nSel), len(conds), arr, w.ptr))
        return w.to_numpy(np.int32, (nSel,))

    def arclength(self, final, ncompSel: int, npts: int, nSel: int, distComp: int, distVal: float) -> np.ndarray:
        """pa_ssel_arclength on final [ncompSel + 1][npts][nSel] (a host array is uploaded) -> the array with component ncompSel filled"""
        f = _dev(self.ctx, final)
        self.ctx.check(self.ctx.lib.pa_ssel_arclength(self.ctx.h, f.ptr, int(ncompSel), int(npts), int(nSel), int(distComp), float(distVal)))
        return f.to_numpy(np.float64, (ncompSel + 1, npts, nSel))

    def close(self):
        if self.h:
            self.ctx.lib.pa_ssel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.close()
        except Exception:
            pass


class StreamSub:
    """pa_ssub (streamSub.cpp): the subset of one stream directory that a list of surface elements needs, on the tables of a StreamSel.
    face [nElts][npe] 1-based node ids and elts [nSel] 0-based element indices: host arrays (uploaded) or DevBufs.  out_fill / int_fill
    as for StreamSel: the pattern every output starts from."""

    PATHS = {1: "one_workgroup", 2: "block_sums"}

    def __init__(self, sel: "StreamSel", face, npe: int, elts, nElts: Optional[int] = None, nSel: Optional[int] = None):
        self.sel, self.ctx, self.npe, self.h = sel, sel.ctx, int(npe), None
        self.face = face if isinstance(face, DevBuf) else _dev(self.ctx, np.ascontiguousarray(face, dtype=np.int32))
        self.nElts = int(nElts) if nElts is not None else np.asarray(face).size // self.npe
        e = elts if isinstance(elts, DevBuf) else _dev(self.ctx, np.ascontiguousarray(elts, dtype=np.int32))
        self.nSel = int(nSel) if nSel is not None else len(elts)
        self.h = self.ctx.lib.pa_ssub_plan(self.ctx.h, sel.h, self.nElts, self.npe, self.face.ptr, self.nSel, e.ptr)
        if not self.h:
            raise PaError(self.ctx.lib.pa_last_error(self.ctx.h).decode())

    @staticmethod
    def select_seedbox(sel: "StreamSel", data, ncomp: int, face, npe: int, lo, hi, nElts: Optional[int] = None, on_device: bool = False):
        """pa_ssub_select_seedbox -> (the kept element indices, ascending; launch = dict(elements, blocks, scan_passes, kept)); on_device: the
        DevBuf of nElts ints and the count instead of the array"""
        ctx = sel.ctx
        f = face if isinstance(face, DevBuf) else _dev(ctx, np.ascontiguousarray(face, dtype=np.int32))
        nElts = int(nElts) if nElts is not None else np.asarray(face).size // int(npe)
        d, e = _dev(ctx, data), sel._i32(nElts)
        n, rec = C.c_int64(-1), np.full(4, -1, np.int64)
        ctx.check(ctx.lib.pa_ssub_select_seedbox(ctx.h, sel.h, d.ptr, int(ncomp), nElts, int(npe), f.ptr, _d3(lo), _d3(hi), e.ptr, C.byref(n),
                                                 rec.ctypes.data_as(C.POINTER(C.c_int64))))
        launch = dict(zip(("elements", "blocks", "scan_passes", "kept"), (int(v) for v in rec)))
        return ((e, n.value) if on_device else e.to_numpy(np.int32, (max(2, nElts),))[:n.value]), launch

    def counts(self):
        """pa_ssub_counts -> (kept boxes, new nodes, points of the kept boxes)"""
        c = np.zeros(3, np.int64)
        self.ctx.check(self.ctx.lib.pa_ssub_counts(self.h, c.ctypes.data_as(C.POINTER(C.c_int64))))
        return int(c[0]), int(c[1]), int(c[2])

    def gather(self, data, ncomp: int, comps, group: Optional[int] = None, on_device: bool = False):
        """pa_ssub_gather -> the compact buffer [len(comps) * points], flat in the layout of Tube.flat over the kept boxes; group: components
        per call (the same bytes)"""
        comps = np.ascontiguousarray(comps, dtype=np.int32)
        d, out = _dev(self.ctx, data), self.sel._f64(len(comps) * self.counts()[2])
        group = group or 64
        for c0 in range(0, len(comps), group):
            part = np.ascontiguousarray(comps[c0:c0 + group])
            self.ctx.check(self.ctx.lib.pa_ssub_gather(self.ctx.h, self.h, d.ptr, int(ncomp), len(part), part.ctypes.data_as(C.POINTER(C.c_int32)), out.ptr, len(comps), c0))
        return out if on_device else out.to_numpy(np.float64, (len(comps) * self.counts()[2],))

    def read(self, fill=None):
        """pa_ssub_read -> dict(kept [boxes] old flat box index, box_desc [boxes][4], newNum [nNodes], faceSel [nSel][npe]); fill: the int
        every entry starts from"""
        nb = self.counts()[0]
        mk = lambda shape, dt: np.full(shape, 0 if fill is None else fill, dtype=dt)
        kept, box, num, face = mk(nb, np.int32), mk((nb, 4), np.int64), mk(self.sel.nNodes, np.int32), mk((self.nSel, self.npe), np.int32)
        p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self.ctx.check(self.ctx.lib.pa_ssub_read(self.ctx.h, self.h, kept.ctypes.data_as(p32), box.ctypes.data_as(p64), num.ctypes.data_as(p32), face.ctypes.data_as(p32)))
        return dict(kept=kept, box_desc=box, newNum=num, faceSel=face)

    def last_launch(self):
        """pa_ssub_last_launch as a dict"""
        rec = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.lib.pa_ssub_last_launch(self.h, rec.ctypes.data_as(C.POINTER(C.c_int64))))
        out = dict(zip(("nElts", "nSel", "boxes", "kept_boxes", "chunks", "path", "scan_blocks", "gather_blocks"), (int(v) for v in rec)))
        out["path"] = self.PATHS.get(out["path"])
        return out

    def close(self):
        if self.h:
            self.ctx.lib.pa_ssub_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.close()
        except Exception:
            pass


def iso_merge(ctx: Context, fragments, ncomp: int):
    """pa_iso_merge on host fragments [(verts [nv][ncomp], tris [nt][3])] (uploaded here).  Returns (nodes [n][ncomp],
    elts [m][3] int32), or None when the library reports clusters that are not transitive under the tolerance (code 2)."""
    bufs, arr = [], (PaIsoFrag * max(len(fragments), 1))()
    for f, (v, t) in enumerate(fragments):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, ncomp)
        t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
        bv = DevBuf.from_numpy(ctx, v) if len(v) else None
        bt = DevBuf.from_numpy(ctx, t) if len(t) else None
        bufs += [bv, bt]
        arr[f].verts, arr[f].nvert, arr[f].tris, arr[f].ntri = (bv.ptr if bv else None), len(v), (bt.ptr if bt else None), len(t)
    nn, ne, pn, pe = C.c_int64(0), C.c_int64(0), C.c_void_p(), C.c_void_p()
    rc = ctx.lib.pa_iso_merge(ctx.h, len(fragments), arr, int(ncomp), C.byref(nn), C.byref(pn), C.byref(ne), C.byref(pe))
    if rc == 2:
        return None
    ctx.check(rc)
    try:
        nodes, elts = np.empty((nn.value, ncomp)), np.empty((ne.value, 3), np.int32)
        if nn.value:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, nodes.ctypes.data_as(C.c_void_p), pn, nodes.nbytes))
        if ne.value:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, elts.ctypes.data_as(C.c_void_p), pe, elts.nbytes))
    finally:
        for q in (pn, pe):
            if q.value:
                ctx.lib.pa_device_free(ctx.h, q)
    return nodes, elts


def mc_level(ctx: Context, state: "DevMF", mask: "DevMF", loops, isocomp: int, isoval: float, mcomp: int = 0, squares: bool = False):
    """Level-batched marching cubes (pa_mc_level) or, with squares=True, marching squares on the plane k = 0
    (pa_msq_level; segments come back as rows (id0, id1, -1)).  loops: (nboxes, 6) base-point boxes (lo > hi: skipped).
    Returns per-box lists [(verts [nv][ncomp], vkeys [nv][6], tris [nt][3] FAB-local ids)]."""
    loops = np.asarray(loops, dtype=np.int64).reshape(-1, 6)
    nb = len(loops)
    arr = (PaBox * max(nb, 1))()
    for b in range(nb):
        for d in range(3):
            arr[b].lo[d], arr[b].hi[d] = int(loops[b, d]), int(loops[b, 3 + d])
    nv, nt = (C.c_int64 * max(nb, 1))(), (C.c_int64 * max(nb, 1))()
    pv, pk, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    if mask is None or isinstance(mask, DevLevel):  # mask evaluated in the cell pass from the finer level (or nothing masked)
        fn = ctx.lib.pa_msq_level_fine if squares else ctx.lib.pa_mc_level_fine
        ctx.check(fn(ctx.h, state.h, mask.h if mask is not None else None, 2, arr, isocomp, isoval, nv, nt, C.byref(pv), C.byref(pk), C.byref(pt)))
    else:
        fn = ctx.lib.pa_msq_level if squares else ctx.lib.pa_mc_level
        ctx.check(fn(ctx.h, state.h, mask.h, mcomp, arr, isocomp, isoval, nv, nt, C.byref(pv), C.byref(pk), C.byref(pt)))
    nc = state.ncomp
    tv, tt = int(sum(nv[:nb])), int(sum(nt[:nb]))
    try:
        V = np.empty((tv, nc)); K = np.empty((tv, 6), np.int32); T = np.empty((tt, 3), np.int32)
        if tv:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, V.ctypes.data_as(C.c_void_p), pv, V.nbytes))
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, K.ctypes.data_as(C.c_void_p), pk, K.nbytes))
        if tt:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, T.ctypes.data_as(C.c_void_p), pt, T.nbytes))
    finally:
        if pv.value:  # one allocation, base = the vertex array
            ctx.lib.pa_device_free(ctx.h, pv)
    out, ov, ot = [], 0, 0
    for b in range(nb):
        out.append((V[ov:ov + nv[b]], K[ov:ov + nv[b]], T[ot:ot + nt[b]]))
        ov += nv[b]; ot += nt[b]
    return out


# ----------------------------------------------------------------------------- binned statistics (jpdf.cpp / conditionalMean.cpp)
def minmax_comps_level(ctx: Context, mf: "DevMF", comps):
    """pa_minmax_comps_level: (min, max) arrays over every valid cell of the level for the listed components, one launch"""
    c = np.ascontiguousarray(comps, dtype=np.int32)
    mn, mx = np.zeros(len(c)), np.zeros(len(c))
    pd = C.POINTER(C.c_double)
    ctx.check(ctx.lib.pa_minmax_comps_level(ctx.h, mf.h, len(c), c.ctypes.data_as(C.POINTER(C.c_int32)), mn.ctypes.data_as(pd), mx.ctypes.data_as(pd)))
    return mn, mx


def jpdf_params(nload, vmin, vmax, do_stoichiometry=False, hlist=None, olist=None, do_conditioning=0, cvar=0, norm_cval=0, cnorm_min=0.0,
                cnorm_max=1.0, cmin=0.0, cmax=1.0, uncombined=False) -> PaJpdfParams:
    """pa_jpdf_params: the keys of jpdf.cpp:82-243 that the cell loop reads"""
    p = PaJpdfParams()
    p.nload, p.do_stoichiometry = int(nload), int(bool(do_stoichiometry))
    for v, x in enumerate(hlist if hlist is not None else []):
        p.hlist[v] = float(x)
    for v, x in enumerate(olist if olist is not None else []):
        p.olist[v] = float(x)
    for v, (a, b) in enumerate(zip(vmin, vmax)):
        p.vmin[v], p.vmax[v] = float(a), float(b)
    p.do_conditioning, p.cvar, p.norm_cval = int(do_conditioning), int(cvar), int(norm_cval)
    p.cnorm_min, p.cnorm_max, p.cmin, p.cmax = float(cnorm_min), float(cnorm_max), float(cmin), float(cmax)
    p.uncombined = int(bool(uncombined))
    return p


class _Hist:
    def close(self):
        """pa_hist_destroy (no finaliser, as for levels and multifabs)"""
        if self.h:
            self.ctx.lib.pa_hist_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class JpdfAcc(_Hist):
    """the bin / binX1 / binX2 accumulators of all pairs of nvars variables (pa_jpdf_*)"""

    def __init__(self, ctx: Context, nvars: int, nbins: int):
        self.ctx, self.nvars, self.nbins, self.npairs = ctx, int(nvars), int(nbins), int(nvars) * (int(nvars) - 1) // 2
        self.h = ctx.lib.pa_jpdf_create(ctx.h, int(nvars), int(nbins))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def begin(self, vol_max: float, vabs):
        a = np.ascontiguousarray(vabs, dtype=np.float64)
        assert len(a) == self.nvars
        self.ctx.check(self.ctx.lib.pa_jpdf_begin(self.ctx.h, self.h, float(vol_max), a.ctypes.data_as(C.POINTER(C.c_double))))

    def add_level(self, mf: "DevMF", finer: Optional["DevLevel"], ratio: int, vol: float, params: PaJpdfParams):
        """-> (outside [npairs][4] = v1l v1g v2l v2g, nan_cells [npairs]) of this level"""
        out, nan = np.zeros((self.npairs, 4), np.int64), np.zeros(self.npairs, np.int64)
        pi = C.POINTER(C.c_int64)
        self.ctx.check(self.ctx.lib.pa_jpdf_add_level(self.ctx.h, self.h, mf.h, finer.h if finer is not None else None, int(ratio), float(vol),
                                                      C.byref(params), out.ctypes.data_as(pi), nan.ctypes.data_as(pi)))
        return out, nan

    def read(self):
        """raw sums -> bin, binX1, binX2, each [npairs][nbins][nbins] (v1i, v2i)"""
        sh = (self.npairs, self.nbins, self.nbins)
        b, x1, x2 = np.zeros(sh), np.zeros(sh), np.zeros(sh)
        pd = C.POINTER(C.c_double)
        self.ctx.check(self.ctx.lib.pa_jpdf_read(self.ctx.h, self.h, b.ctypes.data_as(pd), x1.ctypes.data_as(pd), x2.ctypes.data_as(pd)))
        return b, x1, x2


class CondMeanAcc(_Hist):
    """binHits / binVals / binValsSq (/ binMinVals / binMaxVals) of conditionalMean.cpp (pa_condmean_*)"""

    def __init__(self, ctx: Context, navg: int, nbins: int, with_minmax: bool = False):
        self.ctx, self.navg, self.nbins, self.with_minmax = ctx, int(navg), int(nbins), bool(with_minmax)
        self.h = ctx.lib.pa_condmean_create(ctx.h, int(navg), int(nbins), int(bool(with_minmax)))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def begin(self, weight_max: int, vabs):
        a = np.ascontiguousarray(vabs, dtype=np.float64)
        assert len(a) == self.navg
        self.ctx.check(self.ctx.lib.pa_condmean_begin(self.ctx.h, self.h, int(weight_max), a.ctypes.data_as(C.POINTER(C.c_double))))

    def add_level(self, mf: "DevMF", finer: Optional["DevLevel"], ratio: int, domain, weight: int, bin_min: float, bin_max: float, uncombined: bool = False):
        """mf: bin component first, then the averaged ones; domain: (lo0, lo1, lo2, hi0, hi1, hi2) in the level's index space"""
        bx = PaBox()
        for d in range(3):
            bx.lo[d], bx.hi[d] = int(domain[d]), int(domain[3 + d])
        self.ctx.check(self.ctx.lib.pa_condmean_add_level(self.ctx.h, self.h, mf.h, finer.h if finer is not None else None, int(ratio), C.byref(bx),
                                                          int(weight), float(bin_min), float(bin_max), int(bool(uncombined))))

    def read(self):
        """-> hits [nbins] int64, sum, sumsq [nbins][navg], mn, mx [nbins][navg] or None"""
        sh = (self.nbins, self.navg)
        hits, s, s2 = np.zeros(self.nbins, np.int64), np.zeros(sh), np.zeros(sh)
        mn, mx = (np.zeros(sh), np.zeros(sh)) if self.with_minmax else (None, None)
        pd = C.POINTER(C.c_double)
        self.ctx.check(self.ctx.lib.pa_condmean_read(self.ctx.h, self.h, hits.ctypes.data_as(C.POINTER(C.c_int64)), s.ctypes.data_as(pd), s2.ctypes.data_as(pd),
                                                     mn.ctypes.data_as(pd) if mn is not None else None, mx.ctypes.data_as(pd) if mx is not None else None))
        return hits, s, s2, mn, mx


class IntegralAcc:
    """the composite integrals of integral.cpp and the moments of rmsVel.cpp (pa_integral_*): rows = the measure, w * v of every
    variable and, with squares, (v * v) * w of every variable; slots at the finest level's resolution"""

    def __init__(self, ctx: Context, nvars: int, kind: int, dir: int, domain, squares: bool = False):
        """domain: (lo0, lo1, lo2, hi0, hi1, hi2), the index box of the finest integrated level's problem domain"""
        self.ctx, self.nvars, self.kind, self.dir, self.squares = ctx, int(nvars), int(kind), int(dir), bool(squares)
        bx = PaBox()
        for d in range(3):
            bx.lo[d], bx.hi[d] = int(domain[d]), int(domain[3 + d])
        self.h = ctx.lib.pa_integral_create(ctx.h, int(nvars), int(kind), int(dir), C.byref(bx), int(bool(squares)))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        self.nrows = 1 + self.nvars * (2 if self.squares else 1)
        n = [int(domain[3 + d]) - int(domain[d]) + 1 for d in range(3)]
        self.shape = () if self.kind == 3 else ((n[self.dir],) if self.kind == 2 else (n[(self.dir + 1) % 3], n[(self.dir + 2) % 3]))
        assert int(np.prod(self.shape, dtype=np.int64)) == ctx.lib.pa_integral_slots(self.h)

    def close(self):
        if self.h:
            self.ctx.lib.pa_integral_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def begin(self, w_max: float, vabs):
        a = np.ascontiguousarray(vabs, dtype=np.float64)
        assert len(a) == self.nvars
        self.ctx.check(self.ctx.lib.pa_integral_begin(self.ctx.h, self.h, float(w_max), a.ctypes.data_as(C.POINTER(C.c_double))))

    def add_level(self, mf: "DevMF", finer: Optional["DevLevel"], ratio: int, R: int, w: float, ccomp: int = -1, cmin: float = 0.0, cmax: float = 0.0,
                  uncombined: bool = False):
        self.ctx.check(self.ctx.lib.pa_integral_add_level(self.ctx.h, self.h, mf.h, finer.h if finer is not None else None, int(ratio), int(R), float(w),
                                                          int(ccomp), float(cmin), float(cmax), int(bool(uncombined))))

    def read(self):
        """raw sums -> array [rows] + shape (kind 3: [rows]; kind 2: [rows][ldir]; kind 1: [rows][ldir1][ldir2])"""
        out = np.zeros((self.nrows,) + self.shape)
        self.ctx.check(self.ctx.lib.pa_integral_read(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out


class Resample:
    """a hierarchy's data on output BoxArrays that are not its own, summed over files (avgPlotfiles.cpp; pa_resample_*).  The caller
    owns the running multifabs (one per output level) and the work multifabs (every level but the finest, Resample.ghosts)"""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.h = ctx.lib.pa_resample_create(ctx.h)
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    @staticmethod
    def ghosts(nlev: int, lev: int, ratios: Sequence[int], interp_type: int = 1) -> int:
        """ghost layers of the work multifab of level lev (0 on the finest level): ceil(g_finer / ratio) + interp_type"""
        g = 0
        for l in range(nlev - 2, lev - 1, -1):
            g = -(-g // int(ratios[l])) + int(interp_type)
        return g

    def close(self):
        if self.h:
            self.ctx.lib.pa_resample_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def begin(self, running: Sequence["DevMF"], nvar: int):
        self._keep = list(running)
        self.ctx.check(self.ctx.lib.pa_resample_begin(self.ctx.h, self.h, len(running), _handles(running), int(nvar)))

    def add_file_level(self, lev: int, file: Optional["DevMF"], comp_map, crse_work: Optional["DevMF"], ratio: int, interp_type: int = 1,
                       work: Optional["DevMF"] = None):
        m = np.ascontiguousarray(comp_map, dtype=np.int32)
        self.ctx.check(self.ctx.lib.pa_resample_add_file_level(self.ctx.h, self.h, int(lev), file.h if file is not None else None,
                                                               m.ctypes.data_as(C.POINTER(C.c_int32)), crse_work.h if crse_work is not None else None,
                                                               int(ratio), int(interp_type), work.h if work is not None else None))

    def finish(self, nfiles: int) -> int:
        """scale by 1.0 / nfiles; returns the number of cells that found no source data"""
        n = C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_resample_finish(self.ctx.h, self.h, int(nfiles), C.byref(n)))
        return int(n.value)


class Flatten:
    """one level of one file on any list of disjoint boxes of the level's domain, without a running sum (flattenAMRFile.cpp:77-89;
    pa_flatten_level): the file's own cells bit for bit, the interpolant of the coarser multifab elsewhere"""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._n = C.c_int64(0)

    ghosts = staticmethod(Resample.ghosts)

    def level(self, file: Optional["DevMF"], comp_map, crse: Optional["DevMF"], ratio: int, interp_type: int, out: "DevMF", nvar: int) -> int:
        """V(f, l) into every valid and ghost cell of out; waits, and returns the number of cells that found no source data"""
        m = np.ascontiguousarray(comp_map if comp_map is not None else [0] * int(nvar), dtype=np.int32)
        self.ctx.check(self.ctx.lib.pa_flatten_level(self.ctx.h, file.h if file is not None else None, m.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     crse.h if crse is not None else None, int(ratio), int(interp_type), out.h, int(nvar), C.byref(self._n)))
        self.ctx.sync()
        return int(self._n.value)

    def last_launch(self):
        """(boxes on the wide route, on the general route, skipped as fully covered, overlay rectangles) of the last call"""
        a = (C.c_int64 * 4)()
        self.ctx.lib.pa_flatten_last_launch(a)
        return tuple(int(x) for x in a)


class Plane:
    """a hierarchy reduced to one plane at the finest level's resolution (avgToPlane.cpp / slicePlot.cpp; pa_plane_*): the sums along
    dir over a sub-box in the reference's order (max_grid_size > 0) or one slice (max_grid_size == 0), min / max, 256 pixel levels"""

    def __init__(self, ctx: Context, ncomp: int, dir: int, subbox, max_grid_size: int):
        """subbox: (lo0, lo1, lo2, hi0, hi1, hi2) in the finest level's indices"""
        self.ctx, self.ncomp, self.dir = ctx, int(ncomp), int(dir)
        bx = PaBox()
        for d in range(3):
            bx.lo[d], bx.hi[d] = int(subbox[d]), int(subbox[3 + d])
        self.h = ctx.lib.pa_plane_create(ctx.h, int(ncomp), int(dir), C.byref(bx), int(max_grid_size))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        d0, d1 = [d for d in range(3) if d != self.dir]
        self.width, self.height = int(subbox[3 + d0]) - int(subbox[d0]) + 1, int(subbox[3 + d1]) - int(subbox[d1]) + 1

    def close(self):
        if self.h:
            self.ctx.lib.pa_plane_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, levels: Sequence["DevMF"], ratios, comps):
        """levels: level 0 .. finestLevel; ratios[l]: between levels l and l + 1; comps[c]: the multifab component of row c"""
        r = np.ascontiguousarray(list(ratios) + [0], dtype=np.int32)
        m = np.ascontiguousarray(comps, dtype=np.int32)
        assert len(m) == self.ncomp
        self.ctx.check(self.ctx.lib.pa_plane_run(self.ctx.h, self.h, len(levels), _handles(levels), r.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 m.ctypes.data_as(C.POINTER(C.c_int32))))

    def read(self, out: Optional[np.ndarray] = None):
        """-> (plane [ncomp][height][width], cells no level holds); out: a C-contiguous float64 array of that shape to fill"""
        if out is None:
            out = np.zeros((self.ncomp, self.height, self.width))
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (self.ncomp, self.height, self.width)
        n = C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_plane_read(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return out, int(n.value)

    def minmax(self, comp: int = 0):
        mn, mx = C.c_double(0.0), C.c_double(0.0)
        self.ctx.check(self.ctx.lib.pa_plane_minmax(self.ctx.h, self.h, int(comp), C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def pixelize(self, comp: int, mn: float, mx: float) -> np.ndarray:
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.pa_plane_pixelize(self.ctx.h, self.h, int(comp), float(mn), float(mx), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out


class SurfBin:
    """the area-weighted (joint) PDF of node fields over a triangulated surface (binMEF.cpp; pa_surfbin_*): up to 4 binned components,
    the table in the order of the reference's map (first component slowest)"""

    COUNTERS = ("n_my", "nonfinite", "rounds", "peak", "sliced", "items", "elements", "capacity")

    def __init__(self, ctx: Context, nbins, bin_min, bin_max, work_items: int = 0):
        self.ctx = ctx
        self.nbins = tuple(int(n) for n in nbins)
        self.nc = len(self.nbins)
        assert len(bin_min) == self.nc and len(bin_max) == self.nc
        nb = (C.c_int32 * self.nc)(*self.nbins)
        mn = (C.c_double * self.nc)(*[float(v) for v in bin_min])
        mx = (C.c_double * self.nc)(*[float(v) for v in bin_max])
        self.h = ctx.lib.pa_surfbin_create(ctx.h, self.nc, nb, mn, mx, int(work_items))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def close(self):
        if self.h:
            self.ctx.lib.pa_surfbin_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _cols(nodes, elts):
        nodes = np.asarray(nodes, dtype=np.float64)
        cols = [np.ascontiguousarray(nodes[:, c]) for c in range(nodes.shape[1])]
        return cols, np.ascontiguousarray(elts, dtype=np.int32).reshape(-1, 3)

    def max_area(self, nodes, elts) -> float:
        """the largest finite element area: the magnitude for begin"""
        cols, e = self._cols(nodes, elts)
        pd = C.POINTER(C.c_double)
        a = self.ctx.lib.pa_surfbin_max_area(len(cols[0]), cols[0].ctypes.data_as(pd), cols[1].ctypes.data_as(pd), cols[2].ctypes.data_as(pd), len(e),
                                             e.ctypes.data_as(C.POINTER(C.c_int32)))
        if a < 0:
            raise PaError("pa_surfbin_max_area: an element names a node that does not exist")
        return a

    def begin(self, area_max: float):
        self.ctx.check(self.ctx.lib.pa_surfbin_begin(self.ctx.h, self.h, float(area_max)))

    def add_surface(self, nodes, elts, bin_comps, cond_apply: bool = False, cond_comp: int = 0, cond_val: float = 0.0, cond_sgn: int = 0,
                    area_eps: float = 1.0e-20, uncombined: bool = False):
        """nodes [N][nComp] with x, y, z first; elts [M][3], 1-based; bin_comps: the node component of every binned component"""
        assert len(bin_comps) == self.nc
        cols, e = self._cols(nodes, elts)
        pd = C.POINTER(C.c_double)
        comps = (pd * self.nc)(*[cols[int(c)].ctypes.data_as(pd) for c in bin_comps])
        cond = cols[int(cond_comp)].ctypes.data_as(pd) if cond_apply else None
        self.ctx.check(self.ctx.lib.pa_surfbin_add_surface(self.ctx.h, self.h, len(cols[0]), cols[0].ctypes.data_as(pd), cols[1].ctypes.data_as(pd),
                                                           cols[2].ctypes.data_as(pd), comps, cond, len(e), e.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           int(bool(cond_apply)), int(cond_sgn), float(cond_val), float(area_eps), int(bool(uncombined))))

    def read(self):
        """(area [prod nbins], hits [prod nbins], total area, area outside the condition, counters by name)"""
        nt = int(np.prod(self.nbins, dtype=np.int64))
        area, hits = np.zeros(nt), np.zeros(nt, dtype=np.int64)
        tot, outside = C.c_double(0.0), C.c_double(0.0)
        cnt = np.zeros(8, dtype=np.int64)
        p64 = C.POINTER(C.c_int64)
        self.ctx.check(self.ctx.lib.pa_surfbin_read(self.ctx.h, self.h, area.ctypes.data_as(C.POINTER(C.c_double)), hits.ctypes.data_as(p64), C.byref(tot),
                                                    C.byref(outside), cnt.ctypes.data_as(p64)))
        return area, hits, tot.value, outside.value, dict(zip(self.COUNTERS, (int(v) for v in cnt)))


def _out_array(shape, dtype, fill):
    """an output array for a read-back; `fill` (tests): the 64-bit pattern every 8 bytes of it hold before the call"""
    a = np.zeros(shape, dtype=dtype)
    if fill is not None:
        raw = np.frombuffer(np.uint64(fill).tobytes(), dtype=np.uint8)
        a.view(np.uint8).reshape(-1)[:] = np.resize(raw, a.nbytes)
    return a


class Decimate:
    """quadric edge-collapse decimation of a triangulated surface (decimateMEF.cpp; pa_decimate_*): xyz [N][3], elts [M][3] 1-based;
    weighting 0 uniform / 1 area, placement 0 endpoints / 1 endpoints or midpoint / 3 optimal.  `fill` (tests): the 64-bit pattern the
    output arrays of read / read_state hold before the call"""

    RECORD = ("edges", "locked", "candidates", "budget", "selected", "applied", "faces_removed", "valid_faces")

    def __init__(self, ctx: Context, xyz, elts, boundary_weight: float = 1000.0, weighting: int = 1, placement: int = 3):
        self.ctx = ctx
        x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64)[:, :3])
        e = np.ascontiguousarray(elts, dtype=np.int32).reshape(-1, 3)
        self.nnodes, self.nelts = len(x), len(e)
        self.h = ctx.lib.pa_decimate_create(ctx.h, len(x), x.ctypes.data_as(C.POINTER(C.c_double)), len(e), e.ctypes.data_as(C.POINTER(C.c_int32)),
                                            float(boundary_weight), int(weighting), int(placement))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())

    def close(self):
        if self.h:
            self.ctx.lib.pa_decimate_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _rc(self, rc: int) -> int:
        if rc < 0:
            raise PaError(self.ctx.lib.pa_last_error(self.ctx.h).decode())
        return rc

    def round(self, face_target: int) -> bool:
        """one round; False when nothing is left to do"""
        return self._rc(self.ctx.lib.pa_decimate_round(self.ctx.h, self.h, int(face_target))) == 1

    def run(self, face_target: int, max_rounds: int = 1000000) -> int:
        return self._rc(self.ctx.lib.pa_decimate_run(self.ctx.h, self.h, int(face_target), int(max_rounds)))

    def last_round(self):
        rec = np.zeros(8, dtype=np.int64)
        self.ctx.check(self.ctx.lib.pa_decimate_last_round(self.h, rec.ctypes.data_as(C.POINTER(C.c_int64))))
        return [int(v) for v in rec]

    def counts(self):
        """(vertices in use, valid faces, rounds applied)"""
        v, f, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_decimate_counts(self.h, C.byref(v), C.byref(f), C.byref(r)))
        return v.value, f.value, r.value

    _out = staticmethod(_out_array)

    def read(self, fill=None):
        """(xyz [nverts][3], elts [nfaces][3] int32, 1-based)"""
        nv, nf, _ = self.counts()
        xyz, elts = self._out((nv, 3), np.float64, fill), self._out((nf, 3), np.int32, fill)
        self.ctx.check(self.ctx.lib.pa_decimate_read(self.ctx.h, self.h, xyz.ctypes.data_as(C.POINTER(C.c_double)), elts.ctypes.data_as(C.POINTER(C.c_int32))))
        return xyz, elts

    def read_state(self, fill=None):
        """(xyz_all [N][3], faces_all [M][3] int32 0-based, face_valid [M] uint8, quadrics [10][N])"""
        xyz, faces = self._out((self.nnodes, 3), np.float64, fill), self._out((self.nelts, 3), np.int32, fill)
        valid, quad = self._out((self.nelts,), np.uint8, fill), self._out((10, self.nnodes), np.float64, fill)
        self.ctx.check(self.ctx.lib.pa_decimate_read_state(self.ctx.h, self.h, xyz.ctypes.data_as(C.POINTER(C.c_double)), faces.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           valid.ctypes.data_as(C.POINTER(C.c_uint8)), quad.ctypes.data_as(C.POINTER(C.c_double))))
        return xyz, faces, valid, quad


class Surf:
    """a triangulated surface with its node fields, kept on the device (sliceMEF.cpp, trimMEFgen.cpp; pa_surf_*): nodes [N][ncomp >= 3],
    elts [M][3] 1-based.  slice / trim / area work on the handle, trim replaces it in place.  `fill` (tests): the 64-bit pattern the
    output arrays of read / slice_read hold before the call"""

    OPS = {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4}
    LAUNCH = {1: ("slice", "elements", "segments", "requests", "vertices", "values", "csr_entries", "kernels"),
              2: ("trim", "nodes", "elements", "nodes_kept", "nodes_out", "elements_out", "values", "kernels"),
              3: ("area", "elements", "terms", None, None, None, None, "kernels"),
              4: ("merge", "nodes_in", "table", "path", "duplicates", "nodes_appended", "elements_appended", "kernels"),
              5: ("scale", "values", None, None, None, None, None, "kernels"),
              6: ("product", "values", None, None, None, None, None, "kernels"),
              7: ("select", "values", None, None, None, None, None, "kernels"),
              8: ("smooth", "elements", "incidence", "neighbours", "iterations", "nodes_written", "max_neighbours", "kernels")}
    PATHS = ("append", "grid", "brute")

    def __init__(self, ctx: Context, nodes, elts):
        self.ctx = ctx
        x = np.ascontiguousarray(nodes, dtype=np.float64)
        if x.ndim != 2:
            raise PaError("Surf: nodes must be [N][ncomp]")
        e = np.ascontiguousarray(elts, dtype=np.int32).reshape(-1, 3)
        self.h = ctx.lib.pa_surf_create(ctx.h, x.shape[0], x.shape[1], x.ctypes.data_as(C.POINTER(C.c_double)), len(e), e.ctypes.data_as(C.POINTER(C.c_int32)))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        self.nverts = self.nsegs = 0

    def close(self):
        if self.h:
            self.ctx.lib.pa_surf_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def counts(self):
        """(nodes, elements, components)"""
        n, m, c = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self.ctx.check(self.ctx.lib.pa_surf_counts(self.h, C.byref(n), C.byref(m), C.byref(c)))
        return n.value, m.value, c.value

    def read(self, fill=None):
        """(nodes [N][ncomp], elts [M][3] int32, 1-based)"""
        n, m, c = self.counts()
        nodes, elts = _out_array((n, c), np.float64, fill), _out_array((m, 3), np.int32, fill)
        self.ctx.check(self.ctx.lib.pa_surf_read(self.ctx.h, self.h, nodes.ctypes.data_as(C.POINTER(C.c_double)), elts.ctypes.data_as(C.POINTER(C.c_int32))))
        return nodes, elts

    def slice(self, comp: int, val: float):
        """the contour value[comp] == val; -> (vertices, segments)"""
        nv, ns = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_surf_slice(self.ctx.h, self.h, int(comp), float(val), C.byref(nv), C.byref(ns)))
        self.nverts, self.nsegs = nv.value, ns.value
        return self.nverts, self.nsegs

    def slice_read(self, fill=None):
        """(verts [nverts][ncomp], pairs [nverts][2], segs [nsegs][2], src_elt [nsegs], csr_off [nverts + 1], csr_adj [2 nsegs]); ids 0-based"""
        nv, ns, nc = self.nverts, self.nsegs, self.counts()[2]
        o = _out_array
        verts, pairs, segs = o((nv, nc), np.float64, fill), o((nv, 2), np.int32, fill), o((ns, 2), np.int32, fill)
        src, off, adj = o((ns,), np.int32, fill), o((nv + 1,), np.int32, fill), o((2 * ns,), np.int32, fill)
        p32 = C.POINTER(C.c_int32)
        self.ctx.check(self.ctx.lib.pa_surf_slice_read(self.ctx.h, self.h, verts.ctypes.data_as(C.POINTER(C.c_double)), pairs.ctypes.data_as(p32), segs.ctypes.data_as(p32),
                                                       src.ctypes.data_as(p32), off.ctypes.data_as(p32), adj.ctypes.data_as(p32)))
        return verts, pairs, segs, src, off, adj

    def trim(self, conds=(), rxy: float = -1.0, sign_rxy: str = "lt") -> int:
        """conds: (comp, "lt" | "le" | "gt" | "ge" | "eq", val) ...; -> the nodes removed because no surviving element uses them"""
        for _, op, _ in conds:
            if op not in self.OPS:
                raise PaError("Bad signs data. Use one of [lt,le,gt,ge,eq]")
        if rxy >= 0 and sign_rxy not in self.OPS:
            raise PaError("Bad sign data.  Use one of [lt,le,gt,ge,eq]")
        n = len(conds)
        cc = (C.c_int32 * max(n, 1))(*[int(c[0]) for c in conds])
        oo = (C.c_int32 * max(n, 1))(*[self.OPS[c[1]] for c in conds])
        vv = (C.c_double * max(n, 1))(*[float(c[2]) for c in conds])
        unused = C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_surf_trim(self.ctx.h, self.h, n, cc, oo, vv, float(rxy), self.OPS.get(sign_rxy, 0), C.byref(unused)))
        self.nverts = self.nsegs = 0
        return unused.value

    def area(self):
        """(total, smallest, largest triangle area)"""
        t, lo, hi = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self.ctx.check(self.ctx.lib.pa_surf_area(self.ctx.h, self.h, C.byref(t), C.byref(lo), C.byref(hi)))
        return t.value, lo.value, hi.value

    @classmethod
    def _adopt(cls, ctx: Context, handle):
        if not handle:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        s = cls.__new__(cls)
        s.ctx, s.h = ctx, handle
        s.nverts = s.nsegs = 0
        return s

    def merge(self, other: "Surf", eps: float = 1.0e-8, rem_dup_nodes: bool = False, method: int = 0) -> bool:
        """mergeMEF.cpp merge_iso: `other` into this surface; method 0 auto, 1 grid, 2 brute force; -> whether anything was appended"""
        app = C.c_int(0)
        self.ctx.check(self.ctx.lib.pa_surfjoin_merge(self.ctx.h, self.h, other.h, float(eps), int(bool(rem_dup_nodes)), int(method), C.byref(app)))
        self.nverts = self.nsegs = 0
        return bool(app.value)

    def scale(self, comps, vals) -> None:
        """scaleMEF.cpp: value[comps[k]] *= vals[k], in list order"""
        if len(comps) != len(vals):
            raise PaError("Surf.scale: vals needs one value per component")
        n = len(comps)
        cc = (C.c_int32 * max(n, 1))(*[int(c) for c in comps])
        vv = (C.c_double * max(n, 1))(*[float(v) for v in vals])
        self.ctx.check(self.ctx.lib.pa_surfjoin_scale(self.ctx.h, self.h, n, cc, vv))
        self.nverts = self.nsegs = 0

    def product(self, comps) -> "Surf":
        """multMEF.cpp: a new one-component surface, ((1.0 * d[c0]) * d[c1]) * ..."""
        n = len(comps)
        cc = (C.c_int32 * max(n, 1))(*[int(c) for c in comps])
        return Surf._adopt(self.ctx, self.ctx.lib.pa_surfjoin_product(self.ctx.h, self.h, n, cc))

    def select(self, sel, other: Optional["Surf"] = None) -> "Surf":
        """combineMEF.cpp: a new surface whose columns are sel = [(which, comp) ...], which 0 = this surface, 1 = `other`; this one's elements"""
        n = len(sel)
        ww = (C.c_int32 * max(n, 1))(*[int(w) for w, _ in sel])
        cc = (C.c_int32 * max(n, 1))(*[int(c) for _, c in sel])
        return Surf._adopt(self.ctx, self.ctx.lib.pa_surfjoin_select(self.ctx.h, self.h, other.h if other is not None else None, n, ww, cc))

    def smooth(self, comp: int, area_comp: int = -1, nsmooth: int = 1) -> None:
        """smoothMEF.cpp: component comp to the elements, nsmooth area-weighted Jacobi averages over each element and the elements that
        share a node with it, and back to the nodes; the weights are component area_comp where it names one, else the triangles' areas"""
        self.ctx.check(self.ctx.lib.pa_surfsmooth_run(self.ctx.h, self.h, int(comp), int(area_comp), int(nsmooth)))
        self.nverts = self.nsegs = 0

    def smooth_read(self, fill=None):
        """the last smooth: (nbr_off [nelts + 1], nbr_adj, w [nelts], q [nelts] after the last iteration); element ids 0-based"""
        rec = self.last_launch()
        if rec["op"] != "smooth":
            raise PaError("Surf.smooth_read: the last operation on the surface was not a smooth")
        ne, na = rec["elements"], rec["neighbours"]
        o = _out_array
        off, adj, w, q = o((ne + 1,), np.int32, fill), o((na,), np.int32, fill), o((ne,), np.float64, fill), o((ne,), np.float64, fill)
        p32, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self.ctx.check(self.ctx.lib.pa_surfsmooth_read(self.ctx.h, self.h, off.ctypes.data_as(p32), adj.ctypes.data_as(p32), w.ctypes.data_as(pd), q.ctypes.data_as(pd)))
        return off, adj, w, q

    def last_launch(self):
        """{"op": "slice" | "trim" | "area" | "merge" | "scale" | "product" | "select" | "smooth", <item name>: count ...} of the last call; a merge's
        "path" is one of Surf.PATHS"""
        rec = np.zeros(8, dtype=np.int64)
        self.ctx.check(self.ctx.lib.pa_surf_last_launch(self.h, rec.ctypes.data_as(C.POINTER(C.c_int64))))
        names = self.LAUNCH.get(int(rec[0]))
        if names is None:
            return {"op": None}
        out = {"op": names[0]}
        out.update({k: int(v) for k, v in zip(names[1:], rec[1:]) if k})
        if "path" in out:
            out["path"] = self.PATHS[out["path"]]
        return out


class FeMesh:
    """the hex-element mesh of a hierarchy (amrToFE.cpp; pa_fe_*): nodes = the uncovered cells in the reference's id order, bricks in
    the order of its std::set<Element>.  levels: DevLevel per level on the FILE's boxes; ratios: one per level but the finest;
    subbox: (lo0, lo1, lo2, hi0, hi1, hi2) on level 0 or None; finest_level: as the tool's key"""

    STAGES = ("number", "tag", "cubes", "order", "gather")

    def __init__(self, ctx: Context, levels: Sequence["DevLevel"], ratios: Sequence[int], subbox=None, finest_level: Optional[int] = None,
                 connect_cc: bool = True):
        self.ctx = ctx
        levels = list(levels if finest_level is None else levels[:finest_level + 1])
        nlev = len(levels)
        hs = (C.c_void_p * nlev)(*[lv.h for lv in levels])
        rr = (C.c_int32 * max(nlev - 1, 1))(*[int(r) for r in list(ratios)[:nlev - 1]])
        bx = None
        if subbox is not None:
            bx = PaBox()
            for d in range(3):
                bx.lo[d], bx.hi[d] = int(subbox[d]), int(subbox[3 + d])
        used, nn, ne = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self.h = ctx.lib.pa_fe_build(ctx.h, nlev, hs, rr, C.byref(bx) if bx is not None else None, int(bool(connect_cc)), C.byref(used), C.byref(nn), C.byref(ne))
        if not self.h:
            raise PaError(ctx.lib.pa_last_error(ctx.h).decode())
        self.nlev, self.nnodes, self.nelts = used.value, nn.value, ne.value

    def close(self):
        if self.h:
            self.ctx.lib.pa_fe_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def connectivity(self) -> np.ndarray:
        """int32 [nelts][8], 1-based"""
        p = C.c_void_p()
        self.ctx.check(self.ctx.lib.pa_fe_connectivity(self.ctx.h, self.h, C.byref(p)))
        out = np.empty((self.nelts, 8), dtype=np.int32)
        if self.nelts:
            self.ctx.check(self.ctx.lib.pa_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def nodes(self) -> np.ndarray:
        """int32 [ids][4]: (level, i, j, k) of every node id"""
        p, n = C.c_void_p(), C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_fe_nodes(self.ctx.h, self.h, C.byref(n), C.byref(p)))
        out = np.empty((n.value, 4), dtype=np.int32)
        self.ctx.check(self.ctx.lib.pa_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def gather(self, mfs: Sequence["DevMF"], comps: Sequence[int], download: bool = True):
        """float64 [3 + len(comps)][nnodes]: x, y, z, then the components (download=False: the DevBuf)"""
        comps = [int(c) for c in comps]
        buf = DevBuf(self.ctx, 8 * (3 + len(comps)) * max(self.nnodes, 1))
        cc = (C.c_int32 * max(len(comps), 1))(*comps)
        self.ctx.check(self.ctx.lib.pa_fe_gather(self.ctx.h, self.h, len(mfs), _handles(mfs), len(comps), cc, C.c_void_p(buf.ptr)))
        if not download:
            return buf
        return buf.to_numpy(np.float64, (3 + len(comps), self.nnodes))

    def stage_times(self):
        """({stage: ms}, cubes kept before duplicate removal)"""
        ms, nc = (C.c_double * 5)(), C.c_int64(0)
        self.ctx.check(self.ctx.lib.pa_fe_stage_times(self.ctx.h, self.h, ms, C.byref(nc)))
        return dict(zip(self.STAGES, (float(v) for v in ms))), nc.value
