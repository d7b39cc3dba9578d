"""ctypes binding of libsdfk.so (C-ABI declared in include/sdfk.h).

This is the only place the Python layer touches native code. There is no CPU fallback: if the
shared library is missing or no MI355X is visible, evaluation raises.
"""
import atexit
import contextlib
import ctypes
import importlib.util
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdfk.so")

MODE_AUTO, MODE_INTERPRET, MODE_SPECIALIZED, MODE_NOCULL = 0, 1, 2, 3
(FLAVOUR_PLAIN_ARRAY, FLAVOUR_PLAIN_GRID, FLAVOUR_TILE_ARRAY, FLAVOUR_TILE_GRID, FLAVOUR_TILE_MASK, FLAVOUR_ROWS_ARRAY,
 FLAVOUR_ROWS_GRID, FLAVOUR_ROWS_MASK, FLAVOUR_ROWS2D_ARRAY, FLAVOUR_ROWS2D_GRID, FLAVOUR_RAYS, FLAVOUR_OCCUPANCY,
 FLAVOUR_SPANS, FLAVOUR_SECONDARY, FLAVOUR_MOMENTS) = range(15)
FLAVOUR_FLAGS = 0x100      # OR-ed onto a PLAIN / ROWS / ROWS2D flavour: its flag-writing build (fused selection)
FLAVOUR_XY = 0x200         # OR-ed onto PLAIN_ARRAY / ROWS2D_ARRAY: the build for two-row coordinates (z = 0 by contract)

_c = ctypes
_vp, _i64, _int, _sz = _c.c_void_p, _c.c_int64, _c.c_int, _c.c_size_t
_fp = _c.POINTER(_c.c_float)

# name -> (restype, argtypes); every symbol declared in include/sdfk.h
SIGNATURES = {
    "sdfk_abi_version": (_int, []),
    "sdfk_device_count": (_int, []),
    "sdfk_last_error": (_c.c_char_p, []),
    "sdfk_program_create": (_vp, [_vp, _sz, _vp, _sz, _vp, _sz, _int]),
    "sdfk_program_destroy": (None, [_vp]),
    "sdfk_program_set_params": (_int, [_vp, _vp, _sz]),
    "sdfk_program_set_cull": (_int, [_vp, _vp, _sz, _vp]),
    "sdfk_program_source": (_c.c_char_p, [_vp]),
    "sdfk_program_compile_check": (_int, [_vp, _c.POINTER(_sz)]),
    "sdfk_program_chain_members": (_int, [_vp]),
    "sdfk_program_compile_flavour": (_int, [_vp, _int, _c.POINTER(_sz), _c.POINTER(_c.c_double)]),
    "sdfk_debug_compile_external": (_int, [_vp, _int, _c.POINTER(_sz)]),
    "sdfk_debug_jit_stats": (None, [_c.POINTER(_i64), _c.POINTER(_c.c_double)]),
    "sdfk_jit_drain": (None, []),
    "sdfk_jit_cancel": (None, []),
    "sdfk_debug_set_rtc_defs": (None, [_c.c_char_p]),
    "sdfk_eval_device": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _int]),
    "sdfk_eval_device_rows": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int]),
    "sdfk_eval_device_rows2d": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int]),
    "sdfk_eval_device_rows2d_xy": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int]),
    "sdfk_debug_cells_stats": (None, [_int, _c.POINTER(_c.c_longlong)]),
    "sdfk_debug_rays_stats": (None, [_int, _c.POINTER(_c.c_longlong)]),
    "sdfk_eval_device_rows3d": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _int]),
    "sdfk_debug_row_masks": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _c.POINTER(_i64), _c.POINTER(_int), _vp]),
    "sdfk_eval_grid_sharded": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _int, _vp, _vp, _int]),
    "sdfk_eval_grid_sharded_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _int, _vp, _int, _vp, _int]),
    "sdfk_eval_device_aux": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _i64, _vp, _vp, _int]),
    "sdfk_eval_grid_aux": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _int, _i64, _vp, _vp, _int]),
    "sdfk_field_min": (_int, [_vp, _i64, _c.POINTER(_c.c_float), _vp]),
    "sdfk_grid_box_average": (_int, [_vp, _i64, _i64, _i64, _int, _int, _int, _int, _vp, _vp]),
    "sdfk_grid_edge_detect": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "sdfk_debug_box_variant": (_int, [_i64, _i64, _i64, _int, _int, _int, _c.POINTER(_int)]),
    "sdfk_grid_signed": (_int, [_vp, _i64, _i64, _i64, _c.c_float, _int, _vp, _vp]),
    "sdfk_grid_boundary_mask": (_int, [_vp, _i64, _c.c_float, _vp, _vp]),
    "sdfk_grid_signed_slab": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp]),
    "sdfk_eval_host": (_int, [_vp, _vp, _int, _i64, _i64, _vp, _int, _int]),
    "sdfk_eval_host_resident": (_int, [_vp, _vp, _int, _i64, _i64, _vp, _int, _int]),
    "sdfk_field_select_scratch": (_sz, [_i64]),
    "sdfk_field_select": (_int, [_vp, _i64, _c.c_float, _vp, _i64, _c.POINTER(_i64), _vp, _vp]),
    "sdfk_field_select_finish": (_int, [_i64, _i64, _vp, _i64, _vp, _vp]),
    "sdfk_field_gradient": (_int, [_vp, _i64, _i64, _i64, _int, _int, _vp, _i64, _vp]),
    "sdfk_field_crossings_2d": (_int, [_vp, _vp, _i64, _i64, _i64, _c.c_double, _c.c_double, _c.c_double, _vp, _vp]),
    "sdfk_lcwg_eval": (_int, [_int, _vp, _vp, _i64, _i64, _i64, _c.c_double, _c.c_double, _int, _c.c_double, _vp, _vp, _i64,
                              _vp]),
    "sdfk_lcwg_old_eval": (_int, [_int, _vp, _i64, _vp, _i64, _c.c_double, _c.c_double, _vp, _i64, _vp]),
    "sdfk_eval_select_scratch": (_sz, [_i64, _i64]),
    "sdfk_eval_device_select": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _c.c_float, _vp, _i64, _c.POINTER(_i64), _vp, _vp, _int]),
    "sdfk_eval_grid_select": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _c.c_float, _vp, _i64, _c.POINTER(_i64),
                                     _vp, _vp, _int]),
    "sdfk_eval_select_finish": (_int, [_vp, _i64, _i64, _int, _i64, _vp, _i64, _vp, _vp]),
    "sdfk_vec_eval_device": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _int, _i64, _int, _vp, _i64, _vp]),
    "sdfk_vec_set_interpret": (None, [_int]),
    "sdfk_vec_source": (_c.c_char_p, [_vp, _int, _int, _int]),
    "sdfk_vec_compile_check": (_int, [_vp, _int, _int, _int, _c.POINTER(_sz)]),
    "sdfk_vec_eval_host": (_int, [_vp, _int, _vp, _int, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _int, _int, _vp, _int]),
    "sdfk_eval_grid": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _int]),
    "sdfk_eval_grid_host": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _int, _int]),
    "sdfk_set_default_mode": (None, [_int]),
    "sdfk_debug_brick_masks": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "sdfk_debug_eval_plan": (_int, [_vp, _c.POINTER(_i64), _c.POINTER(_i64)]),
    "sdfk_linspace_f32": (_int, [_c.c_double, _c.c_double, _i64, _vp]),
    "sdfk_point_tree_build": (_i64, [_vp, _i64, _int, _vp, _i64, _vp, _vp, _vp]),
    "sdfk_grid_fill": (_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp]),
    "sdfk_set_device": (_int, [_int]),
    "sdfk_malloc": (_vp, [_sz]),
    "sdfk_free": (_int, [_vp]),
    "sdfk_memcpy_h2d": (_int, [_vp, _vp, _sz]),
    "sdfk_memcpy_d2h": (_int, [_vp, _vp, _sz]),
    "sdfk_memcpy_d2d": (_int, [_vp, _vp, _sz]),
    "sdfk_sync": (_int, [_vp]),
    "sdfk_event_create": (_vp, []),
    "sdfk_event_destroy": (_int, [_vp]),
    "sdfk_event_record": (_int, [_vp, _vp]),
    "sdfk_event_elapsed_ms": (_int, [_vp, _vp, _fp]),
    "sdfk_stream_probe": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "sdfk_dual_has_rule": (_int, [_int]),
    "sdfk_program_jvp_check": (_int, [_vp, _c.POINTER(_int)]),
    "sdfk_eval_jvp_device": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _i64, _vp]),
    "sdfk_project_points_device": (_int, [_vp, _vp, _i64, _i64, _c.c_float, _c.c_float, _int, _c.c_float, _vp, _i64, _vp, _vp,
                                          _i64, _vp, _vp, _vp]),
    "sdfk_project_workgroups": (_i64, [_i64]),
    "sdfk_project_points_counted_device": (_int, [_vp, _vp, _i64, _i64, _c.c_float, _c.c_float, _int, _c.c_float, _vp, _i64,
                                                  _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "sdfk_value_jvp_device": (_int, [_int, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "sdfk_program_vjp_check": (_int, [_vp, _c.POINTER(_int), _c.POINTER(_i64)]),
    "sdfk_vjp_limits": (_int, [_c.POINTER(_int), _c.POINTER(_int)]),
    "sdfk_eval_vjp_device": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sdfk_points_bin": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp]),
    "sdfk_points_extent": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "sdfk_points_fill": (_int, [_vp, _i64, _i64, _i64, _int, _i64, _i64, _i64, _vp]),
    "sdfk_points_widen": (_int, [_vp, _i64, _int, _vp, _vp]),
    "sdfk_field_isosurface_scratch": (_sz, [_i64, _i64, _i64]),
    "sdfk_field_isosurface": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _c.POINTER(_i64), _c.POINTER(_i64), _vp,
                                     _vp]),
    "sdfk_field_isosurface_finish": (_int, [_vp, _i64, _i64, _i64, _c.c_float, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp,
                                            _vp]),
    "sdfk_field_contour2d_scratch": (_sz, [_i64, _i64]),
    "sdfk_field_contour2d": (_int, [_vp, _vp, _i64, _vp, _i64, _c.c_float, _c.POINTER(_i64), _c.POINTER(_i64), _vp, _vp]),
    "sdfk_field_contour2d_finish": (_int, [_vp, _i64, _i64, _c.c_float, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, _vp]),
    "sdfk_eval_grid_isosurface_scratch": (_sz, [_i64, _i64, _i64]),
    "sdfk_eval_grid_isosurface": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _c.POINTER(_i64), _c.POINTER(_i64),
                                         _vp, _vp, _int]),
    "sdfk_eval_grid_isosurface_finish": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _i64, _i64, _vp, _i64, _vp,
                                                _i64, _int, _vp, _vp, _int]),
    "sdfk_eval_grid_contour2d_scratch": (_sz, [_i64, _i64]),
    "sdfk_eval_grid_contour2d": (_int, [_vp, _vp, _i64, _vp, _i64, _c.c_float, _c.POINTER(_i64), _c.POINTER(_i64), _vp, _vp,
                                        _int]),
    "sdfk_eval_grid_contour2d_finish": (_int, [_vp, _vp, _i64, _vp, _i64, _c.c_float, _i64, _i64, _vp, _i64, _vp, _i64, _int,
                                               _vp, _vp, _int]),
    "sdfk_eval_grid_slices_scratch": (_sz, [_i64, _i64, _i64]),
    "sdfk_eval_grid_slices": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _c.POINTER(_i64), _c.POINTER(_i64), _vp,
                                     _vp, _int]),
    "sdfk_eval_grid_slices_finish": (_int, [_vp, _i64, _i64, _i64, _c.c_float, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, _vp,
                                            _vp, _vp, _int]),
    "sdfk_eval_grid_slices_measure": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _vp, _vp, _vp, _vp, _vp, _int]),
    "sdfk_label_scratch": (_sz, [_i64, _i64, _i64]),
    "sdfk_field_label": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _int, _int, _vp, _c.POINTER(_i64), _vp, _fp, _vp]),
    "sdfk_eval_grid_label": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _int, _int, _vp, _c.POINTER(_i64), _vp, _fp,
                                    _vp, _int]),
    "sdfk_label_bits": (_int, [_i64, _i64, _i64, _int, _int, _vp, _c.POINTER(_i64), _vp, _fp, _vp]),
    "sdfk_label_finish": (_int, [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfk_field_cell_counts": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _vp, _vp, _vp]),
    "sdfk_eval_grid_cell_counts": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _vp, _vp, _vp, _int]),
    "sdfk_label_field": (_int, [_vp, _i64, _vp, _i64, _c.c_float, _c.c_float, _vp, _vp]),
    "sdfk_label_moments": (_int, [_i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "sdfk_field_layer_label": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _int, _vp, _c.POINTER(_i64), _vp, _fp, _vp]),
    "sdfk_eval_grid_layer_label": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _int, _vp, _c.POINTER(_i64), _vp, _fp,
                                          _vp, _int]),
    "sdfk_layer_label_bits": (_int, [_i64, _i64, _i64, _int, _vp, _c.POINTER(_i64), _vp, _fp, _vp]),
    "sdfk_layer_label_finish": (_int, [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfk_layer_links": (_int, [_i64, _i64, _i64, _i64, _vp, _c.POINTER(_i64), _vp, _vp, _vp]),
    "sdfk_layer_links_finish": (_int, [_i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "sdfk_program_rays_check": (_int, [_vp, _c.POINTER(_int)]),
    "sdfk_trace_rays_device": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _c.c_float, _c.c_float, _c.c_float, _c.c_float,
                                      _c.c_float, _int, _vp, _vp, _vp, _vp, _i64, _vp, _int]),
    "sdfk_trace_camera_device": (_int, [_vp, _vp, _int, _int, _int, _c.c_float, _c.c_float, _c.c_float, _c.c_float,
                                        _c.c_float, _int, _vp, _vp, _vp, _vp, _i64, _vp, _int]),
    "sdfk_span_rays_device": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _c.c_float, _c.c_float, _c.c_float, _c.c_float,
                                     _c.c_float, _int, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _int]),
    "sdfk_span_camera_device": (_int, [_vp, _vp, _int, _int, _int, _c.c_float, _c.c_float, _c.c_float, _c.c_float,
                                       _c.c_float, _int, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _int]),
    "sdfk_visibility_rays_device": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _c.c_float, _c.c_float, _c.c_float, _c.c_float,
                                           _c.c_float, _int, _c.c_float, _vp, _vp, _vp, _vp, _vp, _int]),
    "sdfk_occlusion_rays_device": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _c.c_float, _int, _c.c_float, _c.c_float, _vp, _vp,
                                          _int]),
    "sdfk_eval_grid_occupancy_scratch": (_sz, [_i64, _i64, _i64, _i64]),
    "sdfk_eval_grid_occupancy": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _c.c_float,
                                        _c.c_float, _vp, _vp, _i64, _c.POINTER(_i64), _c.POINTER(_i64), _fp, _vp, _int]),
    "sdfk_field_row_sums": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "sdfk_eval_grid_moments_scratch": (_sz, [_i64, _i64, _i64, _i64]),
    "sdfk_eval_grid_moments": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _c.c_float,
                                      _c.c_float, _vp, _sz, _i64, _c.POINTER(_c.c_uint64), _c.POINTER(_i64), _fp, _vp, _int]),
    "sdfk_field_redistance_scratch": (_sz, [_i64, _i64, _i64]),
    "sdfk_field_redistance": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _c.c_float, _c.c_float, _int, _vp, _vp,
                                     _c.POINTER(_i64), _fp, _vp]),
    "sdfk_box_pad_ulps": (_int, []),
    "sdfk_box_has_rule": (_int, [_int]),
    "sdfk_program_box_check": (_int, [_vp, _c.POINTER(_int)]),
    "sdfk_enclose_boxes_device": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "sdfk_enclose_octree_scratch": (_sz, []),
    "sdfk_enclose_octree_device": (_int, [_vp, _vp, _i64, _c.POINTER(_c.c_double), _int, _c.c_float, _vp, _vp, _vp, _i64,
                                          _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_int), _vp, _vp]),
}


class SdfkError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).
    Two HIP runtimes in one process fight over the device: whichever initialises second sees no GPU. If torch is
    installed but not imported yet, load ITS runtime (and hiprtc) first, so that libsdfk.so — and a later
    `import torch` — resolve to the same copy. No torch: the system ROCm is used."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libamdhip64.so", "libhiprtc.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    """Load libsdfk.so once. Raises (never falls back) when the extension has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise SdfkError(
                        "aegolius_amd: %s is missing - build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, gfx950). "
                        "There is no CPU path." % LIB_PATH)
                _share_torch_hip_runtime()
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.restype, fn.argtypes = res, args
                if handle.sdfk_abi_version() != 1:
                    raise SdfkError("libsdfk.so ABI version mismatch")
                # no background kernel build survives the interpreter (and with it torch's HIP runtime): queued ones are
                # dropped, running compiler processes killed — a big tree's build takes up to a minute
                atexit.register(handle.sdfk_jit_cancel)
                _lib = handle
    return _lib


def last_error():
    msg = lib().sdfk_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what):
    if rc != 0:
        raise SdfkError("%s failed (%d): %s" % (what, rc, last_error()))


def device_count():
    return lib().sdfk_device_count()


def require_gpu():
    if device_count() < 1:
        raise SdfkError("aegolius_amd: no HIP device visible - SDF evaluation runs on an MI355X only "
                        "(there is no CPU path)")


def jit_stats():
    """(hiprtc builds this process has run — cache hits excluded —, seconds they took)."""
    n, t = _i64(0), _c.c_double(0.0)
    lib().sdfk_debug_jit_stats(ctypes.byref(n), ctypes.byref(t))
    return n.value, t.value


def _ptr(a):
    return a.ctypes.data_as(_vp) if a is not None and a.size else None


def _release(owner, attr, destroy):
    """Hand the handle `owner.<attr>` to the library's `destroy`, once (free() and every __del__ here). Never raises,
    and does nothing once the library is gone (interpreter exit)."""
    try:
        h = getattr(owner, attr, None)
        setattr(owner, attr, None)
        if h and _lib is not None:
            getattr(_lib, destroy)(_vp(h))
    except Exception:
        pass


def coords_n(shape):
    """N of a (3, N) coordinate array's shape."""
    if len(shape) != 2 or shape[0] != 3:
        raise ValueError("coordinates must have shape (3, N); got %r" % (tuple(shape),))
    return int(shape[1])


def host_coords(co, dtype=None):
    """A (3, N) host coordinate array, checked and contiguous: float32 / float64 pass through and anything else becomes
    float64 (what sdfk_eval_host takes), or everything becomes `dtype` (the staging paths upload float32)."""
    co = np.asarray(co)
    coords_n(co.shape)
    if dtype is None and co.dtype not in (np.float32, np.float64):
        dtype = np.float64
    return np.ascontiguousarray(co, dtype=dtype)


def axis_args(axes):
    """Per-axis tables of a grid -> (contiguous float32 tables, their flat (ptr, size, ptr, size, ...) C arguments).
    The pointers keep their tables alive (numpy's data_as holds a reference to its array)."""
    ax = [np.ascontiguousarray(a, dtype=np.float32) for a in axes]
    args = []
    for a in ax:
        args += [_ptr(a), a.size]
    return ax, tuple(args)


def _add_pass_ms(timings, names, ms):
    """Add the milliseconds a native call wrote to `ms` to the caller's `timings` dict under `names` (None: no dict)."""
    if timings is not None:
        for name, value in zip(names, ms):
            timings[name] = timings.get(name, 0.0) + float(value)


def row_stride(n):
    """Floats between the rows of a staged (rows, n) fp32 array: every row starts on a 256-byte line."""
    return (n + 63) // 64 * 64


class DeviceBuffer:
    """`nbytes` of raw device memory — the only owner of device memory in the Python layer. `free()`, leaving a `with`
    block or garbage collection releases it; `ptr` is None from then on and every use raises."""

    def __init__(self, nbytes, device=None, what=""):
        self.ptr, self.nbytes, self.device = None, int(nbytes), device if device is None else int(device)
        self.what = what or type(self).__name__
        if device is not None:
            check(lib().sdfk_set_device(self.device), "sdfk_set_device")
        self.ptr = lib().sdfk_malloc(self.nbytes) or None
        if self.ptr is None:
            raise SdfkError("%s: out of device memory (%d bytes): %s" % (self.what, self.nbytes, last_error()))

    def at(self, byte_offset=0, nbytes=0):
        """c_void_p of [byte_offset, byte_offset + nbytes) of the buffer, which must lie inside it."""
        if not self.ptr:
            raise SdfkError("%s has been freed" % self.what)
        if byte_offset < 0 or nbytes < 0 or byte_offset + nbytes > self.nbytes:
            raise SdfkError("%s: bytes [%d, %d) are outside its %d bytes" % (self.what, byte_offset, byte_offset + nbytes,
                                                                             self.nbytes))
        return _vp(self.ptr + byte_offset)

    def _live(self):
        self.at()
        if self.device is not None:
            check(lib().sdfk_set_device(self.device), "sdfk_set_device")

    def upload(self, host, byte_offset=0):
        """The bytes of a host array (C order), to `byte_offset` of the buffer."""
        host = np.ascontiguousarray(host)
        dst = self.at(byte_offset, host.nbytes)
        if host.nbytes:
            check(lib().sdfk_memcpy_h2d(dst, _ptr(host), host.nbytes), "sdfk_memcpy_h2d")

    def download(self, out, byte_offset=0):
        """Fill the C-contiguous host array `out` from `byte_offset` of the buffer -> out."""
        if not out.flags.c_contiguous:
            raise ValueError("%s: download needs a C-contiguous array" % self.what)
        src = self.at(byte_offset, out.nbytes)
        if out.nbytes:
            check(lib().sdfk_memcpy_d2h(_ptr(out), src, out.nbytes), "sdfk_memcpy_d2h")
        return out

    def copy_from(self, device_ptr, nbytes, byte_offset=0):
        """`nbytes` from the device pointer (int) `device_ptr`, to `byte_offset` of the buffer."""
        dst = self.at(byte_offset, nbytes)
        if nbytes:
            check(lib().sdfk_memcpy_d2d(dst, _vp(device_ptr), nbytes), "sdfk_memcpy_d2d")

    def _filled(self, fill, *args):
        """self after fill(*args), freed if that raises: for constructors that fill what they allocate."""
        try:
            fill(*args)
        except BaseException:
            self.free()
            raise
        return self

    def free(self):
        _release(self, "ptr", "sdfk_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        self.free()


class DeviceRows(DeviceBuffer):
    """`rows` fp32 rows of `n` values in device memory, `stride` = row_stride(n) floats apart: the layout of every
    coordinate, auxiliary-field, stream and vector array the kernels take."""

    def __init__(self, rows, n, device=None, what=""):
        self.rows, self.n, self.stride = int(rows), int(n), row_stride(int(n))
        DeviceBuffer.__init__(self, self.rows * self.stride * 4, device, what)

    def offset(self, r):
        """Byte offset of row r."""
        return 4 * r * self.stride

    def row(self, r):
        return self.at(self.offset(r), 4 * self.n)

    def row_ptr(self, r):
        return self.row(r).value

    def upload_rows(self, host):
        """A (k <= rows, n) host array, as float32 to rows 0 .. k - 1."""
        for r, line in enumerate(np.ascontiguousarray(host, dtype=np.float32)):
            self.upload(line, self.offset(r))

    def download_rows(self, count=None):
        """Rows 0 .. count - 1 (default: all) -> (count, n) float32 host array."""
        out = np.empty((self.rows if count is None else count, self.n), dtype=np.float32)
        for r, line in enumerate(out):
            self.download(line, self.offset(r))
        return out


class Program:
    """Owning wrapper of an `sdfk_program*` (a lowered expression tree)."""

    def __init__(self, code, params, tables, result_reg, cull_sites=None, cull_k=None):
        self.code = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1, 2)
        self.params = np.ascontiguousarray(params, dtype=np.float32).ravel()
        self.tables = np.ascontiguousarray(tables, dtype=np.float32).ravel()
        self.result_reg = int(result_reg)
        self._h = lib().sdfk_program_create(_ptr(self.code), self.code.shape[0], _ptr(self.params), self.params.size,
                                            _ptr(self.tables), self.tables.size, self.result_reg)
        if not self._h:
            raise SdfkError("sdfk_program_create rejected the program: " + last_error())
        if cull_sites is not None and len(cull_sites):
            sites = np.ascontiguousarray(cull_sites, dtype=np.uint32).reshape(-1, 5)
            k = np.ascontiguousarray(cull_k, dtype=np.float32).ravel()
            check(lib().sdfk_program_set_cull(self._h, _ptr(sites), sites.shape[0], _ptr(k)), "sdfk_program_set_cull")

    @classmethod
    def from_lowered(cls, low, cull=True):
        """Program of a LoweredProgram (aegolius_amd._lower), with its brick-culling sites."""
        if cull:
            return cls(low.code, low.params, low.tables, low.result_reg, low.cull_sites, low.cull_k)
        return cls(low.code, low.params, low.tables, low.result_reg)

    @property
    def handle(self):
        return self._h

    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=np.float32).ravel()
        check(lib().sdfk_program_set_params(self._h, _ptr(p), p.size), "sdfk_program_set_params")
        self.params = p

    def source(self):
        s = lib().sdfk_program_source(self._h)
        return s.decode() if s else None

    @property
    def chain_members(self):
        """Members of the n-ary chain when the program runs on the table-driven chain kernels, else 0."""
        return int(lib().sdfk_program_chain_members(self._h))

    def compile_check(self):
        n = _sz(0)
        check(lib().sdfk_program_compile_check(self._h, ctypes.byref(n)), "sdfk_program_compile_check")
        return n.value

    def compile_flavour(self, flavour):
        """Build (or fetch) one kernel flavour (FLAVOUR_*), GPU or not -> (code-object bytes, seconds)."""
        n, t = _sz(0), _c.c_double(0.0)
        check(lib().sdfk_program_compile_flavour(self._h, int(flavour), ctypes.byref(n), ctypes.byref(t)),
              "sdfk_program_compile_flavour")
        return n.value, t.value

    def eval_host(self, co, device=0, mode=MODE_AUTO):
        """co: (3, N) float32/float64 host array -> (N,) float32 field."""
        require_gpu()
        co = host_coords(co)
        n = co.shape[1]
        out = np.empty(n, dtype=np.float32)
        check(lib().sdfk_eval_host(self._h, _ptr(co), 0 if co.dtype == np.float32 else 1, n, n, _ptr(out), device,
                                   mode), "sdfk_eval_host")
        return out

    def eval_device(self, d_co, n, row_stride, d_out, stream=None, mode=MODE_AUTO, row_len=None, flat=False,
                    plane_rows=None, first_row_in_plane=0):
        """Device pointers (ints). Asynchronous on `stream` (a hipStream_t as int, None = default).
        `row_len`: layout hint — the points are consecutive rows of that many points (the last grid
        dimension of a generate_grid array); speeds up brick culling, never changes the field.
        `flat`: the rows are those of a flat (two-size) grid: z = 0, rows along y.
        `plane_rows`, `first_row_in_plane`: 3-D grids — rows per plane (the second grid dimension) and where in its
        plane the array starts (x-slabs of whole rows): row blocks then never straddle two planes."""
        if row_len and plane_rows and not flat:
            check(lib().sdfk_eval_device_rows3d(self._h, _vp(d_co), n, row_stride, int(row_len), int(plane_rows),
                                                int(first_row_in_plane), _vp(d_out), _vp(stream or 0), mode),
                  "sdfk_eval_device_rows3d")
            return
        if row_len and flat:
            check(lib().sdfk_eval_device_rows2d(self._h, _vp(d_co), n, row_stride, int(row_len), _vp(d_out),
                                                _vp(stream or 0), mode), "sdfk_eval_device_rows2d")
            return
        if row_len:
            check(lib().sdfk_eval_device_rows(self._h, _vp(d_co), n, row_stride, int(row_len), _vp(d_out),
                                              _vp(stream or 0), mode), "sdfk_eval_device_rows")
            return
        check(lib().sdfk_eval_device(self._h, _vp(d_co), n, row_stride, _vp(d_out), _vp(stream or 0), mode),
              "sdfk_eval_device")

    def eval_device_xy(self, d_xy, n, row_stride, d_out, stream=None, mode=MODE_AUTO, row_len=None):
        """Two coordinate rows (x, y) of a flat grid, z = 0 by contract: 12 instead of 16 bytes per point."""
        check(lib().sdfk_eval_device_rows2d_xy(self._h, _vp(d_xy), n, row_stride, int(row_len or 0), _vp(d_out),
                                               _vp(stream or 0), mode), "sdfk_eval_device_rows2d_xy")

    def eval_grid(self, axes, start, count, d_out, stream=None, mode=MODE_AUTO):
        _, tab = axis_args(axes)
        check(lib().sdfk_eval_grid(self._h, *tab, start, count, _vp(d_out), _vp(stream or 0), mode), "sdfk_eval_grid")

    def _select(self, n, first, device, row_len=0, mode=MODE_AUTO):
        """Two-step protocol of the fused selection: `first(d_scratch, byref(count))` evaluates into flags and counts;
        the indices follow from the flags. -> ascending int64 host array."""
        require_gpu()
        L = lib()
        check(L.sdfk_set_device(int(device)), "sdfk_set_device")

        def finish(m, d_index, d_scratch):
            check(L.sdfk_eval_select_finish(self._h, n, int(row_len), mode, m, d_index, m, d_scratch, None),
                  "sdfk_eval_select_finish")
        return _select(L.sdfk_eval_select_scratch(n, int(row_len)), first, finish)

    def select_grid(self, axes, threshold=0.0, start=0, count=None, device=0, mode=MODE_AUTO):
        """numpy.flatnonzero(field <= threshold) of the grid spanned by three per-axis tables, WITHOUT a field: the
        evaluation kernels write one flag bit per point, the compaction reads the flags (sdfk_eval_grid_select)."""
        ax, tab = axis_args(axes)
        total = ax[0].size * ax[1].size * ax[2].size
        count = total - start if count is None else count

        def first(d_scratch, m):
            check(lib().sdfk_eval_grid_select(self._h, *tab, start, count, float(threshold), None, 0, m, d_scratch, None,
                                              mode), "sdfk_eval_grid_select")
        grow = ax[2].size if ax[2].size > 1 else ax[1].size
        return self._select(count, first, device, row_len=grow if start % grow == 0 and count % grow == 0 else 0, mode=mode)

    def mesh_grid(self, axes, level, device=0, mode=MODE_AUTO, timings=None):
        """Isosurface (three axis tables) or contour (two) of {f = level} on the grid the tables span, WITHOUT a field:
        the evaluation kernels write one inside bit per point, the mesh is counted from the bits, and the program is
        evaluated again at the two ends of every crossing edge (sdfk_eval_grid_isosurface / _contour2d and their
        _finish). The tables must be strictly increasing float32 arrays and `level` not NaN (aegolius_amd.mesh checks
        both). -> (vertices (V, D) float32, faces (F, D) int32, or int64 from 2^31 vertices on). `timings`: a dict that
        receives device-event milliseconds of count (evaluation to bits, count, scan) / emit / copy."""
        require_gpu()
        check(lib().sdfk_set_device(int(device)), "sdfk_set_device")
        ax, tab = axis_args(axes)
        if len(ax) not in (2, 3):
            raise ValueError("mesh_grid: two or three axis tables")
        lead = (self._h,) + tab
        return extract_mesh("sdfk_eval_grid", [a.size for a in ax], level, lead, lead, (mode,), timings)

    def slices_grid(self, tables, level, device=0, mode=MODE_AUTO, timings=None):
        """Plane stack of {f = level} on the grid of `tables` = (heights, U, V), the layer the slowest axis, WITHOUT a
        field (sdfk_eval_grid_slices and its _finish): every layer the contour of mesh_grid on its 2-D grid (U, V). The
        tables must be strictly increasing float32 arrays and `level` not NaN (aegolius_amd.slices checks both).
        -> (vertices (V, 2) float32 as (a, b), segments (S, 2) int32, or int64 from 2^31 vertices on, vertex offsets and
        segment offsets (layers + 1,) int64). `timings`: a dict that receives device-event milliseconds of count
        (evaluation to bits, count, scans, layer offsets) / emit / copy."""
        require_gpu()
        L = lib()
        check(L.sdfk_set_device(int(device)), "sdfk_set_device")
        ax, tab = axis_args(tables)
        if len(ax) != 3:
            raise ValueError("slices_grid: the heights and two in-plane tables")
        shape = [a.size for a in ax]
        lv = _c.c_float(level)
        nv, ns = _i64(0), _i64(0)
        voff, soff = np.zeros(shape[0] + 1, dtype=np.int64), np.zeros(shape[0] + 1, dtype=np.int64)
        timer = Timer(timings)
        with contextlib.ExitStack() as stack:
            def alloc(nbytes):
                return stack.enter_context(DeviceBuffer(nbytes, what="slices"))
            timer.mark("start")
            scratch = alloc(L.sdfk_eval_grid_slices_scratch(*shape))
            check(L.sdfk_eval_grid_slices(self._h, *tab, lv, ctypes.byref(nv), ctypes.byref(ns), scratch.at(), None, mode),
                  "sdfk_eval_grid_slices")
            timer.mark("count")
            V, S = nv.value, ns.value
            wide = V > 0x7fffffff
            d_v = alloc(V * 8)
            d_s = alloc(S * 2 * (8 if wide else 4))
            check(L.sdfk_eval_grid_slices_finish(self._h, *shape, lv, V, S, d_v.at(), V, d_s.at(), S, 8 if wide else 4, _ptr(voff),
                                                 _ptr(soff), scratch.at(), None, mode), "sdfk_eval_grid_slices_finish")
            timer.mark("emit")
            verts = d_v.download(np.empty((V, 2), dtype=np.float32))
            segs = d_s.download(np.empty((S, 2), dtype=np.int64 if wide else np.int32))
            timer.mark("copy")
            timer.finish()
        return verts, segs, voff, soff

    def slices_measure_grid(self, tables, level, device=0, mode=MODE_AUTO, timings=None):
        """Section measures of the plane stack of slices_grid, reduced per layer on the device
        (sdfk_eval_grid_slices_measure): the stack never leaves device memory. -> (measures (layers, 6) float64: area,
        perimeter, first moments in a and b about the rectangle's centre, segments, border crossings; vertex offsets,
        segment offsets). `timings`: a dict that receives device-event milliseconds of the whole call (measure)."""
        require_gpu()
        L = lib()
        check(L.sdfk_set_device(int(device)), "sdfk_set_device")
        ax, tab = axis_args(tables)
        if len(ax) != 3:
            raise ValueError("slices_measure_grid: the heights and two in-plane tables")
        shape = [a.size for a in ax]
        out = np.zeros((shape[0], 6), dtype=np.float64)
        voff, soff = np.zeros(shape[0] + 1, dtype=np.int64), np.zeros(shape[0] + 1, dtype=np.int64)
        timer = Timer(timings)
        with DeviceBuffer(L.sdfk_eval_grid_slices_scratch(*shape), what="slices") as scratch:
            timer.mark("start")
            check(L.sdfk_eval_grid_slices_measure(self._h, *tab, _c.c_float(level), _ptr(out), _ptr(voff), _ptr(soff), scratch.at(),
                                                  None, mode), "sdfk_eval_grid_slices_measure")
            timer.mark("measure")
            timer.finish()
        return out, voff, soff

    def _lattice_args(self, who, axes, sub_tables, half_widths, samples, device, timings):
        """What occupancy_grid and moments_grid (`who`, in the error texts) share: the device and the checked tables ->
        (library, the native call's leading arguments up to the half-widths, the grid's shape, the c_float * 3 of the
        passes' milliseconds or None without `timings`)."""
        require_gpu()
        L = lib()
        check(L.sdfk_set_device(int(device)), "sdfk_set_device")
        ax, tab = axis_args(axes)
        if len(ax) != 3 or len(sub_tables) != 3 or len(half_widths) != 3:
            raise ValueError("%s: three axis, sub-sample and half-width tables" % who)
        k = [int(samples) if a.size > 1 else 1 for a in ax]
        sub = [np.ascontiguousarray(t, dtype=np.float32) for t in sub_tables]
        hw = [np.ascontiguousarray(t, dtype=np.float32) for t in half_widths]
        for a, s, h, ka in zip(ax, sub, hw, k):
            if s.shape != (a.size * ka,) or h.shape != (a.size,):
                raise ValueError("%s: an axis of %d points takes %d sub-samples and %d half-widths; got %r and %r"
                                 % (who, a.size, a.size * ka, a.size, s.shape, h.shape))
        lead = (self._h,) + tab + tuple(_ptr(t) for t in sub + hw)
        return L, lead, [a.size for a in ax], (_c.c_float * 3)() if timings is not None else None

    def occupancy_grid(self, axes, sub_tables, half_widths, samples, level, lipschitz, d_out, slab_cells=0, device=0,
                       mode=MODE_AUTO, timings=None):
        """Occupancy fractions of the cells of the grid the three axis tables span (sdfk_eval_grid_occupancy), written to
        the device pointer `d_out` (one float per cell): count / K of the K sub-samples the three `sub_tables` span per
        cell; `half_widths`: per axis and grid point, a float32 bound of the distance to its farthest sub-sample.
        `lipschitz`: the bound the skip rule uses (inf: nothing is skipped). aegolius_amd.occupancy builds the tables and
        states the definition. -> (inside sub-samples, near cells) as Python ints. `timings`: a dict that receives
        device-event milliseconds of centre / classify / sample."""
        L, lead, shape, ms = self._lattice_args("occupancy_grid", axes, sub_tables, half_widths, samples, device, timings)
        inside, near = _i64(0), _i64(0)
        with DeviceBuffer(L.sdfk_eval_grid_occupancy_scratch(*shape, int(slab_cells)), what="occupancy") as scratch:
            check(L.sdfk_eval_grid_occupancy(*lead, int(samples), float(level), float(lipschitz), _vp(d_out), scratch.at(),
                                             int(slab_cells), ctypes.byref(inside), ctypes.byref(near), ms, None, mode),
                  "sdfk_eval_grid_occupancy")
        _add_pass_ms(timings, ("centre", "classify", "sample"), ms)
        return int(inside.value), int(near.value)

    def moments_grid(self, axes, sub_tables, half_widths, samples, level, lipschitz, slab_cells=0, device=0, mode=MODE_AUTO,
                     timings=None):
        """Integer moments of the solid on the sub-sample lattice of occupancy_grid (sdfk_eval_grid_moments; tables and
        `lipschitz` as there): the sums of 1, u_a and u_a u_b over the inside sub-samples, u_a = 2 (i_a k_a + j_a) + 1.
        aegolius_amd.moments builds the tables, states the definition and turns the sums into physical quantities.
        -> ((N, U0, U1, U2, U00, U01, U02, U11, U12, U22), near cells) as Python ints. `timings`: a dict that receives
        device-event milliseconds of centre / far / sample."""
        L, lead, shape, ms = self._lattice_args("moments_grid", axes, sub_tables, half_widths, samples, device, timings)
        words, near = (_c.c_uint64 * 20)(), _i64(0)
        nbytes = L.sdfk_eval_grid_moments_scratch(*shape, int(slab_cells))
        with DeviceBuffer(nbytes, what="moments") as scratch:
            check(L.sdfk_eval_grid_moments(*lead, int(samples), float(level), float(lipschitz), scratch.at(), nbytes,
                                           int(slab_cells), words, ctypes.byref(near), ms, None, mode),
                  "sdfk_eval_grid_moments")
        _add_pass_ms(timings, ("centre", "far", "sample"), ms)
        return tuple(int(words[2 * t]) + (int(words[2 * t + 1]) << 64) for t in range(10)), int(near.value)

    def select_host(self, co, threshold=0.0, device=0, mode=MODE_AUTO):
        """The same for a (3, N) host array (uploaded once as float32; the row-length hint is detected like create())."""
        require_gpu()
        co32 = host_coords(co, np.float32)
        n = co32.shape[1]
        if n == 0:
            return np.empty(0, dtype=np.int64)
        L = lib()
        check(L.sdfk_set_device(int(device)), "sdfk_set_device")
        with DeviceCoords(co32, what="select") as d_co:
            # rows: the index at which x or y first changes (3-D grids), else at which x first changes (flat grids)
            row_len, flat = 0, 0
            head = co32[:, :min(n, 1 << 22)]
            ch = np.flatnonzero((head[0] != head[0, 0]) | (head[1] != head[1, 0]))
            if ch.size and ch[0] >= 32 and n % int(ch[0]) == 0:
                row_len = int(ch[0])
            else:
                cx = np.flatnonzero(head[0] != head[0, 0])
                if cx.size and cx[0] >= 32 and n % int(cx[0]) == 0:
                    row_len = int(cx[0])
                    flat = int(co32[2, 0] == 0 and co32[2, row_len - 1] == 0 and co32[2, -1] == 0)

            def first(d_scratch, m):
                check(L.sdfk_eval_device_select(self._h, _vp(d_co.ptr), n, d_co.stride, row_len, flat, float(threshold), None,
                                                0, m, d_scratch, None, mode), "sdfk_eval_device_select")
            return self._select(n, first, device, row_len=row_len, mode=mode)

    def eval_grid_host(self, axes, start=0, count=None, device=0, mode=MODE_AUTO):
        """Field of the grid spanned by three per-axis tables (flat index z fastest), straight to a host array."""
        require_gpu()
        ax, tab = axis_args(axes)
        total = ax[0].size * ax[1].size * ax[2].size
        count = total - start if count is None else count
        out = np.empty(count, dtype=np.float32)
        check(lib().sdfk_eval_grid_host(self._h, *tab, start, count, _ptr(out), device, mode), "sdfk_eval_grid_host")
        return out

    def eval_grid_sharded(self, axes, n_shards, devices=None, mode=MODE_AUTO):
        """Whole grid, cut into `n_shards` slabs of whole rows evaluated concurrently on `devices`
        (default: shard d on device d modulo the device count), field returned as one host array."""
        require_gpu()
        ax, tab = axis_args(axes)
        out = np.empty(ax[0].size * ax[1].size * ax[2].size, dtype=np.float32)
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        if dev is not None and dev.size != n_shards:
            raise ValueError("one device per shard")
        check(lib().sdfk_eval_grid_sharded(self._h, *tab, n_shards, _ptr(dev) if dev is not None else None, _ptr(out), mode),
              "sdfk_eval_grid_sharded")
        return out

    def eval_grid_sharded_resident(self, axes, n_shards, devices=None, gather_device=0, mode=MODE_AUTO):
        """The same partition, the field reassembled on `gather_device` by device-to-device copies (no host buffer)
        -> DeviceField on that device."""
        require_gpu()
        ax, tab = axis_args(axes)
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        if dev is not None and dev.size != n_shards:
            raise ValueError("one device per shard")
        field = DeviceField(ax[0].size * ax[1].size * ax[2].size, gather_device)
        check(lib().sdfk_eval_grid_sharded_device(self._h, *tab, n_shards, _ptr(dev) if dev is not None else None,
                                                  int(gather_device), _vp(field.ptr), mode), "sdfk_eval_grid_sharded_device")
        return field

    def __del__(self):
        _release(self, "_h", "sdfk_program_destroy")


def _select(scratch_bytes, count, finish):
    """Count, allocate the exact result, finish, download: `count(d_scratch, byref(m))` marks and counts the selected
    points, `finish(m, d_index, d_scratch)` writes their m indices. -> ascending int64 host array."""
    m = _i64(0)
    with DeviceBuffer(scratch_bytes, what="select") as scratch:
        count(scratch.at(), ctypes.byref(m))
        out = np.empty(m.value, dtype=np.int64)
        if m.value:
            with DeviceBuffer(m.value * 8, what="select") as index:
                finish(m.value, index.at(), scratch.at())
                index.download(out)
        return out


def extract_mesh(family, shape, level, lead_count, lead_finish, tail=(), timings=None):
    """Count, allocate the exact result, finish, download of a mesh on a grid of `shape` (3 sizes: isosurface, 2:
    contour): the entry points `<family>_isosurface` / `_contour2d`, their `_scratch` and `_finish`, called with the
    leading arguments `lead_count` / `lead_finish` and the trailing ones `tail`. -> (vertices (V, D) float32, faces (F, D)
    int32, or int64 from 2^31 vertices on). `timings`: a dict that receives device-event milliseconds of count / emit /
    copy."""
    L = lib()
    dims = len(shape)
    name = family + ("_isosurface" if dims == 3 else "_contour2d")
    lv = _c.c_float(level)
    nv, nf = _i64(0), _i64(0)
    timer = Timer(timings)
    with contextlib.ExitStack() as stack:
        def alloc(nbytes):
            return stack.enter_context(DeviceBuffer(nbytes, what="mesh"))
        timer.mark("start")
        scratch = alloc(getattr(L, name + "_scratch")(*shape))
        check(getattr(L, name)(*lead_count, lv, ctypes.byref(nv), ctypes.byref(nf), scratch.at(), None, *tail), name)
        timer.mark("count")
        V, F = nv.value, nf.value
        wide = V > 0x7fffffff
        d_v = alloc(V * dims * 4)
        d_f = alloc(F * dims * (8 if wide else 4))
        check(getattr(L, name + "_finish")(*lead_finish, lv, V, F, d_v.at(), V, d_f.at(), F, 8 if wide else 4, scratch.at(),
                                           None, *tail), name + "_finish")
        timer.mark("emit")
        verts = d_v.download(np.empty((V, dims), dtype=np.float32))
        faces = d_f.download(np.empty((F, dims), dtype=np.int64 if wide else np.int32))
        timer.mark("copy")
        timer.finish()
        return verts, faces


class DeviceField(DeviceBuffer):
    """An (N,) float32 scalar field resident in HBM (what `create_resident` returns): the consumers of the field run
    on it without the field ever crossing PCIe. Owns its device memory; `free()` (or garbage collection) releases it."""

    def __init__(self, n, device=0):
        require_gpu()
        self.n = int(n)
        DeviceBuffer.__init__(self, self.n * 4, device)

    @classmethod
    def from_host(cls, field, device=0):
        host = np.ascontiguousarray(field, dtype=np.float32).ravel()
        self = cls(host.size, device)
        return self._filled(self.upload, host)

    @classmethod
    def from_device(cls, device_ptr, n, device=0):
        """A copy of the n floats at the device pointer (int) `device_ptr`."""
        self = cls(n, device)
        return self._filled(self.copy_from, device_ptr, self.n * 4)

    def numpy(self):
        self._live()
        return self.download(np.empty(self.n, dtype=np.float32))

    def count(self, threshold=0.0):
        """Number of points with field <= threshold."""
        self._live()
        m = _i64(0)
        check(lib().sdfk_field_select(_vp(self.ptr), self.n, float(threshold), None, 0, ctypes.byref(m), None, None),
              "sdfk_field_select")
        return m.value

    def select(self, threshold=0.0):
        """Ascending int64 indices of the points with field <= threshold (numpy.flatnonzero(field <= threshold));
        only the indices cross PCIe."""
        self._live()
        L = lib()

        def count(d_scratch, m):
            check(L.sdfk_field_select(_vp(self.ptr), self.n, float(threshold), None, 0, m, d_scratch, None), "sdfk_field_select")

        def finish(m, d_index, d_scratch):
            check(L.sdfk_field_select_finish(self.n, m, d_index, m, d_scratch, None), "sdfk_field_select_finish")
        return _select(L.sdfk_field_select_scratch(self.n), count, finish)

    def gradient(self, shape, normalize=True):
        """numpy.gradient (unit spacing) of the field reshaped to `shape` (1 to 3 axes), every vector normalised
        unless its norm is 0 -> (len(shape), N) float32 host array."""
        self._live()
        shape = tuple(int(x) for x in shape)
        if not 1 <= len(shape) <= 3 or int(np.prod(shape)) != self.n:
            raise ValueError("cannot reshape a field of %d points to %r" % (self.n, shape))
        if min(shape) < 2:
            raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.")
        dims = (1,) * (3 - len(shape)) + shape
        with DeviceRows(len(shape), self.n, what="gradient") as vec:
            check(lib().sdfk_field_gradient(_vp(self.ptr), dims[0], dims[1], dims[2], len(shape), 1 if normalize else 0,
                                            vec.at(), vec.stride, None), "sdfk_field_gradient")
            return vec.download_rows()

    def gradient_resident(self, shape, normalize=True):
        """gradient() of a 3-D field, left on the device as a DeviceVectorField."""
        self._live()
        shape = tuple(int(x) for x in shape)
        if len(shape) != 3 or int(np.prod(shape)) != self.n:
            raise ValueError("gradient_resident takes a 3-D grid of %d points; got %r" % (self.n, shape))
        if min(shape) < 2:
            raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.")
        out = DeviceVectorField(self.n, self.device)
        check(lib().sdfk_field_gradient(_vp(self.ptr), shape[0], shape[1], shape[2], 3, 1 if normalize else 0, _vp(out.ptr),
                                        out.stride, None), "sdfk_field_gradient")
        return out


CONNECT_FACES, CONNECT_FULL = 0, 1
REGION_INSIDE, REGION_OUTSIDE = 0, 1
LABEL_PASSES = ("bits", "init", "merge", "compress", "number")


class LabelScratch(DeviceBuffer):
    """The scratch of the topology calls (sdfk_label_scratch) on the grid of 2 or 3 axis tables: the inside bits of the
    last source, and the state of the last labelling. aegolius_amd.topology checks the tables and states the definitions.
    A `source` is a Program (evaluated to inside bits, no field) or a DeviceField of as many values as the grid has
    points."""

    def __init__(self, tables, device=0):
        require_gpu()
        self.tables, tab = axis_args(tables)
        if len(self.tables) not in (2, 3):
            raise ValueError("LabelScratch: two or three axis tables")
        self.shape = tuple(a.size for a in self.tables)
        self.grid = self.shape + (1,) * (3 - len(self.shape))       # (a 2-D grid is n2 = 1 to the library)
        self.tab = tab + (None, 1) * (3 - len(self.shape))
        self.n = int(np.prod(self.shape, dtype=np.int64))
        DeviceBuffer.__init__(self, lib().sdfk_label_scratch(*self.grid), device, "topology")

    def _source(self, source, mode):
        if isinstance(source, Program):
            return "sdfk_eval_grid", (source.handle,), (mode,)
        source._live()
        if source.n != self.n:
            raise ValueError("the field has %d values; the axes span %d points" % (source.n, self.n))
        return "sdfk_field", (_vp(source.ptr),), ()

    def labels(self):
        """A DeviceBuffer for the grid's int32 labels, on the scratch's device."""
        return DeviceBuffer(4 * self.n, self.device, "labels")

    def label(self, source, level, connectivity, region, labels, mode=MODE_AUTO, timings=None):
        """Label the region of `source` into the DeviceBuffer `labels` (sdfk_field_label / sdfk_eval_grid_label);
        source None: the inside bits a previous call left in the scratch, without a second evaluation (sdfk_label_bits).
        -> K. `timings`: a dict that receives device-event milliseconds of LABEL_PASSES."""
        self._live()
        L = lib()
        count = _i64(0)
        ms = (_c.c_float * len(LABEL_PASSES))() if timings is not None else None
        d_labels = labels.at(0, 4 * self.n)
        if source is None:
            check(L.sdfk_label_bits(*self.grid, int(connectivity), int(region), d_labels, ctypes.byref(count), self.at(), ms, None),
                  "sdfk_label_bits")
        else:
            family, lead, tail = self._source(source, mode)
            check(getattr(L, family + "_label")(*lead, *self.tab, _c.c_float(level), int(connectivity), int(region), d_labels,
                                                ctypes.byref(count), self.at(), ms, None, *tail), family + "_label")
        if timings is not None:
            for name, value in zip(LABEL_PASSES, ms):
                timings[name] = timings.get(name, 0.0) + float(value)
        return int(count.value)

    def records(self, count, labels):
        """The records of the last labelling (sdfk_label_finish) -> first (K,) int64, sizes (K,) int64, lower and upper
        (K, D) int32, border (K,) bool."""
        self._live()
        K, D = int(count), len(self.shape)
        first, sizes = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        lower, upper = np.zeros((K, D), dtype=np.int32), np.zeros((K, D), dtype=np.int32)
        border = np.zeros(K, dtype=np.int32)
        check(lib().sdfk_label_finish(*self.grid, K, labels.at(0, 4 * self.n), _ptr(first), _ptr(sizes), _ptr(lower), _ptr(upper),
                                      _ptr(border), self.at(), None), "sdfk_label_finish")
        return first, sizes, lower, upper, border.astype(bool)

    # ---- layer graphs (aegolius_amd.layers states the definitions): the grid is (layers, nu, nv) -------------------------
    def layer_label(self, source, level, connectivity, labels, mode=MODE_AUTO, timings=None):
        """Label the inside points of `source` layer by layer, in-plane connectivity only (sdfk_field_layer_label /
        sdfk_eval_grid_layer_label); source None: the inside bits a previous call left in the scratch
        (sdfk_layer_label_bits). -> K. `timings` as for label()."""
        self._live()
        if len(self.shape) != 3:
            raise ValueError("LabelScratch.layer_label: a stack has three axis tables (heights, U, V)")
        L = lib()
        count = _i64(0)
        ms = (_c.c_float * len(LABEL_PASSES))() if timings is not None else None
        d_labels = labels.at(0, 4 * self.n)
        if source is None:
            check(L.sdfk_layer_label_bits(*self.grid, int(connectivity), d_labels, ctypes.byref(count), self.at(), ms, None),
                  "sdfk_layer_label_bits")
        else:
            family, lead, tail = self._source(source, mode)
            check(getattr(L, family + "_layer_label")(*lead, *self.tab, _c.c_float(level), int(connectivity), d_labels,
                                                      ctypes.byref(count), self.at(), ms, None, *tail), family + "_layer_label")
        if timings is not None:
            for name, value in zip(LABEL_PASSES, ms):
                timings[name] = timings.get(name, 0.0) + float(value)
        return int(count.value)

    def layer_records(self, count, labels):
        """The records of the last layer labelling (sdfk_layer_label_finish): as records(), `border` by the in-plane
        rule."""
        self._live()
        K = int(count)
        first, sizes = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        lower, upper = np.zeros((K, 3), dtype=np.int32), np.zeros((K, 3), dtype=np.int32)
        border = np.zeros(K, dtype=np.int32)
        check(lib().sdfk_layer_label_finish(*self.grid, K, labels.at(0, 4 * self.n), _ptr(first), _ptr(sizes), _ptr(lower),
                                            _ptr(upper), _ptr(border), self.at(), None), "sdfk_layer_label_finish")
        return first, sizes, lower, upper, border.astype(bool)

    def layer_link_count(self, count, labels):
        """The link pass of the last layer labelling, first half (sdfk_layer_links) -> M, the number of link candidates, and
        supported (K,) int64."""
        self._live()
        K, M = int(count), _i64(0)
        supported = np.zeros(K, dtype=np.int64)
        check(lib().sdfk_layer_links(*self.grid, K, labels.at(0, 4 * self.n), ctypes.byref(M), _ptr(supported), self.at(), None),
              "sdfk_layer_links")
        return int(M.value), supported

    def layer_link_candidates(self, count, labels, candidates):
        """The M candidates layer_link_count counted, in word order (sdfk_layer_links_finish) -> child, parent, length (M,)
        int64 — one row per stretch; a pair may come more than once."""
        self._live()
        M = int(candidates)
        keys, lengths = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int32)
        check(lib().sdfk_layer_links_finish(*self.grid, int(count), labels.at(0, 4 * self.n), M, _ptr(keys), _ptr(lengths), self.at(),
                                            None), "sdfk_layer_links_finish")
        return keys >> 32, keys & 0xffffffff, lengths.astype(np.int64)

    def cell_counts(self, source, level, mode=MODE_AUTO):
        """(V, E, F, C) of the cubical complex of the inside points of `source` (sdfk_field_cell_counts /
        sdfk_eval_grid_cell_counts) as Python ints; the inside bits stay in the scratch."""
        self._live()
        counts = np.zeros(4, dtype=np.int64)
        family, lead, tail = self._source(source, mode)
        check(getattr(lib(), family + "_cell_counts")(*lead, *self.tab, _c.c_float(level), _ptr(counts), self.at(), None, *tail),
              family + "_cell_counts")
        return tuple(int(c) for c in counts)


def label_field(labels, n, keep, inside, outside, device=0):
    """A DeviceField of n values: `inside` where the int32 label in the DeviceBuffer `labels` is an id with keep[id] set
    (keep: K bools), `outside` elsewhere (sdfk_label_field)."""
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    field = DeviceField(n, device)
    return field._filled(lambda: check(lib().sdfk_label_field(labels.at(0, 4 * n), n, _ptr(keep), keep.size, float(inside),
                                                              float(outside), _vp(field.ptr), None), "sdfk_label_field"))


def label_moments(labels, shape, count):
    """The integer moment rows of the `count` components in the int32 DeviceBuffer `labels` of the grid `shape` (2 or 3
    axis lengths) -> (count, 10) uint64, 2-D: (count, 6) (sdfk_label_moments; aegolius_amd.topology states the sums)."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64))
    out = np.zeros((int(count), 10 if len(shape) == 3 else 6), dtype=np.uint64)
    labels._live()
    check(lib().sdfk_label_moments(*(shape + (1,) * (3 - len(shape))), labels.at(0, 4 * n), int(count), _ptr(out), None, None),
          "sdfk_label_moments")
    return out


def field_row_sums(d_field, rows, row_len, weights):
    """sum_i field[r, i] * weights[i] in float64 for the `rows` rows of `row_len` floats at the device pointer (int)
    `d_field`, reduced on the device in a fixed order (sdfk_field_row_sums) -> (rows,) float64 host array."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (int(row_len),):
        raise ValueError("field_row_sums: one weight per point of a row")
    out = np.empty(int(rows), dtype=np.float64)
    with DeviceBuffer(max(out.nbytes, 8), what="row sums") as sums:
        check(lib().sdfk_field_row_sums(_vp(d_field), int(rows), int(row_len), _ptr(w), sums.at(), None), "sdfk_field_row_sums")
        return sums.download(out)


class DeviceVectorField(DeviceRows):
    """A (3, N) float32 vector field resident in HBM (what `VectorField.create_resident` returns): three rows of
    `stride` floats. Usable as the input, a second field or the revolution coordinates of another vector-field chain
    without crossing PCIe. Owns its device memory."""

    def __init__(self, n, device=0):
        require_gpu()
        DeviceRows.__init__(self, 3, n, device)

    shape = property(lambda self: (3, self.n))

    @classmethod
    def from_host(cls, vec, device=0):
        host = np.ascontiguousarray(vec, dtype=np.float32)
        if host.ndim != 2 or host.shape[0] != 3:
            raise ValueError("a vector field has shape (3, N); got %r" % (host.shape,))
        self = cls(host.shape[1], device)
        return self._filled(self.upload_rows, host)

    def numpy(self):
        self._live()
        return self.download_rows()


class DeviceCoords:
    """(3, N) coordinates on the device (`ptr`, `stride`, `n`): borrowed from a DeviceVectorField, or owned — points
    [first, first + count) of the grid the per-axis tables `axes` span, filled on the device, or a host array, uploaded
    as float32 (as create() does). free(), or leaving a `with` block, releases what is owned."""

    def __init__(self, co, axes=None, first=0, count=None, device=None, what="coordinates"):
        self.owned = None
        if isinstance(co, DeviceVectorField):
            self.ptr, self.stride, self.n = co.row_ptr(0), co.stride, co.n
            return
        if axes is not None:
            n = int(np.prod([np.asarray(a).size for a in axes])) - first if count is None else count
        else:
            host = host_coords(co, np.float32)
            n = host.shape[1]
        rows = DeviceRows(3, n, device, what)
        if axes is not None:
            rows._filled(grid_fill, rows.ptr, rows.stride, axes, first, n)
        else:
            rows._filled(rows.upload_rows, host)
        self.owned, self.ptr, self.stride, self.n = rows, rows.ptr, rows.stride, n

    def free(self):
        if self.owned is not None:
            self.owned.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def linspace_f32(lo, hi, n):
    out = np.empty(int(n), dtype=np.float32)
    check(lib().sdfk_linspace_f32(float(lo), float(hi), int(n), _ptr(out)), "sdfk_linspace_f32")
    return out


def point_tree(points32, leaf, with_order=False):
    """sdfk_point_tree_build: (m, 3) fp32 points -> (table, n_root, point_base, order or None). Host only."""
    pts = np.ascontiguousarray(points32, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("points must have shape (M, 3), M >= 1; got %r" % (pts.shape,))
    m = int(pts.shape[0])
    half = max(1, int(leaf) // 2)
    cap = 3 * m + 24 * (m // half + 4)
    table = np.empty(cap, dtype=np.float32)
    order = np.empty(m, dtype=np.int64) if with_order else None
    n_root, point_base = _c.c_int64(0), _c.c_int64(0)
    used = lib().sdfk_point_tree_build(_ptr(pts), m, int(leaf), _ptr(table), cap, _ptr(order) if with_order else None,
                                       _c.byref(n_root), _c.byref(point_base))
    if used == -2:
        raise ValueError(last_error())
    if used < 0:
        raise SdfkError("sdfk_point_tree_build: " + last_error())
    return table[:used].copy(), int(n_root.value), int(point_base.value), order


def grid_fill(d_co, row_stride, axes, start, count, stream=None):
    _, tab = axis_args(axes)
    check(lib().sdfk_grid_fill(_vp(d_co), row_stride, *tab, start, count, _vp(stream or 0)), "sdfk_grid_fill")


class Event:
    def __init__(self):
        self._h = lib().sdfk_event_create()
        if not self._h:
            raise SdfkError("sdfk_event_create: " + last_error())

    def record(self, stream=None):
        check(lib().sdfk_event_record(self._h, _vp(stream or 0)), "sdfk_event_record")

    def elapsed_ms(self, stop):
        ms = _c.c_float(0)
        check(lib().sdfk_event_elapsed_ms(self._h, stop._h, ctypes.byref(ms)), "sdfk_event_elapsed_ms")
        return ms.value

    def __del__(self):
        _release(self, "_h", "sdfk_event_destroy")


class Timer:
    """Device-event milliseconds between consecutive mark()s, added to `timings[name]` under the name of the later
    mark. timings=None: no event is created."""

    def __init__(self, timings):
        self.timings = timings
        self.events = []

    def mark(self, name):
        if self.timings is not None:
            ev = Event()
            ev.record()
            self.events.append((name, ev))

    def finish(self):
        if self.timings is None:
            return
        for (_, a), (name, b) in zip(self.events, self.events[1:]):
            self.timings[name] = self.timings.get(name, 0.0) + a.elapsed_ms(b)
