"""ctypes binding of libpyfocusr_hip.so (C-ABI in include/pyfocusr_hip.h).

There is no CPU fallback: if the shared library is missing, or no MI355X is
visible, the product path raises.  The library is built in-tree by
`__graft_entry__.build()` (hipcc --offload-arch=gfx950).
"""
import atexit
import ctypes as C
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYFOCUSR_HIP_LIB", os.path.join(_HERE, "csrc", "libpyfocusr_hip.so"))  # env: tuning builds

PF_OP_RW = 0
PF_OP_SYM = 1

_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


class HipUnavailable(RuntimeError):
    pass


class PfError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libpyfocusr_hip error %d: %s" % (code, msg))
        self.code = code


class _Struct(C.Structure):
    """A structure the library fills in; `as_dict()` gives its fields as Python ints and floats."""

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class GraphInfo(_Struct):
    _fields_ = [("n", C.c_int64), ("n_faces", C.c_int64), ("nnz_w", C.c_int64), ("nnz_l", C.c_int64),
                ("is_symmetric", C.c_int32), ("n_isolated", C.c_int32), ("n_components", C.c_int32),
                ("max_degree", C.c_int32), ("sell_entries", C.c_int64), ("n_pad", C.c_int64), ("n_oneway", C.c_int64),
                ("spectral_bound", C.c_double)]


class EigsStats(_Struct):
    _fields_ = [("matvecs", C.c_int64), ("outer_steps", C.c_int32), ("restarts", C.c_int32), ("filter_resets", C.c_int32),
                ("degree", C.c_int32), ("n_null", C.c_int32), ("cut", C.c_double), ("max_residual", C.c_double),
                ("second_passes", C.c_int32), ("mode", C.c_int32), ("local_steps", C.c_int32), ("reserved", C.c_int32)]


class Timing(_Struct):
    _fields_ = [("op_ms", C.c_double), ("op_launches", C.c_int64), ("op_bytes", C.c_double), ("knn_ms", C.c_double),
                ("build_ms", C.c_double), ("persist_ms", C.c_double), ("persist_launches", C.c_int64),
                ("persist_steps", C.c_int64), ("persist_bytes", C.c_double), ("persist_lds_bytes", C.c_double)]


class AssignStats(_Struct):
    _fields_ = [("phases", C.c_int32), ("dense_passes", C.c_int32), ("rounds", C.c_int64), ("bids", C.c_int64),
                ("dense_bids", C.c_int64), ("candidate_edges", C.c_int64), ("launches", C.c_int64),
                ("device_bytes", C.c_int64), ("k", C.c_int32), ("eps_floor_hit", C.c_int32), ("eps_initial", C.c_double),
                ("eps_final", C.c_double), ("eps_floor", C.c_double), ("total_cost", C.c_double),
                ("gap_bound", C.c_double), ("lower_bound", C.c_double), ("ms_candidates", C.c_double),
                ("ms_auction", C.c_double), ("ms_certificate", C.c_double)]


# name -> (restype, argtypes): every symbol include/pyfocusr_hip.h declares.
SIGNATURES = {
    "pf_version": (C.c_int, []),
    "pf_pool_poison": (C.c_int, [C.c_int]),
    "pf_last_error": (C.c_char_p, []),
    "pf_device_count": (C.c_int, []),
    "pf_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "pf_destroy": (None, [C.c_void_p]),
    "pf_sync": (C.c_int, [C.c_void_p]),
    "pf_stream": (C.c_void_p, [C.c_void_p]),
    "pf_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_timing_get": (C.c_int, [C.c_void_p, C.POINTER(Timing), C.c_int]),
    "pf_graph_build": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_mesh_upload": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_mesh_free": (None, [C.c_void_p]),
    "pf_graph_build_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "pf_graph_build_device2": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "pf_graph_from_matrix": (C.c_int, [C.c_void_p, C.c_int64, _i32p, _i32p, _f64p, C.POINTER(C.c_void_p)]),
    "pf_graph_build_cotan": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_graph_cotan_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pf_graph_cotan_download": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p]),
    "pf_cotan_apply": (C.c_int, [C.c_void_p, _f64p, C.c_int32, _f64p]),
    "pf_graph_free": (None, [C.c_void_p]),
    "pf_graph_get_info": (C.c_int, [C.c_void_p, C.POINTER(GraphInfo)]),
    "pf_graph_rows_compacted": (C.c_int, [C.c_void_p]),
    "pf_graph_download": (C.c_int, [C.c_void_p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "pf_ws_ensure": (C.c_int, [C.c_void_p, C.c_int32]),
    "pf_ws_upload": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "pf_ws_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "pf_ws_copy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "pf_start_vector": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64]),
    "pf_mask_isolated": (C.c_int, [C.c_void_p, C.c_int32]),
    "pf_lock_null_vectors": (C.c_int, [C.c_void_p, C.c_int32, _i32p]),
    "pf_spmv": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "pf_spmv_multi": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pf_knn_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "pf_knn_tree_stats": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pf_persist_enable": (C.c_int, [C.c_int]),
    "pf_persist_two_step": (C.c_int, [C.c_int]),
    "pf_persist_pair_halves": (C.c_int, [C.c_int]),
    "pf_persist_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "pf_persist_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_graph_window_info": (C.c_int, [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 4 + [_i32p, _i32p, _i32p]),
    "pf_persist_test_hook": (C.c_int, [C.c_int]),
    "pf_cheb": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]),
    "pf_cheb2": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                           C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]),
    "pf_dots": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_orth": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p]),
    "pf_orth_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pf_orth_end": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "pf_orth_split": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "pf_orth_one_launch": (C.c_int, [C.c_int32]),
    "pf_orth_begin2": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32]),
    "pf_orth_cheb2": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _i32p, _f64p]),
    "pf_eigsort_costs": (C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, _i64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _f64p, _f64p,
                                   _i64p]),
    "pf_orth_redone": (C.c_int, [C.c_void_p]),
    "pf_orth_strict": (C.c_int, [C.c_void_p, C.c_int32]),
    "pf_scale": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "pf_combine": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int32, C.c_int32]),
    "pf_resnorm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, _f64p]),
    "pf_gram": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_resnorms": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int32, _f64p]),
    "pf_finalize_vectors": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_finalize_vectors_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_finalize_vectors_end": (C.c_int, [C.c_void_p]),
    "pf_final_remap_begin": (C.c_int, [C.c_void_p, _i32p, _f64p, C.c_int32, _f64p]),
    "pf_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "pf_host_free": (C.c_int, [C.c_void_p]),
    "pf_final_rows": (C.c_int, [C.c_void_p, _i64p, C.c_int64, _f64p]),
    "pf_point_rows": (C.c_int, [C.c_void_p, _i64p, C.c_int64, _f64p]),
    "pf_spmv_host": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _f64p]),
    "pf_mean_filter": (C.c_int, [C.c_void_p, _f64p, C.c_int32, C.c_int32, _f64p]),
    "pf_knn1": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, _i64p, _f64p]),
    "pf_knn": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, C.c_int32, _i64p, _f64p]),
    "pf_knn_topk": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, C.c_int32, _i64p, _f64p]),
    "pf_knn1_graphs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _i32p, _f64p, _i32p, _f64p, _i64p, _f64p]),
    "pf_knn1_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                 _i32p, _f64p, _i32p, _f64p, _i64p, _f64p]),
    "pf_final_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _i64p, _i32p]),
    "pf_knn_upload": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32]),
    "pf_knn_run": (C.c_int, [C.c_void_p]),
    "pf_knn_download": (C.c_int, [C.c_void_p, _i64p, _f64p]),
    "pf_eigs_smallest": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, _f64p, C.POINTER(C.c_int32), C.POINTER(EigsStats)]),
    "pf_knn_count": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "pf_knn_wave_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    _f64p]),
    "pf_host_detach": (C.c_int, [C.c_void_p]),
    "pf_orth_device_passes": (C.c_int, [C.c_void_p, C.c_int32]),
    "pf_eigs_smallest_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, C.POINTER(C.c_int32),
                                      C.POINTER(EigsStats)]),
    "pf_eigs_smallest2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    _f64p, _f64p, _f64p, C.POINTER(C.c_int32), C.POINTER(EigsStats),
                                    _f64p, _f64p, _f64p, C.POINTER(C.c_int32), C.POINTER(EigsStats)]),
    "pf_op_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]),
    "pf_cheb_steps": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pf_axpy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_rows_create": (C.c_int, [C.c_void_p, _i64p, C.c_int64, C.POINTER(C.c_void_p)]),
    "pf_rows_free": (None, [C.c_void_p]),
    "pf_rows_gather": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "pf_rows_scatter": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "pf_rows_gather_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "pf_rows_scatter_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "pf_rows_set_sources": (C.c_int, [C.c_void_p, _i64p]),
    "pf_rows_gather2_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "pf_rows_scatter2_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "pf_rows_fill": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "pf_surface_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_surface_free": (None, [C.c_void_p]),
    "pf_surface_closest": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, _i32p, _f64p]),
    "pf_surface_distance": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, _i32p, _f64p]),
    "pf_surface_prepare_signed": (C.c_int, [C.c_void_p, _f64p, _i32p, _i64p]),
    "pf_surface_signed_distance": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, _i32p, _i32p, _i64p]),
    "pf_surface_prepare_winding": (C.c_int, [C.c_void_p]),
    "pf_surface_winding": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_double, _f64p, _f64p]),
    "pf_surface_raycast": (C.c_int, [C.c_void_p, _f64p, _f64p, C.c_int64, C.c_double, C.c_double, C.c_int32, _f64p, _i32p, _f64p,
                                     _i32p]),
    "pf_surface_vertex_normals": (C.c_int, [C.c_void_p, _f64p]),
    "pf_knn1_wide": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, _i64p, _f64p]),
    "pf_knn1_wide_count": (C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    "pf_fmap_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_fmap_free": (None, [C.c_void_p]),
    "pf_fmap_set_p2p": (C.c_int, [C.c_void_p, _i64p]),
    "pf_fmap_get_p2p": (C.c_int, [C.c_void_p, _i64p, _f64p]),
    "pf_fmap_project": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "pf_fmap_convert": (C.c_int, [C.c_void_p, _f64p, C.c_int32, C.c_int32]),
    "pf_fmap_zoomout": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_fmap_set_samples": (C.c_int, [C.c_void_p, _i64p, C.c_int64, _i64p, C.c_int64]),
    "pf_fmap_zoomout_sampled": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64p]),
    "pf_fps": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, _i64p, _i32p, _f64p]),
    "pf_spectral_descriptors": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_int32, _f64p, C.c_int32, _f64p]),
    "pf_descriptor_coefficients": (C.c_int, [C.c_void_p, _f64p, _f64p, C.c_int64, C.c_int32, _f64p, C.c_int32, C.c_int32, _f64p]),
    "pf_surface_nd_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_int32, _i32p, C.c_int64, C.c_int32,
                                       C.POINTER(C.c_void_p)]),
    "pf_surface_nd_free": (None, [C.c_void_p]),
    "pf_surface_nd_closest": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32]),
    "pf_surface_nd_last_search": (C.c_int, [C.c_void_p, _i64p, _i64p, _i64p]),
    "pf_cpd_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "pf_cpd_free": (None, [C.c_void_p]),
    "pf_cpd_estep": (C.c_int, [C.c_void_p, _f64p, C.c_double, C.c_double, _f64p, _f64p, _f64p]),
    "pf_cpd_set_basis": (C.c_int, [C.c_void_p, _f64p, C.c_int32]),
    "pf_cpd_weighted_gram": (C.c_int, [C.c_void_p, _f64p]),
    "pf_cpd_affine_sums": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "pf_cpd_apply_affine": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "pf_cpd_deform_sums": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "pf_cpd_apply_deform": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "pf_cpd_download": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p, _f64p]),
    "pf_cpd_gram": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, C.c_double, _f64p, C.c_int32, _f64p]),
    "pf_assign": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, _i64p, _f64p, _f64p,
                            C.POINTER(AssignStats)]),
    "pf_curvatures": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p,
                                C.POINTER(C.c_uint8), _i64p, _f64p]),
    "pf_mesh_topology": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, C.c_uint32, _i32p, _i32p, C.POINTER(C.c_uint8),
                                   _i32p, C.POINTER(C.c_uint8), _f64p, _i64p, _f64p]),
    "pf_mesh_cluster": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, _f64p, _i64p, C.c_int64, C.c_int32, C.c_uint32,
                                  _f64p, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i64p, _f64p]),
    "pf_map_distortion": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, _f64p, C.c_int64, _f64p, _i32p, _f64p, C.c_int32,
                                    _f64p, _f64p, C.POINTER(C.c_uint8), _f64p, _f64p, C.POINTER(C.c_uint8), _i32p, _f64p, _f64p,
                                    _i64p, _f64p]),
    "pf_shapes_create": (C.c_int, [C.c_void_p, _f64p, C.c_int32, C.c_int64, _f64p, C.POINTER(C.c_void_p)]),
    "pf_shapes_free": (None, [C.c_void_p]),
    "pf_shapes_weight_sum": (C.c_int, [C.c_void_p, _f64p]),
    "pf_shapes_center": (C.c_int, [C.c_void_p, _f64p]),
    "pf_shapes_mean": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, _f64p]),
    "pf_shapes_align_sums": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p]),
    "pf_shapes_transform": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p]),
    "pf_shapes_gram": (C.c_int, [C.c_void_p, _f64p]),
    "pf_shapes_combine": (C.c_int, [C.c_void_p, _f64p, C.c_int32, _f64p]),
    "pf_shapes_scores": (C.c_int, [C.c_void_p, _f64p, C.c_int32, _f64p]),
    "pf_shapes_set_reference": (C.c_int, [C.c_void_p, _f64p]),
    "pf_shapes_download": (C.c_int, [C.c_void_p, _f64p]),
    "pf_shapes_device_ms": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "pf_isosurface_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_double, _f64p, _f64p, C.c_uint32,
                                       C.POINTER(C.c_void_p), _i64p, _f64p]),
    "pf_isosurface_fetch": (C.c_int, [C.c_void_p, _f64p, _i32p, _i64p, _i32p]),
    "pf_isosurface_free": (None, [C.c_void_p]),
    "pf_smoother_create": (C.c_int, [C.c_void_p, _f64p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                     C.POINTER(C.c_void_p)]),
    "pf_smoother_info": (C.c_int, [C.c_void_p, _i64p]),
    "pf_smoother_adjacency": (C.c_int, [C.c_void_p, _i32p, _i32p, _f64p, C.POINTER(C.c_uint8)]),
    "pf_smoother_run": (C.c_int, [C.c_void_p, _f64p, C.c_int32, _f64p, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, _f64p]),
    "pf_smoother_free": (None, [C.c_void_p]),
    "pf_edt_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int64, C.c_int64, C.c_int64, _f64p, C.c_int32, C.c_uint32,
                                C.POINTER(C.c_void_p), _i64p, _f64p]),
    "pf_edt_fetch": (C.c_int, [C.c_void_p, _f64p, _f64p, _i32p]),
    "pf_edt_isosurface": (C.c_int, [C.c_void_p, C.c_double, _f64p, C.POINTER(C.c_void_p), _i64p, _f64p]),
    "pf_edt_free": (None, [C.c_void_p]),
    "pf_ccl_create": (C.c_int, [C.c_void_p, _i32p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32,
                                C.POINTER(C.c_void_p), _i64p, _f64p]),
    "pf_ccl_fetch": (C.c_int, [C.c_void_p, _i32p, _i64p, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_uint8), _i64p]),
    "pf_ccl_select": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "pf_ccl_info": (C.c_int, [C.c_void_p, _i64p]),
    "pf_ccl_combine_stats": (C.c_int, [C.c_int]),
    "pf_ccl_free": (None, [C.c_void_p]),
}

_lib = None
_lib_lock = threading.Lock()
_live_graphs = weakref.WeakSet()
_live_contexts = weakref.WeakSet()


@atexit.register
def _shutdown():
    """Release device objects while the HIP runtime is still alive (its own static
    destructors run after Python's, and freeing into a torn-down runtime aborts)."""
    for g in list(_live_graphs):
        g.close()
    for c in list(_live_contexts):
        c.close()


def load_library():
    """dlopen the in-tree library and bind every declared symbol (no GPU needed)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipUnavailable(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


PF_E_DEGENERATE = -3
PF_E_STATE = -4
PF_E_PERSIST_TIMEOUT = -5
PF_E_INTERNAL = -6
PF_TOPOLOGY_OUTWARD = 1
PF_CLUSTER_UPDATE_ONLY = 1


class _PinnedBlock(object):
    """One hipHostMalloc block; goes back to the module's free list when the last array over it is collected."""
    __slots__ = ("ptr", "nbytes")

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes

    def __del__(self):
        try:
            _pinned_release(self.ptr, self.nbytes)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


_pinned_free = {}  # nbytes -> [ptr]: blocks of collected arrays, reused by the next result of the same size
_pinned_cached = [0]
# (compute_spectra runs one host thread per context; arrays are collected on any thread.)  Re-entrant: the locked region of
# _pinned_release allocates, a collection started there can finalise another block on the same thread, and that comes back here
_pinned_lock = threading.RLock()
# page-locked memory kept for reuse.  A 1M-vertex pair with k = 10 turns over four 84 MB blocks per pipeline step: with the
# 256 MiB of round 3 whether they fitted beside what smaller workloads had left behind decided between 80 and 90 ms per
# step (two hipHostMalloc / hipHostFree of 84 MB each) - 1 GiB, and blocks of OTHER sizes make room first.
_PINNED_CACHE_BYTES = 1 << 30


def _pinned_release(ptr, nbytes):
    if _pinned_free is None or _lib is None:
        return
    # a download the library still OWES to this block (pf_finalize_vectors_begin holds downloads back; a failed call may
    # have left one behind) must never be queued once the block can be handed out again; one in flight is waited for
    _lib.pf_host_detach(C.c_void_p(ptr))
    evicted = []
    with _pinned_lock:
        if nbytes <= _PINNED_CACHE_BYTES:
            # the sizes in use now are the ones worth keeping: blocks of other sizes go first (largest first)
            while _pinned_cached[0] + nbytes > _PINNED_CACHE_BYTES:
                others = [sz for sz, ptrs in _pinned_free.items() if ptrs and sz != nbytes]
                if not others:
                    break
                sz = max(others)
                evicted.append(_pinned_free[sz].pop())
                _pinned_cached[0] -= sz
        keep = _pinned_cached[0] + nbytes <= _PINNED_CACHE_BYTES
        if keep:
            _pinned_free.setdefault(nbytes, []).append(ptr)
            _pinned_cached[0] += nbytes
    for other in evicted:
        _lib.pf_host_free(C.c_void_p(other))
    if not keep:
        _lib.pf_host_free(C.c_void_p(ptr))


def pinned_trim():
    """Give the cached page-locked blocks back to the system (they are kept for reuse otherwise, up to 1 GiB)."""
    with _pinned_lock:
        blocks = [p for ptrs in _pinned_free.values() for p in ptrs]
        _pinned_free.clear()
        _pinned_cached[0] = 0
    for ptr in blocks:
        _lib.pf_host_free(C.c_void_p(ptr))


def pinned_empty(shape, dtype=np.float64):
    """`np.empty(shape, dtype)` over page-locked host memory (pf_host_alloc): device results land in it by one DMA
    instead of the runtime's chunked staging of a pageable destination (hipHostMalloc itself costs 0.1-1 ms: the blocks
    of collected arrays are kept and reused).  Ordinary cacheable host memory for every other purpose."""
    lib = load_library()
    dtype = np.dtype(dtype)
    count = int(np.prod(shape)) if len(shape) else 1
    nbytes = max(count * dtype.itemsize, 1)
    nbytes = (nbytes + 4095) & ~4095
    ptr = None
    with _pinned_lock:
        free = _pinned_free.get(nbytes)
        if free:
            ptr = free.pop()
            _pinned_cached[0] -= nbytes
    if ptr is None:
        p = C.c_void_p()
        _check(lib.pf_host_alloc(C.c_size_t(nbytes), C.byref(p)))
        ptr = int(p.value)
    buf = (C.c_char * nbytes).from_address(ptr)
    buf._pf_block = _PinnedBlock(ptr, nbytes)  # the array's base keeps `buf`, and with it the block, alive
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def persist_enable(on=True):
    """Process-wide switch of the resident Chebyshev kernel (operator in registers, x in LDS, one kernel per filter
    application; on by default, see csrc/pf_persist.hip).  Results are bit-identical either way."""
    _check(load_library().pf_persist_enable(int(bool(on))))


def pool_poison(on=True):
    """Process-wide debugging switch (off by default): every block the device memory pool hands out is filled with
    0xFF bytes (NaN / -1) before its first use with `on` = 1 or True, with zero bytes with `on` = 2; 0 or False is off.
    Results are bit-identical in every mode; a difference is a bug."""
    on = int(on)
    if on not in (0, 1, 2):
        raise ValueError("pool_poison: 0 (off), 1 (0xFF bytes) or 2 (zero bytes), got %r" % (on,))
    _check(load_library().pf_pool_poison(on))


def orth_one_launch(on=True):
    """Process-wide switch of the one-launch local Gram-Schmidt step (csrc/pf_orth.hip: k_orth_local); off: dot
    products and projection as two launches, like every other step.  Results are bit-identical either way."""
    _check(load_library().pf_orth_one_launch(int(bool(on))))


def persist_two_step(level=1):
    """Process-wide level of the two-steps-per-exchange form of the resident kernel (csrc/pf_persist.hip:
    k_cheb_resident2): 0 off, 1 single-graph recurrences (default; a higher level means 1).  Paired recurrences
    always take one step per exchange.  Results are bit-identical at every level."""
    _check(load_library().pf_persist_two_step(int(level)))


def persist_pair_halves(on=True):
    """Process-wide switch of the pair kernel whose halves take the two graphs in opposite order (csrc/pf_persist.hip:
    k_cheb_resident<2,1,8,true>; on by default).  Results are bit-identical either way."""
    _check(load_library().pf_persist_pair_halves(int(bool(on))))


def persist_clock(ctx, reset=False):
    """(summed run time in ms, number) of ctx's completed resident launches since the last reset, on the device's own
    100 MHz clock inside the kernel (csrc/pf_persist.hip: pf_persist_clock).  Synchronises the ctx stream."""
    ms, n = C.c_double(0.0), C.c_int64(0)
    _check(load_library().pf_persist_clock(ctx._h, C.byref(ms), C.byref(n), int(bool(reset))))
    return ms.value, n.value


class _PersistInfo(_Struct):
    _fields_ = [("enabled", C.c_int32), ("two_step", C.c_int32), ("owner", C.c_int32), ("timeouts", C.c_int32),
                ("launches", C.c_int64), ("launches_two_step", C.c_int64), ("suspended_for", C.c_int32), ("rearms", C.c_int32),
                ("owner_switches", C.c_int32), ("hold_ticks", C.c_int32)]


def persist_state(ctx=None):
    """pf_persist_state as a dict: is the resident path on, who owns it, how many waits ran out, launch counters."""
    info = _PersistInfo()
    _check(load_library().pf_persist_state(None if ctx is None else ctx._h, C.byref(info)))
    return info.as_dict()


def persist_test_hook(n_launches=1):
    """Test hook: the next `n_launches` resident launches give up at once (PF_E_PERSIST_TIMEOUT recovery)."""
    _check(load_library().pf_persist_test_hook(int(n_launches)))


def _check(code):
    if code != 0:
        raise PfError(code, load_library().pf_last_error().decode("utf-8", "replace"))


_POINTER_OF = {np.dtype(t): C.POINTER(c) for t, c in ((np.float64, C.c_double), (np.int32, C.c_int32), (np.int64, C.c_int64),
                                                        (np.uint8, C.c_uint8), (np.uint64, C.c_uint64))}


def _ptr(a):
    """The typed pointer to a C-contiguous array, chosen by its dtype, so that the `argtypes` of SIGNATURES check what
    the library is handed (ctypes.ArgumentError on a mismatch); None (an output nobody asked for) stays None."""
    if a is None:
        return None
    try:
        ptype = _POINTER_OF[a.dtype]
    except KeyError:
        raise TypeError("no pointer type for dtype %s: the library takes float64, int32, int64, uint8 and uint64" % a.dtype)
    if not a.flags.c_contiguous:
        raise ValueError("the library needs a C-contiguous array, not a strided view")
    return a.ctypes.data_as(ptype)


def _f64(a):
    """`_ptr` of an array that must hold float64."""
    if a is not None and a.dtype != np.float64:
        raise TypeError("a float64 array is needed, not %s" % a.dtype)
    return _ptr(a)


def _c_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError("expected shape %r, got %r" % (shape, a.shape))
    return a


def _c_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _c_i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


_EQUAL_D = "%s must be (n, d) arrays with equal d"


def _same_d(a, b, message=_EQUAL_D % "ref and qry"):
    """Two point sets as contiguous f64 (n, d) arrays of one d."""
    a, b = _c_f64(a), _c_f64(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(message)
    return a, b


def _queries(a, noun="queries", message=None):
    """Query points as a contiguous f64 array that must be (n, 3) with n > 0."""
    a = _c_f64(a)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError(message or "%s must be a non-empty (n, 3) array" % noun)
    return a


def _rays(origins, directions):
    message = "origins and directions must be non-empty (n, 3) arrays of the same length"
    o, d = _queries(origins, message=message), _c_f64(directions)
    if d.shape != o.shape:
        raise ValueError(message)
    return o, d


def _upload_arrays(points, faces, empty_ok=True):
    """(points (n, 3) f64, faces (F, v) i32, v) of a mesh that goes to the device; v is 3 where there is no face."""
    pts, f = _c_f64(points).reshape(-1, 3), _c_i32(faces)
    if f.ndim != 2 or not (empty_ok or f.shape[0]):
        raise ValueError("faces must be %s" % ("(F, verts_per_face)" if empty_ok else "a non-empty (F, verts_per_face) array"))
    return pts, f, f.shape[1] if f.shape[0] else 3


def degenerate_extent_message(target_points, source_points):
    """The text of the ValueError eigsort raises when its spatial 1-NN found no neighbour: which sample has no extent
    along which axis (raw points: max == min; min-max normalised points: NaN)."""
    found = []
    for name, pts in (("target", target_points), ("source", source_points)):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            flat = np.isnan(pts).any(axis=0) | ~(np.max(pts, axis=0) > np.min(pts, axis=0))
        if flat.any():
            found.append("the %s sample (%d points) has no extent along %s" % (name, len(pts), ", ".join("xyz"[a] for a in np.where(flat)[0])))
    return ("eigsort: degenerate extent - %s: the min-max normalisation of the sampled points divides by zero (a planar "
            "mesh, or a sample of one point), so no point has a nearest neighbour"
            % ("; ".join(found) if found else "the sampled points do not compare"))


KNN_TOPK_MAX_K = 64    # the limits of pf_knn_topk
KNN_TOPK_MAX_D = 128


def check_knn_topk(ref, qry, k):
    """The argument checks of `Context.knn_topk`, which need no library: ValueError, or k as an int."""
    ref_shape, qry_shape = np.shape(ref), np.shape(qry)
    if len(ref_shape) != 2 or len(qry_shape) != 2 or ref_shape[1] != qry_shape[1]:
        raise ValueError(_EQUAL_D % "ref and qry")
    if not 1 <= ref_shape[1] <= KNN_TOPK_MAX_D:
        raise ValueError("d = %d out of range (1 .. %d)" % (ref_shape[1], KNN_TOPK_MAX_D))
    k = int(k)
    if not 1 <= k <= min(KNN_TOPK_MAX_K, ref_shape[0]):
        raise ValueError("k = %d out of range (1 .. min(%d, n_ref = %d))" % (k, KNN_TOPK_MAX_K, ref_shape[0]))
    return k


class Context(object):
    """One HIP stream on one device."""

    def __init__(self, device=0):
        lib = load_library()
        if lib.pf_device_count() <= 0:
            raise HipUnavailable("no HIP device visible: the pyfocusr_amd hot path needs an MI355X (no CPU fallback)")
        h = C.c_void_p()
        _check(lib.pf_create(int(device), C.byref(h)))
        self._lib = lib
        self._h = h
        self.device = int(device)
        self._children = weakref.WeakSet()  # graphs / meshes allocated from this context
        _live_contexts.add(self)

    def close(self):
        if getattr(self, "_h", None):
            for child in list(self._children):  # device objects must go before their allocator
                child.close()
            self._lib.pf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def sync(self):
        _check(self._lib.pf_sync(self._h))

    @property
    def stream_ptr(self):
        """Address of the ctx's hipStream_t (for `torch.cuda.ExternalStream`: a collective enqueued on it is ordered
        with the library's kernels without any host synchronisation)."""
        return int(self._lib.pf_stream(self._h) or 0)

    def timing_enable(self, on=True):
        """HIP-event timing of the filter applications: True / 1 every application, N > 1 every N-th, False off."""
        _check(self._lib.pf_timing_enable(self._h, int(on)))

    def timing(self, reset=False):
        t = Timing()
        _check(self._lib.pf_timing_get(self._h, C.byref(t), int(bool(reset))))
        return t.as_dict()

    # ---- nearest neighbour -------------------------------------------------------------
    def knn_mode(self, mode):
        """How 1-NN searches prune: 0 by depth (grid for d <= 6, box hierarchy for d >= 7), 1 always the grid, 2 always
        the hierarchy.  The results are the same bits."""
        _check(self._lib.pf_knn_mode(self._h, int(mode)))

    def knn_count(self, enable_counting=False):
        """Candidate-query pairs evaluated by the last counted grid search (`pf_knn_count`); sets the switch for the next."""
        pairs = C.c_int64()
        _check(self._lib.pf_knn_count(self._h, int(bool(enable_counting)), C.byref(pairs)))
        return int(pairs.value)

    def knn_tree_stats(self, enable_counting=False):
        """(leaves scanned, supers opened) of the last box-hierarchy search, if counting was on for it; sets the switch."""
        a, b = C.c_int64(), C.c_int64()
        _check(self._lib.pf_knn_tree_stats(self._h, int(bool(enable_counting)), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def knn1(self, ref, qry, return_d2=False):
        """Index (int64) of the nearest `ref` row for every `qry` row."""
        ref, qry = _same_d(ref, qry)
        idx = np.empty(qry.shape[0], dtype=np.int64)
        d2 = np.empty(qry.shape[0], dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_knn1(self._h, _f64(ref), ref.shape[0], _f64(qry), qry.shape[0], ref.shape[1],
                                 _ptr(idx), _f64(d2)))
        return (idx, d2) if return_d2 else idx

    def knn1_wide(self, ref, qry, return_d2=False):
        """`knn1` for 1 <= d <= 128 by the tiled exhaustive scan (`pf_knn1_wide`): the same arithmetic, the same bits."""
        ref, qry = _same_d(ref, qry)
        idx = np.empty(qry.shape[0], dtype=np.int64)
        d2 = np.empty(qry.shape[0], dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_knn1_wide(self._h, _f64(ref), ref.shape[0], _f64(qry), qry.shape[0], ref.shape[1],
                                      _ptr(idx), _f64(d2)))
        return (idx, d2) if return_d2 else idx

    def knn1_wide_count(self, enable_counting=False):
        """Coordinate pairs the last counted `knn1_wide` evaluated (`pf_knn1_wide_count`); sets the switch for the next."""
        pairs = C.c_int64()
        _check(self._lib.pf_knn1_wide_count(self._h, int(bool(enable_counting)), C.byref(pairs)))
        return int(pairs.value)

    # ---- farthest-point sampling --------------------------------------------------------
    def farthest_point_sampling(self, points, m, start=-1, return_owner=False, return_d2=False):
        """`pf_fps`: sel (int64, m) of the (n, d) points, 1 <= d <= 16; `start` -1 begins at the point farthest from the
        centroid.  With `return_owner` the position in sel of every point's nearest sample (int32, n), with `return_d2`
        the squared distance to it.  Samples repeat once m exceeds the number of distinct points.  The library refuses
        d, m or start out of range and non-finite coordinates with `PfError` (PF_E_ARG)."""
        pts = _c_f64(points)
        if pts.ndim != 2:
            raise ValueError("points must be an (n, d) array")
        n, m = pts.shape[0], int(m)
        sel = np.empty(max(m, 0), dtype=np.int64)
        owner = np.empty(n, dtype=np.int32) if return_owner else None
        d2 = np.empty(n, dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_fps(self._h, _f64(pts), n, pts.shape[1], m, int(start), _ptr(sel), _ptr(owner), _f64(d2)))
        out = (sel,) + ((owner,) if return_owner else ()) + ((d2,) if return_d2 else ())
        return out if len(out) > 1 else sel

    # ---- spectral descriptors ----------------------------------------------------------
    def spectral_descriptors(self, phi, G):
        """F (n, T): F[i, t] = sum_a phi[i, a]^2 G[a, t] (`pf_spectral_descriptors`).  Only the shapes are checked
        here; the library refuses K > 128, T > 512 and n = 0 with `PfError` (PF_E_ARG)."""
        phi, G = _c_f64(phi), _c_f64(G)
        if phi.ndim != 2 or G.ndim != 2 or G.shape[0] != phi.shape[1]:
            raise ValueError("phi must be (n, K) and G (K, T)")
        out = np.empty((phi.shape[0], G.shape[1]), dtype=np.float64)
        _check(self._lib.pf_spectral_descriptors(self._h, _f64(phi), phi.shape[0], phi.shape[1], _f64(G), G.shape[1], _f64(out)))
        return out

    def descriptor_coefficients(self, phi, mass, G, k_out):
        """A (k_out, T): A[a, t] = sum_i mass[i] phi[i, a] F[i, t] with F as in `spectral_descriptors`, never stored
        (`pf_descriptor_coefficients`).  Shapes are checked here, the limits by the library (PF_E_ARG)."""
        phi, G = _c_f64(phi), _c_f64(G)
        if phi.ndim != 2 or G.ndim != 2 or G.shape[0] != phi.shape[1]:
            raise ValueError("phi must be (n, K) and G (K, T)")
        mass = _c_f64(mass, (phi.shape[0],))
        out = np.empty((max(int(k_out), 0), G.shape[1]), dtype=np.float64)
        _check(self._lib.pf_descriptor_coefficients(self._h, _f64(phi), _f64(mass), phi.shape[0], phi.shape[1], _f64(G), G.shape[1],
                                                    int(k_out), _f64(out)))
        return out

    # ---- discrete curvatures -----------------------------------------------------------
    def curvatures(self, points, faces):
        """`pf_curvatures` of the triangle mesh (points (n, 3) f64, faces (m, 3) i32): a dict with `area`, `gaussian`,
        `mean` (n,), `tensor` (n, 6) xx yy zz xy xz yz, `k` (n, 4) = k_min, k_max from (H, K) | k_min, k_max of the
        tensor, `dirs` (n, 6) = d_min | d_max, `normals` (n, 3), `boundary` (n,) bool, `topology` (5,) int64 = edges |
        boundary | non-manifold | inconsistent edges | clipped vertices, and `device_ms`.  Only the shapes are checked
        here (`curvature.discrete_curvatures` checks the values); the library refuses an index out of range (PF_E_ARG)."""
        pts = _c_f64(points)
        f = _c_i32(faces)
        if pts.ndim != 2 or pts.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("points must be (n, 3) and faces (m, 3)")
        n = pts.shape[0]
        out = {"area": np.empty(n), "gaussian": np.empty(n), "mean": np.empty(n), "tensor": np.empty((n, 6)), "k": np.empty((n, 4)),
               "dirs": np.empty((n, 6)), "normals": np.empty((n, 3))}
        boundary = np.empty(n, dtype=np.uint8)
        topology = np.zeros(5, dtype=np.int64)
        ms = C.c_double(0.0)
        _check(self._lib.pf_curvatures(self._h, _f64(pts), n, _ptr(f), f.shape[0], _f64(out["area"]),
                                       _f64(out["gaussian"]), _f64(out["mean"]), _f64(out["tensor"]), _f64(out["k"]),
                                       _f64(out["dirs"]), _f64(out["normals"]), _ptr(boundary), _ptr(topology), C.byref(ms)))
        out.update(boundary=boundary.astype(bool), topology=topology, device_ms=ms.value)
        return out

    # ---- mesh topology -----------------------------------------------------------------
    def mesh_topology(self, n_points, faces, points=None, outward=True):
        """`pf_mesh_topology` of the triangle mesh (faces (m, 3) i32 over `n_points` vertices; points (n, 3) f64 or None:
        they only serve the outward rule): a dict with `face_neighbours` (m, 3) int32 (-1 boundary, -2 non-manifold),
        `patch` (m,) int32, `flip` (m,) bool, `boundary_loop` (m, 3) int32 (-1: not on a boundary), `patch_orientable`
        (P,) bool, `patch_volume` (P,), `report` (8,) int64 = edges | boundary | non-manifold | inconsistent edges |
        patches | loops | rounds | loop rounds, and `device_ms`.  Only the shapes are checked here; the library refuses
        an index out of range (PF_E_ARG) and a face that repeats a vertex (PF_E_DEGENERATE)."""
        f = _c_i32(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("faces must be (m, 3)")
        n, m = int(n_points), f.shape[0]
        pts = None
        if points is not None:
            pts = _c_f64(points)
            if pts.shape != (n, 3):
                raise ValueError("points must be (n_points, 3)")
        nbr, loop = np.empty((m, 3), dtype=np.int32), np.empty((m, 3), dtype=np.int32)
        patch, flip = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.uint8)
        orientable, volume = np.empty(m, dtype=np.uint8), np.empty(m)
        report = np.zeros(8, dtype=np.int64)
        ms = C.c_double(0.0)
        _check(self._lib.pf_mesh_topology(self._h, _f64(pts), n, _ptr(f), m, PF_TOPOLOGY_OUTWARD if outward else 0, _ptr(nbr),
                                          _ptr(patch), _ptr(flip), _ptr(loop), _ptr(orientable), _f64(volume), _ptr(report),
                                          C.byref(ms)))
        P = int(report[4])
        return {"face_neighbours": nbr, "patch": patch, "flip": flip.astype(bool), "boundary_loop": loop,
                "patch_orientable": orientable[:P].astype(bool), "patch_volume": volume[:P].copy(), "report": report,
                "device_ms": ms.value}

    # ---- isosurface extraction ---------------------------------------------------------
    def isosurface(self, values, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
        """`pf_isosurface_create` / `_fetch` / `_free` of the volume (nx, ny, nz): a dict with `points` (V, 3) f64, `faces`
        (F, 3) int32, `vertex_key` (V,) int64 = 7 * lattice index + edge kind, `face_cell` (F,) int32, `report` (8,) int64 =
        vertices | faces | cells with a face | lattice points | cells | 0 | 0 | 0, and `device_ms`.  `value < level` is
        inside and the normals point outside.  Shapes and finiteness are checked here (`check_volume`)."""
        with DeviceIsosurface(values, level, spacing, origin, ctx=self) as iso:
            pts, faces, key, cell = iso.fetch()
            return {"points": pts, "faces": faces, "vertex_key": key, "face_cell": cell, "report": iso.report,
                    "device_ms": iso.device_ms}

    # ---- distance transforms of masks ---------------------------------------------------
    def distance_transform(self, mask, spacing=(1.0, 1.0, 1.0), signed=False, dist=True, dist2=True, nearest=True):
        """`pf_edt_create` / `_fetch` / `_free` of the mask (nx, ny, nz): a dict with `dist` and `dist2` (nx, ny, nz) f64,
        `nearest` (nx, ny, nz) int32 = the flat index of the nearest feature or -1 (each only if asked for), `report` (8,)
        int64 = samples | foreground | background | 0 ... and `device_ms`.  Shapes and spacing are checked here
        (`check_mask`)."""
        with DeviceDistanceTransform(mask, spacing, signed, ctx=self) as edt:
            out = dict(zip(("dist", "dist2", "nearest"), edt.fetch(dist, dist2, nearest)))
            out = {k: v for k, v in out.items() if v is not None}
            out.update(report=edt.report, device_ms=edt.device_ms)
            return out

    # ---- connected components of masks and label maps ----------------------------------
    def connected_components(self, vol, connectivity=6, mode=0, component=True, stats=True, keep=None):
        """`pf_ccl_create` / `_fetch` / `_free` of the volume (nx, ny, nz): a dict with `n`, `component` (nx, ny, nz) int32,
        the tables `count`, `value`, `root`, `lo`, `hi`, `border`, `sum` (each group only if asked for), `selected`
        (nx, ny, nz) bool = `pf_ccl_select` of `keep` (a function of the tables dict, or an array; only if given), `report`
        (8,) int64 = samples | labelled voxels | components | union retries | largest count | 0 ... and `device_ms`.
        Shape, dtype and connectivity are checked here (`check_label_volume`)."""
        with DeviceComponents(vol, connectivity, mode, ctx=self) as ccl:
            comp, tables = ccl.fetch(component, stats or callable(keep))
            out = {"n": ccl.n, "report": ccl.report, "device_ms": ccl.device_ms}
            if comp is not None:
                out["component"] = comp
            if stats:
                out.update(tables)
            if keep is not None:
                out["selected"] = ccl.select(keep(tables) if callable(keep) else keep)
            return out

    # ---- mesh resampling ---------------------------------------------------------------
    def cluster_mesh(self, points, faces, mass, seeds=None, n_iter=20, centroids=None, labels=None, update_only=False):
        """`pf_mesh_cluster`: Lloyd clusters of the vertices and their dual triangulation (points (n, 3) f64, faces (f, 3)
        i32 or None, mass (n,) f64).  Start from `seeds` (m vertex indices) or from `centroids` (m, 3); `labels` (n,) only
        warm-starts the first search, except with `update_only`, where one update step runs from them and nothing is
        assigned.  A dict with `labels` (n,) int32, `centroids` (m, 3), `rep`, `count` (m,) int32, `changed` (n_iter_run,)
        int32, `n_iter_run`, `faces` (k, 3) int32, `face_src` (k,) int32, `votes` (k, 2) int32, `n_candidate_faces`,
        `report` (8,) int64 and `device_ms`.  Only the shapes are checked here; the library refuses indices out of range,
        non-finite input, negative masses and m above 2^21 - 1 (PF_E_ARG) and a face that repeats a vertex
        (PF_E_DEGENERATE)."""
        pts = _c_f64(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must be (n, 3)")
        n = pts.shape[0]
        f = np.zeros((0, 3), dtype=np.int32) if faces is None else _c_i32(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("faces must be (f, 3)")
        mass = _c_f64(mass, (n,))
        if (seeds is None) == (centroids is None):
            raise ValueError("give either seeds or centroids")
        sel = cen = lab = None
        if seeds is not None:
            sel = _c_i64(seeds)
            if sel.ndim != 1:
                raise ValueError("seeds must be a vector of vertex indices")
            m = sel.shape[0]
        else:
            cen = _c_f64(centroids)
            if cen.ndim != 2 or cen.shape[1] != 3:
                raise ValueError("centroids must be (m, 3)")
            m = cen.shape[0]
        if labels is not None:
            lab = _c_i32(labels)
            if lab.shape != (n,):
                raise ValueError("labels must be (n,)")
        n_iter, k = int(n_iter), f.shape[0]
        out_labels, out_c = np.empty(n, dtype=np.int32), np.empty((m, 3))
        rep, count = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        changed = np.zeros(max(n_iter, 0), dtype=np.int32)
        out_f, src, votes = np.empty((k, 3), dtype=np.int32), np.empty(k, dtype=np.int32), np.empty((k, 2), dtype=np.int32)
        report = np.zeros(8, dtype=np.int64)
        ms = C.c_double(0.0)
        _check(self._lib.pf_mesh_cluster(
            self._h, _f64(pts), n, _ptr(f if k else None), k, _f64(mass), _ptr(sel), m, n_iter,
            PF_CLUSTER_UPDATE_ONLY if update_only else 0, _f64(cen), _ptr(lab), _ptr(out_labels), _f64(out_c), _ptr(rep),
            _ptr(count), _ptr(changed), _ptr(out_f), _ptr(src), _ptr(votes), _ptr(report), C.byref(ms)))
        run, kept = (0 if update_only else int(report[0])), int(report[1])
        return {"labels": out_labels, "centroids": out_c, "rep": rep, "count": count, "changed": changed[:run].copy(),
                "n_iter_run": int(report[0]), "faces": out_f[:kept].copy(), "face_src": src[:kept].copy(),
                "votes": votes[:kept].copy(), "n_candidate_faces": int(report[2]), "report": report, "device_ms": ms.value}

    # ---- map distortion and coverage ---------------------------------------------------
    def map_distortion(self, src_points, src_faces, tgt_points, map_vertices, map_weights=None, tgt_normals=None):
        """`pf_map_distortion` of a correspondence from the triangle mesh (src_points (n, 3) f64, src_faces (m, 3) i32) onto
        tgt_points (k, 3) f64: map_vertices (n,) or (n, 1) i32 is a vertex map, (n, 3) with map_weights (n, 3) f64 a surface
        map (vertices / bary); a row that starts with -1 is unmapped.  tgt_normals (k, 3) f64 or None: without them nothing is
        flagged as flipped.  A dict with `face_sigma` (m, 2), `face_area_ratio` (m,), `face_flags` (m,) uint8 (1 valid |
        2 collapsed | 4 flipped | 8 unmapped corner), `vertex_area` (n,), `vertex_sigma` (n, 2), `vertex_flags` (n,) uint8,
        `target_count` (k,) int32, `target_premass` (k,), `totals` (8,), `report` (8,) int64 and `device_ms`.  Only the
        shapes are checked here; the library refuses indices out of range and non-finite values of mapped rows (PF_E_ARG)
        and a face that repeats a vertex (PF_E_DEGENERATE)."""
        pts, tgt = _c_f64(src_points), _c_f64(tgt_points)
        f = _c_i32(src_faces)
        if pts.ndim != 2 or pts.shape[1] != 3 or tgt.ndim != 2 or tgt.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("points must be (n, 3) and faces (m, 3)")
        n, m, k = pts.shape[0], f.shape[0], tgt.shape[0]
        mv = _c_i32(map_vertices)
        if mv.ndim == 1:
            mv = mv.reshape(-1, 1)
        if mv.ndim != 2 or mv.shape[0] != n or mv.shape[1] not in (1, 3):
            raise ValueError("map_vertices must be (n,), (n, 1) or (n, 3)")
        c = mv.shape[1]
        mw = None
        if c == 3:
            if map_weights is None:
                raise ValueError("a map of 3 corners needs map_weights (n, 3)")
            mw = _c_f64(map_weights, (n, 3))
        nrm = None if tgt_normals is None else _c_f64(tgt_normals, (k, 3))
        out = {"face_sigma": np.empty((m, 2)), "face_area_ratio": np.empty(m), "face_flags": np.empty(m, dtype=np.uint8),
               "vertex_area": np.empty(n), "vertex_sigma": np.empty((n, 2)), "vertex_flags": np.empty(n, dtype=np.uint8),
               "target_count": np.empty(k, dtype=np.int32), "target_premass": np.empty(k), "totals": np.zeros(8),
               "report": np.zeros(8, dtype=np.int64)}
        ms = C.c_double(0.0)
        _check(self._lib.pf_map_distortion(
            self._h, _f64(pts), n, _ptr(f), m, _f64(tgt), k, _f64(nrm), _ptr(mv), _f64(mw), c, _f64(out["face_sigma"]),
            _f64(out["face_area_ratio"]), _ptr(out["face_flags"]), _f64(out["vertex_area"]), _f64(out["vertex_sigma"]),
            _ptr(out["vertex_flags"]), _ptr(out["target_count"]), _f64(out["target_premass"]), _f64(out["totals"]),
            _ptr(out["report"]), C.byref(ms)))
        out["device_ms"] = ms.value
        return out

    def assign(self, rows, cols, return_duals=False):
        """Optimal one-to-one assignment on Euclidean costs (`pf_assign`): col_of_row (int64, n_rows) minimising
        sum_i ||rows[i] - cols[col_of_row[i]]||, n_rows <= n_cols, 1 <= d <= 16, and the call's AssignStats (total_cost,
        gap_bound, ...).  return_duals: also u (n_rows) and v (n_cols) with u_i + v_j <= C_ij, v <= 0, whose slacks on the
        assigned pairs sum to stats.gap_bound.  Non-finite coordinates raise ValueError."""
        rows, cols = _same_d(rows, cols, _EQUAL_D % "rows and cols")
        if not (np.isfinite(rows).all() and np.isfinite(cols).all()):
            raise ValueError("coordinates must be finite")
        n_r, n_c = rows.shape[0], cols.shape[0]
        col = np.empty(n_r, dtype=np.int64)
        u = np.empty(n_r) if return_duals else None
        v = np.empty(n_c) if return_duals else None
        stats = AssignStats()
        _check(self._lib.pf_assign(self._h, _f64(rows), n_r, _f64(cols), n_c, rows.shape[1], _ptr(col), _f64(u), _f64(v),
                                   C.byref(stats)))
        return (col, stats, u, v) if return_duals else (col, stats)

    def knn(self, ref, qry, k):
        """(idx (n_qry, k) int64, squared distances (n_qry, k)), ascending by (distance, index); k <= 4, d <= 4."""
        ref, qry = _same_d(ref, qry)
        idx = np.empty((qry.shape[0], int(k)), dtype=np.int64)
        d2 = np.empty((qry.shape[0], int(k)), dtype=np.float64)
        _check(self._lib.pf_knn(self._h, _f64(ref), ref.shape[0], _f64(qry), qry.shape[0], ref.shape[1], int(k),
                                _ptr(idx), _f64(d2)))
        return idx, d2

    def knn_topk(self, ref, qry, k, return_d2=True):
        """The k nearest `ref` rows of every `qry` row (`pf_knn_topk`): idx (n_qry, k) int64 and, with `return_d2`, the
        squared distances (n_qry, k), ascending by (distance, index); 1 <= k <= min(64, n_ref), 1 <= d <= 128.  The bits
        of a brute force.  A query with a NaN coordinate gets k times (0x7fffffff, inf)."""
        k = check_knn_topk(ref, qry, k)
        ref, qry = _c_f64(ref), _c_f64(qry)
        idx = np.empty((qry.shape[0], k), dtype=np.int64)
        d2 = np.empty((qry.shape[0], k), dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_knn_topk(self._h, _f64(ref), ref.shape[0], _f64(qry), qry.shape[0], ref.shape[1], k,
                                     _ptr(idx), _f64(d2)))
        return (idx, d2) if return_d2 else idx

    def knn1_graphs(self, dev_ref, dev_qry, col_ref, scale_ref, col_qry, scale_qry, return_d2=False):
        """`knn1` on coordinates built on the device from the two graphs' resident eigenvector blocks:
        ref[:, c] = final_ref[:, col_ref[c]] * scale_ref[c], qry likewise."""
        col_ref, col_qry = _c_i32(col_ref), _c_i32(col_qry)
        scale_ref, scale_qry = _c_f64(scale_ref), _c_f64(scale_qry)
        d = len(col_ref)
        if not (len(col_qry) == len(scale_ref) == len(scale_qry) == d):
            raise ValueError("col / scale arrays must share one length d")
        idx = np.empty(dev_qry.n, dtype=np.int64)
        d2 = np.empty(dev_qry.n, dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_knn1_graphs(dev_ref._h, dev_qry._h, d, _ptr(col_ref), _f64(scale_ref), _ptr(col_qry), _f64(scale_qry),
                                        _ptr(idx), _f64(d2)))
        return (idx, d2) if return_d2 else idx

    def eigsort_costs(self, dev_t, dev_s, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s):
        """eigsort's c_hist, c_hist_f, c_spatial, c_spatial_f (each k x k) and the 3-D 1-NN indices of the sampled points,
        computed on the device from the two graphs' resident eigenvector blocks (`pf_eigsort_costs`)."""
        rows_t, rows_s, col_t, col_s = _c_i64(rows_t), _c_i64(rows_s), _c_i32(col_t), _c_i32(col_s)
        sign_t, sign_s = _c_f64(sign_t), _c_f64(sign_s)
        if min(len(col_t), len(col_s), len(sign_t), len(sign_s)) < k:
            raise ValueError("eigsort_costs: k columns / signs per graph are needed")
        out = np.empty((4, int(k), int(k)), dtype=np.float64)
        idx = np.empty(len(rows_t), dtype=np.int64)
        _check(self._lib.pf_eigsort_costs(dev_t._h, dev_s._h, _ptr(rows_t), len(rows_t), _ptr(rows_s), len(rows_s), int(k),
                                          _ptr(col_t), _f64(sign_t), _ptr(col_s), _f64(sign_s), _f64(out), _ptr(idx)))
        if len(idx) and (idx.min() < 0 or idx.max() >= len(rows_s)):
            # a sample without extent along an axis normalises to NaN there; the search then answers every query with
            # 0x7fffffff and the kernel makes the spatial costs NaN instead of reading at that index
            raise ValueError(degenerate_extent_message(dev_t.point_rows(rows_t), dev_s.point_rows(rows_s)))
        return out, idx

    def knn1_blocks(self, ref_ptr, n_ref, ref_stride, qry_ptr, n_qry, qry_stride, col_ref, scale_ref, col_qry, scale_qry,
                    return_d2=False):
        """`knn1` on coordinates built from two row-major float64 blocks already in this device's memory (integer
        addresses, row strides in doubles): block[:, col[c]] * scale[c] for c < d."""
        col_ref, col_qry = _c_i32(col_ref), _c_i32(col_qry)
        scale_ref, scale_qry = _c_f64(scale_ref), _c_f64(scale_qry)
        d = len(col_ref)
        if not (len(col_qry) == len(scale_ref) == len(scale_qry) == d):
            raise ValueError("col / scale arrays must share one length d")
        idx = np.empty(int(n_qry), dtype=np.int64)
        d2 = np.empty(int(n_qry), dtype=np.float64) if return_d2 else None
        _check(self._lib.pf_knn1_blocks(self._h, C.c_void_p(int(ref_ptr)), int(n_ref), int(ref_stride), C.c_void_p(int(qry_ptr)),
                                        int(n_qry), int(qry_stride), d, _ptr(col_ref), _f64(scale_ref), _ptr(col_qry),
                                        _f64(scale_qry), _ptr(idx), _f64(d2)))
        return (idx, d2) if return_d2 else idx

    def knn_upload(self, ref, qry):
        ref, qry = _c_f64(ref), _c_f64(qry)
        _check(self._lib.pf_knn_upload(self._h, _f64(ref), ref.shape[0], _f64(qry), qry.shape[0], ref.shape[1]))
        self._knn_nq = qry.shape[0]

    def knn_run(self):
        _check(self._lib.pf_knn_run(self._h))

    def knn_download(self):
        idx = np.empty(self._knn_nq, dtype=np.int64)
        d2 = np.empty(self._knn_nq, dtype=np.float64)
        _check(self._lib.pf_knn_download(self._h, _ptr(idx), _f64(d2)))
        return idx, d2


_default_ctx = {}


def default_context(device=None):
    """Process-wide context per device (LOCAL_RANK selects the device under torchrun)."""
    if device is None:
        device = int(os.environ.get("PYFOCUSR_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = load_library().pf_device_count()
        if n > 0:
            device %= n
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class _Handle(object):
    """One object of the library that lives in a context's device memory.  A subclass names the library's function that
    frees it (`_free`) and builds it with `_create`; `close()` frees it once, and so do `with`, the collector, the
    context's own `close()` and the end of the process, whichever comes first."""

    _free = None
    _h = None  # (also of an instance whose constructor raised before the library returned a handle: nothing to free)

    def __init__(self, ctx=None):
        self.ctx = ctx if ctx is not None else default_context()
        self._lib = self.ctx._lib

    def _adopt(self, h):
        self._h = h
        _live_graphs.add(self)
        self.ctx._children.add(self)

    def _create(self, name, *args):
        """Call the library's constructor `name`(*args, &handle) and own the handle."""
        h = C.c_void_p()
        _check(getattr(self._lib, name)(*(args + (C.byref(h),))))
        self._adopt(h)

    def close(self):
        h, self._h = self._h, None
        if h:
            getattr(self._lib, self._free)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class DeviceMesh(_Handle):
    """points (n,3) f64 + faces (F,v) i32 resident in HBM (input side of the assembler)."""

    _free = "pf_mesh_free"

    def __init__(self, points, faces, ctx=None):
        _Handle.__init__(self, ctx)
        pts, f, v = _upload_arrays(points, faces)
        self._create("pf_mesh_upload", self.ctx._h, _f64(pts), pts.shape[0], _ptr(f), f.shape[0], v)
        self.n, self.n_faces = pts.shape[0], f.shape[0]


def _fan_triangles(faces):
    """(F,v) polygons -> (F*(v-2), 3) triangles (0,j+1,j+2), face-major, as the device fan-triangulates them."""
    v = faces.shape[1]
    return np.stack([faces[:, [0, j + 1, j + 2]] for j in range(v - 2)], axis=1).reshape(-1, 3)


class DeviceSurface(_Handle):
    """Triangle soup of one mesh in HBM (Morton-sorted, chunk boxes) for exact closest-point queries
    (`pf_surface_*`): the search inside the ICP pre-alignment."""

    _free = "pf_surface_free"

    def __init__(self, points, faces, ctx=None):
        _Handle.__init__(self, ctx)
        pts, f, v = _upload_arrays(points, faces, empty_ok=False)
        self._create("pf_surface_create", self.ctx._h, _f64(pts), pts.shape[0], _ptr(f), f.shape[0], v)
        self.n, self.n_faces = pts.shape[0], f.shape[0]
        self.points, self.faces = pts, f  # host arrays, for pf_surface_prepare_signed and topology()
        self._topology = None  # edge counts once the signed structure is built
        self._winding_ready = False  # the dipole data of pf_surface_prepare_winding

    def _prepare_signed(self):
        if self._topology is None:
            t = np.zeros(4, dtype=np.int64)
            _check(self._lib.pf_surface_prepare_signed(self._h, _f64(self.points), _ptr(self.faces), _ptr(t)))
            self._topology = t
        return self._topology

    def topology(self):
        """Edges of the fan triangles (built on the device with the signed structure): `n_edges`,
        `n_boundary_edges` (one triangle), `n_nonmanifold_edges` (three or more), `n_inconsistent_edges` (two
        triangles that traverse it in the same direction), `closed` (no boundary edge), and the signed `volume`
        (sum of det / 6 over the triangles, host numpy): negative when the faces point inward."""
        t = self._prepare_signed()
        tri = _fan_triangles(self.faces)
        a, b, c = self.points[tri[:, 0]], self.points[tri[:, 1]], self.points[tri[:, 2]]
        volume = float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c)))) / 6.0
        return {"n_edges": int(t[0]), "n_boundary_edges": int(t[1]), "n_nonmanifold_edges": int(t[2]),
                "n_inconsistent_edges": int(t[3]), "closed": bool(t[1] == 0), "volume": volume}

    def signed_distance(self, queries):
        """(sd (q,) f64, face (q,) i32, feature (q,) i32, n_ambiguous int) of every query (`pf_surface_signed_distance`):
        |sd| is sqrt of `distance`'s d2 bit for bit and face its face; sd > 0 on the side the face normals point to
        (outside of an outward-oriented closed mesh).  feature: 0 face, 1 edge, 2 vertex the closest point lies on (-1
        for a non-finite query, which gives NaN).  n_ambiguous: queries off the surface with a zero pseudonormal
        component (returned positive).  Builds the signed structure on first use."""
        q = _queries(queries)
        self._prepare_signed()
        sd = np.empty(len(q), dtype=np.float64)
        face = np.empty(len(q), dtype=np.int32)
        feature = np.empty(len(q), dtype=np.int32)
        amb = C.c_int64(0)
        _check(self._lib.pf_surface_signed_distance(self._h, _f64(q), len(q), _f64(sd), _ptr(face), _ptr(feature), C.byref(amb)))
        return sd, face, feature, int(amb.value)

    def winding_number(self, queries, beta=0.0):
        """(w (q,) f64, bound (q,) f64): the generalized winding number of every query (`pf_surface_winding`): 1 inside and
        0 outside an outward-oriented closed mesh, smooth across holes; NaN for a non-finite query.  `beta <= 0`: every
        triangle exactly, bound 0.  `beta > 1`: clusters of triangles at least `beta` radii away contribute their dipole
        term, and `bound` is a rigorous bound of |w - exact w|.  Two calls give identical bits.  Builds the dipole data on
        first use."""
        q = _queries(queries)
        if not self._winding_ready:
            _check(self._lib.pf_surface_prepare_winding(self._h))
            self._winding_ready = True
        w = np.empty(len(q), dtype=np.float64)
        bound = np.empty(len(q), dtype=np.float64)
        _check(self._lib.pf_surface_winding(self._h, _f64(q), len(q), float(beta), _f64(w), _f64(bound)))
        return w, bound

    def raycast(self, origins, directions, t_min=0.0, t_max=np.inf, facing=0, count=False):
        """(t (r,) f64, face (r,) i32, uv (r,2) f64[, count (r,) i32]) of every ray origin + t direction
        (`pf_surface_raycast`): the least t in [t_min, t_max] (inclusive; in units of |direction|) at which the exact
        Moeller-Trumbore test accepts a fan triangle (ties: lowest triangle index), that triangle's face and barycentric
        (u, v) (hit point a + u (b - a) + v (c - a)), and with `count` the number of accepted triangles in the interval.
        `facing`: 0 any side, 1 only faces whose normal points against the ray (det > 0), -1 only the others.  A miss gives
        +inf, -1, NaN; a ray with a non-finite component or a zero direction NaN, -1, NaN, count 0.  Equal to a brute-force
        loop over all triangles bit for bit; two calls give identical bits."""
        o, d = _rays(origins, directions)
        t = np.empty(len(o), dtype=np.float64)
        face = np.empty(len(o), dtype=np.int32)
        uv = np.empty((len(o), 2), dtype=np.float64)
        n_hit = np.empty(len(o), dtype=np.int32) if count else None
        _check(self._lib.pf_surface_raycast(self._h, _f64(o), _f64(d), len(o), float(t_min), float(t_max), int(facing), _f64(t),
                                            _ptr(face), _f64(uv), _ptr(n_hit)))
        return (t, face, uv, n_hit) if count else (t, face, uv)

    def vertex_normals(self):
        """(n, 3) f64: the angle-weighted vertex pseudonormals as the device stores them (`pf_surface_vertex_normals`), not
        normalised; zero for a vertex no face references.  Builds the signed structure on first use."""
        self._prepare_signed()
        out = np.empty((self.n, 3), dtype=np.float64)
        _check(self._lib.pf_surface_vertex_normals(self._h, _f64(out)))
        return out

    def closest(self, queries):
        """(points (q,3) f64, face (q,) i32, squared distance (q,) f64) of the closest surface point of each query."""
        q = _c_f64(queries).reshape(-1, 3)
        pts = np.empty_like(q)
        face = np.empty(len(q), dtype=np.int32)
        d2 = np.empty(len(q), dtype=np.float64)
        _check(self._lib.pf_surface_closest(self._h, _f64(q), len(q), _f64(pts), _ptr(face), _f64(d2)))
        return pts, face, d2

    def distance(self, queries, per_point=True):
        """(squared distance (q,) f64, face (q,) i32, stats dict) of every query to the surface (`pf_surface_distance`:
        many queries, no closest points).  A query with a non-finite coordinate gives NaN and face -1.  stats:
        n_finite, n_nan, sum_d, sum_d2, max_d, argmax (-1 if none) over d = sqrt(d2).  per_point=False downloads the
        stats only and returns (None, None, stats)."""
        q = _queries(queries)
        d2 = np.empty(len(q), dtype=np.float64) if per_point else None
        face = np.empty(len(q), dtype=np.int32) if per_point else None
        st = np.empty(6, dtype=np.float64)
        _check(self._lib.pf_surface_distance(self._h, _f64(q), len(q), _f64(d2), _ptr(face), _f64(st)))
        stats = {"n_finite": int(st[0]), "n_nan": int(st[1]), "sum_d": float(st[2]), "sum_d2": float(st[3]),
                 "max_d": float(st[4]), "argmax": int(st[5])}
        return d2, face, stats


class DeviceSurfaceND(_Handle):
    """Triangulated surface embedded in d dimensions (1 <= d <= 16) in HBM, for exact closest-point queries that return
    the face, its corners and barycentric weights (`pf_surface_nd_*`): sub-vertex correspondences in spectral
    coordinates.  `close()` frees it; usable as a context manager."""

    MAX_DIM = 16
    _free = "pf_surface_nd_free"

    def __init__(self, coords, faces, ctx=None):
        x = _c_f64(coords)
        f = _c_i32(faces)
        if x.ndim != 2 or x.shape[0] == 0 or not 1 <= x.shape[1] <= self.MAX_DIM:
            raise ValueError("coords must be a non-empty (n, d) array with 1 <= d <= %d" % self.MAX_DIM)
        if f.ndim != 2 or f.shape[0] == 0 or f.shape[1] < 3:
            raise ValueError("faces must be a non-empty (F, verts_per_face >= 3) array")
        _Handle.__init__(self, ctx)
        self._create("pf_surface_nd_create", self.ctx._h, _f64(x), x.shape[0], x.shape[1], _ptr(f), f.shape[0], f.shape[1])
        self.n, self.d, self.n_faces = x.shape[0], x.shape[1], f.shape[0]

    def closest(self, queries, exhaustive=False):
        """(face (q,) i32, vertices (q,3) i32, bary (q,3) f64, d2 (q,) f64) of the closest surface point of every query
        (`pf_surface_nd_closest`): the face of the winning fan triangle, that triangle's corners, the weights of the
        closest point on them, the squared distance.  A query with a non-finite coordinate (or a surface without a
        triangle of finite distance) gives -1, (-1,-1,-1), NaN, NaN.  Equal to a brute-force loop over all triangles bit
        for bit; `exhaustive` runs that loop on the device."""
        q = _c_f64(queries)
        if q.ndim != 2 or q.shape[0] == 0 or q.shape[1] != self.d:
            raise ValueError("queries must be a non-empty (n, %d) array" % self.d)
        face = np.empty(len(q), dtype=np.int32)
        verts = np.empty((len(q), 3), dtype=np.int32)
        bary = np.empty((len(q), 3), dtype=np.float64)
        d2 = np.empty(len(q), dtype=np.float64)
        _check(self._lib.pf_surface_nd_closest(self._h, _f64(q), len(q), _ptr(face), _ptr(verts),
                                               _f64(bary), _f64(d2), 1 if exhaustive else 0))
        return face, verts, bary, d2

    def last_search(self):
        """{chunks_opened, packets, n_chunks} of the last `closest`: chunks of 64 triangles staged, summed over the
        packets of 8 neighbouring queries; the packets; the chunks the surface has."""
        v = [C.c_int64(0) for _ in range(3)]
        _check(self._lib.pf_surface_nd_last_search(self._h, *[C.byref(x) for x in v]))
        return {"chunks_opened": int(v[0].value), "packets": int(v[1].value), "n_chunks": int(v[2].value)}


class DeviceFunctionalMap(_Handle):
    """Two Laplace-Beltrami bases, the source's vertex areas and a point map T (T[i] in [0, n_t) for every source vertex)
    in HBM for functional-map iterations (`pf_fmap_*`): `project` (point map -> C), `convert` (C -> point map),
    `zoomout`.  `close()` frees it; usable as a context manager."""

    MAX_K = 128
    _free = "pf_fmap_free"

    def __init__(self, phi_t, phi_s, mass_s, ctx=None):
        pt, ps, m = _c_f64(phi_t), _c_f64(phi_s), _c_f64(mass_s)
        if pt.ndim != 2 or ps.ndim != 2 or pt.shape[1] != ps.shape[1] or pt.shape[0] == 0 or ps.shape[0] == 0:
            raise ValueError("phi_t and phi_s must be non-empty (n, K) arrays with equal K")
        if not 1 <= pt.shape[1] <= self.MAX_K:
            raise ValueError("1 <= K <= %d basis functions, got %d" % (self.MAX_K, pt.shape[1]))
        if m.shape != (ps.shape[0],):
            raise ValueError("mass_s must have one entry per source vertex")
        _Handle.__init__(self, ctx)
        self._create("pf_fmap_create", self.ctx._h, _f64(pt), pt.shape[0], _f64(ps), ps.shape[0], _f64(m), pt.shape[1])
        self.n_t, self.n_s, self.K = pt.shape[0], ps.shape[0], pt.shape[1]

    def set_p2p(self, T):
        T = _c_i64(T)
        if T.shape != (self.n_s,):
            raise ValueError("T must have one target index per source vertex")
        _check(self._lib.pf_fmap_set_p2p(self._h, _ptr(T)))

    def get_p2p(self, return_d2=False):
        T = np.empty(self.n_s, dtype=np.int64)
        d2 = np.empty(self.n_s) if return_d2 else None
        _check(self._lib.pf_fmap_get_p2p(self._h, _ptr(T), _f64(d2)))
        return (T, d2) if return_d2 else T

    def project(self, k_s, k_t):
        Cm = np.empty((int(k_s), int(k_t)))
        _check(self._lib.pf_fmap_project(self._h, int(k_s), int(k_t), _f64(Cm)))
        return Cm

    def convert(self, k_s, k_t, Cm=None):
        """The resident functional map (Cm None) or the given k_s x k_t one -> the point map, which stays on the device."""
        if Cm is not None:
            Cm = _c_f64(Cm, (int(k_s), int(k_t)))
        _check(self._lib.pf_fmap_convert(self._h, _f64(Cm), int(k_s), int(k_t)))

    def zoomout(self, k_start, k_end, step=1, n_iter_at_end=0):
        Cm = np.empty((int(k_end), int(k_end)))
        _check(self._lib.pf_fmap_zoomout(self._h, int(k_start), int(k_end), int(step), int(n_iter_at_end), _f64(Cm)))
        return Cm

    def set_samples(self, S_t, S_s):
        """Rows of the target's and of the source's basis that `zoomout_sampled` works on (`pf_fmap_set_samples`)."""
        S_t, S_s = _c_i64(S_t), _c_i64(S_s)
        if S_t.ndim != 1 or S_s.ndim != 1:
            raise ValueError("S_t and S_s must be vectors of indices")
        _check(self._lib.pf_fmap_set_samples(self._h, _ptr(S_t), S_t.shape[0], _ptr(S_s), S_s.shape[0]))

    def zoomout_sampled(self, k_start, k_end, step=1, n_iter_at_end=0):
        """ZoomOut on the samples, least-squares fits, one conversion at full resolution at the end
        (`pf_fmap_zoomout_sampled`); returns the last fit, k_end x k_end."""
        if not 1 <= int(k_end) <= self.K:
            raise ValueError("k_end must lie in 1 .. K = %d" % self.K)
        Cm = np.empty((int(k_end), int(k_end)))
        _check(self._lib.pf_fmap_zoomout_sampled(self._h, int(k_start), int(k_end), int(step), int(n_iter_at_end), _f64(Cm)))
        return Cm


class DeviceCpd(_Handle):
    """Fixed set X (N,d) and moving set Y (M,d) resident in HBM for the E-steps of a CPD registration."""

    _free = "pf_cpd_free"

    def __init__(self, X, Y, ctx=None):
        _Handle.__init__(self, ctx)
        X, Y = _same_d(X, Y, "X (N,d) and Y (M,d) must share d")
        self.N, self.M, self.D = X.shape[0], Y.shape[0], X.shape[1]
        self._create("pf_cpd_create", self.ctx._h, _f64(X), self.N, _f64(Y), self.M, self.D)
        self._P1, self._Pt1, self._PX = np.empty(self.M), np.empty(self.N), np.empty((self.M, self.D))
        self._H = np.empty((0, 0))  # until set_basis: the library refuses the basis calls (PfError), not Python

    def estep(self, TY, sigma2, w=0.0):
        """(P1 (M,), Pt1 (N,), PX (M,d)) for the moving set at TY; the arrays are reused by the next call."""
        TY = _c_f64(TY)
        if TY.shape != (self.M, self.D):
            raise ValueError("TY must be (%d, %d)" % (self.M, self.D))
        _check(self._lib.pf_cpd_estep(self._h, _f64(TY), float(sigma2), float(w), _f64(self._P1), _f64(self._Pt1),
                                      _f64(self._PX)))
        return self._P1, self._Pt1, self._PX

    # ---- device-resident iterations: the posterior sums stay in HBM, small moments out, parameters in
    def estep_resident(self, sigma2, w=0.0):
        _check(self._lib.pf_cpd_estep(self._h, None, float(sigma2), float(w), None, None, None))

    def affine_sums(self):
        """dict of the moment sums of `pf_cpd_affine_sums` (about the centres cx, cy)."""
        D = self.D
        shifts, sums = np.empty(32), np.empty(2 * D * D + 3 * D + 3)
        _check(self._lib.pf_cpd_affine_sums(self._h, _f64(shifts), _f64(sums)))
        o = 1 + 2 * D + 2 * D * D
        return dict(cx=shifts[:D], cy=shifts[16:16 + D], Np=sums[0], sPX=sums[1:1 + D], sP1Y=sums[1 + D:1 + 2 * D],
                    PXY=sums[1 + 2 * D:1 + 2 * D + D * D].reshape(D, D), YPY=sums[1 + 2 * D + D * D:o].reshape(D, D),
                    sPt1=sums[o], sPt1XX=sums[o + 1], sPt1X=sums[o + 2:o + 2 + D])

    def apply_affine(self, B, t):
        B, t = _c_f64(B), _c_f64(t)
        _check(self._lib.pf_cpd_apply_affine(self._h, _f64(B), _f64(t)))

    def deform_sums(self):
        """(H (K,K) = Q^T diag(P1) Q, R (K,d) = Q^T (PX - diag(P1) Y))."""
        K = self._H.shape[0]
        R = np.empty((K, self.D))
        _check(self._lib.pf_cpd_deform_sums(self._h, _f64(self._H), _f64(R)))
        return self._H, R

    def apply_deform(self, Cmat):
        """TY = Y + Q C; returns (Np, yPy, trPXY, sum Pt1, xPx) with the new TY."""
        Cmat = _c_f64(Cmat)
        sums = np.empty(5)
        _check(self._lib.pf_cpd_apply_deform(self._h, _f64(Cmat), _f64(sums)))
        return sums

    def download(self):
        """(TY, P1, Pt1, PX) as they stand on the device."""
        TY = np.empty((self.M, self.D))
        _check(self._lib.pf_cpd_download(self._h, _f64(TY), _f64(self._P1), _f64(self._Pt1), _f64(self._PX)))
        return TY, self._P1, self._Pt1, self._PX

    def set_basis(self, Q):
        """Keep the low-rank basis Q (M,K) on the device for `weighted_gram`."""
        Q = _c_f64(Q)
        if Q.ndim != 2 or Q.shape[0] != self.M:
            raise ValueError("Q must be (%d, K)" % self.M)
        _check(self._lib.pf_cpd_set_basis(self._h, _f64(Q), Q.shape[1]))
        self._H = np.empty((Q.shape[1], Q.shape[1]))

    def weighted_gram(self):
        """Q^T diag(P1) Q with the P1 of the last E-step."""
        _check(self._lib.pf_cpd_weighted_gram(self._h, _f64(self._H)))
        return self._H


SHAPES_MAX_S = 1024  # the limits of pf_shapes_create and pf_shapes_scores
SHAPES_MAX_K = 1024


def check_population(shapes, weights=None):
    """The argument checks of `DeviceShapes`, which need no library: ValueError / TypeError, or (shapes (S, n, 3) f64
    C-contiguous, weights (n,) f64 or None).  A list of (n, 3) arrays is stacked; an array must already be float64."""
    if isinstance(shapes, (list, tuple)):
        parts = [np.asarray(p) for p in shapes]
        if len(parts) == 0:
            raise ValueError("a population needs at least one shape")
        if any(p.ndim != 2 or p.shape[1] != 3 for p in parts):
            raise ValueError("every shape must be an (n, 3) array")
        if any(p.shape != parts[0].shape for p in parts):
            raise ValueError("the shapes of a population must have the same number of points (they are in correspondence)")
        shapes = np.stack(parts)
    shapes = np.asarray(shapes)
    if shapes.dtype != np.float64:
        raise TypeError("shapes must be float64, not %s" % shapes.dtype)
    if shapes.ndim != 3 or shapes.shape[2] != 3:
        raise ValueError("shapes must be an (S, n, 3) array")
    if not 1 <= shapes.shape[0] <= SHAPES_MAX_S:
        raise ValueError("S = %d shapes out of range (1 .. %d)" % (shapes.shape[0], SHAPES_MAX_S))
    if shapes.shape[1] == 0:
        raise ValueError("the shapes have no points")
    if not shapes.flags.c_contiguous:
        raise ValueError("shapes must be C-contiguous, not a strided view")
    if not np.isfinite(shapes).all():
        raise ValueError("shape coordinates must be finite")
    if weights is not None:
        weights = np.asarray(weights)
        if weights.dtype != np.float64:
            raise TypeError("weights must be float64, not %s" % weights.dtype)
        if weights.shape != (shapes.shape[1],):
            raise ValueError("weights must have one entry per point")
        if not np.isfinite(weights).all() or (weights < 0.0).any():
            raise ValueError("weights must be finite and not negative")
        weights = np.ascontiguousarray(weights)
    return shapes, weights


class DeviceShapes(_Handle):
    """A population of S shapes in correspondence (S, n, 3), optional per-point weights and a reference shape in HBM for
    Procrustes alignment and principal modes (`pf_shapes_*`; the definitions are in include/pyfocusr_hip.h)."""

    _free = "pf_shapes_free"

    def __init__(self, shapes, weights=None, ctx=None):
        X, w = check_population(shapes, weights)
        _Handle.__init__(self, ctx)
        self.S, self.n = X.shape[0], X.shape[1]
        self._create("pf_shapes_create", self.ctx._h, _f64(X), self.S, self.n, _f64(w))
        W = np.empty(1)
        _check(self._lib.pf_shapes_weight_sum(self._h, _f64(W)))
        self.weight_sum = float(W[0])

    def center(self):
        """Centres every shape on its weighted centroid; returns the centroids (S, 3)."""
        c = np.empty((self.S, 3))
        _check(self._lib.pf_shapes_center(self._h, _f64(c)))
        return c

    def mean(self, first=0, count=None, return_mean=True):
        """(mean (n, 3) or None, change): the mean of the shapes first .. first + count - 1 becomes the reference."""
        count = self.S - int(first) if count is None else int(count)
        m = np.empty((self.n, 3)) if return_mean else None
        change = np.empty(1)
        _check(self._lib.pf_shapes_mean(self._h, int(first), count, _f64(m), _f64(change)))
        return m, float(change[0])

    def align_sums(self):
        """(H (S, 3, 3), q (S,), rho2) of `pf_shapes_align_sums`."""
        H, q, rho2 = np.empty((self.S, 3, 3)), np.empty(self.S), np.empty(1)
        _check(self._lib.pf_shapes_align_sums(self._h, _f64(H), _f64(q), _f64(rho2)))
        return H, q, float(rho2[0])

    def transform(self, R, scale=None, t=None):
        R = _c_f64(R, (self.S, 3, 3))
        scale = np.ones(self.S) if scale is None else _c_f64(scale, (self.S,))
        t = None if t is None else _c_f64(t, (self.S, 3))
        _check(self._lib.pf_shapes_transform(self._h, _f64(R), _f64(scale), _f64(t)))

    def gram(self):
        G = np.empty((self.S, self.S))
        _check(self._lib.pf_shapes_gram(self._h, _f64(G)))
        return G

    def combine(self, coeff):
        """(K, n, 3): row k is the sum over the shapes of coeff[k][s] (x_s - reference)."""
        coeff = _c_f64(coeff)
        if coeff.ndim != 2 or coeff.shape[1] != self.S or not 1 <= coeff.shape[0] <= self.S:
            raise ValueError("coeff must be (K, S = %d) with 1 <= K <= S" % self.S)
        out = np.empty((coeff.shape[0], self.n, 3))
        _check(self._lib.pf_shapes_combine(self._h, _f64(coeff), coeff.shape[0], _f64(out)))
        return out

    def scores(self, modes):
        """(S, K): the weighted inner products of every shape's offset from the reference with the modes (K, n, 3)."""
        modes = _c_f64(modes)
        if modes.ndim != 3 or modes.shape[1:] != (self.n, 3) or not 1 <= modes.shape[0] <= SHAPES_MAX_K:
            raise ValueError("modes must be (K, %d, 3) with 1 <= K <= %d" % (self.n, SHAPES_MAX_K))
        b = np.empty((self.S, modes.shape[0]))
        _check(self._lib.pf_shapes_scores(self._h, _f64(modes), modes.shape[0], _f64(b)))
        return b

    def set_reference(self, ref):
        ref = _c_f64(ref, (self.n, 3))
        _check(self._lib.pf_shapes_set_reference(self._h, _f64(ref)))

    def download(self):
        X = np.empty((self.S, self.n, 3))
        _check(self._lib.pf_shapes_download(self._h, _f64(X)))
        return X

    def device_ms(self, enable=True):
        """The device time of the last timed primitive in ms; switches the timing on or off for the next ones."""
        ms = np.zeros(1)
        _check(self._lib.pf_shapes_device_ms(self._h, int(bool(enable)), _f64(ms)))
        return float(ms[0])


def check_volume(values, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The argument checks of `DeviceIsosurface`, which need no library: ValueError, or (values (nx, ny, nz) f64
    C-contiguous, level, spacing (3,) f64, origin (3,) f64).  Any real dtype is cast to float64 here."""
    values = np.asarray(values)
    if values.ndim != 3:
        raise ValueError("a volume must be an (nx, ny, nz) array, not one of %d dimensions" % values.ndim)
    if min(values.shape) < 2:
        raise ValueError("every extent of a volume must be at least 2, not %r" % (values.shape,))
    if values.size >= 2 ** 31:
        raise ValueError("a volume must have fewer than 2^31 samples, not %d" % values.size)
    if values.dtype.kind not in "fiub":
        raise TypeError("a volume must hold real numbers, not %s" % values.dtype)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if not np.isfinite(values).all():
        raise ValueError("the values of a volume must be finite")
    level = float(level)
    spacing, origin = _c_f64(spacing).reshape(-1), _c_f64(origin).reshape(-1)
    if spacing.shape != (3,) or origin.shape != (3,):
        raise ValueError("spacing and origin must have three entries each")
    if not (np.isfinite(level) and np.isfinite(spacing).all() and np.isfinite(origin).all()):
        raise ValueError("level, spacing and origin must be finite")
    return values, level, spacing, origin


class DeviceIsosurface(_Handle):
    """The isosurface of a sampled scalar field, extracted on the device and held there until fetched
    (`pf_isosurface_*`; the definition is in include/pyfocusr_hip.h).  `report` (8,) int64 = vertices | faces | cells with a
    face | lattice points | cells | 0 | 0 | 0."""

    _free = "pf_isosurface_free"

    def __init__(self, values, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), ctx=None, _source=None):
        self.report = np.zeros(8, dtype=np.int64)
        h, ms = C.c_void_p(), C.c_double(0.0)
        if _source is not None:  # (DeviceDistanceTransform, level, origin): the field that handle holds (pf_edt_isosurface)
            edt, level, origin = _source
            _Handle.__init__(self, edt.ctx)
            _check(self._lib.pf_edt_isosurface(edt._h, level, _f64(origin), C.byref(h), _ptr(self.report), C.byref(ms)))
        else:
            v, level, spacing, origin = check_volume(values, level, spacing, origin)
            _Handle.__init__(self, ctx)
            _check(self._lib.pf_isosurface_create(self.ctx._h, _f64(v), v.shape[0], v.shape[1], v.shape[2], level, _f64(spacing),
                                                  _f64(origin), 0, C.byref(h), _ptr(self.report), C.byref(ms)))
        self._adopt(h)
        self.n_vertices, self.n_faces, self.device_ms = int(self.report[0]), int(self.report[1]), ms.value

    def fetch(self):
        """(points (V, 3) f64, faces (F, 3) int32, vertex_key (V,) int64, face_cell (F,) int32)."""
        pts, faces = np.empty((self.n_vertices, 3)), np.empty((self.n_faces, 3), dtype=np.int32)
        key, cell = np.empty(self.n_vertices, dtype=np.int64), np.empty(self.n_faces, dtype=np.int32)
        _check(self._lib.pf_isosurface_fetch(self._h, _f64(pts), _ptr(faces), _ptr(key), _ptr(cell)))
        return pts, faces, key, cell


PF_EDT_UNSIGNED, PF_EDT_SIGNED = 0, 1
_TINY = np.finfo(np.float64).tiny


def check_mask(mask, spacing=(1.0, 1.0, 1.0)):
    """The argument checks of `DeviceDistanceTransform`, which need no library: ValueError or TypeError, or (mask
    (nx, ny, nz) bool C-contiguous, True where the argument is not 0, spacing (3,) f64; one number is all three).  A
    contiguous boolean mask comes back as it is, so checking twice costs nothing."""
    mask = np.asarray(mask)
    if mask.ndim != 3:
        raise ValueError("a mask must be an (nx, ny, nz) array, not one of %d dimensions" % mask.ndim)
    if min(mask.shape) < 1:
        raise ValueError("every extent of a mask must be at least 1, not %r" % (mask.shape,))
    if mask.size >= 2 ** 31:
        raise ValueError("a mask must have fewer than 2^31 samples, not %d" % mask.size)
    if mask.dtype.kind not in "biu":
        raise TypeError("a mask must be boolean or a label map of integers, not %s" % mask.dtype)
    mask = np.ascontiguousarray(mask if mask.dtype == np.bool_ else mask != 0)
    spacing = np.asarray(spacing, dtype=np.float64)
    spacing = np.repeat(spacing, 3) if spacing.ndim == 0 else _c_f64(spacing).reshape(-1)
    if spacing.shape != (3,):
        raise ValueError("spacing must be one number or three")
    if not (np.isfinite(spacing).all() and (spacing > 0.0).all()):
        raise ValueError("spacing must be positive and finite")
    with np.errstate(over="ignore", under="ignore"):
        diagonal2 = float(np.sum((spacing * np.maximum(np.array(mask.shape) - 1, 1)) ** 2))
        if (spacing * spacing < _TINY).any() or not np.isfinite(diagonal2):
            raise ValueError("spacing %r: the squared distances leave the range of normal doubles" % (spacing.tolist(),))
    return mask, spacing


class DeviceDistanceTransform(_Handle):
    """The exact Euclidean distance transform of a mask and its feature transform, computed on the device and held there
    until fetched (`pf_edt_*`; the definition is in include/pyfocusr_hip.h).  `report` (8,) int64 = samples | foreground |
    background | 0 ..."""

    _free = "pf_edt_free"

    def __init__(self, mask, spacing=(1.0, 1.0, 1.0), signed=False, ctx=None):
        m, spacing = check_mask(mask, spacing)
        _Handle.__init__(self, ctx)
        self.shape, self.spacing, self.signed = m.shape, spacing, bool(signed)
        self.report = np.zeros(8, dtype=np.int64)
        h, ms = C.c_void_p(), C.c_double(0.0)
        _check(self._lib.pf_edt_create(self.ctx._h, _ptr(m.view(np.uint8)), m.shape[0], m.shape[1], m.shape[2], _f64(spacing),
                                       PF_EDT_SIGNED if signed else PF_EDT_UNSIGNED, 0, C.byref(h), _ptr(self.report), C.byref(ms)))
        self._adopt(h)
        self.n_foreground, self.n_background, self.device_ms = int(self.report[1]), int(self.report[2]), ms.value

    def fetch(self, dist=True, dist2=True, nearest=True):
        """(dist (nx, ny, nz) f64, dist2 (nx, ny, nz) f64, nearest (nx, ny, nz) int32), None for what was not asked for."""
        d = np.empty(self.shape) if dist else None
        d2 = np.empty(self.shape) if dist2 else None
        near = np.empty(self.shape, dtype=np.int32) if nearest else None
        _check(self._lib.pf_edt_fetch(self._h, _f64(d), _f64(d2), _ptr(near)))
        return d, d2, near

    def isosurface(self, level=0.0, origin=(0.0, 0.0, 0.0)):
        """The `DeviceIsosurface` of the resident field at `level` (`pf_edt_isosurface`: no download, no upload)."""
        origin = _c_f64(origin).reshape(-1)
        if origin.shape != (3,) or not (np.isfinite(origin).all() and np.isfinite(float(level))):
            raise ValueError("level and origin (three entries) must be finite")
        return DeviceIsosurface(None, _source=(self, float(level), origin))


PF_CCL_BINARY, PF_CCL_BY_VALUE, PF_CCL_BACKGROUND = 0, 1, 2
CCL_TABLES = ("count", "value", "root", "lo", "hi", "border", "sum")  # the statistics of pf_ccl_fetch, in its order


def check_label_volume(vol, connectivity=6):
    """The argument checks of `DeviceComponents`, which need no library: ValueError or TypeError, or (vol (nx, ny, nz)
    int32 C-contiguous, connectivity).  The rules of shape, size and dtype are `check_mask`'s (`check_volume` is the
    isosurface's check of a float field): bool and integers are taken, floats refused.  Integers wider than 32 bits keep
    which voxels are 0 and which are equal only if they fit int32, which is checked."""
    vol = np.asarray(vol)
    if vol.ndim != 3:
        raise ValueError("a volume must be an (nx, ny, nz) array, not one of %d dimensions" % vol.ndim)
    if min(vol.shape) < 1:
        raise ValueError("every extent of a volume must be at least 1, not %r" % (vol.shape,))
    if vol.size >= 2 ** 31:
        raise ValueError("a volume must have fewer than 2^31 samples, not %d" % vol.size)
    if vol.dtype.kind not in "biu":
        raise TypeError("a volume must be boolean or a label map of integers, not %s" % vol.dtype)
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity must be 6, 18 or 26, not %r" % (connectivity,))
    if vol.dtype != np.int32:
        if vol.dtype.itemsize >= 4 and vol.dtype.kind in "iu" and (vol.max() > 2 ** 31 - 1 or vol.min() < -2 ** 31):
            raise ValueError("the values of a label map must fit int32")
        vol = vol.astype(np.int32)
    return np.ascontiguousarray(vol), int(connectivity)


class DeviceComponents(_Handle):
    """The connected components of a mask or label map, labelled on the device and held there with their statistics until
    fetched (`pf_ccl_*`; the definition is in include/pyfocusr_hip.h).  `n` components; `report` (8,) int64 = samples |
    labelled voxels | components | retries of the unions | largest count | 0 ..."""

    _free = "pf_ccl_free"

    def __init__(self, vol, connectivity=6, mode=PF_CCL_BINARY, ctx=None):
        v, connectivity = check_label_volume(vol, connectivity)
        if mode not in (PF_CCL_BINARY, PF_CCL_BY_VALUE, PF_CCL_BACKGROUND):
            raise ValueError("mode must be PF_CCL_BINARY, PF_CCL_BY_VALUE or PF_CCL_BACKGROUND, not %r" % (mode,))
        _Handle.__init__(self, ctx)
        self.shape, self.connectivity, self.mode = v.shape, connectivity, int(mode)
        self.report = np.zeros(8, dtype=np.int64)
        h, ms = C.c_void_p(), C.c_double(0.0)
        _check(self._lib.pf_ccl_create(self.ctx._h, _ptr(v), v.shape[0], v.shape[1], v.shape[2], connectivity, int(mode), 0,
                                       C.byref(h), _ptr(self.report), C.byref(ms)))
        self._adopt(h)
        n = C.c_int64(0)
        _check(self._lib.pf_ccl_info(self._h, C.byref(n)))
        self.n, self.device_ms = int(n.value), ms.value

    def fetch(self, component=True, stats=True):
        """(component (nx, ny, nz) int32 or None, a dict of the tables `CCL_TABLES` or None): count (C,) int64, value and
        root (C,) int32, lo and hi (C, 3) int32, border (C,) uint8, sum (C, 3) int64."""
        n = self.n
        comp = np.empty(self.shape, dtype=np.int32) if component else None
        t = None
        if stats:
            t = {"count": np.empty(n, dtype=np.int64), "value": np.empty(n, dtype=np.int32), "root": np.empty(n, dtype=np.int32),
                 "lo": np.empty((n, 3), dtype=np.int32), "hi": np.empty((n, 3), dtype=np.int32),
                 "border": np.empty(n, dtype=np.uint8), "sum": np.empty((n, 3), dtype=np.int64)}
        _check(self._lib.pf_ccl_fetch(self._h, _ptr(comp), *[_ptr(t[k]) if t else None for k in CCL_TABLES]))
        return comp, t

    def select(self, keep):
        """(nx, ny, nz) bool: the voxels of the components c (0-based) with keep[c] (`pf_ccl_select`)."""
        keep = np.ascontiguousarray(np.asarray(keep) != 0).reshape(-1)
        if keep.shape != (self.n,):
            raise ValueError("keep must have one entry per component (%d), not %r" % (self.n, keep.shape))
        out = np.empty(self.shape, dtype=np.uint8)
        _check(self._lib.pf_ccl_select(self._h, _ptr(keep.view(np.uint8)) if self.n else None, _ptr(out)))
        return out.view(np.bool_)


SMOOTH_WEIGHTS = {"uniform": 0, "cotangent": 1}  # PF_SMOOTH_UNIFORM, PF_SMOOTH_COTANGENT
SMOOTH_BOUNDARY = {"free": 0, "fixed": 1, "curve": 2}  # PF_SMOOTH_FREE, PF_SMOOTH_FIXED, PF_SMOOTH_CURVE
SMOOTH_MAX_COLUMNS = 32  # the limit of pf_smoother_run
SMOOTH_COUNTS = ("edges", "boundary_edges", "non_manifold_edges", "entries", "largest_row", "movable_vertices")


class DeviceSmoother(_Handle):
    """The adjacency of a triangle mesh in HBM (CSR, weights, vertex kinds) with its points, for explicit smoothing sweeps
    (`pf_smoother_*`; the definitions are in include/pyfocusr_hip.h).  The arguments are the library's own: points (n, 3)
    f64, faces (m, 3) i32, the codes of SMOOTH_WEIGHTS and SMOOTH_BOUNDARY, pinned (n,) uint8 or None
    (`pyfocusr_amd.smoothing` checks and converts what a user passes)."""

    _free = "pf_smoother_free"

    def __init__(self, points, faces, weights=0, boundary=1, pinned=None, ctx=None):
        _Handle.__init__(self, ctx)
        self.n, self.n_faces = points.shape[0], faces.shape[0]
        self._create("pf_smoother_create", self.ctx._h, _f64(points), self.n, _ptr(faces), self.n_faces, int(weights), int(boundary),
                     _ptr(pinned))
        self.counts = np.zeros(len(SMOOTH_COUNTS), dtype=np.int64)
        _check(self._lib.pf_smoother_info(self._h, _ptr(self.counts)))

    def adjacency(self):
        """(rowptr (n + 1,) i32, col (entries,) i32, w (entries,) f64, kind (n,) u8: 1 boundary | 2 pinned | 4 movable)."""
        nnz = int(self.counts[3])
        rowptr, col = np.empty(self.n + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        w, kind = np.empty(nnz), np.empty(self.n, dtype=np.uint8)
        _check(self._lib.pf_smoother_adjacency(self._h, _ptr(rowptr), _ptr(col), _f64(w), _ptr(kind)))
        return rowptr, col, w, kind

    def run(self, values, factors, clamp_every=1, clamp=None, stats=False):
        """(out, stats (6,) or None, device_ms) of `pf_smoother_run`: values (n, c) f64 or None (the mesh's own points),
        factors (s,) f64, clamp (c,) f64 or None."""
        ncols = 3 if values is None else values.shape[1]
        out = np.empty((self.n, ncols))
        st = np.zeros(6) if stats else None
        ms = C.c_double(0.0)
        _check(self._lib.pf_smoother_run(self._h, _f64(values), ncols, _f64(factors), len(factors), int(clamp_every), _f64(clamp),
                                         _f64(out), _f64(st), C.byref(ms)))
        return out, st, ms.value


def gaussian_gram_product(A, B, beta, V, ctx=None):
    """G(A,B) @ V with G_ij = exp(-|a_i - b_j|^2 / (2 beta^2)), evaluated on the device without forming G."""
    ctx = ctx if ctx is not None else default_context()
    A, B, V = _c_f64(A), _c_f64(B), _c_f64(V)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or V.ndim != 2 or V.shape[0] != B.shape[0]:
        raise ValueError("shapes: A (a,d), B (b,d), V (b,c)")
    out = np.empty((A.shape[0], V.shape[1]))
    _check(ctx._lib.pf_cpd_gram(ctx._h, _f64(A), A.shape[0], _f64(B), B.shape[0], A.shape[1], float(beta), _f64(V),
                                V.shape[1], _f64(out)))
    return out


class _Rows(_Handle):
    """A fixed subset of a graph's rows on the device (`pf_rows_*`)."""

    _free = "pf_rows_free"

    def __init__(self, graph, idx):
        _Handle.__init__(self, graph.ctx)
        idx = _c_i64(idx)
        self._create("pf_rows_create", graph._h, _ptr(idx), len(idx))
        self.n = len(idx)


class DeviceLaplacian(_Handle):
    """Device-resident graph of one mesh: CSR(W), deg, SELL-64 operators, workspace.
    Also the `ops` object the Krylov driver (`_krylov.filtered_eigs`) drives."""

    _free = "pf_graph_free"
    _rows = ()
    cotangent = False  # True: built by pf_graph_build_cotan - the operator is S = M^-1/2 (D - W) M^-1/2 of the cotangent weights

    def __init__(self, points=None, faces=None, ctx=None, device_mesh=None, matrix=None, _handle=None, cotangent=False):
        if cotangent:
            if matrix is not None or _handle is not None:
                raise ValueError("cotangent=True needs a mesh (points and faces, or device_mesh)")
            mesh = device_mesh if device_mesh is not None else DeviceMesh(points, faces, ctx=ctx)
            _Handle.__init__(self, mesh.ctx)
            try:
                self._create("pf_graph_build_cotan", mesh._h, 0)
            finally:
                if device_mesh is None:
                    mesh.close()
        elif _handle is not None:  # (ctx, pf_graph*) of a graph the library has already built (build_pair)
            _Handle.__init__(self, _handle[0])
            self._adopt(_handle[1])
        elif matrix is not None:  # (rowptr, colidx, values) of a general CSR matrix, canonical format
            _Handle.__init__(self, ctx)
            rp, ci, va = _c_i32(matrix[0]), _c_i32(matrix[1]), _c_f64(matrix[2])
            self._create("pf_graph_from_matrix", self.ctx._h, len(rp) - 1, _ptr(rp), _ptr(ci), _f64(va))
        elif device_mesh is not None:
            _Handle.__init__(self, device_mesh.ctx)
            self._create("pf_graph_build_device", device_mesh._h)
        else:
            _Handle.__init__(self, ctx)
            pts, f, v = _upload_arrays(points, faces)
            self._create("pf_graph_build", self.ctx._h, _f64(pts), pts.shape[0], _ptr(f), f.shape[0], v)
        h = self._h
        info = GraphInfo()
        _check(self._lib.pf_graph_get_info(h, C.byref(info)))
        self.info = info
        fields = info.as_dict()
        for name in ("n", "nnz_w", "nnz_l", "n_isolated", "n_components", "max_degree", "n_oneway"):
            setattr(self, name, fields[name])
        self.symmetric = bool(info.is_symmetric)
        self.rows_compacted = bool(self._lib.pf_graph_rows_compacted(h))  # the mesh listed a directed edge more than once
        self.spectral_bound = info.spectral_bound if 0.0 < info.spectral_bound <= 2.0 else 2.0
        self.op = PF_OP_SYM if self.symmetric else PF_OP_RW
        self.has_points = matrix is None
        self._rows = []
        if cotangent:
            self.cotangent = True
            hi, area = C.c_double(), C.c_double()
            _check(self._lib.pf_graph_cotan_info(h, C.byref(hi), C.byref(area)))
            self.hi, self.total_area = float(hi.value), float(area.value)
            self.spectral_bound = self.hi
            self.mass = self.cotan_download(w=False, diag=False)["mass"]

    @classmethod
    def build_pair(cls, mesh_a, mesh_b):
        """The graphs of two `DeviceMesh`es of one context assembled side by side on two streams
        (`pf_graph_build_device2`): same results as two constructor calls, in about the time of one."""
        if mesh_a.ctx is not mesh_b.ctx:
            raise ValueError("build_pair: the two meshes must belong to one context")
        ha, hb = C.c_void_p(), C.c_void_p()
        _check(mesh_a.ctx._lib.pf_graph_build_device2(mesh_a._h, mesh_b._h, C.byref(ha), C.byref(hb)))
        return cls(_handle=(mesh_a.ctx, ha)), cls(_handle=(mesh_b.ctx, hb))

    def close(self):
        for rows in self._rows:
            rows.close()
        _Handle.close(self)  # (pf_graph_free collects a download that is still owed or in flight)
        self._final_out = None

    # ---- matrices back to the host (scipy views for the reference-style attributes) ----------
    def download(self, labels=False):
        n, nnz = self.n, self.nnz_w
        out = dict(rowptr=np.empty(n + 1, np.int32), colidx=np.empty(nnz, np.int32), w=np.empty(nnz),
                   l_offdiag=np.empty(nnz), deg=np.empty(n), l_diag=np.empty(n))
        lab = np.empty(n, np.int32) if labels else None
        _check(self._lib.pf_graph_download(self._h, _ptr(out["rowptr"]), _ptr(out["colidx"]), _f64(out["w"]), _f64(out["l_offdiag"]),
                                           _f64(out["deg"]), _f64(out["l_diag"]), _ptr(lab)))
        if labels:
            out["labels"] = lab
        return out

    def cotan_download(self, w=True, diag=True, mass=True):
        """`pf_graph_cotan_download`: the cotangent weights w_ij (CSR order of `download()`), d_i and m_i of a cotangent graph."""
        out = {}
        if w:
            out["w"] = np.empty(self.nnz_w)
        if diag:
            out["diag"] = np.empty(self.n)
        if mass:
            out["mass"] = np.empty(self.n)
        _check(self._lib.pf_graph_cotan_download(self._h, *[_f64(out.get(k)) for k in ("w", "diag", "mass")]))
        return out

    def cotan_apply(self, x):
        """`pf_cotan_apply`: M^-1 (D - W) x for x of shape (n,) or (n, ncols <= 8)."""
        v = _c_f64(x)
        v2 = v.reshape(self.n, -1)
        out = np.empty_like(v2)
        _check(self._lib.pf_cotan_apply(self._h, _f64(v2), v2.shape[1], _f64(out)))
        return out[:, 0] if v.ndim == 1 else out

    # ---- ops interface ------------------------------------------------------------------------
    def ws_ensure(self, n_slots):
        _check(self._lib.pf_ws_ensure(self._h, int(n_slots)))

    def upload(self, slot, x):
        x = _c_f64(x, (self.n,))
        _check(self._lib.pf_ws_upload(self._h, int(slot), _f64(x)))

    def download_slots(self, first, count):
        out = np.empty((int(count), self.n), dtype=np.float64)
        _check(self._lib.pf_ws_download(self._h, int(first), int(count), _f64(out)))
        return out.T

    def copy(self, src, dst, count):
        _check(self._lib.pf_ws_copy(self._h, int(src), int(dst), int(count)))

    def mask_isolated(self, slot):
        _check(self._lib.pf_mask_isolated(self._h, int(slot)))

    def start_vector(self, slot, seed):
        _check(self._lib.pf_start_vector(self._h, int(slot), int(seed)))

    def lock_null_vectors(self):
        k = C.c_int32()
        _check(self._lib.pf_lock_null_vectors(self._h, self.op, C.byref(k)))
        return int(k.value)

    def spmv(self, src, dst):
        _check(self._lib.pf_spmv(self._h, self.op, int(src), int(dst)))

    def spmv_multi(self, src_first, dst_first, count):
        _check(self._lib.pf_spmv_multi(self._h, self.op, int(src_first), int(dst_first), int(count)))

    def cheb(self, src, dst, degree, c, e, rho=1.0):
        _check(self._lib.pf_cheb(self._h, self.op, int(src), int(dst), int(degree), float(c), float(e), float(rho)))

    def window_info(self, rings=False):
        """`pf_graph_window_info`: the window structures of the resident filter kernel as a dict - win_rows, n_windows,
        state (1: covered), state2 (1: two steps per exchange possible, -1: not asked for), and per window ghosts and
        need (None unless state == 1) and ghosts2 (None unless state2 == 1).  rings=True builds the second-ring
        structures now instead of at the graph's third single application.  Read-only otherwise."""
        n_max = int(self.info.n_pad) // 1024 + 1
        scalars = [C.c_int32() for _ in range(4)]
        ghosts, ghosts2, need = (np.full(n_max, -1, np.int32) for _ in range(3))
        _check(self._lib.pf_graph_window_info(self._h, int(bool(rings)), *[C.byref(s) for s in scalars],
                                              _ptr(ghosts), _ptr(ghosts2), _ptr(need)))
        win_rows, nw, state, state2 = (int(s.value) for s in scalars)
        return dict(win_rows=win_rows, n_windows=nw, state=state, state2=state2,
                    ghosts=ghosts[:nw].copy() if state == 1 else None, need=need[:nw].copy() if state == 1 else None,
                    ghosts2=ghosts2[:nw].copy() if state2 == 1 else None)

    def cheb2(self, req_self, other, req_other):
        """One lockstep filter application for two graphs of the same context:
        req = (src, dst, degree, c, e, rho)."""
        a, b = req_self, req_other
        _check(self._lib.pf_cheb2(self._h, self.op, int(a[0]), int(a[1]), int(a[2]), float(a[3]), float(a[4]), float(a[5]),
                                  other._h, other.op, int(b[0]), int(b[1]), int(b[2]), float(b[3]), float(b[4]), float(b[5])))

    def dots(self, w, first, count):
        out = np.empty(int(count), dtype=np.float64)
        _check(self._lib.pf_dots(self._h, int(w), int(first), int(count), _f64(out)))
        return out

    def orth(self, w, first, count):
        h = np.empty(max(int(count), 1), dtype=np.float64)
        nrm = C.c_double()
        _check(self._lib.pf_orth(self._h, int(w), int(first), int(count), _f64(h), C.byref(nrm)))
        return h[: int(count)], float(nrm.value)

    def orth_begin(self, w, first, count, normalize=True):
        _check(self._lib.pf_orth_begin(self._h, int(w), int(first), int(count), int(bool(normalize))))
        self._orth_count = int(count)

    def orth_begin2(self, req, other, req_other):
        """`orth_begin(*req)` of this graph and `other.orth_begin(*req_other)` in shared launches (requests:
        (w, first, count, normalize)); each graph collects with its own `orth_end`."""
        _check(self._lib.pf_orth_begin2(self._h, int(req[0]), int(req[1]), int(req[2]), int(bool(req[3])), other._h, int(req_other[0]),
                                        int(req_other[1]), int(req_other[2]), int(bool(req_other[3]))))
        self._orth_count, other._orth_count = int(req[2]), int(req_other[2])

    def orth_cheb2(self, orth, req, other, orth_other, req_other):
        """`orth_begin2` and, right behind it, `cheb2` in one library call (orth: (w, first, count, normalize); req as for
        `cheb2`)."""
        o = (C.c_int32 * 8)(int(orth[0]), int(orth[1]), int(orth[2]), int(bool(orth[3])), int(orth_other[0]), int(orth_other[1]),
                            int(orth_other[2]), int(bool(orth_other[3])))
        ci = (C.c_int32 * 8)(self.op, int(req[0]), int(req[1]), int(req[2]), other.op, int(req_other[0]), int(req_other[1]),
                             int(req_other[2]))
        cd = (C.c_double * 6)(float(req[3]), float(req[4]), float(req[5]), float(req_other[3]), float(req_other[4]), float(req_other[5]))
        _check(self._lib.pf_orth_cheb2(self._h, other._h, o, ci, cd))
        self._orth_count, other._orth_count = int(orth[2]), int(orth_other[2])

    def orth_split(self, first2, split):
        """The next `orth_begin` / `orth_begin2` / `orth_cheb2` step of this graph takes its basis from the slots
        [first, first + split) and [first2, first2 + count - split) (`pf_orth_split`)."""
        _check(self._lib.pf_orth_split(self._h, int(first2), int(split)))

    def orth_strict(self, on):
        """Second Gram-Schmidt pass at the classical threshold (|w'| < 0.71 |w|) instead of the loose one (0.3); on = 2:
        every step takes its second pass."""
        _check(self._lib.pf_orth_strict(self._h, 2 if on == 2 and on is not True else int(bool(on))))

    def orth_device_passes(self, on):
        """The second Gram-Schmidt pass queued with the first, run on the device's own verdict (`pf_orth_device_passes`):
        nothing queued behind a step ever reads a stale vector (`orth_redone` stays False, `orth_twice` tells)."""
        _check(self._lib.pf_orth_device_passes(self._h, int(bool(on))))

    def orth_end(self):
        h = np.empty(max(self._orth_count, 1), dtype=np.float64)
        nrm = C.c_double()
        _check(self._lib.pf_orth_end(self._h, _f64(h), C.byref(nrm)))
        # the step needed its second Gram-Schmidt pass, run only now: anything queued since orth_begin that read w is stale
        r = self._lib.pf_orth_redone(self._h)
        self.orth_redone = r == 1
        self.orth_twice = r == 2  # (both passes ran on the device, before anything queued behind them)
        return h[: self._orth_count], float(nrm.value)

    def orth_abandon(self):
        """Collect and discard an orthogonalisation left in flight by a solve that was aborted."""
        try:
            self.orth_end()
        except PfError:
            pass

    def scale(self, slot, alpha):
        _check(self._lib.pf_scale(self._h, int(slot), float(alpha)))

    def combine(self, src_first, m, Y, dst_first):
        Y = _c_f64(Y)
        if Y.ndim != 2 or Y.shape[0] != m:
            raise ValueError("Y must be (m, k)")
        _check(self._lib.pf_combine(self._h, int(src_first), int(m), _f64(Y), Y.shape[1], int(dst_first)))

    def resnorm(self, ax, x, lam):
        out = C.c_double()
        _check(self._lib.pf_resnorm(self._h, int(ax), int(x), float(lam), C.byref(out)))
        return float(out.value)

    def gram(self, first_a, count_a, first_b, count_b):
        """(count_a, count_b) matrix of inner products <slot first_a+i, slot first_b+j>, one synchronisation."""
        out = np.empty((int(count_a), int(count_b)), dtype=np.float64)
        _check(self._lib.pf_gram(self._h, int(first_a), int(count_a), int(first_b), int(count_b), _f64(out)))
        return out

    def resnorms(self, ax_first, x_first, lams):
        """||slot(ax_first+i) - lams[i] slot(x_first+i)||_2 for every i, one synchronisation."""
        lams = _c_f64(lams)
        out = np.empty(len(lams), dtype=np.float64)
        _check(self._lib.pf_resnorms(self._h, int(ax_first), int(x_first), _f64(lams), len(lams), _f64(out)))
        return out

    def finalize_vectors(self, first, count, minmax, wait=True):
        """Normalised eigenvectors of `count` slots -> (n, count) array in PINNED host memory (one DMA on the ctx's copy
        stream).  `wait=False`: the array is returned while the download is still in flight - `finalize_wait()` before
        anybody reads it (`Graph.eig_vecs` does); the device-resident twin of the block is usable at once."""
        out = pinned_empty((self.n, int(count)))
        _check(self._lib.pf_finalize_vectors_begin(self._h, int(first), int(count), int(self.op == PF_OP_SYM), int(bool(minmax)),
                                                   _f64(out)))
        self._final_count = int(count)  # the same block stays resident on the device (final_rows, Context.knn1_graphs)
        self._final_pending = True
        # the download may not even be queued yet (the library holds it back until a long kernel runs): the array must
        # outlive it whatever the caller does with its own reference - a pinned block that is freed under an owed
        # download is a write into unmapped memory from the device
        self._final_out = out
        if wait:
            self.finalize_wait()
        return out

    def final_remap(self, cols, signs, out):
        """out[:, c] <- (device-resident block)[:, cols[c]] * signs[c], by a kernel and one DMA on the copy stream (`out`: the
        pinned array `finalize_vectors` returned, all of its columns); `finalize_wait()` before anybody reads it."""
        cols = _c_i32(cols)
        signs = np.ascontiguousarray(signs, dtype=np.float64)
        assert out.flags.c_contiguous and out.shape == (self.n, len(cols))
        _check(self._lib.pf_final_remap_begin(self._h, _ptr(cols), _f64(signs), len(cols), _f64(out)))
        self._final_pending = True
        self._final_out = out

    def finalize_wait(self):
        """Collect the download a `finalize_vectors(..., wait=False)` left in flight (no-op otherwise)."""
        if getattr(self, "_final_pending", False) and self._h:
            self._final_pending = False
            try:
                _check(self._lib.pf_finalize_vectors_end(self._h))
            finally:
                self._final_out = None

    def final_rows(self, rows):
        """Rows of the block the last `finalize_vectors` left on the device -> (len(rows), count) array."""
        rows = _c_i64(rows)
        out = np.empty((len(rows), self._final_count), dtype=np.float64)
        _check(self._lib.pf_final_rows(self._h, _ptr(rows), len(rows), _f64(out)))
        return out

    def final_device(self):
        """(device address, n_rows, n_cols) of the block the last `finalize_vectors` left in HBM (row-major float64)."""
        ptr, n_rows, n_cols = C.c_void_p(), C.c_int64(), C.c_int32()
        _check(self._lib.pf_final_device(self._h, C.byref(ptr), C.byref(n_rows), C.byref(n_cols)))
        return int(ptr.value), int(n_rows.value), int(n_cols.value)

    def point_rows(self, rows):
        """Rows of the mesh's points as they sit on the device -> (len(rows), 3) array (mesh-built graphs only)."""
        rows = _c_i64(rows)
        out = np.empty((len(rows), 3), dtype=np.float64)
        _check(self._lib.pf_point_rows(self._h, _ptr(rows), len(rows), _f64(out)))
        return out

    def spmv_host(self, x, op=None):
        x = _c_f64(x, (self.n,))
        y = np.empty(self.n, dtype=np.float64)
        _check(self._lib.pf_spmv_host(self._h, self.op if op is None else int(op), _f64(x), _f64(y)))
        return y

    def eigs_smallest(self, n_wanted, minmax=False, wait=True):
        """`pf_eigs_smallest_ex`: the eigensolve as ONE C call -> (vals, vecs (n, m) in pinned memory, stats dict with a
        `residuals` array).  `wait=False`: the eigenvector download is still in flight (`finalize_wait()`)."""
        m = int(n_wanted)
        vals, vecs, resid, n_out, st = np.empty(m), pinned_empty((self.n, m)), np.zeros(m), C.c_int32(), EigsStats()
        _check(self._lib.pf_eigs_smallest_ex(self._h, m, int(bool(minmax)), 0 if wait else 1, _f64(vals), _f64(vecs), _f64(resid),
                                             C.byref(n_out), C.byref(st)))
        return self._eigs_result(vals, vecs, resid, n_out.value, st, wait)

    def _eigs_result(self, vals, vecs, resid, m, st, wait):
        self._final_count = m
        self._final_pending = (not wait) and m > 0
        self._final_out = vecs if self._final_pending else None  # (kept alive until the download has been collected)
        if m != vecs.shape[1]:  # fewer pairs than asked for: the library wrote an (n, m) block
            if self._final_pending:
                self.finalize_wait()
            vecs = np.ascontiguousarray(vecs.reshape(-1)[: self.n * m].reshape(self.n, m))
        stats = st.as_dict()
        stats["residuals"] = resid[:m].copy()
        return vals[:m].copy(), vecs, stats

    def eigs_smallest2(self, other, n_wanted, n_wanted_other, minmax=False, wait=True):
        """`pf_eigs_smallest2`: this graph and `other` (same ctx) solved together in ONE C call -
        the pipelined pair driver in C++.  Returns two tuples (vals, vecs (n, m) in pinned memory, stats dict with a
        `residuals` array).  `wait=False`: the eigenvector downloads are still in flight (`finalize_wait()` on each)."""
        outs = []
        for dev, m in ((self, int(n_wanted)), (other, int(n_wanted_other))):
            outs.append((np.empty(m), pinned_empty((dev.n, m)), np.zeros(m), C.c_int32(), EigsStats()))
        (va, xa, ra, na, sa), (vb, xb, rb, nb, sb) = outs
        _check(self._lib.pf_eigs_smallest2(self._h, other._h, int(n_wanted), int(n_wanted_other), int(bool(minmax)), 0 if wait else 1,
                                           _f64(va), _f64(xa), _f64(ra), C.byref(na), C.byref(sa),
                                           _f64(vb), _f64(xb), _f64(rb), C.byref(nb), C.byref(sb)))
        return tuple(dev._eigs_result(vals, vecs, resid, n_out.value, st, wait) for dev, (vals, vecs, resid, n_out, st) in zip((self, other), outs))

    # ---- primitives of the row-partitioned solve (pyfocusr_amd/rowpart.py)
    def op_step(self, x, prev, out, alpha, c, beta, op=None):
        """out = alpha (c x - A x) - beta prev (slots; prev None: no prev term; out may be the prev slot)."""
        _check(self._lib.pf_op_step(self._h, self.op if op is None else int(op), int(x), -1 if prev is None else int(prev),
                                    int(out), float(alpha), float(c), float(beta)))

    def cheb_steps(self, prev, cur, k_first, n_steps, c, e, rho=1.0, op=None):
        """Steps k_first.. of the Chebyshev recurrence on explicit state slots; returns (prev, cur) afterwards."""
        op_, oc = C.c_int32(), C.c_int32()
        _check(self._lib.pf_cheb_steps(self._h, self.op if op is None else int(op), int(prev), int(cur), int(k_first),
                                       int(n_steps), float(c), float(e), float(rho), C.byref(op_), C.byref(oc)))
        return op_.value, oc.value

    def axpy(self, w, first, count, coef):
        coef = _c_f64(coef)
        _check(self._lib.pf_axpy(self._h, int(w), int(first), int(count), _f64(coef)))

    def rows_create(self, idx):
        rows = _Rows(self, idx)
        self._rows.append(rows)
        return rows

    def rows_gather(self, slot, rows):
        out = np.empty(rows.n)
        _check(self._lib.pf_rows_gather(rows._h, int(slot), _f64(out)))
        return out

    def rows_scatter(self, slot, rows, values):
        values = _c_f64(values, (rows.n,))
        _check(self._lib.pf_rows_scatter(rows._h, int(slot), _f64(values)))

    def rows_gather_dev(self, slot, rows, device_ptr):
        """Values of the row subset into a device buffer of the caller (int address); no host sync."""
        _check(self._lib.pf_rows_gather_dev(rows._h, int(slot), C.c_void_p(int(device_ptr))))

    def rows_scatter_dev(self, slot, rows, device_ptr):
        _check(self._lib.pf_rows_scatter_dev(rows._h, int(slot), C.c_void_p(int(device_ptr))))

    def rows_set_sources(self, rows, offsets):
        offsets = _c_i64(offsets)
        if len(offsets) != rows.n:
            raise ValueError("one offset per row")
        _check(self._lib.pf_rows_set_sources(rows._h, _ptr(offsets)))

    def rows_gather2_dev(self, slot_a, slot_b, rows, device_ptr, stride):
        _check(self._lib.pf_rows_gather2_dev(rows._h, int(slot_a), -1 if slot_b is None else int(slot_b),
                                             C.c_void_p(int(device_ptr)), int(stride)))

    def rows_scatter2_dev(self, slot_a, slot_b, rows, device_ptr, stride):
        _check(self._lib.pf_rows_scatter2_dev(rows._h, int(slot_a), -1 if slot_b is None else int(slot_b),
                                              C.c_void_p(int(device_ptr)), int(stride)))

    def sync(self):
        self.ctx.sync()

    def rows_fill(self, slot, rows, value):
        _check(self._lib.pf_rows_fill(rows._h, int(slot), float(value)))

    def mean_filter(self, values, iterations):
        v = _c_f64(values)
        one_d = v.ndim == 1
        v2 = v.reshape(self.n, -1)
        out = np.empty_like(v2)
        _check(self._lib.pf_mean_filter(self._h, _f64(v2), v2.shape[1], int(iterations), _f64(out)))
        return out[:, 0] if one_d else out
