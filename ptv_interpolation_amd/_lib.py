"""ctypes binding of the C ABI in include/ptv_api.h (libptv_amd.so, built in-tree).

The shipped path has no CPU fallback: if the library is missing or no GPU is
visible, ``lib()`` / ``Context`` raise.  Structures mirror the header field by
field.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(HERE, "libptv_amd.so")
LIB_PATH = os.environ.get("PTV_LIB", _DEFAULT_LIB)

PTV_OK = 0
PTV_E_ARG = -1
PTV_E_HIP = -2
PTV_E_NOMEM = -3
PTV_E_UNSUPPORTED = -4
PTV_E_INEXACT = -5
PTV_E_SINGULAR = -6

METHOD_IDW = 0
METHOD_SIBSON = 1
METHOD_NEAREST = 2
METHOD_IDW_RADIUS = 3  # extension: IDW over every particle within a radius (parity unpinned)

FLAG_NAN_TO_NUM = 1

# local RBF kernels (include/ptv_api.h PTV_RBF_*), scipy names
RBF_KERNELS = {
    "linear": 0,
    "thin_plate_spline": 1,
    "cubic": 2,
    "quintic": 3,
    "multiquadric": 4,
    "inverse_multiquadric": 5,
    "inverse_quadratic": 6,
    "gaussian": 7,
}

_dp = C.POINTER(C.c_double)


class Particles(C.Structure):
    _fields_ = [("n", C.c_int64), ("x", _dp), ("y", _dp), ("z", _dp), ("u", _dp), ("v", _dp), ("w", _dp)]


class Grid(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64),
                ("ax", _dp), ("ay", _dp), ("az", _dp),
                ("px", _dp), ("py", _dp), ("pz", _dp),
                ("z_begin", C.c_int64), ("z_end", C.c_int64)]


class KnnParams(C.Structure):
    _fields_ = [("method", C.c_int), ("k", C.c_int), ("power", C.c_double), ("eps", C.c_double),
                ("fluid_mask", C.POINTER(C.c_uint8)), ("flags", C.c_uint32), ("cell_occupancy", C.c_double),
                ("r0_scale", C.c_double), ("lattice_bounds", C.c_int), ("slab_halo", C.c_double),
                ("radius", C.c_double)]


class RbfParams(C.Structure):
    _fields_ = [("k", C.c_int), ("kernel", C.c_int), ("epsilon", C.c_double), ("degree", C.c_int),
                ("smoothing", C.c_double), ("smoothing_per_point", _dp), ("fluid_mask", C.POINTER(C.c_uint8)),
                ("flags", C.c_uint32), ("chunk_planes", C.c_int)]


_i32p = C.POINTER(C.c_int32)


class LinearParams(C.Structure):
    _fields_ = [("nsimplex", C.c_int64), ("simplices", _i32p), ("neighbors", _i32p), ("transform", _dp),
                ("vertex_to_simplex", _i32p), ("min_bound", C.c_double * 3), ("max_bound", C.c_double * 3),
                ("fill_value", C.c_double), ("fluid_mask", C.POINTER(C.c_uint8)), ("flags", C.c_uint32),
                ("chunk_planes", C.c_int)]


F64 = 0
F32 = 1
FLAG_OUT_F32 = 2  # U, V, W written as float32 (main.py:230 astype, fused)
FLAG_RBF_SPD_LDS = 4  # local RBF diagnostics: SPD systems through the LDS-broadcast kernel
FLAG_RBF_PIVOTING = 8  # local RBF diagnostics: scale-invariant kernels through the pivoting solver
FLAG_KNN_REPAIR_ALL = 16  # k-NN diagnostics: near-tie repair reruns the whole launch past one tile
FLAG_SLAB_CULL_AUTO = 32  # k-NN z-slab calls: per-column cull map, cached per context and proven (ABI v10)


class DivParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("z_begin", C.c_int64),
                ("z_end", C.c_int64), ("edge_lo", C.c_int), ("edge_hi", C.c_int), ("field_dtype", C.c_int),
                ("result_dtype", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("fluid_mask", C.POINTER(C.c_uint8))]


_u8p = C.POINTER(C.c_uint8)


class CleanParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("dx", C.c_double), ("dy", C.c_double),
                ("dz", C.c_double), ("fluid_mask", _u8p), ("iterations", C.c_int), ("damp", C.c_double),
                ("atol", C.c_double), ("btol", C.c_double), ("iter_lim", C.c_int)]


CLEAN_MAX_OUTER = 16


class CleanStats(C.Structure):
    _fields_ = [("n_outer", C.c_int32), ("nan_stop", C.c_int32), ("n_fluid", C.c_int64),
                ("istop", C.c_int32 * CLEAN_MAX_OUTER), ("itn", C.c_int32 * CLEAN_MAX_OUTER),
                ("rnorm", C.c_double * CLEAN_MAX_OUTER), ("mean_abs_div", C.c_double * CLEAN_MAX_OUTER),
                ("ms_iter_median", C.c_double * CLEAN_MAX_OUTER), ("mean_abs_div_final", C.c_double),
                ("flux_initial", C.c_double), ("flux_final", C.c_double), ("ms_total", C.c_double),
                ("ms_solve", C.c_double)]

    def as_dict(self):
        n = min(self.n_outer, CLEAN_MAX_OUTER)
        d = {f: getattr(self, f) for f, t in self._fields_ if not hasattr(t, "_length_")}
        for f in ("istop", "itn", "rnorm", "ms_iter_median"):
            d[f] = list(getattr(self, f))[:n]
        # the divergence of the input is measured even when no solve runs (iterations = 0)
        d["mean_abs_div"] = list(self.mean_abs_div)[:max(n, 1)]
        return d


class VariationalParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("dx", C.c_double), ("dy", C.c_double),
                ("dz", C.c_double), ("fluid_mask", _u8p), ("lambda_reg", C.c_double), ("rtol", C.c_double),
                ("maxiter", C.c_int)]


class VariationalStats(C.Structure):
    _fields_ = [("n_fluid", C.c_int64), ("itn", C.c_int32), ("info", C.c_int32), ("bnorm", C.c_double),
                ("rnorm", C.c_double), ("mean_abs_div_initial", C.c_double), ("mean_abs_div_final", C.c_double),
                ("ms_total", C.c_double), ("ms_solve", C.c_double), ("ms_iter_median", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


FLOW_OUTPUTS = ("strain_rate", "dissipation", "vorticity", "flow_type")  # PTV_FLOW_* order


class FlowParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("z_begin", C.c_int64),
                ("z_end", C.c_int64), ("edge_lo", C.c_int), ("edge_hi", C.c_int), ("field_dtype", C.c_int),
                ("spacing_strong", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("viscosity", C.c_double), ("fluid_mask", _u8p)]


class FlowStats(C.Structure):
    _fields_ = [("n_voxels", C.c_int64), ("n_fluid", C.c_int64), ("sum_u", C.c_double), ("sum_v", C.c_double),
                ("sum_w", C.c_double), ("sum", C.c_double * 4), ("sum_fluid", C.c_double * 4),
                ("max", C.c_double * 4), ("min", C.c_double * 4), ("ms_stencil", C.c_double)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, t in self._fields_ if not hasattr(t, "_length_")}
        for f in ("sum", "sum_fluid", "max", "min"):
            d[f] = dict(zip(FLOW_OUTPUTS, getattr(self, f)))
        return d


class DragParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("field_dtype", C.c_int),
                ("n_labels", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("viscosity", C.c_double), ("labels", C.POINTER(C.c_int32))]


class DragStats(C.Structure):
    """One (label, axis, direction) record of the interface drag."""
    _fields_ = [("count", C.c_int64), ("sum_p", C.c_double), ("sum_u", C.c_double), ("sum_v", C.c_double),
                ("sum_w", C.c_double)]


# the records as a numpy array: (n_labels, 3 axes, 2 directions) of this dtype
DRAG_RECORD = np.dtype([("count", np.int64), ("sum_p", np.float64), ("sum_u", np.float64), ("sum_v", np.float64),
                        ("sum_w", np.float64)])

class SplineParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("field_dtype", C.c_int), ("order", C.c_int),
                ("n_points", C.c_int64)]


SPLINE_PAD = 12  # PTV_SPLINE_PAD: edge-replicated samples on every side of the coefficient array
# the sums of one label in the order of the reference's result (velocity_analysis.py:621-643)
MESH_KEYS = ("Fx_v", "Fy_v", "Fz_v", "Fx_v_tan", "Fy_v_tan", "Fz_v_tan", "Fx_v_nor", "Fy_v_nor", "Fz_v_nor",
             "Fx_p", "Fy_p", "Fz_p", "Area", "Fx_water", "Fy_water", "Fz_water", "Fx_solid", "Fy_solid", "Fz_solid",
             "Area_water", "Area_solid")


class MeshParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("field_dtype", C.c_int),
                ("vert_dtype", C.c_int), ("n_verts", C.c_int64), ("n_tris", C.c_int64), ("n_labels", C.c_int),
                ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double), ("viscosity", C.c_double),
                ("reuse", C.c_int), ("tri_offsets", C.POINTER(C.c_int64)), ("mesh_resident", C.c_int)]


class MeshRecord(C.Structure):
    """The triangle count and the sums (MESH_KEYS) of one label of the mesh drag."""
    _fields_ = [("n_tris", C.c_int64), ("sums", C.c_double * len(MESH_KEYS))]


MESH_RECORD = np.dtype([("n_tris", np.int64), ("sums", np.float64, (len(MESH_KEYS),))])


class SurfaceParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("step_size", C.c_int),
                ("n_labels", C.c_int), ("labels", C.POINTER(C.c_int32))]


class LabelParams(C.Structure):
    _fields_ = [("nz", C.c_int64), ("ny", C.c_int64), ("nx", C.c_int64), ("connectivity", C.c_int)]


class LabelStats(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_foreground", C.c_int64), ("ms_merge", C.c_double),
                ("ms_number", C.c_double)]


WALL_BC = {"zero-neumann": 0, "inhomogeneous": 1}  # PTV_WALL_*
ANCHOR = {"none": 0, "outlet": 1, "inlet": 2}      # PTV_ANCHOR_*
FLOW_DIRECTION = {"auto": 0, "positive": 1, "negative": -1}


class PressureParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("dx", C.c_double), ("dy", C.c_double),
                ("dz", C.c_double), ("mu", C.c_double), ("rho", C.c_double), ("wall_bc", C.c_int),
                ("anchor", C.c_int), ("flow_direction", C.c_int), ("maxiter", C.c_int), ("rtol", C.c_double),
                ("lsqr_damp", C.c_double), ("lsqr_atol", C.c_double), ("lsqr_btol", C.c_double),
                ("lsqr_iter_lim", C.c_int), ("fluid_mask", _u8p)]


class PressureStats(C.Structure):
    _fields_ = [("n_fluid", C.c_int64), ("n_dirichlet", C.c_int64), ("itn", C.c_int32), ("info", C.c_int32),
                ("solver", C.c_int32), ("anchor_plane", C.c_int32), ("bnorm", C.c_double), ("rnorm", C.c_double),
                ("sum_abs_fx", C.c_double), ("sum_abs_fy", C.c_double), ("sum_abs_fz", C.c_double),
                ("sum_w", C.c_double), ("ms_force", C.c_double), ("ms_divergence", C.c_double),
                ("ms_solve", C.c_double), ("ms_iter_median", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


MG_MAX_LEVELS = 32  # PTV_MG_MAX_LEVELS


class MgParams(C.Structure):
    """The multigrid preconditioner's parameters; a zero means the default (2, 16, 2/3, no cap)."""
    _fields_ = [("max_levels", C.c_int), ("nu", C.c_int), ("coarse_sweeps", C.c_int), ("omega", C.c_double)]


class MgStats(C.Structure):
    _fields_ = [("levels", C.c_int32), ("tail_level", C.c_int32), ("cells", C.c_int64 * MG_MAX_LEVELS),
                ("active", C.c_int64 * MG_MAX_LEVELS), ("ms_setup", C.c_double), ("ms_vcycle_median", C.c_double)]

    def as_dict(self):
        n = int(self.levels)
        return {"levels": n, "tail_level": int(self.tail_level), "cells": list(self.cells)[:n],
                "active": list(self.active)[:n], "ms_setup": self.ms_setup,
                "ms_vcycle_median": self.ms_vcycle_median}


def mg_params(multigrid=None):
    """``multigrid``: None or a dict with any of max_levels, nu, coarse_sweeps, omega."""
    kw = dict(multigrid or {})
    prm = MgParams(int(kw.pop("max_levels", 0)), int(kw.pop("nu", 0)), int(kw.pop("coarse_sweeps", 0)),
                   float(kw.pop("omega", 0.0)))
    if kw:
        raise ValueError(f"unknown multigrid parameters {sorted(kw)} (max_levels, nu, coarse_sweeps, omega)")
    return prm


class EdtParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("keep_distance", C.c_int)]


class EdtStats(C.Structure):
    _fields_ = [("max_d2", C.c_int64), ("ms", C.c_double)]


class AlignParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("n_points", C.c_int64),
                ("n_offsets", C.c_int)]


class AlignRecord(C.Structure):
    """One offset's record of the alignment score."""
    _fields_ = [("n_inside", C.c_int64), ("n_outside", C.c_int64), ("sum", C.c_double)]


# the records as a numpy array: (n_offsets,) of this dtype
ALIGN_RECORD = np.dtype([("n_inside", np.int64), ("n_outside", np.int64), ("sum", np.float64)])

MASK_BOOL = 0
MASK_BITS = 1


class MaskGrid(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("raw", _u8p),
                ("ax", _dp), ("ay", _dp), ("az", _dp)]


class BoundaryParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("mask", _u8p),
                ("encoding", C.c_int), ("thickness", C.c_int), ("sampling_step", C.c_int64),
                ("lo", C.c_double * 3), ("span", C.c_double * 3), ("den", C.c_double * 3)]


class FilterParams(C.Structure):
    _fields_ = [("k", C.c_int), ("threshold", C.c_double), ("mad_eps", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("ms_h2d", C.c_double), ("ms_bin", C.c_double), ("ms_lattice", C.c_double), ("ms_knn", C.c_double),
                ("ms_d2h", C.c_double),
                ("ms_total", C.c_double), ("n_particles", C.c_int64), ("n_voxels", C.c_int64),
                ("n_cells", C.c_int64), ("cells", C.c_int32 * 3), ("cell_size", C.c_double * 3),
                ("r0", C.c_double), ("ms_solve", C.c_double), ("n_singular", C.c_int64),
                ("ms_stencil", C.c_double), ("n_binned", C.c_int64), ("halo_required", C.c_double),
                ("ms_cull", C.c_double), ("n_repair_tiles", C.c_int64),
                ("n_rbf_pivoted", C.c_int64)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["cells"] = list(self.cells)
        d["cell_size"] = list(self.cell_size)
        return d


EXPORTS = {
    "ptv_version": (C.c_int, []),
    "ptv_abi_sizes": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_abi_sizes2": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_abi_sizes3": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_interp_linear": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid), C.POINTER(LinearParams),
                                    _dp, _dp, _dp, C.POINTER(Stats)]),
    "ptv_interp_linear_dev": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid),
                                        C.POINTER(LinearParams), _dp, _dp, _dp, C.c_void_p, C.POINTER(Stats)]),
    "ptv_last_error": (C.c_char_p, []),
    "ptv_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ptv_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "ptv_free": (C.c_int, [C.c_void_p]),
    "ptv_interp_knn": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid), C.POINTER(KnnParams),
                                 _dp, _dp, _dp, C.POINTER(Stats)]),
    "ptv_interp_knn_dev": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid), C.POINTER(KnnParams),
                                     _dp, _dp, _dp, C.c_void_p, C.POINTER(Stats)]),
    "ptv_interp_rbf_local": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid), C.POINTER(RbfParams),
                                       _dp, _dp, _dp, C.POINTER(Stats)]),
    "ptv_interp_rbf_local_dev": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(Grid),
                                           C.POINTER(RbfParams), _dp, _dp, _dp, C.c_void_p, C.POINTER(Stats)]),
    "ptv_divergence": (C.c_int, [C.c_void_p, C.POINTER(DivParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(Stats)]),
    "ptv_divergence_dev": (C.c_int, [C.c_void_p, C.POINTER(DivParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "ptv_sample_mask": (C.c_int, [C.c_void_p, C.POINTER(MaskGrid), C.POINTER(Grid), _u8p]),
    "ptv_sample_mask_dev": (C.c_int, [C.c_void_p, C.POINTER(MaskGrid), C.POINTER(Grid), _u8p, C.c_void_p]),
    "ptv_boundary_particles": (C.c_int, [C.c_void_p, C.POINTER(BoundaryParams), _dp, _dp, _dp, C.c_int64,
                                         C.POINTER(C.c_int64)]),
    "ptv_boundary_particles_dev": (C.c_int, [C.c_void_p, C.POINTER(BoundaryParams), _dp, _dp, _dp, C.c_int64,
                                             C.POINTER(C.c_int64), C.c_void_p]),
    "ptv_filter_outliers_knn": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(FilterParams), _u8p, _dp,
                                          C.POINTER(Stats)]),
    "ptv_filter_outliers_knn_dev": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(FilterParams), _u8p,
                                              _dp, C.c_void_p, C.POINTER(Stats)]),
    "ptv_abi_sizes4": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_clean_divergence": (C.c_int, [C.c_void_p, C.POINTER(CleanParams), _dp, _dp, _dp, _dp, _dp, _dp,
                                       C.POINTER(CleanStats)]),
    "ptv_clean_divergence_dev": (C.c_int, [C.c_void_p, C.POINTER(CleanParams), _dp, _dp, _dp, _dp, _dp, _dp,
                                           C.c_void_p, C.POINTER(CleanStats)]),
    "ptv_apply_correction": (C.c_int, [C.c_void_p, C.POINTER(CleanParams), _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ptv_laplacian_apply": (C.c_int, [C.c_void_p, C.POINTER(CleanParams), _dp, _dp]),
    "ptv_abi_sizes5": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_clean_variational": (C.c_int, [C.c_void_p, C.POINTER(VariationalParams), _dp, _dp, _dp, _dp, _dp, _dp,
                                        C.POINTER(VariationalStats)]),
    "ptv_clean_variational_dev": (C.c_int, [C.c_void_p, C.POINTER(VariationalParams), _dp, _dp, _dp, _dp, _dp, _dp,
                                            C.c_void_p, C.POINTER(VariationalStats)]),
    "ptv_variational_apply": (C.c_int, [C.c_void_p, C.POINTER(VariationalParams), _dp, _dp, _dp, _dp, _dp, _dp]),
    "ptv_divergence_operator_apply": (C.c_int, [C.c_void_p, C.POINTER(VariationalParams), _dp, _dp, _dp, _dp]),
    "ptv_abi_sizes6": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_flow_analysis": (C.c_int, [C.c_void_p, C.POINTER(FlowParams)] + [C.c_void_p] * 7 + [C.POINTER(FlowStats)]),
    "ptv_flow_analysis_dev": (C.c_int, [C.c_void_p, C.POINTER(FlowParams)] + [C.c_void_p] * 8 +
                              [C.POINTER(FlowStats)]),
    "ptv_flow_derived": (C.c_int, [C.c_void_p, C.POINTER(FlowParams)] + [C.c_void_p] * 4 + [C.POINTER(FlowStats)]),
    "ptv_flow_derived_dev": (C.c_int, [C.c_void_p, C.POINTER(FlowParams)] + [C.c_void_p] * 5 +
                             [C.POINTER(FlowStats)]),
    "ptv_abi_sizes7": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_interface_drag": (C.c_int, [C.c_void_p, C.POINTER(DragParams)] + [C.c_void_p] * 6 + [_dp]),
    "ptv_interface_drag_dev": (C.c_int, [C.c_void_p, C.POINTER(DragParams)] + [C.c_void_p] * 7 + [_dp]),
    "ptv_gradient_sums": (C.c_int, [C.c_void_p, C.POINTER(FlowParams), C.c_void_p, _dp]),
    "ptv_gradient_sums_dev": (C.c_int, [C.c_void_p, C.POINTER(FlowParams), C.c_void_p, C.c_void_p, _dp]),
    "ptv_abi_sizes8": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_edt": (C.c_int, [C.c_void_p, C.POINTER(EdtParams)] + [C.c_void_p] * 3 + [C.POINTER(EdtStats)]),
    "ptv_edt_dev": (C.c_int, [C.c_void_p, C.POINTER(EdtParams)] + [C.c_void_p] * 4 + [C.POINTER(EdtStats)]),
    "ptv_align_score": (C.c_int, [C.c_void_p, C.POINTER(AlignParams)] + [C.c_void_p] * 4 + [_dp]),
    "ptv_align_score_dev": (C.c_int, [C.c_void_p, C.POINTER(AlignParams)] + [C.c_void_p] * 5 + [_dp]),
    "ptv_abi_sizes9": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_force_field": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 6 + [C.POINTER(PressureStats)]),
    "ptv_force_field_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 6 +
                            [C.c_void_p, C.POINTER(PressureStats)]),
    "ptv_force_divergence": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4),
    "ptv_force_divergence_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 + [C.c_void_p]),
    "ptv_poisson_solve": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 + [_u8p, _dp,
                                                                                           C.POINTER(PressureStats)]),
    "ptv_poisson_solve_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                              [_u8p, _dp, C.c_void_p, C.POINTER(PressureStats)]),
    "ptv_pressure_recover": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                             [C.POINTER(PressureStats)]),
    "ptv_pressure_recover_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                                 [C.c_void_p, C.POINTER(PressureStats)]),
    "ptv_abi_sizes10": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_spline_prefilter": (C.c_int, [C.c_void_p, C.POINTER(SplineParams)] + [C.c_void_p] * 2 + [_dp]),
    "ptv_spline_prefilter_dev": (C.c_int, [C.c_void_p, C.POINTER(SplineParams)] + [C.c_void_p] * 3 + [_dp]),
    "ptv_map_coordinates": (C.c_int, [C.c_void_p, C.POINTER(SplineParams)] + [C.c_void_p] * 3 + [_dp]),
    "ptv_map_coordinates_dev": (C.c_int, [C.c_void_p, C.POINTER(SplineParams)] + [C.c_void_p] * 4 + [_dp]),
    "ptv_mesh_drag": (C.c_int, [C.c_void_p, C.POINTER(MeshParams)] + [C.c_void_p] * 8 + [_dp]),
    "ptv_mesh_drag_dev": (C.c_int, [C.c_void_p, C.POINTER(MeshParams)] + [C.c_void_p] * 9 + [_dp]),
    "ptv_abi_sizes11": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_marching_cubes": (C.c_int, [C.c_void_p, C.POINTER(SurfaceParams), C.c_void_p, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), _dp]),
    "ptv_marching_cubes_dev": (C.c_int, [C.c_void_p, C.POINTER(SurfaceParams), C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp]),
    "ptv_surface_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptv_abi_sizes12": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_label": (C.c_int, [C.c_void_p, C.POINTER(LabelParams)] + [C.c_void_p] * 3 + [C.POINTER(LabelStats)]),
    "ptv_label_dev": (C.c_int, [C.c_void_p, C.POINTER(LabelParams)] + [C.c_void_p] * 4 + [C.POINTER(LabelStats)]),
    "ptv_abi_sizes13": (C.c_int, [C.POINTER(C.c_int64)]),
    "ptv_poisson_mg_apply": (C.c_int, [C.c_void_p, C.POINTER(PressureParams), C.POINTER(MgParams), _u8p, _dp, _dp,
                                       C.POINTER(MgStats)]),
    "ptv_poisson_mg_apply_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams), C.POINTER(MgParams), _u8p, _dp, _dp,
                                           C.c_void_p, C.POINTER(MgStats)]),
    "ptv_poisson_solve_mg": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                             [_u8p, _dp, C.POINTER(MgParams), C.POINTER(PressureStats), C.POINTER(MgStats)]),
    "ptv_poisson_solve_mg_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                                 [_u8p, _dp, C.c_void_p, C.POINTER(MgParams), C.POINTER(PressureStats),
                                  C.POINTER(MgStats)]),
    "ptv_pressure_recover_mg": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                                [C.POINTER(MgParams), C.POINTER(PressureStats), C.POINTER(MgStats)]),
    "ptv_pressure_recover_mg_dev": (C.c_int, [C.c_void_p, C.POINTER(PressureParams)] + [_dp] * 4 +
                                    [C.c_void_p, C.POINTER(MgParams), C.POINTER(PressureStats), C.POINTER(MgStats)]),
    "ptv_last_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "ptv_debug_stamps": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "ptv_debug_xcd_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_longlong, C.POINTER(C.c_longlong)]),
    "ptv_debug_xcd_chunk": (C.c_int, [C.c_int]),
    "ptv_xcd_chunk_map": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
}

_lib = None
_lock = threading.Lock()


class PtvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptv error {code}: {msg}")
        self.code = code
        self.msg = msg


def lib():
    """Load libptv_amd.so (raises if it is missing: there is no CPU fallback)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} not found: build it with `python -m ptv_interpolation_amd.build` "
                    "(hipcc, gfx950). The k-NN path has no CPU fallback.")
            L = C.CDLL(LIB_PATH)
            for name, (res, args) in EXPORTS.items():
                if LIB_PATH != _DEFAULT_LIB and not hasattr(L, name):
                    continue  # an older build under PTV_LIB (same-box A/B): its missing entry points stay unbound
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class InexactError(PtvError):
    """PTV_E_INEXACT: the slab_halo cull could not be proven exact (ptv_knn_params.slab_halo);
    ``halo_required`` is the halo that would be."""

    def __init__(self, code, msg, halo_required=None):
        super().__init__(code, msg)
        self.halo_required = halo_required


def check(rc):
    if rc != PTV_OK:
        msg = lib().ptv_last_error().decode(errors="replace")
        if rc == PTV_E_ARG:
            raise ValueError(msg)
        if rc == PTV_E_NOMEM:
            raise MemoryError(msg)
        if rc == PTV_E_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == PTV_E_SINGULAR:
            raise np.linalg.LinAlgError(msg)
        if rc == PTV_E_INEXACT:
            raise InexactError(rc, msg)
        raise PtvError(rc, msg)
    return rc


def _check_knn(rc, st):
    if rc == PTV_E_INEXACT:
        raise InexactError(rc, lib().ptv_last_error().decode(errors="replace"), st.halo_required)
    check(rc)


def abi_sizes():
    """(C sizeof, ctypes sizeof) for each ABI struct: they must agree."""
    out = (C.c_int64 * 6)()
    check(lib().ptv_abi_sizes(out))
    py = [C.sizeof(Particles), C.sizeof(Grid), C.sizeof(KnnParams), C.sizeof(Stats), C.sizeof(RbfParams),
          C.sizeof(DivParams)]
    return list(out), py


def abi_sizes2():
    """(C sizeof, ctypes sizeof) of the pore-mask / filter structs."""
    out = (C.c_int64 * 3)()
    check(lib().ptv_abi_sizes2(out))
    return list(out), [C.sizeof(MaskGrid), C.sizeof(BoundaryParams), C.sizeof(FilterParams)]


def abi_sizes3():
    """(C sizeof, ctypes sizeof) of ptv_linear_params."""
    out = (C.c_int64 * 1)()
    check(lib().ptv_abi_sizes3(out))
    return list(out), [C.sizeof(LinearParams)]


def abi_sizes4():
    """(C sizeof, ctypes sizeof) of ptv_clean_params and ptv_clean_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes4(out))
    return list(out), [C.sizeof(CleanParams), C.sizeof(CleanStats)]


def abi_sizes5():
    """(C sizeof, ctypes sizeof) of ptv_variational_params and ptv_variational_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes5(out))
    return list(out), [C.sizeof(VariationalParams), C.sizeof(VariationalStats)]


def abi_sizes6():
    """(C sizeof, ctypes sizeof) of ptv_flow_params and ptv_flow_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes6(out))
    return list(out), [C.sizeof(FlowParams), C.sizeof(FlowStats)]


def abi_sizes7():
    """(C sizeof, ctypes sizeof) of ptv_drag_params and ptv_drag_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes7(out))
    return list(out), [C.sizeof(DragParams), C.sizeof(DragStats)]


def abi_sizes8():
    """(C sizeof, ctypes sizeof) of ptv_edt_params, ptv_edt_stats, ptv_align_params, ptv_align_record."""
    out = (C.c_int64 * 4)()
    check(lib().ptv_abi_sizes8(out))
    return list(out), [C.sizeof(EdtParams), C.sizeof(EdtStats), C.sizeof(AlignParams), C.sizeof(AlignRecord)]


def abi_sizes9():
    """(C sizeof, ctypes sizeof) of ptv_pressure_params and ptv_pressure_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes9(out))
    return list(out), [C.sizeof(PressureParams), C.sizeof(PressureStats)]


def abi_sizes10():
    """(C sizeof, ctypes sizeof) of ptv_spline_params, ptv_mesh_params and ptv_mesh_record."""
    out = (C.c_int64 * 3)()
    check(lib().ptv_abi_sizes10(out))
    return list(out), [C.sizeof(SplineParams), C.sizeof(MeshParams), C.sizeof(MeshRecord)]


def abi_sizes11():
    """(C sizeof, ctypes sizeof) of ptv_surface_params."""
    out = (C.c_int64 * 1)()
    check(lib().ptv_abi_sizes11(out))
    return list(out), [C.sizeof(SurfaceParams)]


def abi_sizes12():
    """(C sizeof, ctypes sizeof) of ptv_label_params and ptv_label_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes12(out))
    return list(out), [C.sizeof(LabelParams), C.sizeof(LabelStats)]


def abi_sizes13():
    """(C sizeof, ctypes sizeof) of ptv_mg_params and ptv_mg_stats."""
    out = (C.c_int64 * 2)()
    check(lib().ptv_abi_sizes13(out))
    return list(out), [C.sizeof(MgParams), C.sizeof(MgStats)]


def label_check_shape(shape):
    """The (nz, ny, nx) the labelling takes: 3-D and fewer than 2^31 voxels (``NotImplementedError``
    otherwise).  Looks at the shape alone."""
    if len(shape) != 3:
        raise NotImplementedError(f"the GPU labelling is 3-D only (got {len(shape)}-D)")
    shape = tuple(int(n) for n in shape)
    if shape[0] * shape[1] * shape[2] >= 2**31:
        raise NotImplementedError(f"shape {shape}: 2^31 or more voxels (voxel indices are 32-bit on the GPU)")
    return shape


def label_sizes_room(n_voxels):
    """Entries a ``sizes`` buffer needs before the component count is known: no mask of ``n_voxels``
    has more than ceil(n / 2) components (the 6-neighbour checkerboard), plus the background."""
    return (int(n_voxels) + 1) // 2 + 1


def edt_check_shape(shape):
    """The (nz, ny, nx) a 32-bit squared distance can hold: 3-D and nz^2 + ny^2 + nx^2 < 2^31
    (``NotImplementedError`` otherwise).  Looks at the shape alone."""
    if len(shape) != 3:
        raise NotImplementedError(f"the GPU distance transform is 3-D only (got {len(shape)}-D)")
    if sum(int(n) * int(n) for n in shape) >= 2**31:
        raise NotImplementedError(f"shape {tuple(shape)}: nz^2 + ny^2 + nx^2 must be below 2^31 "
                                  "(squared distances are 32-bit on the GPU)")
    return tuple(int(n) for n in shape)


def drag_label_table(labels):
    """The sorted unique int32 table the device takes and, per given label, its slot in it.  The
    labels must be positive integers of the int32 range (``NotImplementedError`` otherwise)."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.size == 0:
        raise ValueError("labels must be a non-empty 1-D sequence")
    if lab.dtype.kind not in "biu":
        raise NotImplementedError(f"labels of dtype {lab.dtype} (GPU path: integers or bool)")
    lab = lab.astype(np.int64) if lab.dtype != np.uint64 else lab
    if lab.max() > np.iinfo(np.int32).max or lab.min() < np.iinfo(np.int32).min:
        raise NotImplementedError("labels outside the int32 range are not supported on the GPU path")
    if lab.min() <= 0:
        raise NotImplementedError("labels must be positive on the GPU path (0 is the fluid)")
    table, slot = np.unique(lab.astype(np.int32), return_inverse=True)
    return np.ascontiguousarray(table), slot.reshape(-1)


class Triangulation:
    """The arrays of ``scipy.spatial.Delaunay(points)`` the linear kernels read, as contiguous
    int32 / float64 (``tri.transform`` is scipy's own barycentric transforms, computed on first
    access exactly as LinearNDInterpolator does).  Particles that are not vertices (Qhull
    "coplanar" points, e.g. duplicates) start their walks in the simplex Qhull assigned them."""

    def __init__(self, tri):
        self.simplices = np.ascontiguousarray(tri.simplices, dtype=np.int32)
        self.neighbors = np.ascontiguousarray(tri.neighbors, dtype=np.int32)
        self.transform = np.ascontiguousarray(tri.transform, dtype=np.float64)
        v2s = np.array(tri.vertex_to_simplex, dtype=np.int32)
        cp = np.asarray(tri.coplanar)
        if cp.size:
            v2s[cp[:, 0]] = cp[:, 1]
        self.vertex_to_simplex = np.ascontiguousarray(v2s)
        self.min_bound = [float(v) for v in tri.min_bound]
        self.max_bound = [float(v) for v in tri.max_bound]
        self.nsimplex = int(self.simplices.shape[0])

    def params(self, fill_value=0.0, fluid_mask=None, flags=0, chunk_planes=0):
        return LinearParams(self.nsimplex, self.simplices.ctypes.data_as(_i32p), self.neighbors.ctypes.data_as(_i32p),
                            as_dp(self.transform), self.vertex_to_simplex.ctypes.data_as(_i32p),
                            (C.c_double * 3)(*self.min_bound), (C.c_double * 3)(*self.max_bound), float(fill_value),
                            fluid_mask, int(flags), int(chunk_planes))


def device_count() -> int:
    n = C.c_int(0)
    check(lib().ptv_device_count(C.byref(n)))
    return n.value


def xcd_chunk_map(nblocks: int, chunk: int) -> np.ndarray:
    """The block that each dispatch slot of a k-NN launch without a block order runs (host copy of
    the kernel's map; slot lb runs on XCD lb % 8)."""
    out = np.empty(int(nblocks), dtype=np.int32)
    check(lib().ptv_xcd_chunk_map(int(nblocks), int(chunk), out.ctypes.data_as(C.POINTER(C.c_int))))
    return out


def debug_xcd_chunk(blocks: int) -> None:
    """Chunk length of that map in blocks for every later launch (0: contiguous ranges, < 0: the
    launcher's own choice).  Diagnostics and tests; results do not depend on it."""
    check(lib().ptv_debug_xcd_chunk(int(blocks)))


def as_dp(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def dev_dp(ptr: int):
    return C.cast(C.c_void_p(ptr), _dp)


class ParticleColumns:
    """The particle set as six contiguous float64 columns x, y, z, u, v, w (no copy when the
    caller's columns already are, e.g. a DataFrame's float64 block rows)."""

    def __init__(self, cols):
        cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in cols]
        if len(cols) != 6 or len({len(c) for c in cols}) != 1:
            raise ValueError("ParticleColumns: six equal-length columns x, y, z, u, v, w")
        self.cols = cols
        self.n = len(cols[0])

    @classmethod
    def from_frame(cls, df):
        """x, y, z, u, v, w of a DataFrame coerced to float64 as interpolator.py:78-79 does."""
        return cls([df[c].to_numpy(dtype=np.float64) for c in ("x", "y", "z", "u", "v", "w")])

    @property
    def points(self):
        return np.stack(self.cols[:3], 1)

    @property
    def values(self):
        return np.stack(self.cols[3:], 1)


def _columns(points, values):
    """Six contiguous float64 columns from (N, 3) points and values, or a ParticleColumns
    passed as ``points`` (``values`` None)."""
    if isinstance(points, ParticleColumns):
        return list(points.cols)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, 3)
    return [np.ascontiguousarray(pts[:, i]) for i in range(3)] + [np.ascontiguousarray(vals[:, i]) for i in range(3)]


def _into(out, res):
    """``res`` copied into the caller's ``out`` arrays (same contract as _outputs) when given."""
    if out is None:
        return res
    out = _outputs(out, res[0].shape, res[0].dtype)
    for o, r in zip(out, res):
        np.copyto(o, r)
    return tuple(out)


def _outputs(out, shape, dtype):
    """Three output arrays: the caller's (checked: C-contiguous, shape, dtype) or new ones."""
    if out is None:
        return [np.empty(shape, dtype=dtype) for _ in range(3)]
    out = list(out)
    for a in out:
        if a.shape != tuple(shape) or a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"out arrays must be writeable C-contiguous {dtype} of shape {tuple(shape)}")
    return out


def _flat_tiles(gp, shape, fluid_mask, z_range):
    """A flat point list (shape (1, 1, n)) as a (npad / 64, 4, 16) point grid, padded with
    the last point: the k-NN kernels tile 4 x 4 x 4 (x, y, z) blocks of the shape, so a
    (1, 1, n) list would keep only 4 of a wave's 64 lanes busy.  Every query is independent,
    so the results are the same; returns (gp, shape, mask, unpad) or None."""
    nz, ny, nx = shape
    if nz != 1 or ny != 1 or z_range is not None or nx < 64:
        return None
    n = nx
    npad = (n + 255) // 256 * 256
    ext = [np.concatenate([a, np.full(npad - n, a[-1])]) if npad > n else a for a in gp]
    mk = None
    if fluid_mask is not None:
        m = np.ascontiguousarray(fluid_mask, dtype=np.uint8).ravel()
        mk = np.concatenate([m, np.zeros(npad - n, dtype=np.uint8)]) if npad > n else m
    return ext, (npad // 64, 4, 16), mk, (lambda a: a.reshape(-1)[:n].reshape(shape))


class Context:
    """One device context (stream + reusable device buffers)."""

    _cache = {}

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        check(L.ptv_init(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)

    @classmethod
    def get(cls, device: int = 0) -> "Context":
        with _lock:
            ctx = cls._cache.get(device)
        if ctx is None:
            ctx = cls(device)
            with _lock:
                cls._cache[device] = ctx
        return ctx

    def close(self):
        if self.h:
            lib().ptv_free(self.h)
            self.h = None

    def last_stats(self) -> dict:
        st = Stats()
        check(lib().ptv_last_stats(self.h, C.byref(st)))
        return st.as_dict()

    def debug_stamps(self, mode=2):
        """mode 1: enable+zero, 0: disable, 2: read.  Per-wave phase cycles (mean / max)."""
        out = (C.c_double * 23)()
        check(lib().ptv_debug_stamps(self.h, int(mode), out))
        keys = ("setup", "seeds", "rows", "copy", "compute", "epilogue", "candidates", "merges", "rounds",
                "passes", "kept")
        v = list(out)
        return {"waves": v[0], "mean": dict(zip(keys, v[1:12])), "max": dict(zip(keys, v[12:23]))}

    def debug_xcd_stamps(self, waves=1 << 21):
        """(waves, 3) uint64 of the stamped launch, in dispatch order: XCD, first and last value of
        the device's 100 MHz real-time clock; both 0 for a wave that wrote nothing."""
        out = np.zeros((int(waves), 3), dtype=np.uint64)
        n = C.c_longlong(0)
        check(lib().ptv_debug_xcd_stamps(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(waves), C.byref(n)))
        return out[:n.value]

    # -- pore-mask path and outlier filter -------
    def sample_mask(self, raw, raw_axes, axes=None, grid_points=None, shape=None, z_range=None):
        """Nearest resampling of a raw byte mask (1 = value > 0.5) onto a grid -> uint8 (nz', ny, nx).

        raw: (rnz, rny, rnx) bytes; raw_axes: (x, y, z) raw voxel coordinates (host)."""
        rw = np.ascontiguousarray(raw, dtype=np.uint8)
        rnz, rny, rnx = rw.shape
        rax, ray, raz = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in raw_axes)
        M = MaskGrid(rnx, rny, rnz, rw.ctypes.data_as(_u8p), as_dp(rax), as_dp(ray), as_dp(raz))
        keep = [rw, rax, ray, raz]
        if axes is not None:
            ax, ay, az = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in axes)
            nx, ny, nz = len(ax), len(ay), len(az)
            keep += [ax, ay, az]
            G = Grid(nx, ny, nz, as_dp(ax), as_dp(ay), as_dp(az), None, None, None, 0, nz)
        else:
            nz, ny, nx = shape
            gp = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in grid_points]
            keep += gp
            G = Grid(nx, ny, nz, None, None, None, as_dp(gp[0]), as_dp(gp[1]), as_dp(gp[2]), 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        out = np.empty((z1 - z0, ny, nx), dtype=np.uint8)
        check(lib().ptv_sample_mask(self.h, C.byref(M), C.byref(G), out.ctypes.data_as(_u8p)))
        return out

    def boundary_particles(self, mask_bytes, encoding, thickness, step, lo, span, den):
        """Boundary voxel coordinates (x, y, z) float64 arrays; mask_bytes (nz, ny, nx) uint8."""
        mb = np.ascontiguousarray(mask_bytes, dtype=np.uint8)
        nz, ny, nx = mb.shape
        prm = BoundaryParams(nx, ny, nz, mb.ctypes.data_as(_u8p), int(encoding), int(thickness), int(step),
                             (C.c_double * 3)(*lo), (C.c_double * 3)(*span), (C.c_double * 3)(*den))
        cnt = C.c_int64(0)
        check(lib().ptv_boundary_particles(self.h, C.byref(prm), None, None, None, 0, C.byref(cnt)))
        n = cnt.value
        out = [np.empty(n, dtype=np.float64) for _ in range(3)]
        if n > 0:
            check(lib().ptv_boundary_particles(self.h, C.byref(prm), as_dp(out[0]), as_dp(out[1]),
                                               as_dp(out[2]), n, C.byref(cnt)))
        return tuple(out)

    def filter_outliers_knn(self, points, values, k=25, threshold=3.0, mad_eps=1e-6):
        """(keep uint8 (n,), kth_dist float64 (n,)) of the median/MAD k-NN filter."""
        cols = _columns(points, values)
        P = Particles(len(cols[0]), *[as_dp(c) for c in cols])
        prm = FilterParams(int(k), float(threshold), float(mad_eps))
        keep = np.empty(len(cols[0]), dtype=np.uint8)
        kth = np.empty(len(cols[0]), dtype=np.float64)
        st = Stats()
        check(lib().ptv_filter_outliers_knn(self.h, C.byref(P), C.byref(prm), keep.ctypes.data_as(_u8p),
                                            as_dp(kth), C.byref(st)))
        self.stats = st.as_dict()
        return keep, kth

    # device-pointer variants (bench.py: inputs resident in HBM)
    def sample_mask_dev(self, raw_ptr, raw_shape, raw_axes, axes_ptrs, shape, out_ptr, stream=None):
        """raw_ptr: device (rnz, rny, rnx) bytes; raw_axes: host arrays; axes_ptrs: device grid axes."""
        rnz, rny, rnx = raw_shape
        rax, ray, raz = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in raw_axes)
        M = MaskGrid(rnx, rny, rnz, C.cast(C.c_void_p(raw_ptr), _u8p), as_dp(rax), as_dp(ray), as_dp(raz))
        nz, ny, nx = shape
        G = Grid(nx, ny, nz, dev_dp(axes_ptrs[0]), dev_dp(axes_ptrs[1]), dev_dp(axes_ptrs[2]), None, None, None,
                 0, nz)
        check(lib().ptv_sample_mask_dev(self.h, C.byref(M), C.byref(G), C.cast(C.c_void_p(out_ptr), _u8p),
                                        C.c_void_p(stream) if stream else None))

    def boundary_particles_dev(self, mask_ptr, shape, thickness, step, lo, span, den, out_ptrs=None, cap=0,
                               stream=None, encoding=MASK_BOOL):
        """Returns the particle count; writes device x, y, z when out_ptrs is given and cap suffices."""
        nz, ny, nx = shape
        prm = BoundaryParams(nx, ny, nz, C.cast(C.c_void_p(mask_ptr), _u8p), int(encoding), int(thickness),
                             int(step), (C.c_double * 3)(*lo), (C.c_double * 3)(*span), (C.c_double * 3)(*den))
        cnt = C.c_int64(0)
        o = [dev_dp(p) for p in out_ptrs] if out_ptrs else [None, None, None]
        check(lib().ptv_boundary_particles_dev(self.h, C.byref(prm), o[0], o[1], o[2], int(cap), C.byref(cnt),
                                               C.c_void_p(stream) if stream else None))
        return cnt.value

    def filter_outliers_knn_dev(self, n, col_ptrs, keep_ptr, kth_ptr, k=25, threshold=3.0, mad_eps=1e-6,
                                stream=None):
        """col_ptrs: six device float64 columns x, y, z, u, v, w."""
        P = Particles(int(n), *[dev_dp(p) for p in col_ptrs])
        prm = FilterParams(int(k), float(threshold), float(mad_eps))
        st = Stats()
        check(lib().ptv_filter_outliers_knn_dev(self.h, C.byref(P), C.byref(prm),
                                                C.cast(C.c_void_p(keep_ptr), _u8p),
                                                dev_dp(kth_ptr) if kth_ptr else None,
                                                C.c_void_p(stream) if stream else None, C.byref(st)))
        return st.as_dict()

    # -- host buffers ------------------------------------------------------
    def interp_knn(self, points, values, axes=None, grid_points=None, shape=None, method=METHOD_IDW, k=8,
                   power=2.0, eps=1e-10, fluid_mask=None, flags=0, z_range=None, cell_occupancy=0.0,
                   r0_scale=0.0, lattice_bounds=0, slab_halo=0.0, out=None, radius=0.0):
        """Host-array k-NN interpolation. Returns (U, V, W) float64 (nz', ny, nx).

        ``out``: optional three C-contiguous (nz', ny, nx) arrays of the output dtype (e.g.
        z-slices of the caller's full arrays) written in place by the D2H."""
        cols = _columns(points, values)
        P = Particles(len(cols[0]), *[as_dp(c) for c in cols])
        keep = list(cols)
        if axes is not None:
            ax, ay, az = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in axes)
            nx, ny, nz = len(ax), len(ay), len(az)
            keep += [ax, ay, az]
            G = Grid(nx, ny, nz, as_dp(ax), as_dp(ay), as_dp(az), None, None, None, 0, nz)
        else:
            gp = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in grid_points]
            ft = _flat_tiles(gp, shape, fluid_mask, z_range)
            if ft is not None:
                gp, tshape, fm, unpad = ft
                res = self.interp_knn(points, values, grid_points=gp, shape=tshape, method=method, k=k,
                                      power=power, eps=eps, fluid_mask=fm, flags=flags,
                                      cell_occupancy=cell_occupancy, r0_scale=r0_scale,
                                      lattice_bounds=lattice_bounds, slab_halo=slab_halo, radius=radius)
                return _into(out, tuple(unpad(a) for a in res))
            nz, ny, nx = shape
            keep += gp
            G = Grid(nx, ny, nz, None, None, None, as_dp(gp[0]), as_dp(gp[1]), as_dp(gp[2]), 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        mk = None
        if fluid_mask is not None:
            mk = np.ascontiguousarray(fluid_mask, dtype=np.uint8).reshape(nz, ny, nx)
            keep.append(mk)
        prm = KnnParams(method, int(k), float(power), float(eps),
                        mk.ctypes.data_as(C.POINTER(C.c_uint8)) if mk is not None else None, flags,
                        float(cell_occupancy), float(r0_scale), int(lattice_bounds), float(slab_halo),
                        float(radius))
        odt = np.float32 if flags & FLAG_OUT_F32 else np.float64
        out = _outputs(out, (z1 - z0, ny, nx), odt)
        st = Stats()
        rc = lib().ptv_interp_knn(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                  as_dp(out[0]), as_dp(out[1]), as_dp(out[2]), C.byref(st))
        self.stats = st.as_dict()
        _check_knn(rc, st)
        return tuple(out)

    def interp_rbf(self, points, values, axes=None, grid_points=None, shape=None, k=20,
                   kernel="thin_plate_spline", epsilon=1.0, degree=1, smoothing=0.0, fluid_mask=None, flags=0,
                   z_range=None, chunk_planes=0, out=None):
        """Host-array local RBF (scipy RBFInterpolator(neighbors=k) semantics; the arguments are
        already resolved by ptv_interpolation_amd.rbf).  ``smoothing``: scalar or (n,) array.
        Returns (U, V, W) float64 (nz', ny, nx)."""
        cols = _columns(points, values)
        P = Particles(len(cols[0]), *[as_dp(c) for c in cols])
        keep = list(cols)
        if axes is not None:
            ax, ay, az = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in axes)
            nx, ny, nz = len(ax), len(ay), len(az)
            keep += [ax, ay, az]
            G = Grid(nx, ny, nz, as_dp(ax), as_dp(ay), as_dp(az), None, None, None, 0, nz)
        else:
            gp = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in grid_points]
            ft = _flat_tiles(gp, shape, fluid_mask, z_range)
            if ft is not None:
                gp, tshape, fm, unpad = ft
                res = self.interp_rbf(points, values, grid_points=gp, shape=tshape, k=k, kernel=kernel,
                                      epsilon=epsilon, degree=degree, smoothing=smoothing, fluid_mask=fm,
                                      flags=flags, chunk_planes=chunk_planes)
                return _into(out, tuple(unpad(a) for a in res))
            nz, ny, nx = shape
            keep += gp
            G = Grid(nx, ny, nz, None, None, None, as_dp(gp[0]), as_dp(gp[1]), as_dp(gp[2]), 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        mk = None
        if fluid_mask is not None:
            mk = np.ascontiguousarray(fluid_mask, dtype=np.uint8).reshape(nz, ny, nx)
            keep.append(mk)
        sm_arr = None
        if np.ndim(smoothing) > 0:
            sm_arr = np.ascontiguousarray(smoothing, dtype=np.float64).ravel()
            keep.append(sm_arr)
        prm = RbfParams(int(k), RBF_KERNELS[kernel], float(epsilon), int(degree),
                        0.0 if sm_arr is not None else float(smoothing),
                        as_dp(sm_arr) if sm_arr is not None else None,
                        mk.ctypes.data_as(C.POINTER(C.c_uint8)) if mk is not None else None, int(flags),
                        int(chunk_planes))
        out = _outputs(out, (z1 - z0, ny, nx), np.float64)
        st = Stats()
        check(lib().ptv_interp_rbf_local(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                         as_dp(out[0]), as_dp(out[1]), as_dp(out[2]), C.byref(st)))
        self.stats = st.as_dict()
        return tuple(out)

    def interp_linear(self, points, values, tri, axes=None, grid_points=None, shape=None, fill_value=0.0,
                      fluid_mask=None, flags=0, z_range=None, chunk_planes=0, out=None):
        """Host-array linear (Delaunay) interpolation (griddata(method='linear') semantics) over
        ``tri`` (a Triangulation of these points).  Returns (U, V, W) float64 (nz', ny, nx)."""
        cols = _columns(points, values)
        P = Particles(len(cols[0]), *[as_dp(c) for c in cols])
        keep = list(cols)
        if axes is not None:
            ax, ay, az = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in axes)
            nx, ny, nz = len(ax), len(ay), len(az)
            keep += [ax, ay, az]
            G = Grid(nx, ny, nz, as_dp(ax), as_dp(ay), as_dp(az), None, None, None, 0, nz)
        else:
            gp = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in grid_points]
            ft = _flat_tiles(gp, shape, fluid_mask, z_range)
            if ft is not None:
                gp, tshape, fm, unpad = ft
                res = self.interp_linear(points, values, tri, grid_points=gp, shape=tshape, fill_value=fill_value,
                                         fluid_mask=fm, flags=flags, chunk_planes=chunk_planes)
                return _into(out, tuple(unpad(a) for a in res))
            nz, ny, nx = shape
            keep += gp
            G = Grid(nx, ny, nz, None, None, None, as_dp(gp[0]), as_dp(gp[1]), as_dp(gp[2]), 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        mk = None
        if fluid_mask is not None:
            mk = np.ascontiguousarray(fluid_mask, dtype=np.uint8).reshape(nz, ny, nx)
            keep.append(mk)
        prm = tri.params(fill_value, mk.ctypes.data_as(C.POINTER(C.c_uint8)) if mk is not None else None, flags,
                         chunk_planes)
        out = _outputs(out, (z1 - z0, ny, nx), np.float64)
        st = Stats()
        check(lib().ptv_interp_linear(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                      as_dp(out[0]), as_dp(out[1]), as_dp(out[2]), C.byref(st)))
        self.stats = st.as_dict()
        return tuple(out)

    def interp_linear_dev(self, n, pptrs, nx, ny, nz, tri_ptrs, nsimplex, min_bound, max_bound, axes_ptrs=None,
                          point_ptrs=None, out_ptrs=None, fill_value=0.0, mask_ptr=0, flags=0, z_range=None,
                          stream=0, chunk_planes=0):
        """Device-pointer linear interpolation; tri_ptrs: device (simplices, neighbors, transform,
        vertex_to_simplex).  Returns the call's stats."""
        P = Particles(int(n), *[dev_dp(p) for p in pptrs])
        if axes_ptrs is not None:
            G = Grid(nx, ny, nz, *[dev_dp(p) for p in axes_ptrs], None, None, None, 0, nz)
        else:
            G = Grid(nx, ny, nz, None, None, None, *[dev_dp(p) for p in point_ptrs], 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        i32 = lambda p: C.cast(C.c_void_p(p), _i32p)
        prm = LinearParams(int(nsimplex), i32(tri_ptrs[0]), i32(tri_ptrs[1]), dev_dp(tri_ptrs[2]), i32(tri_ptrs[3]),
                           (C.c_double * 3)(*min_bound), (C.c_double * 3)(*max_bound), float(fill_value),
                           C.cast(C.c_void_p(mask_ptr), C.POINTER(C.c_uint8)) if mask_ptr else None, int(flags),
                           int(chunk_planes))
        st = Stats()
        check(lib().ptv_interp_linear_dev(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                          *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream) if stream else None,
                                          C.byref(st)))
        return st.as_dict()

    def interp_rbf_dev(self, n, pptrs, nx, ny, nz, axes_ptrs=None, point_ptrs=None, out_ptrs=None, k=20,
                       kernel="thin_plate_spline", epsilon=1.0, degree=1, smoothing=0.0, smoothing_ptr=0,
                       mask_ptr=0, flags=0, z_range=None, stream=0, chunk_planes=0):
        """Device-pointer local RBF (inputs resident in HBM); returns the call's stats."""
        P = Particles(int(n), *[dev_dp(p) for p in pptrs])
        if axes_ptrs is not None:
            G = Grid(nx, ny, nz, *[dev_dp(p) for p in axes_ptrs], None, None, None, 0, nz)
        else:
            G = Grid(nx, ny, nz, None, None, None, *[dev_dp(p) for p in point_ptrs], 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        prm = RbfParams(int(k), RBF_KERNELS[kernel], float(epsilon), int(degree), float(smoothing),
                        dev_dp(smoothing_ptr) if smoothing_ptr else None,
                        C.cast(C.c_void_p(mask_ptr), C.POINTER(C.c_uint8)) if mask_ptr else None, int(flags),
                        int(chunk_planes))
        st = Stats()
        check(lib().ptv_interp_rbf_local_dev(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                             *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream or 0),
                                             C.byref(st)))
        return st.as_dict()

    # -- device buffers (integer device pointers, e.g. torch tensor data_ptr()) --
    def interp_knn_dev(self, n, pptrs, nx, ny, nz, axes_ptrs=None, point_ptrs=None, out_ptrs=None,
                       method=METHOD_IDW, k=8, power=2.0, eps=1e-10, mask_ptr=0, flags=0, z_range=None,
                       stream=0, cell_occupancy=0.0, r0_scale=0.0, lattice_bounds=0, slab_halo=0.0, radius=0.0):
        """Device-pointer k-NN interpolation (inputs resident in HBM), enqueued on `stream`;
        returns the call's stats.  ``slab_halo`` > 0: see ptv_knn_params.slab_halo (raises
        InexactError carrying ``halo_required`` when the halo is too small)."""
        P = Particles(int(n), *[dev_dp(p) for p in pptrs])
        if axes_ptrs is not None:
            G = Grid(nx, ny, nz, *[dev_dp(p) for p in axes_ptrs], None, None, None, 0, nz)
        else:
            G = Grid(nx, ny, nz, None, None, None, *[dev_dp(p) for p in point_ptrs], 0, nz)
        z0, z1 = (0, nz) if z_range is None else z_range
        G.z_begin, G.z_end = z0, z1
        prm = KnnParams(method, int(k), float(power), float(eps),
                        C.cast(C.c_void_p(mask_ptr), C.POINTER(C.c_uint8)) if mask_ptr else None, flags,
                        float(cell_occupancy), float(r0_scale), int(lattice_bounds), float(slab_halo),
                        float(radius))
        st = Stats()
        rc = lib().ptv_interp_knn_dev(self.h, C.byref(P), C.byref(G), C.byref(prm),
                                      *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream or 0), C.byref(st))
        _check_knn(rc, st)
        return st.as_dict()

    # -- consistent divergence (physics.py:6-53) ---------------------------
    def divergence(self, u, v, w, fluid_mask, dx, dy, dz, result_dtype=None, z_range=None, edges=(True, True)):
        """Host-array divergence of (nz, ny, nx) fields; returns (z1 - z0, ny, nx) of
        ``result_dtype`` (default: the fields' dtype).  ``edges``: whether buffer plane 0 /
        nz-1 is a domain edge (else a halo plane, read but not computed)."""
        ft = np.result_type(u.dtype, v.dtype, w.dtype)
        if ft not in (np.float32, np.float64):
            ft = np.dtype(np.float64)
        rt = np.dtype(result_dtype) if result_dtype is not None else np.dtype(ft)
        f = [np.ascontiguousarray(a, dtype=ft) for a in (u, v, w)]
        nz, ny, nx = f[0].shape
        mk = np.ascontiguousarray(fluid_mask, dtype=bool).view(np.uint8).reshape(nz, ny, nx)
        z0, z1 = (0, nz) if z_range is None else z_range
        prm = DivParams(nx, ny, nz, z0, z1, int(bool(edges[0])), int(bool(edges[1])),
                        F32 if ft == np.float32 else F64, F32 if rt == np.float32 else F64,
                        float(dx), float(dy), float(dz), mk.ctypes.data_as(C.POINTER(C.c_uint8)))
        out = np.empty((z1 - z0, ny, nx), dtype=rt)
        st = Stats()
        check(lib().ptv_divergence(self.h, C.byref(prm), *[a.ctypes.data_as(C.c_void_p) for a in f],
                                   out.ctypes.data_as(C.c_void_p), C.byref(st)))
        self.stats = st.as_dict()
        return out

    def divergence_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptr, dx, dy, dz, field_dtype=F64, result_dtype=F64,
                       z_range=None, edges=(True, True), stream=0):
        """Device-pointer divergence (fields, mask and output resident in HBM); returns stats."""
        z0, z1 = (0, nz) if z_range is None else z_range
        prm = DivParams(nx, ny, nz, z0, z1, int(bool(edges[0])), int(bool(edges[1])), int(field_dtype),
                        int(result_dtype), float(dx), float(dy), float(dz),
                        C.cast(C.c_void_p(mask_ptr), C.POINTER(C.c_uint8)) if mask_ptr else None)
        st = Stats()
        check(lib().ptv_divergence_dev(self.h, C.byref(prm), *[C.c_void_p(p) for p in ptrs], C.c_void_p(out_ptr),
                                       C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    # -- divergence cleaning, projection method (physics.py:55-209) --------
    @staticmethod
    def _clean_params(shape, fluid_mask, dx, dy, dz, iterations=0, damp=0.0, atol=0.0, btol=0.0, iter_lim=0):
        nz, ny, nx = shape
        mk = np.ascontiguousarray(fluid_mask, dtype=bool).view(np.uint8).reshape(nz, ny, nx)
        prm = CleanParams(nx, ny, nz, float(dx), float(dy), float(dz), mk.ctypes.data_as(_u8p), int(iterations),
                          float(damp), float(atol), float(btol), int(iter_lim))
        return prm, mk  # mk keeps the mask bytes alive for the call

    def clean_divergence(self, u, v, w, fluid_mask, dx, dy, dz, iterations=3, damp=1e-8, atol=1e-10, btol=1e-10,
                         iter_lim=3000):
        """Projection-method cleaning of float64 (nz, ny, nx) host fields (physics.py:149-209 with its
        lsqr arguments as defaults); returns ``((u_c, v_c, w_c), stats dict)``."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w)]
        prm, _mk = self._clean_params(f[0].shape, fluid_mask, dx, dy, dz, iterations, damp, atol, btol, iter_lim)
        out = [np.empty_like(a) for a in f]
        st = CleanStats()
        check(lib().ptv_clean_divergence(self.h, C.byref(prm), *[as_dp(a) for a in f], *[as_dp(a) for a in out],
                                         C.byref(st)))
        return tuple(out), st.as_dict()

    def clean_divergence_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptrs, dx, dy, dz, iterations=3, damp=1e-8,
                             atol=1e-10, btol=1e-10, iter_lim=3000, stream=0):
        """Device-pointer cleaning (float64 fields, uint8 mask and outputs resident in HBM; the outputs
        may be the inputs); returns the stats dict."""
        prm = CleanParams(nx, ny, nz, float(dx), float(dy), float(dz), C.cast(C.c_void_p(mask_ptr), _u8p),
                          int(iterations), float(damp), float(atol), float(btol), int(iter_lim))
        st = CleanStats()
        check(lib().ptv_clean_divergence_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs],
                                             *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def apply_correction(self, u, v, w, phi_grid, fluid_mask, dx, dy, dz):
        """physics.py:110-147 with phi on the grid; float64 (nz, ny, nx) host arrays."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w, phi_grid)]
        prm, _mk = self._clean_params(f[0].shape, fluid_mask, dx, dy, dz)
        out = [np.empty_like(a) for a in f[:3]]
        check(lib().ptv_apply_correction(self.h, C.byref(prm), *[as_dp(a) for a in f], *[as_dp(a) for a in out]))
        return tuple(out)

    def laplacian_apply(self, x_grid, fluid_mask, dx, dy, dz):
        """``A @ x`` for the masked Laplacian of physics.py:55-108, x and the result on the grid."""
        x = np.ascontiguousarray(x_grid, dtype=np.float64)
        prm, _mk = self._clean_params(x.shape, fluid_mask, dx, dy, dz)
        y = np.empty_like(x)
        check(lib().ptv_laplacian_apply(self.h, C.byref(prm), as_dp(x), as_dp(y)))
        return y

    # -- divergence cleaning, variational method (physics.py:356-514) ------
    @staticmethod
    def _variational_params(shape, fluid_mask, dx, dy, dz, lambda_reg=0.0, rtol=0.0, maxiter=0):
        nz, ny, nx = shape
        mk = np.ascontiguousarray(fluid_mask, dtype=bool).view(np.uint8).reshape(nz, ny, nx)
        prm = VariationalParams(nx, ny, nz, float(dx), float(dy), float(dz), mk.ctypes.data_as(_u8p),
                                float(lambda_reg), float(rtol), int(maxiter))
        return prm, mk  # mk keeps the mask bytes alive for the call

    def clean_variational(self, u, v, w, fluid_mask, dx, dy, dz, lambda_reg=1e3, rtol=1e-8, maxiter=2000):
        """Variational cleaning of float64 (nz, ny, nx) host fields (physics.py:440-514 with its cg
        arguments as defaults); returns ``((u_c, v_c, w_c), stats dict)``."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w)]
        prm, _mk = self._variational_params(f[0].shape, fluid_mask, dx, dy, dz, lambda_reg, rtol, maxiter)
        out = [np.empty_like(a) for a in f]
        st = VariationalStats()
        check(lib().ptv_clean_variational(self.h, C.byref(prm), *[as_dp(a) for a in f], *[as_dp(a) for a in out],
                                          C.byref(st)))
        return tuple(out), st.as_dict()

    def clean_variational_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptrs, dx, dy, dz, lambda_reg=1e3, rtol=1e-8,
                              maxiter=2000, stream=0):
        """Device-pointer variational cleaning (float64 fields, uint8 mask and outputs resident in HBM;
        the outputs may be the inputs); returns the stats dict."""
        prm = VariationalParams(nx, ny, nz, float(dx), float(dy), float(dz), C.cast(C.c_void_p(mask_ptr), _u8p),
                                float(lambda_reg), float(rtol), int(maxiter))
        st = VariationalStats()
        check(lib().ptv_clean_variational_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs],
                                              *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def variational_apply(self, xu, xv, xw, fluid_mask, dx, dy, dz, lambda_reg):
        """``A @ x`` for A = I + lambda D^T D of physics.py:460-480, x and the result on the grid."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (xu, xv, xw)]
        prm, _mk = self._variational_params(f[0].shape, fluid_mask, dx, dy, dz, lambda_reg)
        out = [np.empty_like(a) for a in f]
        check(lib().ptv_variational_apply(self.h, C.byref(prm), *[as_dp(a) for a in f], *[as_dp(a) for a in out]))
        return tuple(out)

    def divergence_operator_apply(self, xu, xv, xw, fluid_mask, dx, dy, dz):
        """``Dx @ xu + Dy @ xv + Dz @ xw`` for the operators of physics.py:356-438, on the grid."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (xu, xv, xw)]
        prm, _mk = self._variational_params(f[0].shape, fluid_mask, dx, dy, dz)
        d = np.empty_like(f[0])
        check(lib().ptv_divergence_operator_apply(self.h, C.byref(prm), *[as_dp(a) for a in f], as_dp(d)))
        return d

    # -- flow analysis (velocity_analysis.py:10-188) ------------------------
    def flow_analysis(self, u, v, w, dx, dy, dz, viscosity=0.0, fluid_mask=None, outputs=FLOW_OUTPUTS,
                      spacing_strong=False, z_range=None, edges=(True, True)):
        """One stencil pass over float32 / float64 (nz, ny, nx) host fields of one dtype.  Returns
        ``(fields, stats)``: a dict with the requested ``outputs`` (names of FLOW_OUTPUTS), each
        (z1 - z0, ny, nx) of the fields' dtype, and the statistics dict.  ``spacing_strong``: numpy's
        division rule for float32 fields (np.float64 spacings); ``z_range`` / ``edges`` as
        ``divergence``."""
        ft = u.dtype
        f = [np.ascontiguousarray(a, dtype=ft) for a in (u, v, w)]
        nz, ny, nx = f[0].shape
        mk = None
        if fluid_mask is not None:
            mk = np.ascontiguousarray(fluid_mask, dtype=bool).view(np.uint8).reshape(nz, ny, nx)
        z0, z1 = (0, nz) if z_range is None else z_range
        prm = FlowParams(nx, ny, nz, z0, z1, int(bool(edges[0])), int(bool(edges[1])),
                         F32 if ft == np.float32 else F64, int(bool(spacing_strong)), float(dx), float(dy),
                         float(dz), float(viscosity), mk.ctypes.data_as(_u8p) if mk is not None else None)
        out = {name: np.empty((max(z1 - z0, 0), ny, nx), dtype=ft) for name in FLOW_OUTPUTS if name in outputs}
        st = FlowStats()
        check(lib().ptv_flow_analysis(self.h, C.byref(prm), *[a.ctypes.data_as(C.c_void_p) for a in f],
                                      *[out[n].ctypes.data_as(C.c_void_p) if n in out else None
                                        for n in FLOW_OUTPUTS], C.byref(st)))
        return out, st.as_dict()

    def flow_analysis_dev(self, nx, ny, nz, ptrs, out_ptrs, dx, dy, dz, viscosity=0.0, mask_ptr=0, field_dtype=F64,
                          spacing_strong=False, z_range=None, edges=(True, True), stream=0):
        """Device-pointer flow analysis (fields, mask and outputs resident in HBM).  ``out_ptrs``: four
        device pointers in FLOW_OUTPUTS order, 0 = not computed.  Returns the statistics dict."""
        z0, z1 = (0, nz) if z_range is None else z_range
        prm = FlowParams(nx, ny, nz, z0, z1, int(bool(edges[0])), int(bool(edges[1])), int(field_dtype),
                         int(bool(spacing_strong)), float(dx), float(dy), float(dz), float(viscosity),
                         C.cast(C.c_void_p(mask_ptr), _u8p) if mask_ptr else None)
        st = FlowStats()
        check(lib().ptv_flow_analysis_dev(self.h, C.byref(prm), *[C.c_void_p(p) for p in ptrs],
                                          *[C.c_void_p(p) if p else None for p in out_ptrs],
                                          C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def flow_derived(self, strain_rate, vorticity_mag=None, viscosity=0.0, fluid_mask=None,
                     outputs=("dissipation", "flow_type")):
        """The elementwise mode: dissipation and / or flow type of host S (and O) arrays of one
        float32 / float64 dtype and any one shape.  Returns ``(fields, stats)`` as flow_analysis."""
        ft = strain_rate.dtype
        s = np.ascontiguousarray(strain_rate, dtype=ft)
        o = np.ascontiguousarray(vorticity_mag, dtype=ft) if "flow_type" in outputs else None
        mk = None
        if fluid_mask is not None:
            mk = np.ascontiguousarray(fluid_mask, dtype=bool).view(np.uint8)
        nx, ny, nz = s.shape[::-1] if s.ndim == 3 else (s.size, 1, 1)
        prm = FlowParams(nx, ny, nz, 0, nz, 1, 1, F32 if ft == np.float32 else F64, 0, 1.0, 1.0, 1.0,
                         float(viscosity), mk.ctypes.data_as(_u8p) if mk is not None else None)
        out = {name: np.empty(s.shape, dtype=ft) for name in ("dissipation", "flow_type") if name in outputs}
        st = FlowStats()
        check(lib().ptv_flow_derived(self.h, C.byref(prm), s.ctypes.data_as(C.c_void_p),
                                     o.ctypes.data_as(C.c_void_p) if o is not None else None,
                                     *[out[n].ctypes.data_as(C.c_void_p) if n in out else None
                                       for n in ("dissipation", "flow_type")], C.byref(st)))
        return out, st.as_dict()

    def flow_derived_dev(self, n, strain_ptr, vorticity_ptr, dissipation_ptr, flow_type_ptr, viscosity=0.0,
                         mask_ptr=0, field_dtype=F64, stream=0):
        """Device-pointer elementwise mode over ``n`` voxels; a 0 output pointer = not computed."""
        prm = FlowParams(int(n), 1, 1, 0, 1, 1, 1, int(field_dtype), 0, 1.0, 1.0, 1.0, float(viscosity),
                         C.cast(C.c_void_p(mask_ptr), _u8p) if mask_ptr else None)
        st = FlowStats()
        check(lib().ptv_flow_derived_dev(self.h, C.byref(prm), C.c_void_p(strain_ptr),
                                         C.c_void_p(vorticity_ptr) if vorticity_ptr else None,
                                         C.c_void_p(dissipation_ptr) if dissipation_ptr else None,
                                         C.c_void_p(flow_type_ptr) if flow_type_ptr else None,
                                         C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    # -- interface drag, gradient sums (velocity_analysis.py:332-511, :659-697) ----
    def _drag_call(self, fn, shape, ptrs, labels, dx, dy, dz, viscosity, field_dtype, extra=()):
        table, slot = drag_label_table(labels)
        nz, ny, nx = shape
        prm = DragParams(nx, ny, nz, int(field_dtype), int(table.size), float(dx), float(dy), float(dz),
                         float(viscosity), table.ctypes.data_as(C.POINTER(C.c_int32)))
        rec = np.zeros((table.size, 3, 2), dtype=DRAG_RECORD)
        ms = C.c_double(0.0)
        check(fn(self.h, C.byref(prm), *[C.c_void_p(p) if p else None for p in ptrs], *extra,
                 rec.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return rec[slot], ms.value

    def interface_drag(self, mask, u, v, w, pressure, viscosity, dx, dy, dz, labels):
        """Staircase interface drag of host arrays: an integer / bool label ``mask`` (nz, ny, nx), the
        fields (one float32 / float64 dtype; ``pressure`` may be None).  ``labels``: positive
        integers in any order, repeats allowed.  Returns ``(records, ms)``: a (len(labels), 3, 2)
        array of DRAG_RECORD, one per given label, axis (0 = z, 1 = y, 2 = x) and direction (0 = A,
        fluid -> label; 1 = B), and the kernels' time."""
        ft = u.dtype
        mk = np.ascontiguousarray(mask, dtype=np.int32)
        f = [np.ascontiguousarray(a, dtype=ft) for a in (u, v, w)]
        if pressure is not None:
            f.append(np.ascontiguousarray(pressure, dtype=ft))
        ptrs = [mk.ctypes.data] + [a.ctypes.data for a in f] + [0] * (4 - len(f))
        return self._drag_call(lib().ptv_interface_drag, mk.shape, ptrs, labels, dx, dy, dz, viscosity,
                               F32 if ft == np.float32 else F64)

    def interface_drag_dev(self, nx, ny, nz, mask_ptr, ptrs, pressure_ptr, viscosity, dx, dy, dz, labels,
                           field_dtype=F64, stream=0):
        """Device-pointer interface drag: an int32 mask, u, v, w (``ptrs``) and the pressure (0 = none)
        resident in HBM; the labels and the records stay on the host.  Returns as interface_drag."""
        return self._drag_call(lib().ptv_interface_drag_dev, (nz, ny, nx), [mask_ptr, *ptrs, pressure_ptr], labels,
                               dx, dy, dz, viscosity, field_dtype, extra=(C.c_void_p(stream or 0),))

    def gradient_sums(self, pressure, dx, dy, dz, spacing_strong=False):
        """The float64 sums over the volume of ``np.gradient(pressure, dz, dy, dx)``'s three components,
        in that order, for a host float32 / float64 (nz, ny, nx) array."""
        p = np.ascontiguousarray(pressure)
        nz, ny, nx = p.shape
        prm = FlowParams(nx, ny, nz, 0, nz, 1, 1, F32 if p.dtype == np.float32 else F64, int(bool(spacing_strong)),
                         float(dx), float(dy), float(dz), 0.0, None)
        out = (C.c_double * 3)()
        check(lib().ptv_gradient_sums(self.h, C.byref(prm), p.ctypes.data_as(C.c_void_p), out))
        return [float(x) for x in out]

    def gradient_sums_dev(self, nx, ny, nz, ptr, dx, dy, dz, field_dtype=F64, spacing_strong=False, stream=0):
        """The same for a field resident in HBM."""
        prm = FlowParams(nx, ny, nz, 0, nz, 1, 1, int(field_dtype), int(bool(spacing_strong)), float(dx), float(dy),
                         float(dz), 0.0, None)
        out = (C.c_double * 3)()
        check(lib().ptv_gradient_sums_dev(self.h, C.byref(prm), C.c_void_p(ptr), C.c_void_p(stream or 0), out))
        return [float(x) for x in out]

    # -- pressure recovery (velocity_analysis.py:190-330, physics.py:211-345) ----
    @staticmethod
    def _mask_bytes(mask, shape):
        """A bool or uint8 (any non-zero byte = fluid) mask as contiguous uint8 of ``shape``."""
        mk = np.asarray(mask)
        mk = mk.view(np.uint8) if mk.dtype == np.bool_ else mk.astype(np.uint8, copy=False)
        return np.ascontiguousarray(mk).reshape(shape)

    @staticmethod
    def _pressure_params(shape, mask_ptr, dx, dy, dz, mu=0.0, rho=0.0, wall_bc="zero-neumann", anchor="none",
                         flow_direction="auto", rtol=1e-10, maxiter=3000, damp=1e-8, atol=1e-10, btol=1e-10,
                         iter_lim=3000):
        nz, ny, nx = shape
        return PressureParams(nx, ny, nz, float(dx), float(dy), float(dz), float(mu), float(rho), WALL_BC[wall_bc],
                              ANCHOR[anchor], FLOW_DIRECTION[flow_direction], int(maxiter), float(rtol), float(damp),
                              float(atol), float(btol), int(iter_lim), C.cast(C.c_void_p(mask_ptr), _u8p))

    def force_field(self, u, v, w, fluid_mask, dx, dy, dz, mu, rho=0.0):
        """``mu * laplacian_mask_aware(vel) - rho * advection`` of float64 (nz, ny, nx) host fields
        (velocity_analysis.py:210-289); returns ``((fx, fy, fz), stats dict)``."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w)]
        mk = self._mask_bytes(fluid_mask, f[0].shape)
        prm = self._pressure_params(f[0].shape, mk.ctypes.data, dx, dy, dz, mu, rho)
        out = [np.empty_like(a) for a in f]
        st = PressureStats()
        check(lib().ptv_force_field(self.h, C.byref(prm), *[as_dp(a) for a in f], *[as_dp(a) for a in out],
                                    C.byref(st)))
        return tuple(out), st.as_dict()

    def force_field_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptrs, dx, dy, dz, mu, rho=0.0, stream=0):
        """Device-pointer force field (the outputs must not alias the inputs); returns the stats dict."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, mu, rho)
        st = PressureStats()
        check(lib().ptv_force_field_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs],
                                        *[dev_dp(p) for p in out_ptrs], C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def force_divergence(self, fx, fy, fz, fluid_mask, dx, dy, dz, wall_bc="zero-neumann"):
        """physics.py:211-262 for float64 host fields: the divergence at every voxel."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (fx, fy, fz)]
        mk = self._mask_bytes(fluid_mask, f[0].shape)
        prm = self._pressure_params(f[0].shape, mk.ctypes.data, dx, dy, dz, wall_bc=wall_bc)
        d = np.empty_like(f[0])
        check(lib().ptv_force_divergence(self.h, C.byref(prm), *[as_dp(a) for a in f], as_dp(d)))
        return d

    def force_divergence_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptr, dx, dy, dz, wall_bc="zero-neumann", stream=0):
        """Device-pointer force divergence; enqueues only (synchronise the stream to read it)."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, wall_bc=wall_bc)
        check(lib().ptv_force_divergence_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs], dev_dp(out_ptr),
                                             C.c_void_p(stream or 0)))

    def poisson_solve(self, fluid_mask, dx, dy, dz, rhs=None, force_field=None, dirichlet=None,
                      wall_bc="inhomogeneous", **solver):
        """physics.py:264-345 for host arrays: ``rhs`` or the divergence of ``force_field`` under
        ``wall_bc``; a ``dirichlet`` grid (fixed to 0) selects CG (``rtol``, ``maxiter``), None LSQR
        (``damp``, ``atol``, ``btol``, ``iter_lim``).  Returns ``(x, stats dict)``."""
        src = [rhs] if rhs is not None else list(force_field)
        src = [np.ascontiguousarray(a, dtype=np.float64) for a in src]
        shape = src[0].shape
        mk = self._mask_bytes(fluid_mask, shape)
        dm = self._mask_bytes(dirichlet, shape) if dirichlet is not None else None
        prm = self._pressure_params(shape, mk.ctypes.data, dx, dy, dz, wall_bc=wall_bc, **solver)
        x = np.empty(shape, dtype=np.float64)
        st = PressureStats()
        ptrs = [as_dp(src[0]), None, None, None] if rhs is not None else [None] + [as_dp(a) for a in src]
        check(lib().ptv_poisson_solve(self.h, C.byref(prm), *ptrs, dm.ctypes.data_as(_u8p) if dm is not None else None,
                                      as_dp(x), C.byref(st)))
        return x, st.as_dict()

    def poisson_solve_dev(self, nx, ny, nz, mask_ptr, out_ptr, dx, dy, dz, rhs_ptr=0, force_ptrs=None,
                          dirichlet_ptr=0, wall_bc="inhomogeneous", stream=0, **solver):
        """Device-pointer Poisson solve (``out_ptr`` may be ``rhs_ptr``); returns the stats dict."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, wall_bc=wall_bc, **solver)
        st = PressureStats()
        ptrs = [dev_dp(rhs_ptr) if rhs_ptr else None] + [dev_dp(p) if p else None for p in (force_ptrs or (0, 0, 0))]
        check(lib().ptv_poisson_solve_dev(self.h, C.byref(prm), *ptrs,
                                          C.cast(C.c_void_p(dirichlet_ptr), _u8p) if dirichlet_ptr else None,
                                          dev_dp(out_ptr), C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def pressure_recover(self, u, v, w, fluid_mask, dx, dy, dz, mu, rho=0.0, wall_bc="zero-neumann", anchor="outlet",
                         flow_direction="auto", **solver):
        """The whole chain of compute_pressure_field for float64 host fields, resident on the device:
        one copy in, one copy out.  Returns ``(p, stats dict)``."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w)]
        mk = self._mask_bytes(fluid_mask, f[0].shape)
        prm = self._pressure_params(f[0].shape, mk.ctypes.data, dx, dy, dz, mu, rho, wall_bc, anchor, flow_direction,
                                    **solver)
        p = np.empty_like(f[0])
        st = PressureStats()
        check(lib().ptv_pressure_recover(self.h, C.byref(prm), *[as_dp(a) for a in f], as_dp(p), C.byref(st)))
        return p, st.as_dict()

    def pressure_recover_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptr, dx, dy, dz, mu, rho=0.0,
                             wall_bc="zero-neumann", anchor="outlet", flow_direction="auto", stream=0, **solver):
        """Device-pointer chain (fields, mask and the pressure resident in HBM); returns the stats dict."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, mu, rho, wall_bc, anchor, flow_direction,
                                    **solver)
        st = PressureStats()
        check(lib().ptv_pressure_recover_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs], dev_dp(out_ptr),
                                             C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    # -- the anchored solve with the multigrid preconditioner ----
    @staticmethod
    def _with_mg(st, mst):
        d = st.as_dict()
        d["multigrid"] = mst.as_dict()
        return d

    def poisson_mg_apply(self, fluid_mask, dx, dy, dz, r, dirichlet=None, multigrid=None):
        """``z = M r``: one V-cycle of the preconditioner for host arrays.  Returns ``(z, multigrid stats)``."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        mk = self._mask_bytes(fluid_mask, r.shape)
        dm = self._mask_bytes(dirichlet, r.shape) if dirichlet is not None else None
        prm = self._pressure_params(r.shape, mk.ctypes.data, dx, dy, dz)
        mg = mg_params(multigrid)
        z = np.empty_like(r)
        mst = MgStats()
        check(lib().ptv_poisson_mg_apply(self.h, C.byref(prm), C.byref(mg),
                                         dm.ctypes.data_as(_u8p) if dm is not None else None, as_dp(r), as_dp(z),
                                         C.byref(mst)))
        return z, mst.as_dict()

    def poisson_mg_apply_dev(self, nx, ny, nz, mask_ptr, r_ptr, z_ptr, dx, dy, dz, dirichlet_ptr=0, multigrid=None,
                             stream=0):
        """Device-pointer V-cycle (``z_ptr`` must not be ``r_ptr``); returns the multigrid stats."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz)
        mg = mg_params(multigrid)
        mst = MgStats()
        check(lib().ptv_poisson_mg_apply_dev(self.h, C.byref(prm), C.byref(mg),
                                             C.cast(C.c_void_p(dirichlet_ptr), _u8p) if dirichlet_ptr else None,
                                             dev_dp(r_ptr), dev_dp(z_ptr), C.c_void_p(stream or 0), C.byref(mst)))
        return mst.as_dict()

    def poisson_solve_mg(self, fluid_mask, dx, dy, dz, rhs=None, force_field=None, dirichlet=None,
                         wall_bc="inhomogeneous", multigrid=None, **solver):
        """``poisson_solve`` with scipy's preconditioned recurrence, M = the V-cycle; ``dirichlet`` is
        required (``NotImplementedError`` without).  The stats carry a ``multigrid`` dict."""
        src = [rhs] if rhs is not None else list(force_field)
        src = [np.ascontiguousarray(a, dtype=np.float64) for a in src]
        shape = src[0].shape
        mk = self._mask_bytes(fluid_mask, shape)
        dm = self._mask_bytes(dirichlet, shape) if dirichlet is not None else None
        prm = self._pressure_params(shape, mk.ctypes.data, dx, dy, dz, wall_bc=wall_bc, **solver)
        mg = mg_params(multigrid)
        x = np.empty(shape, dtype=np.float64)
        st, mst = PressureStats(), MgStats()
        ptrs = [as_dp(src[0]), None, None, None] if rhs is not None else [None] + [as_dp(a) for a in src]
        check(lib().ptv_poisson_solve_mg(self.h, C.byref(prm), *ptrs,
                                         dm.ctypes.data_as(_u8p) if dm is not None else None, as_dp(x), C.byref(mg),
                                         C.byref(st), C.byref(mst)))
        return x, self._with_mg(st, mst)

    def poisson_solve_mg_dev(self, nx, ny, nz, mask_ptr, out_ptr, dx, dy, dz, rhs_ptr=0, force_ptrs=None,
                             dirichlet_ptr=0, wall_bc="inhomogeneous", multigrid=None, stream=0, **solver):
        """Device-pointer preconditioned solve (``out_ptr`` may be ``rhs_ptr``); returns the stats dict."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, wall_bc=wall_bc, **solver)
        mg = mg_params(multigrid)
        st, mst = PressureStats(), MgStats()
        ptrs = [dev_dp(rhs_ptr) if rhs_ptr else None] + [dev_dp(p) if p else None for p in (force_ptrs or (0, 0, 0))]
        check(lib().ptv_poisson_solve_mg_dev(self.h, C.byref(prm), *ptrs,
                                             C.cast(C.c_void_p(dirichlet_ptr), _u8p) if dirichlet_ptr else None,
                                             dev_dp(out_ptr), C.c_void_p(stream or 0), C.byref(mg), C.byref(st),
                                             C.byref(mst)))
        return self._with_mg(st, mst)

    def pressure_recover_mg(self, u, v, w, fluid_mask, dx, dy, dz, mu, rho=0.0, wall_bc="zero-neumann",
                            anchor="outlet", flow_direction="auto", multigrid=None, **solver):
        """``pressure_recover`` with the anchored solve preconditioned (``anchor='none'`` raises
        ``NotImplementedError``).  Returns ``(p, stats dict)``."""
        f = [np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, w)]
        mk = self._mask_bytes(fluid_mask, f[0].shape)
        prm = self._pressure_params(f[0].shape, mk.ctypes.data, dx, dy, dz, mu, rho, wall_bc, anchor, flow_direction,
                                    **solver)
        mg = mg_params(multigrid)
        p = np.empty_like(f[0])
        st, mst = PressureStats(), MgStats()
        check(lib().ptv_pressure_recover_mg(self.h, C.byref(prm), *[as_dp(a) for a in f], as_dp(p), C.byref(mg),
                                            C.byref(st), C.byref(mst)))
        return p, self._with_mg(st, mst)

    def pressure_recover_mg_dev(self, nx, ny, nz, ptrs, mask_ptr, out_ptr, dx, dy, dz, mu, rho=0.0,
                                wall_bc="zero-neumann", anchor="outlet", flow_direction="auto", multigrid=None,
                                stream=0, **solver):
        """Device-pointer chain with the anchored solve preconditioned; returns the stats dict."""
        prm = self._pressure_params((nz, ny, nx), mask_ptr, dx, dy, dz, mu, rho, wall_bc, anchor, flow_direction,
                                    **solver)
        mg = mg_params(multigrid)
        st, mst = PressureStats(), MgStats()
        check(lib().ptv_pressure_recover_mg_dev(self.h, C.byref(prm), *[dev_dp(p) for p in ptrs], dev_dp(out_ptr),
                                                C.c_void_p(stream or 0), C.byref(mg), C.byref(st), C.byref(mst)))
        return self._with_mg(st, mst)

    # -- distance transform and alignment score (auto_align.py:10-62) ----
    def edt(self, mask, want_d2=True, want_distance=True, keep_distance=False):
        """Exact Euclidean distance transform of a host uint8 (nz, ny, nx) ``mask`` (scipy's meaning:
        per nonzero voxel the distance to the nearest zero voxel).  Returns ``(d2, dist, stats)``:
        the int32 squared distances and the float64 distances (None where not asked for) and
        ``{"max_d2", "ms"}``.  ``keep_distance`` leaves the float64 field in the context for
        ``align_score(..., dt=None)``.  ``ValueError`` when the mask has no zero voxel."""
        nz, ny, nx = edt_check_shape(mask.shape)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        d2 = np.empty(mk.shape, dtype=np.int32) if want_d2 else None
        dist = np.empty(mk.shape, dtype=np.float64) if want_distance else None
        prm = EdtParams(nx, ny, nz, int(bool(keep_distance)))
        st = EdtStats()
        self._align_owner = None  # the resident field is rewritten: no session's upload survives
        check(lib().ptv_edt(self.h, C.byref(prm), mk.ctypes.data_as(C.c_void_p),
                            d2.ctypes.data_as(C.c_void_p) if want_d2 else None,
                            dist.ctypes.data_as(C.c_void_p) if want_distance else None, C.byref(st)))
        return d2, dist, {"max_d2": int(st.max_d2), "ms": st.ms}

    def edt_dev(self, nx, ny, nz, mask_ptr, d2_ptr=0, dist_ptr=0, keep_distance=False, stream=0):
        """The same for a uint8 mask resident in HBM; ``d2_ptr`` (int32) and ``dist_ptr`` (float64)
        are device pointers, 0 = not wanted.  Returns the stats."""
        edt_check_shape((nz, ny, nx))
        prm = EdtParams(nx, ny, nz, int(bool(keep_distance)))
        st = EdtStats()
        check(lib().ptv_edt_dev(self.h, C.byref(prm), C.c_void_p(mask_ptr), C.c_void_p(d2_ptr) if d2_ptr else None,
                                C.c_void_p(dist_ptr) if dist_ptr else None, C.c_void_p(stream or 0), C.byref(st)))
        return {"max_d2": int(st.max_d2), "ms": st.ms}

    def _align_call(self, fn, shape, n_points, ptrs, offsets, extra=()):
        nz, ny, nx = shape
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 3)
        rec = np.zeros(off.shape[0], dtype=ALIGN_RECORD)
        if off.shape[0] == 0:
            return rec, 0.0
        prm = AlignParams(nx, ny, nz, int(n_points), int(off.shape[0]))
        ms = C.c_double(0.0)
        check(fn(self.h, C.byref(prm), *[C.c_void_p(p) if p else None for p in ptrs], off.ctypes.data_as(C.c_void_p),
                 *extra, rec.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return rec, ms.value

    def align_score(self, shape, n_points, offsets, points=None, dt=None):
        """The alignment records of ``offsets`` (m, 3).  ``points`` (n, 3) float64 and ``dt`` (nz, ny, nx)
        float64 are uploaded and stay in the context; None scores against what it holds (``shape`` and
        ``n_points`` must be the upload's).  Returns ``(records, ms)``, records of ALIGN_RECORD."""
        keep = []
        for a in (points, dt):
            keep.append(None if a is None else np.ascontiguousarray(a, dtype=np.float64))
        if keep[0] is not None and keep[0].shape != (int(n_points), 3):
            raise ValueError(f"points must be ({n_points}, 3), got {keep[0].shape}")
        if keep[1] is not None and keep[1].shape != tuple(shape):
            raise ValueError(f"dt must be {tuple(shape)}, got {keep[1].shape}")
        return self._align_call(lib().ptv_align_score, shape, n_points,
                                [0 if a is None else a.ctypes.data for a in keep], offsets)

    def align_score_dev(self, shape, n_points, points_ptr, dt_ptr, offsets, stream=0):
        """The same for points and a distance field resident in HBM (device pointers)."""
        return self._align_call(lib().ptv_align_score_dev, shape, n_points, [points_ptr, dt_ptr], offsets,
                                extra=(C.c_void_p(stream or 0),))

    # -- cubic B-spline sampling and the mesh interface drag (velocity_analysis.py:513-657) ----
    @staticmethod
    def _spline_field(field):
        f = np.ascontiguousarray(field)
        if f.ndim != 3 or f.dtype not in (np.float32, np.float64):
            raise ValueError(f"a 3-D float32 / float64 field, got {f.ndim}-D {f.dtype}")
        return f, (F32 if f.dtype == np.float32 else F64)

    def spline_prefilter(self, field):
        """The float64 cubic B-spline coefficients of a host float32 / float64 (nz, ny, nx) field padded
        by SPLINE_PAD edge-replicated samples per side: scipy's ``spline_filter(np.pad(field, 12,
        mode='edge'), 3, mode='nearest')``.  Returns ``(coefficients, ms)``."""
        f, dt = self._spline_field(field)
        nz, ny, nx = f.shape
        coef = np.empty((nz + 2 * SPLINE_PAD, ny + 2 * SPLINE_PAD, nx + 2 * SPLINE_PAD), dtype=np.float64)
        prm = SplineParams(nx, ny, nz, dt, 3, 0)
        ms = C.c_double(0.0)
        check(lib().ptv_spline_prefilter(self.h, C.byref(prm), f.ctypes.data_as(C.c_void_p),
                                         coef.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return coef, ms.value

    def spline_prefilter_dev(self, nx, ny, nz, field_ptr, coef_ptr, field_dtype=F64, stream=0):
        """The same for a field resident in HBM into a device buffer of (nz + 24)(ny + 24)(nx + 24)
        float64.  Returns the kernels' time."""
        prm = SplineParams(nx, ny, nz, int(field_dtype), 3, 0)
        ms = C.c_double(0.0)
        check(lib().ptv_spline_prefilter_dev(self.h, C.byref(prm), C.c_void_p(field_ptr), C.c_void_p(coef_ptr),
                                             C.c_void_p(stream or 0), C.byref(ms)))
        return ms.value

    def map_coordinates(self, field, coordinates, order=3, shape=None):
        """Samples of a host (nz, ny, nx) field at ``coordinates`` (3, n) float64 rows z, y, x, as
        scipy's ``map_coordinates(field, coordinates, order=order, mode='nearest')`` for order 0, 1
        or 3.  An order-3 call filters the field into the context; ``field`` None (with ``shape``)
        samples the coefficients the last order-3 call left.  Returns ``(samples, ms)``."""
        co = np.ascontiguousarray(coordinates, dtype=np.float64)
        if co.ndim != 2 or co.shape[0] != 3:
            raise ValueError(f"coordinates must be (3, n), got {co.shape}")
        if field is None:
            nz, ny, nx = (int(n) for n in shape)
            f, dt = None, F64
        else:
            f, dt = self._spline_field(field)
            nz, ny, nx = f.shape
        out = np.empty(co.shape[1], dtype=np.float64)
        prm = SplineParams(nx, ny, nz, dt, int(order), co.shape[1])
        ms = C.c_double(0.0)
        check(lib().ptv_map_coordinates(self.h, C.byref(prm), None if f is None else f.ctypes.data_as(C.c_void_p),
                                        co.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return out, ms.value

    def map_coordinates_dev(self, nx, ny, nz, field_ptr, coords_ptr, n_points, out_ptr, order=3, field_dtype=F64,
                            stream=0):
        """The same on device pointers (``field_ptr`` 0: the resident coefficients, order 3 only);
        coordinates (3, n) and samples (n,) float64 in HBM.  Returns the kernels' time."""
        prm = SplineParams(nx, ny, nz, int(field_dtype), int(order), int(n_points))
        ms = C.c_double(0.0)
        check(lib().ptv_map_coordinates_dev(self.h, C.byref(prm), C.c_void_p(field_ptr) if field_ptr else None,
                                            C.c_void_p(coords_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0),
                                            C.byref(ms)))
        return ms.value

    def _mesh_call(self, fn, shape, ptrs, tri_offsets, n_verts, field_dtype, vert_dtype, viscosity, dx, dy, dz, reuse,
                   extra=(), resident_labels=None):
        nz, ny, nx = shape
        if resident_labels is None:
            off = np.ascontiguousarray(tri_offsets, dtype=np.int64).reshape(-1)
            prm = MeshParams(nx, ny, nz, int(field_dtype), int(vert_dtype), int(n_verts), int(off[-1]),
                             int(off.size - 1), float(dx), float(dy), float(dz), float(viscosity), int(bool(reuse)),
                             off.ctypes.data_as(C.POINTER(C.c_int64)), 0)
            rec = np.zeros(off.size - 1, dtype=MESH_RECORD)
        else:  # the context's mesh: the library fills in the counts and the offsets
            prm = MeshParams(nx, ny, nz, int(field_dtype), F32, 0, 0, int(resident_labels), float(dx), float(dy), float(dz),
                             float(viscosity), int(bool(reuse)), None, 1)
            rec = np.zeros(int(resident_labels), dtype=MESH_RECORD)
        ms = (C.c_double * 2)()
        check(fn(self.h, C.byref(prm), *[C.c_void_p(p) if p else None for p in ptrs], *extra,
                 rec.ctypes.data_as(C.c_void_p), ms))
        return rec, {"ms_prefilter": ms[0], "ms_traction": ms[1]}

    def mesh_drag(self, fields, pressure, background, verts, faces, tri_offsets, viscosity, dx, dy, dz, shape=None,
                  resident_labels=None):
        """Mesh interface drag of host arrays.  ``fields``: u, v, w of one float32 / float64 dtype,
        (nz, ny, nx); ``pressure`` (the same dtype) and ``background`` (uint8 / bool, nonzero = pore
        space) may be None.  ``verts`` (n, 3) float32 / float64 rows z, y, x, ``faces`` (m, 3) indices
        into them, ``tri_offsets`` (labels + 1,): label l owns faces [tri_offsets[l],
        tri_offsets[l + 1]).  ``fields`` None (with ``shape``): the fields, their coefficients, the
        pressure and the background of the previous call stay as they are in the context (no upload,
        no prefilter).  ``resident_labels`` (the label count of the context's last ``marching_cubes``):
        that call's mesh is integrated where it lies on the device; ``verts``, ``faces`` and
        ``tri_offsets`` are not read and one record per label of that call comes back.  Returns
        ``(records, times)``: MESH_RECORD per label, and the prefilters' and the traction kernels' ms."""
        if resident_labels is not None:
            verts, faces = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
        vt = np.ascontiguousarray(verts)
        if vt.dtype not in (np.float32, np.float64):
            vt = vt.astype(np.float64)
        fc = np.ascontiguousarray(faces, dtype=np.int32)
        if vt.ndim != 2 or vt.shape[1] != 3 or fc.ndim != 2 or fc.shape[1] != 3:
            raise ValueError(f"verts (n, 3) and faces (m, 3), got {vt.shape} and {fc.shape}")
        keep = [vt, fc]
        if fields is None:
            ptrs, ft, shape = [0] * 5, getattr(self, "_mesh_dtype", F64), tuple(int(n) for n in shape)
        else:
            f = [self._spline_field(a)[0] for a in fields]
            ft = F32 if f[0].dtype == np.float32 else F64
            if pressure is not None:
                f.append(np.ascontiguousarray(pressure, dtype=f[0].dtype))
            if len({a.shape for a in f}) != 1 or len({a.dtype for a in f}) != 1:
                raise ValueError("u, v, w and the pressure must share one shape and dtype")
            shape = f[0].shape
            ptrs = [a.ctypes.data for a in f] + [0] * (4 - len(f))
            if background is not None:
                bg = np.ascontiguousarray(background).view(np.uint8) if np.asarray(background).dtype == np.bool_ \
                    else np.ascontiguousarray(background, dtype=np.uint8)
                if bg.shape != shape:
                    raise ValueError(f"background shape {bg.shape} does not match the fields' {shape}")
                keep.append(bg)
                ptrs.append(bg.ctypes.data)
            else:
                ptrs.append(0)
            keep.append(f)
        res = self._mesh_call(lib().ptv_mesh_drag, shape, ptrs + [vt.ctypes.data, fc.ctypes.data], tri_offsets,
                              vt.shape[0], ft, F32 if vt.dtype == np.float32 else F64, viscosity, dx, dy, dz,
                              reuse=fields is None, resident_labels=resident_labels)
        self._mesh_dtype = ft
        return res

    # -- marching cubes of a label mask (the triangulation in front of the mesh drag) ----
    def _surface_call(self, fn, shape, mask_ptr, table, step_size, extra=()):
        tab = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
        nz, ny, nx = (int(n) for n in shape)
        prm = SurfaceParams(nx, ny, nz, int(step_size), tab.size, tab.ctypes.data_as(C.POINTER(C.c_int32)))
        nv, nt = np.zeros(tab.size, dtype=np.int64), np.zeros(tab.size, dtype=np.int64)
        ms = (C.c_double * 2)()
        check(fn(self.h, C.byref(prm), C.c_void_p(mask_ptr), *extra, nv.ctypes.data_as(C.POINTER(C.c_int64)),
                 nt.ctypes.data_as(C.POINTER(C.c_int64)), ms))
        return nv, nt, {"ms_count": ms[0], "ms_emit": ms[1]}

    def marching_cubes(self, mask, table, step_size=1):
        """Marching cubes of a host int32 (nz, ny, nx) mask for the ascending, distinct, positive int32
        labels of ``table`` (drag_label_table's), all in one pass.  The mesh stays in the context
        (``surface_fetch`` copies it out, ``mesh_drag(..., resident_labels=len(table))`` integrates it in
        place).  Returns ``(vert_counts, tri_counts, times)`` per label of the table."""
        mk = np.ascontiguousarray(mask, dtype=np.int32)
        if mk.ndim != 3:
            raise ValueError(f"a 3-D mask, got {mk.ndim}-D")
        return self._surface_call(lib().ptv_marching_cubes, mk.shape, mk.ctypes.data, table, step_size)

    def marching_cubes_dev(self, nx, ny, nz, mask_ptr, table, step_size=1, stream=0):
        """The same for an int32 mask resident in HBM (device pointer)."""
        return self._surface_call(lib().ptv_marching_cubes_dev, (nz, ny, nx), mask_ptr, table, step_size,
                                  extra=(C.c_void_p(stream or 0),))

    def surface_fetch(self, vert_counts, tri_counts):
        """The context's mesh as host arrays: ``[(verts float32 (n, 3), faces int32 (m, 3)), ...]``, one
        pair per label of the last ``marching_cubes`` (whose counts these are); a label's faces index
        its own vertices."""
        nv, nt = int(np.sum(vert_counts)), int(np.sum(tri_counts))
        verts, faces = np.empty((nv, 3), dtype=np.float32), np.empty((nt, 3), dtype=np.int32)
        check(lib().ptv_surface_fetch(self.h, verts.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
        v0 = np.concatenate([[0], np.cumsum(vert_counts)]).astype(np.int64)
        t0 = np.concatenate([[0], np.cumsum(tri_counts)]).astype(np.int64)
        return [(verts[v0[l]:v0[l + 1]], faces[t0[l]:t0[l + 1]]) for l in range(len(v0) - 1)]

    # -- connected-component labelling (scipy.ndimage.label) ----
    @staticmethod
    def _label_stats(st):
        return {"n_components": int(st.n_components), "n_foreground": int(st.n_foreground),
                "ms_merge": st.ms_merge, "ms_number": st.ms_number}

    def label(self, mask, connectivity=6, want_sizes=False):
        """Labels the components of a host uint8 (nz, ny, nx) ``mask`` (nonzero = foreground) under 6, 18
        or 26 neighbours, numbered as scipy.ndimage.label numbers them.  Returns ``(labels, sizes,
        stats)``: int32 labels, the int64 voxel counts per label with the background first (None
        unless ``want_sizes``) and ``{"n_components", "n_foreground", "ms_merge", "ms_number"}``."""
        nz, ny, nx = label_check_shape(mask.shape)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        labels = np.empty(mk.shape, dtype=np.int32)
        sizes = np.empty(label_sizes_room(mk.size), dtype=np.int64) if want_sizes else None
        prm = LabelParams(nz, ny, nx, int(connectivity))
        st = LabelStats()
        check(lib().ptv_label(self.h, C.byref(prm), mk.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p),
                              sizes.ctypes.data_as(C.c_void_p) if want_sizes else None, C.byref(st)))
        if want_sizes:
            sizes = sizes[:int(st.n_components) + 1].copy()
        return labels, sizes, self._label_stats(st)

    def label_dev(self, nx, ny, nz, mask_ptr, labels_ptr, connectivity=6, sizes_ptr=0, stream=0):
        """The same for a uint8 mask resident in HBM: ``labels_ptr`` (int32, the mask's shape) and
        ``sizes_ptr`` (int64, ``label_sizes_room(n)`` entries, 0 = not wanted) are device pointers.  The
        labels stay on the device.  Returns the stats."""
        label_check_shape((nz, ny, nx))
        prm = LabelParams(nz, ny, nx, int(connectivity))
        st = LabelStats()
        check(lib().ptv_label_dev(self.h, C.byref(prm), C.c_void_p(mask_ptr), C.c_void_p(labels_ptr),
                                  C.c_void_p(sizes_ptr) if sizes_ptr else None, C.c_void_p(stream or 0),
                                  C.byref(st)))
        return self._label_stats(st)

    def mesh_drag_dev(self, nx, ny, nz, ptrs, pressure_ptr, background_ptr, verts_ptr, n_verts, faces_ptr, tri_offsets,
                      viscosity, dx, dy, dz, field_dtype=F64, vert_dtype=F32, reuse=False, stream=0):
        """Device-pointer mesh drag: u, v, w (``ptrs``), the pressure and the uint8 background (0 =
        none), the vertices and the int32 faces resident in HBM; ``tri_offsets`` and the records stay on
        the host.  ``reuse``: skip the prefilters, the context holds these fields' coefficients."""
        return self._mesh_call(lib().ptv_mesh_drag_dev, (nz, ny, nx),
                               [*ptrs, pressure_ptr, background_ptr, verts_ptr, faces_ptr], tri_offsets, n_verts,
                               field_dtype, vert_dtype, viscosity, dx, dy, dz, reuse, extra=(C.c_void_p(stream or 0),))


class AlignSession:
    """Points and a distance field uploaded once, offsets scored against them: what an optimiser
    that evaluates the objective some tens of times needs.  ``dt`` None takes the field the
    context's last ``edt(..., keep_distance=True)`` left.  The resident buffers belong to the
    context; a session that finds another one has used them since uploads again."""

    def __init__(self, ctx, points, shape, dt=None):
        self.ctx = ctx
        self.shape = tuple(int(n) for n in shape)
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.dt = dt
        self.ms = 0.0
        self.calls = 0

    def score(self, offsets):
        """Records (ALIGN_RECORD) of the offsets (m, 3)."""
        mine = getattr(self.ctx, "_align_owner", None) is self
        if not mine and self.dt is None and getattr(self.ctx, "_align_owner", None) is not None:
            raise RuntimeError("AlignSession: the context's kept distance field has been replaced by another session")
        rec, ms = self.ctx.align_score(self.shape, len(self.points), offsets,
                                       points=None if mine else self.points, dt=None if mine else self.dt)
        self.ctx._align_owner = self
        self.ms += ms
        self.calls += 1
        return rec
