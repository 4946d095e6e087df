"""Host-side binding of the HIP dose engine (raytracedicom_amd/librtd_hip.so) through its C ABI (include/rtd.h).

This is the product path: every call goes to the hand-written HIP kernels. There is NO CPU fallback — if the
shared library is missing or no GPU is present the calls raise RtdError loudly.

`cudaWrapperProtons` mirrors the reference entry point of the same name (src/kernel_wrapper.cuh:161): same
argument meaning, dose accumulated in place, log text written to the stream argument, errors raised.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librtd_hip.so")
_LIB = None

_FETCH_DTYPES = {"first_inside": np.int32, "first_outside": np.int32, "first_passive": np.int32,
                 "eff_radius": np.int32, "tile_radius": np.uint8, "fill_debug": np.int64, "sweep_debug": np.int64, "uniform_debug": np.int64, "sweep_big_debug": np.int64, "scan_debug": np.int64,
                 "dij_batch": np.int32, "trace_reused": np.int32, "sigma_reused": np.int32, "dose_reused": np.int32, "launch_builds": np.int32, "active": np.int32, "target_bev": np.uint32, "target_hit": np.uint8}


class RtdError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("rtd status %d: %s" % (status, message))
        self.status = status


def build(verbose=False):
    """Compile the HIP engine for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "all"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """Load librtd_hip.so. Raises if it has not been built: the product never substitutes another path."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RtdError(abi.RTD_ERR_NO_DEVICE, "%s not built (run __graft_entry__.build() or make -C raytracedicom_amd/csrc)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
        u3 = C.POINTER(C.c_uint32)
        L.rtd_abi_version.restype = C.c_uint32
        L.rtd_last_error.restype = C.c_char_p
        L.rtd_last_error.argtypes = [vp]
        L.rtd_global_error.restype = C.c_char_p
        L.rtd_create.argtypes = [C.c_int, vpp]
        L.rtd_destroy.argtypes = [vp]
        L.rtd_set_options.argtypes = [vp, C.POINTER(abi.RtdOptions)]
        L.rtd_set_luts.argtypes = [vp, C.POINTER(abi.RtdLuts)]
        L.rtd_load_luts_dir.argtypes = [vp, C.c_char_p, C.c_int]
        L.rtd_set_ct.argtypes = [vp, abi.c_float_p, u3]
        L.rtd_set_ct_device.argtypes = [vp, vp, u3]
        L.rtd_compute.argtypes = [vp, C.POINTER(abi.RtdBeam), C.c_int, abi.c_float_p, u3, C.POINTER(abi.RtdTiming)]
        L.rtd_field_create.argtypes = [vp, C.POINTER(abi.RtdBeam), u3, vpp]
        L.rtd_field_compute.argtypes = [vp, vp, vp]
        L.rtd_field_finish.argtypes = [vp, vp, C.POINTER(abi.RtdTiming), C.POINTER(abi.RtdFieldInfo)]
        L.rtd_field_clear_dose.argtypes = [vp, vp, vp]
        L.rtd_field_destroy.argtypes = [vp, vp]
        L.rtd_field_fetch.argtypes = [vp, vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        i3 = C.POINTER(C.c_int32)
        L.rtd_field_compute_bev.argtypes = [vp, vp]
        L.rtd_field_transfer.argtypes = [vp, vp, vp, i3, i3]
        L.rtd_field_transfer_init.argtypes = [vp, vp, vp, i3, i3]
        L.rtd_fields_transfer_init.argtypes = [vp, C.POINTER(C.c_void_p), C.c_uint32, vp, i3, i3]
        L.rtd_field_wait_plan.argtypes = [vp, vp, C.POINTER(abi.RtdFieldInfo), C.POINTER(C.c_size_t)]
        L.rtd_bev_message_bound.argtypes = [vp, vp]
        L.rtd_bev_message_bound.restype = C.c_size_t
        L.rtd_field_export_bev.argtypes = [vp, vp, vp, C.c_size_t]
        L.rtd_field_create_remote.argtypes = [vp, C.POINTER(abi.RtdBeam), u3, vpp]
        L.rtd_field_attach_bev.argtypes = [vp, vp, vp]
        L.rtd_field_clear_dose_box.argtypes = [vp, vp, vp, i3, i3]
        L.rtd_field_release.argtypes = [vp, vp]
        L.rtd_field_spot_gradient.argtypes = [vp, vp, vp, vp]
        L.rtd_spot_gradient.argtypes = [vp, C.POINTER(abi.RtdBeam), C.c_int, abi.c_float_p, u3, abi.c_float_p]
        L.rtd_field_dose_influence.argtypes = [vp, vp, C.c_float, C.POINTER(C.c_size_t)]
        L.rtd_field_dose_influence_copy.argtypes = [vp, vp, vp, vp, vp]
        L.rtd_field_set_spot_weights.argtypes = [vp, vp, vp]
        L.rtd_field_dose_influence_prepare.argtypes = [vp, vp]
        L.rtd_field_dose_influence_apply.argtypes = [vp, vp, vp, vp, C.c_int]
        L.rtd_field_dose_influence_apply_t.argtypes = [vp, vp, vp, vp]
        L.rtd_field_dose_influence_device.argtypes = [vp, vp, vpp, vpp, vpp, C.POINTER(C.c_size_t)]
        L.rtd_objective_create.argtypes = [vp, u3, vpp]
        L.rtd_objective_add_roi.argtypes = [vp, vp, i3, C.c_size_t, i3]
        L.rtd_objective_add_term.argtypes = [vp, vp, C.POINTER(abi.RtdObjectiveTerm)]
        L.rtd_objective_eval.argtypes = [vp, vp, vp, vp, vp]
        L.rtd_objective_destroy.argtypes = [vp, vp]
        L.rtd_objective_add_dvh_term.argtypes = [vp, vp, C.POINTER(abi.RtdObjectiveDvhTerm)]
        L.rtd_objective_dose_at_volume.argtypes = [vp, vp, vp, C.POINTER(abi.RtdDvhQuery), C.c_uint32, vp]
        L.rtd_objective_dvh.argtypes = [vp, vp, vp, C.c_uint32, C.c_double, vp]
        L.rtd_objective_add_eud_term.argtypes = [vp, vp, C.POINTER(abi.RtdObjectiveEudTerm)]
        L.rtd_objective_eud.argtypes = [vp, vp, vp, C.POINTER(abi.RtdEudQuery), C.c_uint32, vp]
        L.rtd_default_optimizer_options.argtypes = [C.POINTER(abi.RtdOptimizerOptions)]
        L.rtd_default_optimizer_options.restype = None
        L.rtd_optimizer_create.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_optimizer_set_weights.argtypes = [vp, vp, C.c_uint32, vp]
        L.rtd_optimizer_run.argtypes = [vp, vp, C.c_uint32]
        L.rtd_optimizer_result.argtypes = [vp, vp, C.POINTER(abi.RtdOptimizerReport), C.POINTER(C.c_double), C.c_uint32]
        L.rtd_optimizer_weights.argtypes = [vp, vp, C.c_uint32, vp, C.c_int]
        L.rtd_optimizer_dose.argtypes = [vp, vp, vpp]
        L.rtd_optimizer_destroy.argtypes = [vp, vp]
        L.rtd_optimizer_create_robust.argtypes = [vp, vpp, C.c_uint32, C.POINTER(abi.RtdRobustOptions), vp, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_optimizer_scenario_values.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.rtd_optimizer_scenario_dose.argtypes = [vp, vp, C.c_uint32, vpp]
        L.rtd_objective_eval_voxelwise.argtypes = [vp, vp, vpp, C.c_uint32, vp, vpp, vp]
        L.rtd_scenario_dose_extremes.argtypes = [vp, vpp, C.c_uint32, C.c_size_t, vp, vp]
        L.rtd_optimizer_create_voxelwise.argtypes = [vp, vpp, C.c_uint32, C.c_uint32, vp, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_roi_rasterize.argtypes = [vp, C.POINTER(abi.RtdRoiGrid), C.POINTER(abi.RtdContourSet), vpp]
        L.rtd_roi_get_info.argtypes = [vp, vp, C.POINTER(abi.RtdRoiInfo)]
        L.rtd_roi_voxels.argtypes = [vp, vp, i3, C.c_size_t]
        L.rtd_roi_device.argtypes = [vp, vp, vpp, C.POINTER(C.c_size_t)]
        L.rtd_roi_fill_mask.argtypes = [vp, vp, vp]
        L.rtd_roi_kernel_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.rtd_roi_destroy.argtypes = [vp, vp]
        L.rtd_roi_margin.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, vpp]
        L.rtd_roi_combine.argtypes = [vp, vp, vp, C.c_int, vpp]
        L.rtd_roi_from_mask.argtypes = [vp, u3, vp, vpp]
        L.rtd_field_project_target.argtypes = [vp, vp, vp, C.POINTER(abi.RtdTargetInfo)]
        L.rtd_field_select_spots.argtypes = [vp, vp, C.POINTER(abi.RtdTargetOptions), vp, C.POINTER(C.c_uint32)]
        L.rtd_default_gamma_options.argtypes = [C.POINTER(abi.RtdGammaOptions)]
        L.rtd_default_gamma_options.restype = None
        L.rtd_dose_gamma.argtypes = [vp, vp, vp, u3, C.POINTER(C.c_float), C.POINTER(abi.RtdGammaOptions), vp, vp, vp]
        L.rtd_dose_gamma_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.rtd_default_resample_options.argtypes = [C.POINTER(abi.RtdResampleOptions)]
        L.rtd_default_resample_options.restype = None
        L.rtd_dose_resample.argtypes = [vp, vp, u3, C.POINTER(abi.RtdAffine), vp, u3, C.POINTER(abi.RtdResampleOptions)]
        L.rtd_dose_resample_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.rtd_dose_quantize.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(C.c_double), vp, C.POINTER(C.c_uint64)]
        L.rtd_dose_warp.argtypes = [vp, vp, u3, C.POINTER(abi.RtdWarp), vp, u3, C.POINTER(abi.RtdResampleOptions)]
        L.rtd_dose_warp_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.rtd_dose_warp_t_workspace_bytes.argtypes = [u3, C.POINTER(C.c_size_t)]
        L.rtd_dose_warp_t.argtypes = [vp, vp, u3, C.POINTER(abi.RtdWarp), vp, u3, C.c_float, C.c_uint32, vp, C.c_size_t]
        L.rtd_dose_warp_t_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.rtd_dose_warp_sum.argtypes = [vp, vpp, u3, C.POINTER(abi.RtdWarp), abi.c_float_p, C.c_uint32, vp, u3]
        L.rtd_dose_warp_t_phases_workspace_bytes.argtypes = [u3, C.c_uint32, C.POINTER(C.c_size_t)]
        L.rtd_dose_warp_t_phases.argtypes = [vp, vp, u3, C.POINTER(abi.RtdWarp), abi.c_float_p, C.c_uint32, vpp, u3, vp, C.c_size_t]
        L.rtd_optimizer_create_4d.argtypes = [vp, vpp, C.c_uint32, C.POINTER(abi.Rtd4dOptions), vp, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_set_let_table.argtypes = [vp, abi.c_float_p, C.c_int32, C.c_int32]
        L.rtd_field_water_depth.argtypes = [vp, vp, vp]
        L.rtd_field_let_influence.argtypes = [vp, vp]
        L.rtd_field_let_influence_apply.argtypes = [vp, vp, vp, vp, C.c_int]
        L.rtd_field_let_influence_apply_t.argtypes = [vp, vp, vp, vp]
        L.rtd_field_let_influence_device.argtypes = [vp, vp, vpp, C.POINTER(C.c_size_t)]
        L.rtd_let_average.argtypes = [vp, vp, vp, C.c_size_t, C.c_float, vp]
        L.rtd_optimizer_set_let_objective.argtypes = [vp, vp, vp]
        L.rtd_optimizer_let_dose.argtypes = [vp, vp, vpp]
        L.rtd_optimizer_let_values.argtypes = [vp, vp, C.POINTER(C.c_double)]
        L.rtd_rbe_create.argtypes = [vp, u3, C.POINTER(abi.RtdRbeTissue), vpp]
        L.rtd_rbe_add_tissue.argtypes = [vp, vp, C.POINTER(abi.RtdRbeTissue), C.POINTER(C.c_int32)]
        L.rtd_rbe_assign_voxels.argtypes = [vp, vp, i3, C.c_size_t, C.c_int32]
        L.rtd_rbe_assign_roi.argtypes = [vp, vp, vp, C.c_int32]
        L.rtd_rbe_classes_device.argtypes = [vp, vp, vpp]
        L.rtd_rbe_dose.argtypes = [vp, vp, vp, vp, i3, vp]
        L.rtd_rbe_backward.argtypes = [vp, vp, vp, vp, vp, i3, vp, vp]
        L.rtd_rbe_destroy.argtypes = [vp, vp]
        L.rtd_optimizer_set_rbe.argtypes = [vp, vp, vp]
        L.rtd_optimizer_rbe_dose.argtypes = [vp, vp, vpp]
        L.rtd_field_dose_influence_apply_set.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int]
        L.rtd_field_dose_influence_apply_t_set.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32]
        L.rtd_planset_create.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdObjectiveTerm), C.c_uint32, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_planset_set_weights.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
        L.rtd_planset_run.argtypes = [vp, vp, C.c_uint32]
        L.rtd_planset_result.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.RtdOptimizerReport), C.POINTER(C.c_double), C.c_uint32]
        L.rtd_planset_weights.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_int, vp]
        L.rtd_planset_dose.argtypes = [vp, vp, C.c_uint32, vp]
        L.rtd_planset_values.argtypes = [vp, vp, C.POINTER(C.c_double)]
        L.rtd_planset_blend.argtypes = [vp, vp, C.POINTER(C.c_double), C.c_uint32, C.c_int, vp]
        L.rtd_planset_destroy.argtypes = [vp, vp]
        L.rtd_default_lbfgs_options.argtypes = [C.POINTER(abi.RtdLbfgsOptions)]
        L.rtd_default_lbfgs_options.restype = None
        L.rtd_optimizer_create_lbfgs.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdLbfgsOptions), vpp]
        L.rtd_optimizer_lbfgs_report.argtypes = [vp, vp, C.POINTER(abi.RtdLbfgsReport)]
        L.rtd_optimizer_lbfgs_buffers.argtypes = [vp, vp, C.POINTER(abi.RtdLbfgsBuffers)]
        L.rtd_optimizer_create_lbfgs_ex.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdLbfgsOptions), C.c_uint32, vpp]
        L.rtd_optimizer_lbfgs_line_buffers.argtypes = [vp, vp, C.POINTER(abi.RtdLbfgsLineBuffers)]
        L.rtd_objective_add_constraint.argtypes = [vp, vp, C.POINTER(abi.RtdDoseConstraint), C.POINTER(C.c_int32)]
        L.rtd_objective_constraint_layout.argtypes = [vp, vp, C.POINTER(abi.RtdConstraintLayout)]
        L.rtd_objective_eval_constrained.argtypes = [vp, vp, vp, vp, vp, C.c_double, vp, vp, vp]
        L.rtd_objective_update_multipliers.argtypes = [vp, vp, vp, C.c_double, C.c_double, C.c_double, vp, vp, vp]
        L.rtd_objective_constraint_violations.argtypes = [vp, vp, vp, C.c_double, vp]
        L.rtd_default_constrained_options.argtypes = [C.POINTER(abi.RtdConstrainedOptions)]
        L.rtd_default_constrained_options.restype = None
        L.rtd_optimizer_create_constrained.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdOptimizerOptions), C.POINTER(abi.RtdConstrainedOptions), vpp]
        L.rtd_optimizer_constraint_report.argtypes = [vp, vp, C.POINTER(abi.RtdConstraintReport), C.POINTER(abi.RtdConstraintOuter), C.c_uint32]
        L.rtd_optimizer_constraint_buffers.argtypes = [vp, vp, C.POINTER(abi.RtdConstraintBuffers)]
        L.rtd_optimizer_create_constrained_lbfgs.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdLbfgsOptions), C.POINTER(abi.RtdConstrainedOptions), C.c_uint32, vpp]
        L.rtd_optimizer_lbfgs_constraint_line.argtypes = [vp, vp, C.POINTER(abi.RtdLbfgsConstraintLineBuffers)]
        L.rtd_objective_constraint_trials.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_double, vp, vp]
        L.rtd_default_dij_compact_options.argtypes = [C.POINTER(abi.RtdDijCompactOptions)]
        L.rtd_default_dij_compact_options.restype = None
        L.rtd_field_dose_influence_compact.argtypes = [vp, vp, C.POINTER(abi.RtdDijCompactOptions)]
        L.rtd_field_dose_influence_compact_info.argtypes = [vp, vp, C.POINTER(abi.RtdDijCompactInfo)]
        L.rtd_field_dose_influence_compact_device.argtypes = [vp, vp, C.POINTER(abi.RtdDijCompactDevice)]
        L.rtd_field_dose_influence_apply_compact.argtypes = [vp, vp, vp, vp, C.c_int]
        L.rtd_field_dose_influence_apply_t_compact.argtypes = [vp, vp, vp, vp]
        L.rtd_optimizer_create_compact.argtypes = [vp, vpp, C.c_uint32, vp, C.POINTER(abi.RtdOptimizerOptions), vpp]
        L.rtd_optimizer_create_robust_compact.argtypes = L.rtd_optimizer_create_robust.argtypes
        L.rtd_optimizer_create_voxelwise_compact.argtypes = L.rtd_optimizer_create_voxelwise.argtypes
        L.rtd_host_register.argtypes = [vp, C.c_size_t]
        L.rtd_host_unregister.argtypes = [vp]
        L.rtd_plan_create.argtypes = [C.POINTER(C.c_int), C.c_int, vpp]
        L.rtd_plan_destroy.argtypes = [vp]
        L.rtd_plan_last_error.argtypes = [vp]
        L.rtd_plan_last_error.restype = C.c_char_p
        L.rtd_plan_set_options.argtypes = [vp, C.POINTER(abi.RtdOptions)]
        L.rtd_plan_set_luts.argtypes = [vp, C.POINTER(abi.RtdLuts)]
        L.rtd_plan_load_luts_dir.argtypes = [vp, C.c_char_p, C.c_int]
        L.rtd_plan_set_ct.argtypes = [vp, abi.c_float_p, u3]
        L.rtd_plan_set_ct_deferred.argtypes = [vp, abi.c_float_p, u3]
        L.rtd_set_ct_deferred.argtypes = [vp, abi.c_float_p, u3]
        L.rtd_plan_compute.argtypes = [vp, C.POINTER(abi.RtdBeam), C.c_int, abi.c_float_p, u3, C.POINTER(abi.RtdTiming),
                                       C.POINTER(abi.RtdPlanTiming)]
        L.rtd_device_alloc.argtypes = [vp, C.c_size_t, vpp]
        L.rtd_device_free.argtypes = [vp, vp]
        L.rtd_device_zero.argtypes = [vp, vp, C.c_size_t]
        L.rtd_copy_to_device.argtypes = [vp, vp, vp, C.c_size_t]
        L.rtd_copy_to_host.argtypes = [vp, vp, vp, C.c_size_t]
        L.rtd_sync.argtypes = [vp]
        L.rtd_stream.argtypes = [vp]
        L.rtd_stream.restype = vp
        L.rtd_set_stream.argtypes = [vp, vp]
        _LIB = L
    return _LIB


class DoseInfluence:
    """A field's dose-influence matrix in CSC form: column j (spot j of the [L][ny][nx] map) holds the dose of that spot at unit
    weight; rows are linear voxel indices of the dose grid (x fastest). shape = (n_voxels, n_spots). matvec / rmatvec in float64.
    scipy users: scipy.sparse.csc_matrix((d.data, d.indices, d.indptr), shape=d.shape)."""

    def __init__(self, indptr, indices, data, dose_dims, spot_shape):
        self.indptr = indptr
        self.indices = indices
        self.data = data
        self.dose_dims = tuple(int(v) for v in dose_dims)
        self.spot_shape = tuple(int(v) for v in spot_shape)
        self.shape = (int(np.prod(self.dose_dims)), int(indptr.size - 1))

    @property
    def nnz(self):
        return int(self.indptr[-1])

    def column(self, j):
        """(rows, values) of column j."""
        a, b = int(self.indptr[j]), int(self.indptr[j + 1])
        return self.indices[a:b], self.data[a:b]

    def _col_of_entry(self):
        return np.repeat(np.arange(self.shape[1], dtype=np.int64), np.diff(self.indptr))

    def matvec(self, w):
        """Dij w: the dose volume (float64, flat, n_voxels) of spot weights w ([L][ny][nx] or flat)."""
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        assert w.size == self.shape[1]
        out = np.zeros(self.shape[0], dtype=np.float64)
        np.add.at(out, self.indices, self.data.astype(np.float64) * w[self._col_of_entry()])
        return out

    def rmatvec(self, g):
        """Dij^T g: per-spot sums (float64, flat, n_spots) of a voxel-weight volume g (dose-grid shape or flat)."""
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        assert g.size == self.shape[0]
        prod = self.data.astype(np.float64) * g[self.indices]
        out = np.zeros(self.shape[1], dtype=np.float64)
        np.add.at(out, self._col_of_entry(), prod)
        return out


class Field:
    """One beam prepared on the device (rtd_field_*)."""

    def __init__(self, eng, beam, dose_dims, remote=False):
        self.eng = eng
        self._beam = beam            # keeps the numpy arrays alive
        self._h = C.c_void_p()
        ba = beam.as_abi()
        self._dims = tuple(int(d) for d in dose_dims)
        create = lib().rtd_field_create_remote if remote else lib().rtd_field_create
        eng._check(create(eng._h, C.byref(ba), abi.uint3(dose_dims), C.byref(self._h)))
        self.remote = remote
        self.computed = False        # a compute() has been launched (clear_dose / finish are valid)

    @staticmethod
    def _clip(lo, hi):
        if lo is None:
            return None, None
        return (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi])

    def compute_bev(self):
        """All kernels up to the beam's-eye-view dose; asynchronous."""
        self.eng._check(lib().rtd_field_compute_bev(self.eng._h, self._h))
        self.computed = True

    def transfer(self, dev_dose, clip_min=None, clip_max=None):
        """Fan -> dose-grid transfer of the field's BEV dose (its own or an attached slab) into dev_dose, optionally restricted
        to the inclusive dose-index box [clip_min, clip_max]; asynchronous."""
        lo, hi = self._clip(clip_min, clip_max)
        self.eng._check(lib().rtd_field_transfer(self.eng._h, self._h, C.c_void_p(int(dev_dose)), lo, hi))

    def transfer_init(self, dev_dose, clip_min=None, clip_max=None):
        """transfer() for the first field of a plan: the field's dose box is written (dose or zero), not accumulated into."""
        lo, hi = self._clip(clip_min, clip_max)
        self.eng._check(lib().rtd_field_transfer_init(self.eng._h, self._h, C.c_void_p(int(dev_dose)), lo, hi))

    def wait_plan(self):
        """(info, packed_bytes) once the device-side plan of the field is known (the superposition may still be running)."""
        i, n = abi.RtdFieldInfo(), C.c_size_t(0)
        self.eng._check(lib().rtd_field_wait_plan(self.eng._h, self._h, C.byref(i), C.byref(n)))
        return i.as_dict(), int(n.value)

    def message_bound(self):
        return int(lib().rtd_bev_message_bound(self.eng._h, self._h))

    def export_bev(self, dev_buf, capacity):
        """Pack [state record | non-zero block of the BEV dose] into dev_buf (device pointer); asynchronous."""
        self.eng._check(lib().rtd_field_export_bev(self.eng._h, self._h, C.c_void_p(int(dev_buf)), int(capacity)))

    def attach_bev(self, dev_buf):
        """Remote field: sample the message at dev_buf (device pointer; not copied)."""
        self.eng._check(lib().rtd_field_attach_bev(self.eng._h, self._h, C.c_void_p(int(dev_buf))))
        self.computed = True

    def clear_dose_box(self, dev_dose, clip_min=None, clip_max=None):
        lo, hi = self._clip(clip_min, clip_max)
        self.eng._check(lib().rtd_field_clear_dose_box(self.eng._h, self._h, C.c_void_p(int(dev_dose)), lo, hi))

    def compute(self, dev_dose):
        """Launch all kernels of the field; asynchronous. dev_dose: device pointer (int) of the dose volume."""
        self.eng._check(lib().rtd_field_compute(self.eng._h, self._h, C.c_void_p(int(dev_dose))))
        self.computed = True

    def spot_gradient(self, dev_g, dev_out):
        """rtd_field_spot_gradient: the gradient of <dose, g> with respect to the spot weights of the last compute, written to
        dev_out ([L][ny][nx] float32, device pointer); dev_g: the voxel-weight volume (device pointer, dose-grid shape).
        Asynchronous after the field's plan is known; the live rays are those of the last compute."""
        self.eng._check(lib().rtd_field_spot_gradient(self.eng._h, self._h, C.c_void_p(int(dev_g)), C.c_void_p(int(dev_out))))

    def dose_influence(self, rel_threshold=0.0):
        """rtd_field_dose_influence: the field's dose-influence matrix (n_voxels x n_spots, CSC) as a DoseInfluence. Needs
        ray_weight_cutoff = 0; the field's own state is that of a compute at its own weights afterwards."""
        e = lib()
        nnz = C.c_size_t(0)
        self.eng._check(e.rtd_field_dose_influence(self.eng._h, self._h, C.c_float(rel_threshold), C.byref(nnz)))
        shape = np.asarray(self._beam.spotWeights).shape
        n_spots = int(np.prod(shape))
        indptr = np.empty(n_spots + 1, dtype=np.int64)
        indices = np.empty(max(nnz.value, 1), dtype=np.int32)
        data = np.empty(max(nnz.value, 1), dtype=np.float32)
        self.eng._check(e.rtd_field_dose_influence_copy(self.eng._h, self._h, indptr.ctypes.data_as(C.c_void_p),
                                                        indices.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p)))
        self.computed = True
        return DoseInfluence(indptr, indices[:nnz.value], data[:nnz.value], self._dims, shape)

    def dose_influence_prepare(self):
        """rtd_field_dose_influence_prepare: builds, once per matrix, what dose_influence_apply / _apply_t need (synchronous)."""
        self.eng._check(lib().rtd_field_dose_influence_prepare(self.eng._h, self._h))

    def dose_influence_apply(self, dev_w, dev_dose, init=False):
        """rtd_field_dose_influence_apply: Dij w with the resident matrix of the last dose_influence(); dev_w [L][ny][nx] float32,
        dev_dose the dose volume (device pointers). init=False adds to the voxels that have entries; init=True writes the field's
        dose box (sum or 0). Asynchronous once prepared."""
        self.eng._check(lib().rtd_field_dose_influence_apply(self.eng._h, self._h, C.c_void_p(int(dev_w)), C.c_void_p(int(dev_dose)), int(bool(init))))

    def dose_influence_apply_t(self, dev_g, dev_out):
        """rtd_field_dose_influence_apply_t: Dij^T g written to dev_out ([L][ny][nx] float32); dev_g: the voxel-weight volume (device
        pointers). Asynchronous once prepared."""
        self.eng._check(lib().rtd_field_dose_influence_apply_t(self.eng._h, self._h, C.c_void_p(int(dev_g)), C.c_void_p(int(dev_out))))

    def dose_influence_apply_set(self, dev_w, dev_dose, n_plans, plan_stride=None, init=False):
        """rtd_field_dose_influence_apply_set: Dij w for n_plans weight vectors in one pass over the matrix. Plan-minor: element i of
        plan p at x[i * plan_stride + p] (pareto.interleave), for dev_w and dev_dose alike; plan_stride defaults to n_plans. Slot p
        holds the bits dose_influence_apply gives for plan p alone; slots p >= n_plans are not written."""
        stride = int(n_plans if plan_stride is None else plan_stride)
        self.eng._check(lib().rtd_field_dose_influence_apply_set(self.eng._h, self._h, C.c_void_p(int(dev_w)), C.c_void_p(int(dev_dose)), int(n_plans), stride,
                                                                 int(bool(init))))

    def dose_influence_apply_t_set(self, dev_g, dev_out, n_plans, plan_stride=None):
        """rtd_field_dose_influence_apply_t_set: Dij^T g for n_plans voxel-weight volumes in one pass over the matrix, plan-minor as
        dose_influence_apply_set; dev_out[j * plan_stride + p] is written for p < n_plans."""
        stride = int(n_plans if plan_stride is None else plan_stride)
        self.eng._check(lib().rtd_field_dose_influence_apply_t_set(self.eng._h, self._h, C.c_void_p(int(dev_g)), C.c_void_p(int(dev_out)), int(n_plans), stride))

    def dose_influence_device(self):
        """rtd_field_dose_influence_device: (col_ptr, row_idx, values, nnz) — the device pointers of the resident CSC arrays as ints
        (owned by the field, valid until its next dose_influence(), release or destroy) and the entry count."""
        cp, ri, va, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self.eng._check(lib().rtd_field_dose_influence_device(self.eng._h, self._h, C.byref(cp), C.byref(ri), C.byref(va), C.byref(n)))
        return int(cp.value or 0), int(ri.value or 0), int(va.value or 0), int(n.value)

    def dose_influence_compact(self, release_plain=False, options=None):
        """rtd_field_dose_influence_compact: builds the compact form of the matrix of the last dose_influence() (binary16 codes under
        one scale per spot, 16-bit indices; synchronous). release_plain=True then frees the plain form's bulk: until the next
        dose_influence() only the compact calls and Engine.create_compact_optimizer, create_robust_compact_optimizer and
        create_voxelwise_compact_optimizer work on the field. options: an
        abi.RtdDijCompactOptions instead of the keyword."""
        o = options if options is not None else abi.default_dij_compact_options()
        if options is None:
            o.release_plain = int(bool(release_plain))
        self.eng._check(lib().rtd_field_dose_influence_compact(self.eng._h, self._h, C.byref(o)))

    def dose_influence_compact_info(self):
        """rtd_field_dose_influence_compact_info: a dict of value_bits, col_bits, row_bits, lanes_per_row (G), entries_per_lane (E),
        plain_released, nnz, row_entries, compact_bytes, plain_bytes and released_bytes."""
        i = abi.RtdDijCompactInfo()
        self.eng._check(lib().rtd_field_dose_influence_compact_info(self.eng._h, self._h, C.byref(i)))
        return i.as_dict()

    def dose_influence_compact_device(self):
        """rtd_field_dose_influence_compact_device: the device pointers and sizes of the compact form (abi.RtdDijCompactDevice; owned
        by the field, valid until its next dose_influence(), release or destroy)."""
        d = abi.RtdDijCompactDevice()
        self.eng._check(lib().rtd_field_dose_influence_compact_device(self.eng._h, self._h, C.byref(d)))
        return d

    def dose_influence_apply_compact(self, dev_w, dev_dose, init=False):
        """rtd_field_dose_influence_apply_compact: Dij w with the compact form; arguments as dose_influence_apply. Launches only."""
        self.eng._check(lib().rtd_field_dose_influence_apply_compact(self.eng._h, self._h, C.c_void_p(int(dev_w)), C.c_void_p(int(dev_dose)), int(bool(init))))

    def dose_influence_apply_t_compact(self, dev_g, dev_out):
        """rtd_field_dose_influence_apply_t_compact: Dij^T g with the compact form; arguments as dose_influence_apply_t. Launches only."""
        self.eng._check(lib().rtd_field_dose_influence_apply_t_compact(self.eng._h, self._h, C.c_void_p(int(dev_g)), C.c_void_p(int(dev_out))))

    def water_depth(self, dev_depth):
        """rtd_field_water_depth: WRITES the field's water-equivalent depth (mm) of every voxel of its dose box into dev_depth (a
        volume on the dose grid, device pointer); nothing outside the box is touched. One launch after a compute of the field."""
        self.eng._check(lib().rtd_field_water_depth(self.eng._h, self._h, C.c_void_p(int(dev_depth))))

    def let_influence(self):
        """rtd_field_let_influence: the LET-weighted values N = float32(D * L) on the structure of the last dose_influence() matrix,
        from the engine's LET table (Engine.set_let_table). They live with the matrix."""
        self.eng._check(lib().rtd_field_let_influence(self.eng._h, self._h))

    def let_apply(self, dev_w, dev_out, init=False):
        """rtd_field_let_influence_apply: N w, the LET-weighted dose (keV/um x dose unit); arguments as dose_influence_apply."""
        self.eng._check(lib().rtd_field_let_influence_apply(self.eng._h, self._h, C.c_void_p(int(dev_w)), C.c_void_p(int(dev_out)), int(bool(init))))

    def let_apply_t(self, dev_g, dev_out):
        """rtd_field_let_influence_apply_t: N^T g; arguments as dose_influence_apply_t."""
        self.eng._check(lib().rtd_field_let_influence_apply_t(self.eng._h, self._h, C.c_void_p(int(dev_g)), C.c_void_p(int(dev_out))))

    def let_influence_device(self):
        """rtd_field_let_influence_device: (values, nnz) — the device pointer of the CSC LET values as an int and the entry count; the
        indices are those of dose_influence_device()."""
        va, n = C.c_void_p(), C.c_size_t(0)
        self.eng._check(lib().rtd_field_let_influence_device(self.eng._h, self._h, C.byref(va), C.byref(n)))
        return int(va.value or 0), int(n.value)

    def set_spot_weights(self, dev_spot_weights):
        """rtd_field_set_spot_weights: new [L][ny][nx] float32 weights from device memory (stream-ordered)."""
        self.eng._check(lib().rtd_field_set_spot_weights(self.eng._h, self._h, C.c_void_p(int(dev_spot_weights))))

    def project_target(self, mask_or_roi):
        """rtd_field_project_target: the target in the field's beam's-eye view, kept with the field for select_spots(); returns the
        summary as a dict (n_samples, wepl_min, wepl_max, ray_lo, ray_hi, step_lo, step_hi). mask_or_roi: a device pointer (int) of a
        uint8 mask on the dose grid (x fastest, non-zero = inside), a numpy [Z][Y][X] uint8 or bool array (uploaded), or a Roi (its
        fill_mask). Needs a compute of the field; synchronous."""
        n = self._dims[0] * self._dims[1] * self._dims[2]
        own = None
        if isinstance(mask_or_roi, Roi):
            if tuple(mask_or_roi.dims) != self._dims:
                raise ValueError("the ROI's grid %r is not the field's dose grid %r" % (mask_or_roi.dims, self._dims))
            own = self.eng.device_alloc(n)
            mask_or_roi.fill_mask(own)
        elif isinstance(mask_or_roi, np.ndarray):
            a = np.ascontiguousarray(mask_or_roi != 0, dtype=np.uint8)
            if a.size != n:
                raise ValueError("the mask has %d voxels, the dose grid %d" % (a.size, n))
            own = self.eng.device_alloc(n)
            self.eng.to_device(own, a)
        info = abi.RtdTargetInfo()
        try:
            ptr = own if own is not None else (int(mask_or_roi) if mask_or_roi else None)
            self.eng._check(lib().rtd_field_project_target(self.eng._h, self._h, C.c_void_p(ptr) if ptr else None, C.byref(info)))
        finally:
            if own is not None:
                self.eng.device_free(own)      # (the call has waited for its kernel)
        return info.as_dict()

    def select_spots(self, lateral=0.0, proximal=0.0, distal=0.0, dev_out=None):
        """rtd_field_select_spots: the [L][ny][nx] uint8 mask (1 = selected) of the spots whose layer's Bragg peak, widened by the
        water-equivalent margins proximal / distal (mm), lands on the projected target on a ray within lateral (mm, isocentre plane)
        of the spot. Without dev_out the mask is returned as a numpy array; with dev_out (device pointer, L * ny * nx bytes) it is
        written there, launches only, and None is returned."""
        o = abi.RtdTargetOptions()
        o.lateral_margin_mm, o.proximal_margin_mm, o.distal_margin_mm = float(lateral), float(proximal), float(distal)
        if dev_out is not None:
            self.eng._check(lib().rtd_field_select_spots(self.eng._h, self._h, C.byref(o), C.c_void_p(int(dev_out)), None))
            return None
        out = np.empty(np.asarray(self._beam.spotWeights).shape, dtype=np.uint8)
        d = self.eng.device_alloc(max(out.nbytes, 1))
        try:
            self.eng._check(lib().rtd_field_select_spots(self.eng._h, self._h, C.byref(o), C.c_void_p(d), None))
            self.eng.to_host(out, d)
        finally:
            self.eng.device_free(d)
        return out

    def clear_dose(self, dev_dose):
        """Zero the voxels of dev_dose that the last compute() of this field could have changed; asynchronous."""
        self.eng._check(lib().rtd_field_clear_dose(self.eng._h, self._h, C.c_void_p(int(dev_dose))))

    def finish(self):
        t, i = abi.RtdTiming(), abi.RtdFieldInfo()
        self.eng._check(lib().rtd_field_finish(self.eng._h, self._h, C.byref(t), C.byref(i)))
        return t.as_dict(), i.as_dict()

    def fetch(self, name):
        n = C.c_size_t(0)
        self.eng._check(lib().rtd_field_fetch(self.eng._h, self._h, name.encode(), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        self.eng._check(lib().rtd_field_fetch(self.eng._h, self._h, name.encode(), out.ctypes.data_as(C.c_void_p), n.value, None))
        return out.view(_FETCH_DTYPES.get(name, np.float32))

    def destroy(self):
        if self._h:
            lib().rtd_field_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()

    def release(self):
        """Like destroy(), but the device workspace stays with the engine for the next field of the same shape."""
        if self._h:
            lib().rtd_field_release(self.eng._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Objective:
    """rtd_objective_*: ROIs and penalty terms on one dose grid; eval() gives the objective, its terms and the voxel gradient on the
    device. Kinds: abi.RTD_OBJ_SQ_DEVIATION / _SQ_OVERDOSE / _SQ_UNDERDOSE / _MEAN; through add_dvh_term abi.RTD_OBJ_MAX_DVH / _MIN_DVH.
    dose_at_volume() and dvh() report on a dose volume in dose-volume terms. Through add_eud_term abi.RTD_OBJ_SQ_EUD / _SQ_MAX_EUD /
    _SQ_MIN_EUD; eud() reports the generalised equivalent uniform dose of ROIs."""

    def __init__(self, eng, dose_dims):
        self.eng = eng
        self._h = C.c_void_p()
        self.dims = tuple(int(d) for d in dose_dims)
        self.n_terms = 0
        self.n_rois = 0
        self.n_constraints = 0
        eng._check(lib().rtd_objective_create(eng._h, abi.uint3(self.dims), C.byref(self._h)))

    def add_roi(self, mask_or_indices):
        """A boolean mask of the dose grid ([Z][Y][X] or flat) or linear voxel indices (strictly ascending) -> the ROI's id."""
        a = np.asarray(mask_or_indices)
        idx = np.flatnonzero(a) if a.dtype == np.bool_ else a.reshape(-1)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        rid = C.c_int32(-1)
        self.eng._check(lib().rtd_objective_add_roi(self.eng._h, self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size, C.byref(rid)))
        self.n_rois += 1
        return int(rid.value)

    def add_term(self, kind, roi, weight, level=0.0):
        t = abi.RtdObjectiveTerm(int(kind), int(roi), float(weight), float(level))
        self.eng._check(lib().rtd_objective_add_term(self.eng._h, self._h, C.byref(t)))
        self.n_terms += 1

    def add_dvh_term(self, kind, roi, weight, level, volume_fraction):
        """A dose-volume term: RTD_OBJ_MAX_DVH (at most volume_fraction of the ROI above level) or RTD_OBJ_MIN_DVH (at least
        volume_fraction of the ROI receives level). It takes the next term number, like add_term."""
        t = abi.RtdObjectiveDvhTerm(int(kind), int(roi), float(weight), float(level), float(volume_fraction))
        self.eng._check(lib().rtd_objective_add_dvh_term(self.eng._h, self._h, C.byref(t)))
        self.n_terms += 1

    def dose_at_volume(self, dev_dose, queries, dev_out=None):
        """rtd_objective_dose_at_volume: queries = [(roi, volume_fraction), ...] (at most abi.RTD_DVH_MAX_QUERIES). With dev_out (device
        pointer, float32[n]) asynchronous, returns None; without, returns the doses as a float32 array."""
        qs = list(queries)
        arr = (abi.RtdDvhQuery * max(1, len(qs)))(*[abi.RtdDvhQuery(int(r), 0, float(v)) for r, v in qs])
        own = dev_out is None
        do = self.eng.device_alloc(4 * abi.RTD_DVH_MAX_QUERIES) if own else dev_out
        try:
            self.eng._check(lib().rtd_objective_dose_at_volume(self.eng._h, self._h, C.c_void_p(int(dev_dose)), arr, len(qs), C.c_void_p(int(do))))
            if own:
                out = np.empty(len(qs), dtype=np.float32)
                self.eng.to_host(out, do)
                return out
        finally:
            if own:
                self.eng.device_free(do)
        return None

    def add_eud_term(self, kind, roi, weight, level, exponent):
        """A term on the ROI's generalised equivalent uniform dose E = level * mean((d / level)^exponent)^(1 / exponent):
        RTD_OBJ_SQ_EUD (E equal to level), RTD_OBJ_SQ_MAX_EUD (at most) or RTD_OBJ_SQ_MIN_EUD (at least); weight * (E - level)^2. It
        takes the next term number, like add_term."""
        t = abi.RtdObjectiveEudTerm(int(kind), int(roi), float(weight), float(level), float(exponent), 0.0)
        self.eng._check(lib().rtd_objective_add_eud_term(self.eng._h, self._h, C.byref(t)))
        self.n_terms += 1

    def eud(self, dev_dose, queries, dev_out=None):
        """rtd_objective_eud: queries = [(roi, level, exponent), ...] (at most abi.RTD_EUD_MAX_QUERIES; level is the normalisation).
        With dev_out (device pointer, float64[n]) asynchronous, returns None; without, returns the gEUDs as a float64 array."""
        qs = list(queries)
        arr = (abi.RtdEudQuery * max(1, len(qs)))(*[abi.RtdEudQuery(int(r), 0, float(lv), float(a)) for r, lv, a in qs])
        own = dev_out is None
        do = self.eng.device_alloc(8 * abi.RTD_EUD_MAX_QUERIES) if own else dev_out
        try:
            self.eng._check(lib().rtd_objective_eud(self.eng._h, self._h, C.c_void_p(int(dev_dose)), arr, len(qs), C.c_void_p(int(do))))
            if own:
                out = np.empty(len(qs), dtype=np.float64)
                self.eng.to_host(out, do)
                return out
        finally:
            if own:
                self.eng.device_free(do)
        return None

    def dvh(self, dev_dose, n_bins, dose_max, dev_counts=None):
        """rtd_objective_dvh: the cumulative dose-volume histogram of every ROI, counts[roi][b] = voxels of the ROI with
        dose >= b * dose_max / n_bins. With dev_counts (device pointer, uint32[rois * n_bins]) asynchronous, returns None; without,
        returns a uint32 array [rois, n_bins]."""
        own = dev_counts is None
        nbytes = 4 * max(1, self.n_rois) * max(1, int(n_bins))
        dc = self.eng.device_alloc(nbytes) if own else dev_counts
        try:
            self.eng._check(lib().rtd_objective_dvh(self.eng._h, self._h, C.c_void_p(int(dev_dose)), int(n_bins), float(dose_max), C.c_void_p(int(dc))))
            if own:
                out = np.empty((self.n_rois, int(n_bins)), dtype=np.uint32)
                self.eng.to_host(out, dc)
                return out
        finally:
            if own:
                self.eng.device_free(dc)
        return None

    def eval(self, dev_dose, dev_g, dev_values=None):
        """rtd_objective_eval: dev_dose, dev_g device pointers of float32 volumes (dev_g zeroed once by the caller: only the voxels
        of the ROIs are written). With dev_values (device pointer, float64[1 + n_terms]) asynchronous, returns None; without,
        returns the values as a float64 array ([0] the objective, [1 + t] term t)."""
        own = dev_values is None
        dv = self.eng.device_alloc(8 * (1 + abi.RTD_OBJ_MAX_TERMS)) if own else dev_values
        try:
            self.eng._check(lib().rtd_objective_eval(self.eng._h, self._h, C.c_void_p(int(dev_dose)), C.c_void_p(int(dv)), C.c_void_p(int(dev_g))))
            if own:
                out = np.empty(1 + self.n_terms, dtype=np.float64)
                self.eng.to_host(out, dv)
                return out
        finally:
            if own:
                self.eng.device_free(dv)
        return None

    def eval_voxelwise(self, dose_ptrs, grad_ptrs, dev_values=None, dev_active=None):
        """rtd_objective_eval_voxelwise: the composite (voxel-wise worst case) objective of the scenario volumes dose_ptrs (device
        pointers of float32 volumes, at most abi.RTD_ROBUST_MAX_SCENARIOS), its voxel gradient scattered over the volumes grad_ptrs
        (one per scenario, zeroed once by the caller: only the voxels of the ROIs are written). With dev_values (float64[1 + n_terms])
        and dev_active (one uint32), both device pointers, asynchronous, returns None; without, returns (values float64 array,
        active mask: bit s set iff scenario s received a gradient that is not zero)."""
        doses, grads = [int(p) for p in dose_ptrs], [int(p) for p in grad_ptrs]
        if len(doses) != len(grads):
            raise ValueError("one gradient volume per scenario")
        own = dev_values is None or dev_active is None
        nv = 8 * (1 + abi.RTD_OBJ_MAX_TERMS)
        buf = self.eng.device_alloc(nv + 8) if own else None
        dv, da = (buf, buf + nv) if own else (dev_values, dev_active)
        try:
            self.eng._check(lib().rtd_objective_eval_voxelwise(self.eng._h, self._h, (C.c_void_p * max(1, len(doses)))(*doses), len(doses), C.c_void_p(int(dv)),
                                                               (C.c_void_p * max(1, len(grads)))(*grads), C.c_void_p(int(da))))
            if own:
                out, active = np.empty(1 + self.n_terms, dtype=np.float64), np.zeros(1, dtype=np.uint32)
                self.eng.to_host(out, dv)
                self.eng.to_host(active, da)
                return out, int(active[0])
        finally:
            if own:
                self.eng.device_free(buf)
        return None

    def add_constraint(self, kind, roi, level):
        """rtd_objective_add_constraint: a hard bound, abi.RTD_CON_MAX_DOSE / _MIN_DOSE on every voxel of the ROI or abi.RTD_CON_MAX_MEAN /
        _MIN_MEAN on its mean dose -> the constraint's number. eval() and the other calls above ignore constraints; only
        Engine.create_constrained_optimizer accepts an objective that has one."""
        c = abi.RtdDoseConstraint(int(kind), int(roi), float(level))
        cid = C.c_int32(-1)
        self.eng._check(lib().rtd_objective_add_constraint(self.eng._h, self._h, C.byref(c), C.byref(cid)))
        self.n_constraints = getattr(self, "n_constraints", 0) + 1
        return int(cid.value)

    def constraint_layout(self):
        """rtd_objective_constraint_layout: builds the constraint tables where needed; an abi.RtdConstraintLayout (device pointers of the
        union of the constrained ROIs and the CSR of the per-voxel constraints; n_entries floats of multipliers)."""
        lay = abi.RtdConstraintLayout()
        self.eng._check(lib().rtd_objective_constraint_layout(self.eng._h, self._h, C.byref(lay)))
        return lay

    def eval_constrained(self, dev_dose, dev_lambda, dev_mu, rho, dev_g, dev_values=None, dev_con_values=None):
        """rtd_objective_eval_constrained: the augmented Lagrangian F of the dose, the multipliers dev_lambda (float32[n_entries]) and
        dev_mu (float64[abi.RTD_CON_MAX_CONSTRAINTS]) and the penalty rho; dev_g receives the combined voxel gradient. With dev_values
        (float64[1 + n_terms]) and dev_con_values (float64[1 + n_constraints]), both device pointers, asynchronous, returns None;
        without, returns (values, con_values): values[0] = F, con_values[0] the terms alone, con_values[1 + c] = psi_c."""
        own = dev_values is None or dev_con_values is None
        nv = 8 * (1 + abi.RTD_OBJ_MAX_TERMS)
        buf = self.eng.device_alloc(nv + 8 * (1 + abi.RTD_CON_MAX_CONSTRAINTS)) if own else None
        dv, dc = (buf, buf + nv) if own else (dev_values, dev_con_values)
        try:
            self.eng._check(lib().rtd_objective_eval_constrained(self.eng._h, self._h, C.c_void_p(int(dev_dose)), C.c_void_p(int(dev_lambda)), C.c_void_p(int(dev_mu)),
                                                                 float(rho), C.c_void_p(int(dv)), C.c_void_p(int(dc)), C.c_void_p(int(dev_g))))
            if own:
                vals = np.empty(1 + self.n_terms, dtype=np.float64)
                cons = np.empty(1 + getattr(self, "n_constraints", 0), dtype=np.float64)
                self.eng.to_host(vals, dv)
                self.eng.to_host(cons, dc)
                return vals, cons
        finally:
            if own:
                self.eng.device_free(buf)
        return None

    def constraint_trials(self, dev_d0, dev_d1, n_trials, dev_lambda, dev_mu, rho, dev_psi=None, dev_mean=None):
        """rtd_objective_constraint_trials: the constraint half of an L-BFGS line search on the float32 trial volumes r_k formed from
        dev_d0 and dev_d1, k < n_trials: psi[k][c] and the means mean[k][c] (rows of abi.RTD_CON_MAX_CONSTRAINTS float64). With dev_psi
        and dev_mean (device pointers) asynchronous, returns None; without, returns (psi, mean) as float64[n_trials][16]."""
        own = dev_psi is None or dev_mean is None
        nb = 8 * abi.RTD_CON_MAX_CONSTRAINTS * max(1, int(n_trials))
        buf = self.eng.device_alloc(2 * nb) if own else None
        dp, dm = (buf, buf + nb) if own else (dev_psi, dev_mean)
        try:
            self.eng._check(lib().rtd_objective_constraint_trials(self.eng._h, self._h, C.c_void_p(int(dev_d0)), C.c_void_p(int(dev_d1)), int(n_trials),
                                                                  C.c_void_p(int(dev_lambda)), C.c_void_p(int(dev_mu)), float(rho), C.c_void_p(int(dp)), C.c_void_p(int(dm))))
            if own:
                psi = np.empty((int(n_trials), abi.RTD_CON_MAX_CONSTRAINTS), dtype=np.float64)
                mean = np.empty_like(psi)
                self.eng.to_host(psi, dp)
                self.eng.to_host(mean, dm)
                return psi, mean
        finally:
            if own:
                self.eng.device_free(buf)
        return None

    def _violations(self, call, dev_out):
        own = dev_out is None
        do = self.eng.device_alloc(16 * abi.RTD_CON_MAX_CONSTRAINTS) if own else dev_out
        try:
            self.eng._check(call(C.c_void_p(int(do))))
            if own:
                out = (abi.RtdConstraintViolation * abi.RTD_CON_MAX_CONSTRAINTS)()
                raw = np.empty(16 * abi.RTD_CON_MAX_CONSTRAINTS, dtype=np.uint8)
                self.eng.to_host(raw, do)
                C.memmove(out, raw.ctypes.data, raw.nbytes)
                n = getattr(self, "n_constraints", 0)
                return np.array([out[c].max_violation for c in range(n)], dtype=np.float64), np.array([out[c].n_violating for c in range(n)], dtype=np.uint32)
        finally:
            if own:
                self.eng.device_free(do)
        return None

    def update_multipliers(self, dev_dose, rho, dev_lambda, dev_mu, lambda_max=1e20, tol=0.0, dev_out=None):
        """rtd_objective_update_multipliers: lambda <- min(max(lambda + rho h, 0), lambda_max) in place (mu likewise), and per
        constraint the largest violation and the number of entries with h > tol. With dev_out (device pointer of
        abi.RtdConstraintViolation[n_constraints]) asynchronous, returns None; without, returns (max_violation float64[n_constraints],
        n_violating uint32[n_constraints])."""
        return self._violations(lambda do: lib().rtd_objective_update_multipliers(self.eng._h, self._h, C.c_void_p(int(dev_dose)), float(rho), float(lambda_max), float(tol),
                                                                                 C.c_void_p(int(dev_lambda)), C.c_void_p(int(dev_mu)), do), dev_out)

    def constraint_violations(self, dev_dose, tol=0.0, dev_out=None):
        """rtd_objective_constraint_violations: what update_multipliers measures, without the update."""
        return self._violations(lambda do: lib().rtd_objective_constraint_violations(self.eng._h, self._h, C.c_void_p(int(dev_dose)), float(tol), do), dev_out)

    def destroy(self):
        if self._h:
            lib().rtd_objective_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()


class Roi:
    """rtd_roi_*: the voxels of the dose grid inside the closed planar contours of one structure (Engine.rasterize_roi). voxels() is what
    Objective.add_roi takes."""

    def __init__(self, eng, dims, world_to_idx, contours, plane_thickness_mm):
        self.eng = eng
        self._h = C.c_void_p()
        self.dims = tuple(int(d) for d in dims)
        g = abi.RtdRoiGrid()
        for i in range(3):
            g.dims[i] = self.dims[i]
        g.world_to_idx = world_to_idx if isinstance(world_to_idx, abi.RtdAffine) else abi.make_affine(*world_to_idx)
        g.plane_thickness_mm = float(plane_thickness_mm)
        cs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in contours]
        pts = np.ascontiguousarray(np.concatenate(cs, axis=0)) if cs else np.zeros((1, 3), dtype=np.float32)
        offs = np.zeros(len(cs) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(c) for c in cs], dtype=np.int64)
        s = abi.RtdContourSet()
        s.points = abi.fptr(pts)
        s.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
        s.n_contours = len(cs)
        eng._check(lib().rtd_roi_rasterize(eng._h, C.byref(g), C.byref(s), C.byref(self._h)))
        self._read_info()

    def _read_info(self):
        i = abi.RtdRoiInfo()
        self.eng._check(lib().rtd_roi_get_info(self.eng._h, self._h, C.byref(i)))
        self.info = i.as_dict()

    @classmethod
    def _adopt(cls, eng, dims, handle):
        """The Roi of a handle that a call returned (rtd_roi_margin, rtd_roi_combine, rtd_roi_from_mask): it owns the handle."""
        r = cls.__new__(cls)
        r.eng = eng
        r._h = handle
        r.dims = tuple(int(d) for d in dims)
        r._read_info()
        return r

    @staticmethod
    def _six(margin_mm):
        """A scalar, 3 values (one per axis, both sides) or 6 values (-x, +x, -y, +y, -z, +z) -> 6 floats."""
        m = np.atleast_1d(np.asarray(margin_mm, dtype=np.float32)).reshape(-1)
        if m.size == 1:
            m = np.repeat(m, 6)
        elif m.size == 3:
            m = np.repeat(m, 2)
        elif m.size != 6:
            raise ValueError("margin_mm: a scalar, 3 or 6 values, not %d" % m.size)
        return (C.c_float * 6)(*[float(v) for v in m])

    def _margin(self, margin_mm, spacing_mm, contract):
        sp = (C.c_float * 3)(*[float(np.float32(v)) for v in spacing_mm])
        out = C.c_void_p()
        self.eng._check(lib().rtd_roi_margin(self.eng._h, self._h, sp, self._six(margin_mm), int(contract), C.byref(out)))
        return Roi._adopt(self.eng, self.dims, out)

    def expand(self, margin_mm, spacing_mm):
        """rtd_roi_margin: the ROI grown by margin_mm (a scalar, one value per axis, or (-x, +x, -y, +y, -z, +z)) on the grid of
        spacing_mm (x, y, z) -> a new Roi; this one is unchanged."""
        return self._margin(margin_mm, spacing_mm, 0)

    def contract(self, margin_mm, spacing_mm):
        """rtd_roi_margin with contract = 1: the +x margin moves the +x surface inward; the grid boundary does not erode."""
        return self._margin(margin_mm, spacing_mm, 1)

    def _combine(self, o, op):
        out = C.c_void_p()
        self.eng._check(lib().rtd_roi_combine(self.eng._h, self._h, o._h, int(op), C.byref(out)))
        return Roi._adopt(self.eng, self.dims, out)

    def union(self, o):
        return self._combine(o, abi.RTD_ROI_OR)

    def intersect(self, o):
        return self._combine(o, abi.RTD_ROI_AND)

    def subtract(self, o):
        """The voxels of this ROI that are not in o."""
        return self._combine(o, abi.RTD_ROI_ANDNOT)

    def xor(self, o):
        return self._combine(o, abi.RTD_ROI_XOR)

    def ring(self, inner_mm, outer_mm, spacing_mm):
        """expand(outer_mm) without expand(inner_mm); the two expansions are closed."""
        outer = self.expand(outer_mm, spacing_mm)
        try:
            inner = self.expand(inner_mm, spacing_mm)
            try:
                return outer.subtract(inner)
            finally:
                inner.close()
        finally:
            outer.close()

    def voxels(self):
        """The linear voxel indices ((k ny + j) nx + i, strictly ascending) as a numpy int32 array."""
        out = np.empty(self.info["n_voxels"], dtype=np.int32)
        self.eng._check(lib().rtd_roi_voxels(self.eng._h, self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    def device(self):
        """(device pointer of the int32 list, its length); owned by the ROI."""
        p, n = C.c_void_p(), C.c_size_t(0)
        self.eng._check(lib().rtd_roi_device(self.eng._h, self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def fill_mask(self, t):
        """Writes the whole uint8 volume t (a device pointer, or anything with data_ptr(): a torch.uint8 tensor of the grid's size)
        with 1 inside and 0 outside; asynchronous on the engine's stream."""
        ptr = t.data_ptr() if hasattr(t, "data_ptr") else int(t)
        self.eng._check(lib().rtd_roi_fill_mask(self.eng._h, self._h, C.c_void_p(ptr)))

    def kernel_ms(self):
        ms = C.c_float(0.0)
        self.eng._check(lib().rtd_roi_kernel_ms(self.eng._h, self._h, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if self._h:
            lib().rtd_roi_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()


class Rbe:
    """rtd_rbe_*: a variable-RBE model on a dose grid (Engine.create_rbe): one tissue class per voxel, class 0 (the default tissue)
    everywhere until assign() says otherwise. Tissues are abi.RtdRbeTissue records; raytracedicom_amd.rbe.tissue makes the named ones."""

    def __init__(self, eng, dims, tissue):
        self.eng = eng
        self._h = C.c_void_p()
        self.dims = tuple(int(d) for d in dims)
        self.n_voxels = self.dims[0] * self.dims[1] * self.dims[2]
        eng._check(lib().rtd_rbe_create(eng._h, abi.uint3(self.dims), C.byref(tissue), C.byref(self._h)))

    def add_tissue(self, tissue):
        """rtd_rbe_add_tissue -> the new class (1 .. 255)."""
        c = C.c_int32(-1)
        self.eng._check(lib().rtd_rbe_add_tissue(self.eng._h, self._h, C.byref(tissue), C.byref(c)))
        return int(c.value)

    def assign(self, where, class_id):
        """The class of a set of voxels: a Roi (its resident list, no copy to the host), a bool mask of the grid's size or an array of
        linear voxel indices. A later assignment overwrites an earlier one."""
        if isinstance(where, Roi):
            self.eng._check(lib().rtd_rbe_assign_roi(self.eng._h, self._h, where._h, int(class_id)))
            return
        a = np.asarray(where)
        idx = np.flatnonzero(a) if a.dtype == np.bool_ else a.reshape(-1)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.eng._check(lib().rtd_rbe_assign_voxels(self.eng._h, self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size, int(class_id)))

    @staticmethod
    def _box(box):
        if box is None:
            return None
        lo, hi = box
        return (C.c_int32 * 6)(*[int(v) for v in lo], *[int(v) for v in hi])

    def dose(self, dev_dose, dev_let_dose, dev_out, box=None):
        """rtd_rbe_dose: WRITES the RBE-weighted dose of the voxels of box ((min[3], max[3]) inclusive; None: the grid) into dev_out
        (device pointers; dev_out may be one of the inputs). One launch on the engine's stream."""
        self.eng._check(lib().rtd_rbe_dose(self.eng._h, self._h, C.c_void_p(int(dev_dose)), C.c_void_p(int(dev_let_dose)), self._box(box),
                                           C.c_void_p(int(dev_out))))

    def backward(self, dev_dose, dev_let_dose, dev_g_rbe, dev_g_dose, dev_g_let, box=None):
        """rtd_rbe_backward: WRITES g_d = g_R * dR/dd and g_n = g_R * dR/dn of the voxels of box into two volumes."""
        self.eng._check(lib().rtd_rbe_backward(self.eng._h, self._h, C.c_void_p(int(dev_dose)), C.c_void_p(int(dev_let_dose)), C.c_void_p(int(dev_g_rbe)),
                                               self._box(box), C.c_void_p(int(dev_g_dose)), C.c_void_p(int(dev_g_let))))

    def classes_device(self):
        """Device pointer of the uint8 class volume (owned by the object)."""
        p = C.c_void_p()
        self.eng._check(lib().rtd_rbe_classes_device(self.eng._h, self._h, C.byref(p)))
        return int(p.value or 0)

    def classes(self):
        """Waits; the class volume as a flat numpy uint8 array."""
        out = np.empty(self.n_voxels, dtype=np.uint8)
        self.eng.to_host(out, self.classes_device())
        return out

    def destroy(self):
        if self._h:
            lib().rtd_rbe_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()


class Optimizer:
    """rtd_optimizer_*: the resident spectral projected gradient iteration on an Objective of the dose of `fields` (each with a
    dose_influence() matrix). Destroy it before its fields, its objective and its engine."""

    def __init__(self, eng, fields, objective, options=None, scenario_fields=None, mode=None, probabilities=None, voxelwise=False, phase_warps=None,
                 phase_weights=None, lbfgs=False, compact=False, lbfgs_flags=None, constrained=None):
        """scenario_fields (a list of per-scenario field lists, scenario 0 the nominal one) makes it a robust optimiser
        (rtd_optimizer_create_robust) in mode abi.RTD_ROBUST_EXPECTED / _WORST_CASE, or with voxelwise=True the voxel-wise worst case
        (rtd_optimizer_create_voxelwise; mode and probabilities are then not used); `fields` is then ignored. With phase_warps (a list
        of abi.RtdWarp, one per row of scenario_fields) the rows are breathing phases and it is a 4D optimiser
        (rtd_optimizer_create_4d; phase_weights: one positive weight per phase, None for equal ones). With lbfgs=True it is the
        L-BFGS iteration with its line search on the device (rtd_optimizer_create_lbfgs; options: an abi.RtdLbfgsOptions or None). With
        compact=True it is the spectral iteration on the fields' compact matrices (rtd_optimizer_create_compact), and with
        scenario_fields the robust or voxel-wise one on them (rtd_optimizer_create_robust_compact, _create_voxelwise_compact). With
        lbfgs=True and lbfgs_flags (an int, abi.RTD_LBFGS_COMPACT or 0) it is rtd_optimizer_create_lbfgs_ex: L-BFGS on an objective
        of any term kind, on the compact matrices with the flag. With constrained (an abi.RtdConstrainedOptions, or True for the
        defaults) it is the augmented Lagrangian of rtd_optimizer_create_constrained on an objective that has hard constraints; with
        lbfgs=True beside it, the one of rtd_optimizer_create_constrained_lbfgs (options: an abi.RtdLbfgsOptions or None)."""
        self.eng = eng
        self.objective = objective
        self._h = C.c_void_p()
        self.is_lbfgs = bool(lbfgs)
        po = C.byref(options) if options is not None else None
        if scenario_fields is None:
            self.fields = list(fields)
            self.scenario_fields = [self.fields]
            arr = (C.c_void_p * max(1, len(self.fields)))(*[f._h for f in self.fields])
            if constrained is not None and constrained is not False:
                pc = C.byref(constrained) if isinstance(constrained, abi.RtdConstrainedOptions) else None
                if lbfgs:
                    eng._check(lib().rtd_optimizer_create_constrained_lbfgs(eng._h, arr, len(self.fields), objective._h, po, pc, int(lbfgs_flags or 0),
                                                                            C.byref(self._h)))
                    return
                eng._check(lib().rtd_optimizer_create_constrained(eng._h, arr, len(self.fields), objective._h, po, pc, C.byref(self._h)))
                return
            if lbfgs and lbfgs_flags is not None:
                eng._check(lib().rtd_optimizer_create_lbfgs_ex(eng._h, arr, len(self.fields), objective._h, po, int(lbfgs_flags), C.byref(self._h)))
                return
            if lbfgs:
                eng._check(lib().rtd_optimizer_create_lbfgs(eng._h, arr, len(self.fields), objective._h, po, C.byref(self._h)))
                return
            if compact:
                eng._check(lib().rtd_optimizer_create_compact(eng._h, arr, len(self.fields), objective._h, po, C.byref(self._h)))
                return
            eng._check(lib().rtd_optimizer_create(eng._h, arr, len(self.fields), objective._h, po, C.byref(self._h)))
            return
        self.scenario_fields = [list(fs) for fs in scenario_fields]
        self.fields = self.scenario_fields[0] if self.scenario_fields else []
        n_fields = len(self.fields)
        if any(len(fs) != n_fields for fs in self.scenario_fields):
            raise ValueError("every scenario needs the same number of fields")
        flat = [f._h for fs in self.scenario_fields for f in fs]
        arr = (C.c_void_p * max(1, len(flat)))(*flat)
        if phase_warps is not None:
            fo = abi.Rtd4dOptions()
            fo.n_phases = len(self.scenario_fields)
            if len(phase_warps) != len(self.scenario_fields):
                raise ValueError("one warp per phase")
            self._warps = (abi.RtdWarp * max(1, len(phase_warps)))(*phase_warps)
            fo.warps = self._warps
            if phase_weights is not None:
                pw = np.ascontiguousarray(phase_weights, dtype=np.float32).reshape(-1)
                if pw.size != len(self.scenario_fields):
                    raise ValueError("one weight per phase")
                fo.weights = abi.fptr(pw)
            eng._check(lib().rtd_optimizer_create_4d(eng._h, arr, n_fields, C.byref(fo), objective._h, po, C.byref(self._h)))
            return
        if voxelwise:
            create = lib().rtd_optimizer_create_voxelwise_compact if compact else lib().rtd_optimizer_create_voxelwise
            eng._check(create(eng._h, arr, n_fields, len(self.scenario_fields), objective._h, po, C.byref(self._h)))
            return
        ro = abi.RtdRobustOptions()
        ro.mode = int(abi.RTD_ROBUST_EXPECTED if mode is None else mode)
        ro.n_scenarios = len(self.scenario_fields)
        if probabilities is not None:
            pr = np.ascontiguousarray(probabilities, dtype=np.float64).reshape(-1)
            if pr.size != len(self.scenario_fields):
                raise ValueError("one probability per scenario")
            ro.probabilities = pr.ctypes.data_as(C.POINTER(C.c_double))
        create = lib().rtd_optimizer_create_robust_compact if compact else lib().rtd_optimizer_create_robust
        eng._check(create(eng._h, arr, n_fields, C.byref(ro), objective._h, po, C.byref(self._h)))

    def set_weights(self, field_index, dev_w):
        self.eng._check(lib().rtd_optimizer_set_weights(self.eng._h, self._h, int(field_index), C.c_void_p(int(dev_w))))

    def run(self, n_iterations):
        """Launches n_iterations iterations on the engine's stream; asynchronous."""
        self.eng._check(lib().rtd_optimizer_run(self.eng._h, self._h, int(n_iterations)))

    def result(self, capacity=None):
        """Waits; (report dict, history float64 array). A start whose objective is not finite raises RtdError (INVALID_ARG)."""
        r = abi.RtdOptimizerReport()
        self.eng._check(lib().rtd_optimizer_result(self.eng._h, self._h, C.byref(r), None, 0))
        n = r.history_len if capacity is None else min(int(capacity), r.history_len)
        hist = np.empty(n, dtype=np.float64)
        if n:
            self.eng._check(lib().rtd_optimizer_result(self.eng._h, self._h, C.byref(r), hist.ctypes.data_as(C.POINTER(C.c_double)), n))
        return r.as_dict(), hist

    def weights(self, field_index, dev_w_out=None, best=False):
        """Field field_index's part of the current (or best) iterate: copied to dev_w_out (device pointer, asynchronous), or, without
        one, returned as a float32 array of the field's [L][ny][nx] shape."""
        if dev_w_out is not None:
            self.eng._check(lib().rtd_optimizer_weights(self.eng._h, self._h, int(field_index), C.c_void_p(int(dev_w_out)), int(bool(best))))
            return None
        shape = np.asarray(self.fields[field_index]._beam.spotWeights).shape
        out = np.empty(shape, dtype=np.float32)
        d = self.eng.device_alloc(out.nbytes)
        try:
            self.eng._check(lib().rtd_optimizer_weights(self.eng._h, self._h, int(field_index), C.c_void_p(d), int(bool(best))))
            self.eng.to_host(out, d)
        finally:
            self.eng.device_free(d)
        return out

    def dose(self):
        """Device pointer of the optimiser's dose volume: the dose of the iterate that entered the last iteration (an L-BFGS
        optimiser: the tracked dose of the current weights)."""
        p = C.c_void_p()
        self.eng._check(lib().rtd_optimizer_dose(self.eng._h, self._h, C.byref(p)))
        return int(p.value or 0)

    def lbfgs_report(self):
        """rtd_optimizer_lbfgs_report: waits; a dict of the pairs held, the unit and backtracked steps, halvings, resets, stalls, the
        last accepted step, the last directional derivative and the trial values of the last line search. Only on an optimiser from
        Engine.create_lbfgs_optimizer (RtdError INVALID_ARG otherwise)."""
        r = abi.RtdLbfgsReport()
        self.eng._check(lib().rtd_optimizer_lbfgs_report(self.eng._h, self._h, C.byref(r)))
        return r.as_dict()

    def lbfgs_buffers(self):
        """rtd_optimizer_lbfgs_buffers: the device pointers and sizes of an L-BFGS optimiser's own arrays (abi.RtdLbfgsBuffers), for
        inspection."""
        b = abi.RtdLbfgsBuffers()
        self.eng._check(lib().rtd_optimizer_lbfgs_buffers(self.eng._h, self._h, C.byref(b)))
        return b

    def lbfgs_line_buffers(self):
        """rtd_optimizer_lbfgs_line_buffers: what the line search of an L-BFGS optimiser reads and leaves (abi.RtdLbfgsLineBuffers): the
        device pointers of d0 and d1 and, with DVH or EUD terms, of the per-trial thresholds float[n_trials][RTD_OBJ_MAX_TERMS] and
        {E, K, value} double[n_trials][RTD_OBJ_MAX_TERMS][3] (None without such terms)."""
        b = abi.RtdLbfgsLineBuffers()
        self.eng._check(lib().rtd_optimizer_lbfgs_line_buffers(self.eng._h, self._h, C.byref(b)))
        return b

    def lbfgs_constraint_line(self):
        """rtd_optimizer_lbfgs_constraint_line: the device arrays the last line search of a constrained L-BFGS optimiser left
        (abi.RtdLbfgsConstraintLineBuffers): con_trial[k] = (the terms' value, psi_c ...) and mean_trial[k][c]. No synchronisation. Only
        on an optimiser from Engine.create_constrained_lbfgs_optimizer (RtdError INVALID_ARG otherwise)."""
        b = abi.RtdLbfgsConstraintLineBuffers()
        self.eng._check(lib().rtd_optimizer_lbfgs_constraint_line(self.eng._h, self._h, C.byref(b)))
        return b

    def constraint_report(self):
        """rtd_optimizer_constraint_report: waits; (report dict, outer history as a list of (iteration, rho, max_violation)). Only on an
        optimiser from Engine.create_constrained_optimizer (RtdError INVALID_ARG otherwise)."""
        r = abi.RtdConstraintReport()
        self.eng._check(lib().rtd_optimizer_constraint_report(self.eng._h, self._h, C.byref(r), None, 0))
        n = int(r.outer_history_len)
        hist = (abi.RtdConstraintOuter * max(1, n))()
        if n:
            self.eng._check(lib().rtd_optimizer_constraint_report(self.eng._h, self._h, C.byref(r), hist, n))
        return r.as_dict(), [(int(hist[i].iteration), float(hist[i].rho), float(hist[i].max_violation)) for i in range(n)]

    def constraint_buffers(self):
        """rtd_optimizer_constraint_buffers: the device pointers and sizes of a constrained optimiser's own arrays
        (abi.RtdConstraintBuffers; the multipliers are .lambda_ and .mu), for inspection."""
        b = abi.RtdConstraintBuffers()
        self.eng._check(lib().rtd_optimizer_constraint_buffers(self.eng._h, self._h, C.byref(b)))
        return b

    def set_let_objective(self, let_objective):
        """rtd_optimizer_set_let_objective: a second Objective, evaluated on the LET-weighted dose sum_f N_f w_f (every field needs
        let_influence() first); None removes it. Everything it needs is allocated here, never in run()."""
        h = let_objective._h if let_objective is not None else None
        self.eng._check(lib().rtd_optimizer_set_let_objective(self.eng._h, self._h, h))
        self.let_objective = let_objective

    def let_dose(self):
        """Device pointer of the optimiser's LET-weighted dose volume (of the iterate that entered the last iteration)."""
        p = C.c_void_p()
        self.eng._check(lib().rtd_optimizer_let_dose(self.eng._h, self._h, C.byref(p)))
        return int(p.value or 0)

    def let_values(self):
        """Waits; float64 [f, f_dose, f_let] of the last iteration."""
        v = np.zeros(3, dtype=np.float64)
        self.eng._check(lib().rtd_optimizer_let_values(self.eng._h, self._h, v.ctypes.data_as(C.POINTER(C.c_double))))
        return v

    def set_rbe(self, rbe):
        """rtd_optimizer_set_rbe: the objective is then evaluated on the RBE-weighted dose R(dose, LET-weighted dose) of an Rbe object
        (every field needs let_influence() first; not together with a LET objective); None removes it. Everything it needs is
        allocated here, never in run(). The Rbe must outlive its use."""
        self.eng._check(lib().rtd_optimizer_set_rbe(self.eng._h, self._h, rbe._h if rbe is not None else None))
        self.rbe = rbe

    def rbe_dose(self):
        """Device pointer of the optimiser's RBE-weighted dose volume (of the iterate that entered the last iteration); dose() stays
        the physical dose."""
        p = C.c_void_p()
        self.eng._check(lib().rtd_optimizer_rbe_dose(self.eng._h, self._h, C.byref(p)))
        return int(p.value or 0)

    def scenario_values(self):
        """Waits; (values float64[S], lambdas float64[S], worst): every scenario's objective, its share of the combined gradient and
        the worst scenario, of the iterate that entered the last iteration. A plain optimiser is a set of one scenario."""
        n = len(self.scenario_fields)
        vals, lams, worst = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64), C.c_int32(0)
        dp = C.POINTER(C.c_double)
        self.eng._check(lib().rtd_optimizer_scenario_values(self.eng._h, self._h, vals.ctypes.data_as(dp), lams.ctypes.data_as(dp), C.byref(worst)))
        return vals, lams, int(worst.value)

    def scenario_dose(self, s):
        """Device pointer of scenario s's dose volume (scenario 0: dose())."""
        p = C.c_void_p()
        self.eng._check(lib().rtd_optimizer_scenario_dose(self.eng._h, self._h, int(s), C.byref(p)))
        return int(p.value or 0)

    def destroy(self):
        if self._h:
            lib().rtd_optimizer_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()


class PlanSet:
    """rtd_planset_*: P plans optimised at once over the fields' resident matrices: P weight vectors under P variants of one
    Objective, every step of the iteration one launch for all of them. Each plan has the bits of a plain Optimizer on a plain objective
    with that plan's terms. `variants`: per plan one (kind, roi, weight, level) per term of `objective`, in term order (kind and roi
    those of the objective's term; pareto.anchor_variants makes such tables). Destroy it before its fields, objective and engine."""

    def __init__(self, eng, fields, objective, variants, options=None):
        self.eng = eng
        self.objective = objective
        self.fields = list(fields)
        self.n_plans = len(variants)
        self.n_terms = int(objective.n_terms)
        if any(len(v) != self.n_terms for v in variants):
            raise ValueError("every plan needs one variant per term of the objective")
        self._h = C.c_void_p()
        flat = [t if isinstance(t, abi.RtdObjectiveTerm) else abi.RtdObjectiveTerm(int(t[0]), int(t[1]), float(t[2]), float(t[3]))
                for v in variants for t in v]
        tab = (abi.RtdObjectiveTerm * max(1, len(flat)))(*flat)
        arr = (C.c_void_p * max(1, len(self.fields)))(*[f._h for f in self.fields])
        po = C.byref(options) if options is not None else None
        eng._check(lib().rtd_planset_create(eng._h, arr, len(self.fields), objective._h, tab, self.n_plans, po, C.byref(self._h)))

    def set_weights(self, plan, field_index, dev_w):
        """Plan `plan`'s weights of field field_index from dev_w ([L][ny][nx] float32, contiguous, device pointer)."""
        self.eng._check(lib().rtd_planset_set_weights(self.eng._h, self._h, int(plan), int(field_index), C.c_void_p(int(dev_w))))

    def run(self, n_iterations):
        """Launches n_iterations iterations of every plan on the engine's stream; asynchronous, launches only."""
        self.eng._check(lib().rtd_planset_run(self.eng._h, self._h, int(n_iterations)))

    def result(self, plan, capacity=None):
        """Waits; (report dict, history float64 array) of plan `plan`, as Optimizer.result."""
        r = abi.RtdOptimizerReport()
        self.eng._check(lib().rtd_planset_result(self.eng._h, self._h, int(plan), C.byref(r), None, 0))
        n = r.history_len if capacity is None else min(int(capacity), r.history_len)
        hist = np.empty(n, dtype=np.float64)
        if n:
            self.eng._check(lib().rtd_planset_result(self.eng._h, self._h, int(plan), C.byref(r), hist.ctypes.data_as(C.POINTER(C.c_double)), n))
        return r.as_dict(), hist

    def _fetch(self, call, shape, dev_out):
        if dev_out is not None:
            self.eng._check(call(C.c_void_p(int(dev_out))))
            return None
        out = np.empty(shape, dtype=np.float32)
        d = self.eng.device_alloc(out.nbytes)
        try:
            self.eng._check(call(C.c_void_p(d)))
            self.eng.to_host(out, d)
        finally:
            self.eng.device_free(d)
        return out

    def weights(self, plan, field_index, best=False, dev_w_out=None):
        """Plan `plan`'s current (or best) weights of field field_index: de-interleaved to dev_w_out (device pointer, asynchronous),
        or, without one, returned as a float32 array of the field's [L][ny][nx] shape."""
        shape = np.asarray(self.fields[field_index]._beam.spotWeights).shape
        return self._fetch(lambda p: lib().rtd_planset_weights(self.eng._h, self._h, int(plan), int(field_index), int(bool(best)), p), shape, dev_w_out)

    def dose(self, plan, dev_out=None):
        """Plan `plan`'s dose volume (of the iterate that entered the last iteration): copied out of the interleaved volume to dev_out
        (device pointer, the whole grid), or, without one, returned as a float32 [Z][Y][X] array."""
        dims = self.objective.dims
        return self._fetch(lambda p: lib().rtd_planset_dose(self.eng._h, self._h, int(plan), p), (dims[2], dims[1], dims[0]), dev_out)

    def values(self):
        """Waits; float64 [n_plans][1 + n_terms]: per plan the objective and its terms of the iterate that entered the last iteration."""
        v = np.zeros((self.n_plans, 1 + self.n_terms), dtype=np.float64)
        self.eng._check(lib().rtd_planset_values(self.eng._h, self._h, v.ctypes.data_as(C.POINTER(C.c_double))))
        return v

    def blend(self, coeffs, field_index, best=True, dev_w_out=None):
        """The navigated plan's weights of field field_index: float32(sum_p coeffs[p] * float64(w_p)), p ascending, of the plans' best
        (or current) weights; coeffs finite and >= 0, one per plan. To dev_w_out, or returned as an array."""
        c = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1)
        if c.size != self.n_plans:
            raise ValueError("one coefficient per plan")
        shape = np.asarray(self.fields[field_index]._beam.spotWeights).shape
        cp = c.ctypes.data_as(C.POINTER(C.c_double))
        return self._fetch(lambda p: lib().rtd_planset_blend(self.eng._h, self._h, cp, int(field_index), int(bool(best)), p), shape, dev_w_out)

    def destroy(self):
        if self._h:
            lib().rtd_planset_destroy(self.eng._h, self._h)
            self._h = C.c_void_p()


class Engine:
    """One rtd_handle: one GPU, one stream, resident CT and LUTs."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        st = lib().rtd_create(int(device_id), C.byref(self._h))
        if st != 0:
            raise RtdError(st, lib().rtd_global_error().decode())
        self._keep = []

    def _check(self, st):
        if st != 0:
            raise RtdError(st, lib().rtd_last_error(self._h).decode())

    def close(self):
        if self._h:
            lib().rtd_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_options(self, opt):
        self._check(lib().rtd_set_options(self._h, C.byref(opt)))

    def set_luts(self, es):
        la = es.as_abi()
        self._check(lib().rtd_set_luts(self._h, C.byref(la)))

    def set_let_table(self, table):
        """rtd_set_let_table: the LET table [n_energies][n_energy_samples] float32 in keV/um on the rows and the depth sampling of the
        LUTs' cidd_matrix (luts.synth_let makes one); None removes it. Not an input of the dose."""
        if table is None:
            self._check(lib().rtd_set_let_table(self._h, None, 0, 0))
            return
        t = abi.f32(table)
        if t.ndim != 2:
            raise ValueError("the LET table is [n_energies][n_energy_samples]")
        self._check(lib().rtd_set_let_table(self._h, abi.fptr(t), int(t.shape[0]), int(t.shape[1])))

    def let_average(self, dev_let_dose, dev_dose, n_voxels, dev_out, dose_floor=0.0):
        """rtd_let_average: LETd = let_dose / dose where dose > dose_floor, 0 elsewhere (device pointers; in place is allowed)."""
        self._check(lib().rtd_let_average(self._h, C.c_void_p(int(dev_let_dose)), C.c_void_p(int(dev_dose)), int(n_voxels), C.c_float(dose_floor),
                                          C.c_void_p(int(dev_out))))

    def load_luts_dir(self, directory, water_cube_test=False):
        self._check(lib().rtd_load_luts_dir(self._h, directory.encode(), int(water_cube_test)))

    def set_ct(self, ct, deferred=False):
        """deferred: rtd_set_ct_deferred — ct (C-contiguous float32, kept alive here) must stay unchanged until the computes that use
        it are done; each field then uploads only the box of it that its rays cross."""
        if deferred:
            assert ct.dtype == np.float32 and ct.flags["C_CONTIGUOUS"]
            self._ct_keep = ct
            self._check(lib().rtd_set_ct_deferred(self._h, abi.fptr(ct), abi.uint3((ct.shape[2], ct.shape[1], ct.shape[0]))))
            return
        ct = abi.f32(ct)
        self._check(lib().rtd_set_ct(self._h, abi.fptr(ct), abi.uint3((ct.shape[2], ct.shape[1], ct.shape[0]))))

    def set_ct_device(self, dev_ptr, dims):
        self._check(lib().rtd_set_ct_device(self._h, C.c_void_p(int(dev_ptr)), abi.uint3(dims)))

    def compute(self, beams, dose):
        """rtd_compute: reference-shaped, accumulates into the host array dose ([Z][Y][X] float32)."""
        from .scenarios import beams_abi
        assert dose.dtype == np.float32 and dose.flags["C_CONTIGUOUS"]
        ba = beams_abi(beams)
        tm = (abi.RtdTiming * max(1, len(beams)))()
        self._check(lib().rtd_compute(self._h, ba, len(beams), abi.fptr(dose), abi.uint3((dose.shape[2], dose.shape[1], dose.shape[0])), tm))
        return [tm[i].as_dict() for i in range(len(beams))]

    def spot_gradient(self, beams, voxel_weights):
        """rtd_spot_gradient: for every beam the gradient of <its dose, voxel_weights> with respect to its spot weights, at the
        beam's own weights; voxel_weights: host array [Z][Y][X] float32. Returns one [L][ny][nx] float32 array per beam."""
        from .scenarios import beams_abi
        g = abi.f32(voxel_weights)
        ba = beams_abi(beams)
        sizes = [int(np.prod(np.asarray(b.spotWeights).shape)) for b in beams]
        out = np.zeros(max(1, sum(sizes)), dtype=np.float32)
        self._check(lib().rtd_spot_gradient(self._h, ba, len(beams), abi.fptr(g), abi.uint3((g.shape[2], g.shape[1], g.shape[0])),
                                            abi.fptr(out)))
        res, off = [], 0
        for b, n in zip(beams, sizes):
            res.append(out[off:off + n].reshape(np.asarray(b.spotWeights).shape).copy())
            off += n
        return res

    def dose_influence(self, beams, dose_dims, rel_threshold=0.0):
        """The dose-influence matrix of every beam on the dose grid dose_dims (x, y, z): one DoseInfluence per beam, as
        spot_gradient returns one array per beam. Needs ray_weight_cutoff = 0."""
        out = []
        for b in beams:
            f = self.create_field(b, dose_dims)
            try:
                out.append(f.dose_influence(rel_threshold))
            finally:
                f.release()
        return out

    def create_field(self, beam, dose_dims, remote=False):
        return Field(self, beam, dose_dims, remote=remote)

    def create_objective(self, dose_dims):
        return Objective(self, dose_dims)

    def rasterize_roi(self, dims, world_to_idx, contours, plane_thickness_mm):
        """rtd_roi_rasterize: dims (x, y, z) of the dose grid; world_to_idx an abi.RtdAffine or (m 3x3, v 3) taking mm to voxel indices;
        contours a list of (n, 3) arrays of xyz mm (closed polygons, each planar in the grid's k); plane_thickness_mm the slice spacing
        of the contoured image. Returns a Roi."""
        return Roi(self, dims, world_to_idx, contours, plane_thickness_mm)

    def roi_from_mask(self, t, dims=None):
        """rtd_roi_from_mask: the Roi of the non-zero bytes of a device mask on the grid (x fastest, as Roi.fill_mask writes it). t: a
        torch.uint8 tensor on this device ([Z][Y][X]; dims default to its shape reversed) or a device pointer (int) with dims (x, y, z).
        The mask is read on the engine's stream: whatever wrote it must have finished (or the engine be on that stream, set_stream)."""
        if hasattr(t, "data_ptr"):
            if dims is None:
                if len(t.shape) != 3:
                    raise ValueError("roi_from_mask: dims are needed for a tensor of shape %r" % (tuple(t.shape),))
                dims = (t.shape[2], t.shape[1], t.shape[0])
            if t.element_size() != 1 or not t.is_contiguous():
                raise ValueError("roi_from_mask: a contiguous one-byte tensor is needed")
            if t.numel() != int(dims[0]) * int(dims[1]) * int(dims[2]):
                raise ValueError("roi_from_mask: %d bytes do not fill dims %r" % (t.numel(), tuple(int(d) for d in dims)))
            if not t.is_cuda:
                raise ValueError("roi_from_mask: the tensor must be on the device, not on %s" % (t.device,))
            ptr = t.data_ptr()
        else:
            if dims is None:
                raise ValueError("roi_from_mask: a device pointer needs dims")
            ptr = int(t)
        out = C.c_void_p()
        self._check(lib().rtd_roi_from_mask(self._h, abi.uint3(dims), C.c_void_p(ptr), C.byref(out)))
        return Roi._adopt(self, dims, out)

    def create_rbe(self, dims, tissue):
        """rtd_rbe_create: a variable-RBE model on the dose grid dims (x, y, z) with `tissue` (an abi.RtdRbeTissue, e.g. from
        raytracedicom_amd.rbe.tissue) everywhere. Returns an Rbe."""
        return Rbe(self, dims, tissue)

    def create_optimizer(self, fields, objective, options=None):
        return Optimizer(self, fields, objective, options)

    def create_lbfgs_optimizer(self, fields, objective, options=None):
        """rtd_optimizer_create_lbfgs: an Optimizer whose iteration is L-BFGS with a backtracking line search on the device (the
        objective must not have DVH or EUD terms); options: an abi.RtdLbfgsOptions (abi.default_lbfgs_options) or None. It also has
        .lbfgs_report()."""
        return Optimizer(self, fields, objective, options, lbfgs=True)

    def create_lbfgs_optimizer_ex(self, fields, objective, options=None, compact=False):
        """rtd_optimizer_create_lbfgs_ex: the L-BFGS Optimizer on an objective of any term kind (DVH and EUD terms are evaluated per trial
        of the line search, on the float32-rounded trial volume); compact=True: its products read the fields' compact matrices
        (Field.dose_influence_compact first; works after release_plain). It also has .lbfgs_line_buffers()."""
        return Optimizer(self, fields, objective, options, lbfgs=True, lbfgs_flags=abi.RTD_LBFGS_COMPACT if compact else 0)

    def create_constrained_lbfgs_optimizer(self, fields, objective, lbfgs_options=None, constrained_options=None, compact=False):
        """rtd_optimizer_create_constrained_lbfgs: an Optimizer whose iteration is the augmented Lagrangian around L-BFGS, the outer
        update at the current iterate; the objective needs a term (any kind) and a constraint. lbfgs_options: an abi.RtdLbfgsOptions or
        None; constrained_options: an abi.RtdConstrainedOptions or None; compact=True: the products read the fields' compact matrices.
        It has .lbfgs_report(), .lbfgs_buffers(), .lbfgs_line_buffers(), .lbfgs_constraint_line(), .constraint_report() and
        .constraint_buffers()."""
        return Optimizer(self, fields, objective, lbfgs_options, lbfgs=True, lbfgs_flags=abi.RTD_LBFGS_COMPACT if compact else 0,
                         constrained=constrained_options if constrained_options is not None else True)

    def create_constrained_optimizer(self, fields, objective, options=None, constrained=None):
        """rtd_optimizer_create_constrained: an Optimizer whose iteration is the augmented Lagrangian around the spectral one, on an
        objective with at least one term and one constraint (Objective.add_constraint); constrained: an abi.RtdConstrainedOptions
        (abi.default_constrained_options) or None. It also has .constraint_report() and .constraint_buffers()."""
        return Optimizer(self, fields, objective, options, constrained=constrained if constrained is not None else True)

    def create_compact_optimizer(self, fields, objective, options=None):
        """rtd_optimizer_create_compact: the spectral optimiser of create_optimizer whose two products read the fields' compact
        matrices (every field needs dose_influence_compact() first)."""
        return Optimizer(self, fields, objective, options, compact=True)

    def create_planset(self, fields, objective, variants, options=None):
        """rtd_planset_create: len(variants) plans on `fields` under variants of `objective` (PlanSet)."""
        return PlanSet(self, fields, objective, variants, options)

    def create_robust_optimizer(self, scenario_fields, objective, mode, probabilities=None, options=None):
        """rtd_optimizer_create_robust: scenario_fields is a list of per-scenario field lists (scenario 0 the nominal one, every field
        with a dose_influence() matrix); mode abi.RTD_ROBUST_EXPECTED or abi.RTD_ROBUST_WORST_CASE. See raytracedicom_amd.robust."""
        return Optimizer(self, None, objective, options, scenario_fields=scenario_fields, mode=mode, probabilities=probabilities)

    def create_voxelwise_optimizer(self, scenario_fields, objective, options=None):
        """rtd_optimizer_create_voxelwise: the voxel-wise worst case over the scenarios (every voxel takes, per term, the scenario
        dose that is worst for it). scenario_fields as create_robust_optimizer; the objective must not have DVH or EUD terms."""
        return Optimizer(self, None, objective, options, scenario_fields=scenario_fields, voxelwise=True)

    def create_robust_compact_optimizer(self, sfields, obj, mode, probabilities=None, options=None):
        """rtd_optimizer_create_robust_compact: create_robust_optimizer on the fields' compact matrices (every field of sfields, a list
        of per-scenario field lists, needs dose_influence_compact() first; it works after release_plain). Field f of every scenario
        must have been built with the forward tree of field f of scenario 0."""
        return Optimizer(self, None, obj, options, scenario_fields=sfields, mode=mode, probabilities=probabilities, compact=True)

    def create_voxelwise_compact_optimizer(self, sfields, obj, options=None):
        """rtd_optimizer_create_voxelwise_compact: create_voxelwise_optimizer on the fields' compact matrices; sfields as
        create_robust_compact_optimizer."""
        return Optimizer(self, None, obj, options, scenario_fields=sfields, voxelwise=True, compact=True)

    def create_4d_optimizer(self, phase_fields, warps, objective, weights=None, options=None):
        """rtd_optimizer_create_4d: phase_fields is a list of per-phase field lists (the same beams computed on every phase's CT, each
        with a dose_influence() matrix, all on one dose grid); warps one abi.RtdWarp per phase, reference voxel -> that phase's dose
        grid, its field already on the device (raytracedicom_amd.fourd.phase_warps) and alive as long as the optimiser; the objective
        lives on the reference grid; weights: the time spent in each phase (None: equal)."""
        return Optimizer(self, None, objective, options, scenario_fields=phase_fields, phase_warps=list(warps), phase_weights=weights)

    def dose_extremes(self, dose_ptrs, n_voxels, d_min=None, d_max=None):
        """rtd_scenario_dose_extremes: d_min[v] / d_max[v] (device pointers of float32[n_voxels], either may be None) = the smallest /
        largest of the scenario volumes dose_ptrs at v; asynchronous. Point Objective.dvh and .dose_at_volume at them for worst-case
        DVH bands."""
        doses = [int(p) for p in dose_ptrs]
        self._check(lib().rtd_scenario_dose_extremes(self._h, (C.c_void_p * max(1, len(doses)))(*doses), len(doses), int(n_voxels),
                                                     C.c_void_p(int(d_min)) if d_min else None, C.c_void_p(int(d_max)) if d_max else None))

    def transfer_fields_init(self, fields, dev_dose, box_min=None, box_max=None):
        """rtd_fields_transfer_init: every voxel of the inclusive dose-index box is written with 0 + fields[0] + fields[1] + ...
        in one launch (bit for bit the loop of Field.transfer over the fields into a zeroed box); asynchronous."""
        arr = (C.c_void_p * len(fields))(*[f._h for f in fields])
        lo, hi = Field._clip(box_min, box_max)
        self._check(lib().rtd_fields_transfer_init(self._h, arr, len(fields), C.c_void_p(int(dev_dose)), lo, hi))

    _GAMMA_NAMES = {"dd": "dd_fraction", "dta": "dta_mm", "threshold": "threshold_fraction"}

    def gamma_device(self, ref_ptr, eval_ptr, dims, spacing, result_ptr, *, mask=None, gamma_map=None, opt=None, **options):
        """rtd_dose_gamma: the gamma index of the device volume eval_ptr against ref_ptr (float32, dims (x, y, z), spacing (x, y, z) mm)
        into the 32-byte device record result_ptr (abi.RtdGammaResult); asynchronous. mask: device bytes, non-zero = evaluate;
        gamma_map: device floats, every one written (-1 where nothing is evaluated). options: the fields of abi.RtdGammaOptions over
        their defaults (dd, dta and threshold are short for dd_fraction, dta_mm and threshold_fraction), or a whole record as opt."""
        if opt is None:
            opt = abi.RtdGammaOptions()
            lib().rtd_default_gamma_options(C.byref(opt))
        for k, val in options.items():
            name = self._GAMMA_NAMES.get(k, k)
            if name not in ("dd_fraction", "dta_mm", "threshold_fraction", "search_mult", "norm_dose", "local", "interp"):
                raise TypeError("gamma_device: unknown option %r" % k)
            setattr(opt, name, int(val) if name in ("local", "interp") else float(val))
        sp = (C.c_float * 3)(*[float(s) for s in spacing])
        self._check(lib().rtd_dose_gamma(self._h, C.c_void_p(int(ref_ptr)), C.c_void_p(int(eval_ptr)), abi.uint3(dims), sp, C.byref(opt),
                                         C.c_void_p(int(mask)) if mask else None, C.c_void_p(int(gamma_map)) if gamma_map else None,
                                         C.c_void_p(int(result_ptr))))

    def gamma(self, ref, ev, spacing, dd=0.01, dta=1.0, threshold=0.10, *, local=False, interp=1, norm_dose=0.0, search_mult=1.5, mask=None,
              want_map=False):
        """The gamma(dd, dta mm) index of the host volume ev against ref ([Z][Y][X] float32, spacing (x, y, z) mm) above
        threshold * norm, on the device -> (pass_rate, n_evaluated, max_gamma) (what the CPU checker of the tests returns), and the map
        ([Z][Y][X] float32, -1 where nothing is evaluated) as a fourth entry with want_map. mask: a [Z][Y][X] array, non-zero = evaluate.
        pass_rate is 1.0 when nothing is evaluated."""
        ref, ev = abi.f32(ref), abi.f32(ev)
        assert ref.ndim == 3 and ref.shape == ev.shape
        dims = (ref.shape[2], ref.shape[1], ref.shape[0])
        bufs = []

        def up(a):
            p = self.device_alloc(a.nbytes)
            bufs.append(p)
            self.to_device(p, a)
            return p
        try:
            d_ref, d_ev = up(ref), up(ev)
            d_mask = None
            if mask is not None:
                m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
                assert m.shape == ref.shape
                d_mask = up(m)
            d_map = None
            if want_map:
                d_map = self.device_alloc(ref.nbytes)
                bufs.append(d_map)
            d_res = self.device_alloc(C.sizeof(abi.RtdGammaResult))
            bufs.append(d_res)
            self.gamma_device(d_ref, d_ev, dims, spacing, d_res, mask=d_mask, gamma_map=d_map, dd=dd, dta=dta, threshold=threshold,
                              local=bool(local), interp=interp, norm_dose=norm_dose, search_mult=search_mult)
            res = abi.RtdGammaResult()
            self._check(lib().rtd_copy_to_host(self._h, C.byref(res), C.c_void_p(d_res), C.sizeof(res)))
            n, n_pass = int(res.n_evaluated), int(res.n_passed)
            out = (n_pass / n if n else 1.0, n, float(res.max_gamma))
            if want_map:
                gmap = np.empty(ref.shape, dtype=np.float32)
                self.to_host(gmap, d_map)
                out = out + (gmap,)
            return out
        finally:
            self.sync()
            for p in bufs:
                self.device_free(p)

    def gamma_kernel_ms(self):
        """rtd_dose_gamma_kernel_ms: the search kernel of the last gamma / gamma_device call, in ms (waits for it)."""
        ms = C.c_float(0)
        self._check(lib().rtd_dose_gamma_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    _DOSE_TYPES = {np.dtype(np.float32): abi.RTD_DOSE_F32, np.dtype(np.uint16): abi.RTD_DOSE_U16, np.dtype(np.uint32): abi.RTD_DOSE_U32}

    def resample_dose_device(self, src_ptr, src_dims, affine, dst_ptr, dst_dims, *, opt=None, **options):
        """rtd_dose_resample: the device volume src_ptr (dims (x, y, z); float32, or uint16 / uint32 with src_type and src_scale) onto
        the float32 device volume dst_ptr through affine, the map from destination voxel index to source voxel index (an
        abi.RtdAffine, or (m, v) for abi.make_affine; grids.index_map makes one from two grids); asynchronous. options: the fields of
        abi.RtdResampleOptions over their defaults, or a whole record as opt."""
        if opt is None:
            opt = abi.RtdResampleOptions()
            lib().rtd_default_resample_options(C.byref(opt))
        for k, val in options.items():
            if k not in ("src_type", "accumulate", "scale", "src_scale"):
                raise TypeError("resample_dose_device: unknown option %r" % k)
            setattr(opt, k, int(val) if k in ("src_type", "accumulate") else float(val))
        if not isinstance(affine, abi.RtdAffine):
            affine = abi.make_affine(*affine)
        self._check(lib().rtd_dose_resample(self._h, C.c_void_p(int(src_ptr)) if src_ptr else None, abi.uint3(src_dims), C.byref(affine),
                                            C.c_void_p(int(dst_ptr)) if dst_ptr else None, abi.uint3(dst_dims), C.byref(opt)))

    def resample_dose(self, src, affine, dst_dims, *, dst=None, **options):
        """The host volume src ([Z][Y][X]; float32, uint16 or uint32 — the integer ones with src_scale) resampled onto a grid of
        dst_dims (x, y, z) -> [Z][Y][X] float32. dst: the volume to accumulate into with accumulate=1 (it is not modified)."""
        src = np.ascontiguousarray(src)
        if src.dtype not in self._DOSE_TYPES:
            src = src.astype(np.float32)
        assert src.ndim == 3
        shape = (int(dst_dims[2]), int(dst_dims[1]), int(dst_dims[0]))
        out = np.zeros(shape, dtype=np.float32) if dst is None else abi.f32(dst).copy()
        assert out.shape == shape
        d_src, d_dst = self.device_alloc(src.nbytes), None
        try:
            d_dst = self.device_alloc(out.nbytes)
            self.to_device(d_src, src)
            self.to_device(d_dst, out)
            self.resample_dose_device(d_src, (src.shape[2], src.shape[1], src.shape[0]), affine, d_dst, dst_dims,
                                      src_type=self._DOSE_TYPES[src.dtype], **options)
            self.to_host(out, d_dst)
            return out
        finally:
            self.sync()
            for p in (d_src, d_dst):
                if p:
                    self.device_free(p)

    def resample_kernel_ms(self):
        """rtd_dose_resample_kernel_ms: the kernel of the last resample_dose / resample_dose_device call, in ms (waits for it)."""
        ms = C.c_float(0)
        self._check(lib().rtd_dose_resample_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # deformable dose warping (include/rtd.h "Deformable dose warping"). A host-side warp is (maps, dvf): maps the triple of
    # grids.warp_maps (dst_idx_to_src_idx, dst_idx_to_dvf_idx, k), dvf the field as a host array [3][Z][Y][X] float32.
    def warp_dose_device(self, src_ptr, src_dims, warp, dst_ptr, dst_dims, *, opt=None, **options):
        """rtd_dose_warp: the device volume src_ptr (dims (x, y, z); the types of resample_dose_device) pulled through warp (an
        abi.RtdWarp, abi.make_warp) onto the float32 device volume dst_ptr; asynchronous. options as for resample_dose_device."""
        if opt is None:
            opt = abi.RtdResampleOptions()
            lib().rtd_default_resample_options(C.byref(opt))
        for k, val in options.items():
            if k not in ("src_type", "accumulate", "scale", "src_scale"):
                raise TypeError("warp_dose_device: unknown option %r" % k)
            setattr(opt, k, int(val) if k in ("src_type", "accumulate") else float(val))
        self._check(lib().rtd_dose_warp(self._h, C.c_void_p(int(src_ptr)) if src_ptr else None, abi.uint3(src_dims), C.byref(warp) if warp is not None else None,
                                        C.c_void_p(int(dst_ptr)) if dst_ptr else None, abi.uint3(dst_dims), C.byref(opt)))

    def _upload_dvf(self, dvf):
        """The host field [3][Z][Y][X] on the device -> (pointer, dims (x, y, z))."""
        dvf = abi.f32(dvf)
        assert dvf.ndim == 4 and dvf.shape[0] == 3
        d = self.device_alloc(dvf.nbytes)
        try:
            self.to_device(d, dvf)
        except Exception:
            self.device_free(d)
            raise
        return d, (dvf.shape[3], dvf.shape[2], dvf.shape[1])

    def warp_dose(self, src, maps, dvf, dst_dims, *, dst=None, **options):
        """The host volume src ([Z][Y][X]; float32, uint16 or uint32 — the integer ones with src_scale) pulled through the field dvf
        ([3][Z][Y][X] float32) and the maps of grids.warp_maps onto a grid of dst_dims (x, y, z) -> [Z][Y][X] float32. dst: the volume
        to accumulate into with accumulate=1 (it is not modified)."""
        src = np.ascontiguousarray(src)
        if src.dtype not in self._DOSE_TYPES:
            src = src.astype(np.float32)
        assert src.ndim == 3
        shape = (int(dst_dims[2]), int(dst_dims[1]), int(dst_dims[0]))
        out = np.zeros(shape, dtype=np.float32) if dst is None else abi.f32(dst).copy()
        assert out.shape == shape
        bufs = []
        try:
            d_dvf, dvf_dims = self._upload_dvf(dvf)
            bufs.append(d_dvf)
            d_src = self.device_alloc(src.nbytes)
            bufs.append(d_src)
            d_dst = self.device_alloc(out.nbytes)
            bufs.append(d_dst)
            self.to_device(d_src, src)
            self.to_device(d_dst, out)
            self.warp_dose_device(d_src, (src.shape[2], src.shape[1], src.shape[0]), abi.make_warp(*maps, d_dvf, dvf_dims), d_dst, dst_dims,
                                  src_type=self._DOSE_TYPES[src.dtype], **options)
            self.to_host(out, d_dst)
            return out
        finally:
            self.sync()
            for p in bufs:
                self.device_free(p)

    def warp_kernel_ms(self):
        """rtd_dose_warp_kernel_ms: the kernel of the last warp_dose / warp_dose_device call, in ms (waits for it)."""
        ms = C.c_float(0)
        self._check(lib().rtd_dose_warp_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    @staticmethod
    def warp_t_workspace_bytes(src_dims):
        """rtd_dose_warp_t_workspace_bytes: the workspace of warp_dose_t_device for a source grid of src_dims (x, y, z)."""
        n = C.c_size_t(0)
        if lib().rtd_dose_warp_t_workspace_bytes(abi.uint3(src_dims), C.byref(n)) != abi.RTD_OK:
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "warp_t_workspace_bytes: a zero dimension or more than 2^31 - 1 voxels")
        return int(n.value)

    def warp_dose_t_device(self, g_dst_ptr, dst_dims, warp, g_src_ptr, src_dims, workspace_ptr, workspace_bytes, *, scale=1.0, accumulate=0):
        """rtd_dose_warp_t: the float32 device gradient g_dst_ptr on the destination grid pushed back through warp onto the float32
        device volume g_src_ptr on the source grid (written, or added to with accumulate=1); asynchronous. workspace_ptr: device
        memory of at least warp_t_workspace_bytes(src_dims) bytes, the caller's."""
        self._check(lib().rtd_dose_warp_t(self._h, C.c_void_p(int(g_dst_ptr)) if g_dst_ptr else None, abi.uint3(dst_dims),
                                          C.byref(warp) if warp is not None else None, C.c_void_p(int(g_src_ptr)) if g_src_ptr else None,
                                          abi.uint3(src_dims), float(scale), int(accumulate),
                                          C.c_void_p(int(workspace_ptr)) if workspace_ptr else None, int(workspace_bytes)))

    def warp_dose_t(self, g, maps, dvf, src_dims, *, scale=1.0, accumulate=0, base=None):
        """The host gradient g ([Z][Y][X] float32 on the destination grid) pushed back through the field and the maps of
        grids.warp_maps -> [Z][Y][X] float32 on the source grid of src_dims (x, y, z). base: the volume added to with accumulate=1 (it
        is not modified). The workspace is allocated here."""
        g = abi.f32(g)
        assert g.ndim == 3
        shape = (int(src_dims[2]), int(src_dims[1]), int(src_dims[0]))
        out = np.zeros(shape, dtype=np.float32) if base is None else abi.f32(base).copy()
        assert out.shape == shape
        bufs = []
        try:
            d_dvf, dvf_dims = self._upload_dvf(dvf)
            bufs.append(d_dvf)
            d_g = self.device_alloc(g.nbytes)
            bufs.append(d_g)
            d_out = self.device_alloc(out.nbytes)
            bufs.append(d_out)
            nws = self.warp_t_workspace_bytes(src_dims)
            d_ws = self.device_alloc(nws)
            bufs.append(d_ws)
            self.to_device(d_g, g)
            self.to_device(d_out, out)
            self.warp_dose_t_device(d_g, (g.shape[2], g.shape[1], g.shape[0]), abi.make_warp(*maps, d_dvf, dvf_dims), d_out, src_dims, d_ws, nws,
                                    scale=scale, accumulate=accumulate)
            self.to_host(out, d_out)
            return out
        finally:
            self.sync()
            for p in bufs:
                self.device_free(p)

    def warp_t_kernel_ms(self):
        """rtd_dose_warp_t_kernel_ms: the four launches of the last warp_dose_t / warp_dose_t_device call -> (memset, maximum,
        scatter, finish) in ms (waits for them)."""
        ms = (C.c_float * 4)()
        self._check(lib().rtd_dose_warp_t_kernel_ms(self._h, ms))
        return tuple(float(v) for v in ms)

    def accumulate_phases(self, doses, warps, weights, dst_dims):
        """The doses of several anatomies summed on a reference grid: sum_i weights[i] * warp_i(doses[i]) -> [Z][Y][X] float32 on
        dst_dims (x, y, z). doses: host volumes as warp_dose takes them; warps: one (maps, dvf) per dose. Phase 0 is written with
        scale weights[0], every later phase is accumulated with its weight in list order: a fixed sequence of float32 sums."""
        if not (len(doses) == len(warps) == len(weights)) or not doses:
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "accumulate_phases: as many doses as warps and weights, and at least one")
        shape = (int(dst_dims[2]), int(dst_dims[1]), int(dst_dims[0]))
        out = np.empty(shape, dtype=np.float32)
        d_dst = self.device_alloc(out.nbytes)
        try:
            for i, (dose, (maps, dvf), wgt) in enumerate(zip(doses, warps, weights)):
                src = np.ascontiguousarray(dose)
                if src.dtype not in self._DOSE_TYPES:
                    src = src.astype(np.float32)
                assert src.ndim == 3
                bufs = []
                try:
                    d_dvf, dvf_dims = self._upload_dvf(dvf)
                    bufs.append(d_dvf)
                    d_src = self.device_alloc(src.nbytes)
                    bufs.append(d_src)
                    self.to_device(d_src, src)
                    self.warp_dose_device(d_src, (src.shape[2], src.shape[1], src.shape[0]), abi.make_warp(*maps, d_dvf, dvf_dims), d_dst, dst_dims,
                                          src_type=self._DOSE_TYPES[src.dtype], scale=wgt, accumulate=1 if i else 0)
                finally:
                    self.sync()
                    for p in bufs:
                        self.device_free(p)
            self.to_host(out, d_dst)
            return out
        finally:
            self.sync()
            self.device_free(d_dst)

    # the warps over a phase axis (include/rtd.h "4D dose: phases warped and summed")
    @staticmethod
    def _phase_arrays(ptrs, warps, weights):
        n = len(warps)
        if not (len(ptrs) == len(weights) == n):
            raise ValueError("as many volumes as warps and weights")
        arr = (C.c_void_p * max(1, n))(*[int(p) if p else None for p in ptrs])
        wa = (abi.RtdWarp * max(1, n))(*warps)
        wt = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        return arr, wa, wt, n

    def warp_sum_device(self, src_ptrs, src_dims, warps, weights, dst_ptr, dst_dims):
        """rtd_dose_warp_sum: dst = sum_p weights[p] * warp_p(src_p) in one launch, bit for bit the sequence of warp_dose_device calls
        (phase 0 written, the others accumulated). src_ptrs: float32 device volumes on src_dims; warps: abi.RtdWarp records."""
        arr, wa, wt, n = self._phase_arrays(src_ptrs, warps, weights)
        self._check(lib().rtd_dose_warp_sum(self._h, arr, abi.uint3(src_dims), wa, abi.fptr(wt) if wt.size else None, n,
                                            C.c_void_p(int(dst_ptr)) if dst_ptr else None, abi.uint3(dst_dims)))

    def warp_sum(self, doses, warps, weights, dst_dims):
        """The host float32 volumes `doses` ([Z][Y][X], one grid) summed on dst_dims (x, y, z) through warps, one (maps, dvf) per dose as
        accumulate_phases takes them -> [Z][Y][X] float32: accumulate_phases's bits from one launch."""
        if not (len(doses) == len(warps) == len(weights)) or not doses:
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "warp_sum: as many doses as warps and weights, and at least one")
        srcs = [abi.f32(d) for d in doses]
        assert all(s.ndim == 3 and s.shape == srcs[0].shape for s in srcs)
        out = np.empty((int(dst_dims[2]), int(dst_dims[1]), int(dst_dims[0])), dtype=np.float32)
        bufs, recs, ptrs = [], [], []
        try:
            for src, (maps, dvf) in zip(srcs, warps):
                d_dvf, dvf_dims = self._upload_dvf(dvf)
                bufs.append(d_dvf)
                d_src = self.device_alloc(src.nbytes)
                bufs.append(d_src)
                self.to_device(d_src, src)
                recs.append(abi.make_warp(*maps, d_dvf, dvf_dims))
                ptrs.append(d_src)
            d_dst = self.device_alloc(out.nbytes)
            bufs.append(d_dst)
            self.warp_sum_device(ptrs, (srcs[0].shape[2], srcs[0].shape[1], srcs[0].shape[0]), recs, weights, d_dst, dst_dims)
            self.to_host(out, d_dst)
            return out
        finally:
            self.sync()
            for p in bufs:
                self.device_free(p)

    @staticmethod
    def warp_t_phases_workspace_bytes(src_dims, n):
        """rtd_dose_warp_t_phases_workspace_bytes: n slices of warp_t_workspace_bytes(src_dims)."""
        b = C.c_size_t(0)
        if lib().rtd_dose_warp_t_phases_workspace_bytes(abi.uint3(src_dims), int(n), C.byref(b)) != abi.RTD_OK:
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "warp_t_phases_workspace_bytes: a zero dimension, more than 2^31 - 1 voxels, or not 1 to 16 phases")
        return int(b.value)

    def warp_dose_t_phases_device(self, g_dst_ptr, dst_dims, warps, weights, g_src_ptrs, src_dims, workspace_ptr, workspace_bytes):
        """rtd_dose_warp_t_phases: g_src_ptrs[p] = weights[p] * W_p^T g, bit for bit warp_dose_t_device per phase, in four operations.
        workspace_ptr: device memory of at least warp_t_phases_workspace_bytes(src_dims, len(warps)) bytes, the caller's."""
        arr, wa, wt, n = self._phase_arrays(g_src_ptrs, warps, weights)
        self._check(lib().rtd_dose_warp_t_phases(self._h, C.c_void_p(int(g_dst_ptr)) if g_dst_ptr else None, abi.uint3(dst_dims), wa,
                                                 abi.fptr(wt) if wt.size else None, n, arr, abi.uint3(src_dims),
                                                 C.c_void_p(int(workspace_ptr)) if workspace_ptr else None, int(workspace_bytes)))

    def warp_dose_t_phases(self, g, warps, weights, src_dims):
        """The host gradient g ([Z][Y][X] float32 on the destination grid) pushed back through every (maps, dvf) of warps -> a list of
        [Z][Y][X] float32 volumes on src_dims (x, y, z), one per phase. The workspace is allocated here."""
        if len(warps) != len(weights) or not warps:
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "warp_dose_t_phases: as many warps as weights, and at least one")
        g = abi.f32(g)
        assert g.ndim == 3
        shape = (int(src_dims[2]), int(src_dims[1]), int(src_dims[0]))
        outs = [np.empty(shape, dtype=np.float32) for _ in warps]
        bufs, recs, ptrs = [], [], []
        try:
            for out, (maps, dvf) in zip(outs, warps):
                d_dvf, dvf_dims = self._upload_dvf(dvf)
                bufs.append(d_dvf)
                d_out = self.device_alloc(out.nbytes)
                bufs.append(d_out)
                recs.append(abi.make_warp(*maps, d_dvf, dvf_dims))
                ptrs.append(d_out)
            d_g = self.device_alloc(g.nbytes)
            bufs.append(d_g)
            self.to_device(d_g, g)
            nws = self.warp_t_phases_workspace_bytes(src_dims, len(warps))
            d_ws = self.device_alloc(nws)
            bufs.append(d_ws)
            self.warp_dose_t_phases_device(d_g, (g.shape[2], g.shape[1], g.shape[0]), recs, weights, ptrs, src_dims, d_ws, nws)
            for out, d_out in zip(outs, ptrs):
                self.to_host(out, d_out)
            return outs
        finally:
            self.sync()
            for p in bufs:
                self.device_free(p)

    def quantize_dose_device(self, dose_ptr, n_voxels, out_ptr, bits=16, scaling=0.0):
        """rtd_dose_quantize on device buffers -> (scaling used, n_clamped); synchronous."""
        s, n = C.c_double(float(scaling)), C.c_uint64(0)
        self._check(lib().rtd_dose_quantize(self._h, C.c_void_p(int(dose_ptr)), int(n_voxels), int(bits), C.byref(s), C.c_void_p(int(out_ptr)), C.byref(n)))
        return float(s.value), int(n.value)

    def quantize_dose(self, dose, bits=16, scaling=0.0):
        """The host dose (float32, any shape) as the unsigned integers of an RT Dose file -> (ints of the same shape, scaling,
        n_clamped): ints * scaling is the dose to within scaling / 2. scaling 0: chosen from the largest dose."""
        dose = abi.f32(dose)
        if bits not in (16, 32):
            raise RtdError(abi.RTD_ERR_INVALID_ARG, "quantize_dose: bits must be 16 or 32")
        out = np.empty(dose.shape, dtype=np.uint16 if bits == 16 else np.uint32)
        d_dose, d_out = self.device_alloc(dose.nbytes), None
        try:
            d_out = self.device_alloc(out.nbytes)
            self.to_device(d_dose, dose)
            s, n = self.quantize_dose_device(d_dose, dose.size, d_out, bits, scaling)
            self.to_host(out, d_out)
            return out, s, n
        finally:
            self.sync()
            for p in (d_dose, d_out):
                if p:
                    self.device_free(p)

    # device buffers owned by the handle
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._check(lib().rtd_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, p):
        self._check(lib().rtd_device_free(self._h, C.c_void_p(p)))

    def device_zero(self, p, nbytes):
        self._check(lib().rtd_device_zero(self._h, C.c_void_p(p), nbytes))

    def to_device(self, p, arr):
        arr = np.ascontiguousarray(arr)
        self._check(lib().rtd_copy_to_device(self._h, C.c_void_p(p), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def to_host(self, arr, p):
        assert arr.flags["C_CONTIGUOUS"]
        self._check(lib().rtd_copy_to_host(self._h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(p), arr.nbytes))

    def sync(self):
        self._check(lib().rtd_sync(self._h))

    def stream(self):
        return lib().rtd_stream(self._h)

    def set_stream(self, s):
        self._check(lib().rtd_set_stream(self._h, C.c_void_p(s) if s else None))


class Plan:
    """rtd_plan_*: the reference-shaped call on several GPUs of one process (one host thread per device)."""

    def __init__(self, device_ids):
        self._h = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        st = lib().rtd_plan_create(ids, len(device_ids), C.byref(self._h))
        if st != 0:
            raise RtdError(st, lib().rtd_global_error().decode())

    def _check(self, st):
        if st != 0:
            raise RtdError(st, lib().rtd_plan_last_error(self._h).decode())

    def close(self):
        if self._h:
            lib().rtd_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_options(self, opt):
        self._check(lib().rtd_plan_set_options(self._h, C.byref(opt)))

    def set_luts(self, es):
        la = es.as_abi()
        self._check(lib().rtd_plan_set_luts(self._h, C.byref(la)))

    def set_ct(self, ct, deferred=False):
        """deferred: rtd_plan_set_ct_deferred — ct (a C-contiguous float32 array, kept alive here) must stay unchanged until the
        computes that use it are done; each beam then uploads only the box of it that its rays cross."""
        if deferred:
            assert ct.dtype == np.float32 and ct.flags["C_CONTIGUOUS"]
            self._ct_keep = ct
            self._check(lib().rtd_plan_set_ct_deferred(self._h, abi.fptr(ct), abi.uint3((ct.shape[2], ct.shape[1], ct.shape[0]))))
            return
        ct = abi.f32(ct)
        self._check(lib().rtd_plan_set_ct(self._h, abi.fptr(ct), abi.uint3((ct.shape[2], ct.shape[1], ct.shape[0]))))

    def compute(self, beams, dose):
        """All beams accumulated into the host array dose ([Z][Y][X] float32); returns (per-beam timings, plan timing)."""
        from .scenarios import beams_abi
        assert dose.dtype == np.float32 and dose.flags["C_CONTIGUOUS"]
        ba = beams_abi(beams)
        tm = (abi.RtdTiming * max(1, len(beams)))()
        pt = abi.RtdPlanTiming()
        self._check(lib().rtd_plan_compute(self._h, ba, len(beams), abi.fptr(dose), abi.uint3((dose.shape[2], dose.shape[1], dose.shape[0])), tm,
                                           C.byref(pt)))
        return [tm[i].as_dict() for i in range(len(beams))], pt.as_dict()


def host_register(arr):
    """Page-lock a numpy array (HostPinnedImage3D's cudaHostRegister, host_image_3d.cuh:23-32)."""
    st = lib().rtd_host_register(arr.ctypes.data_as(C.c_void_p), arr.nbytes)
    if st != 0:
        raise RtdError(st, lib().rtd_global_error().decode())


def host_unregister(arr):
    lib().rtd_host_unregister(arr.ctypes.data_as(C.c_void_p))


def cudaWrapperProtons(imVol, doseVol, beams, iddData, outStream=None, device_id=0, options=None):
    """Drop-in for the reference's cudaWrapperProtons (src/kernel_wrapper.cuh:161).

    imVol   [Z][Y][X] float32 HU+1000; doseVol [Z][Y][X] float32, accumulated in place;
    beams   list of scenarios.BeamSettings; iddData luts.EnergyStruct; outStream file-like for the log text.
    """
    out = outStream if outStream is not None else sys.stdout
    opt = options or abi.default_options()
    with Engine(device_id) as eng:
        eng.set_options(opt)
        eng.set_luts(iddData)
        eng.set_ct(imVol)
        timings = eng.compute(beams, doseVol)
    total = sum(t["total_ms"] for t in timings)
    if opt.fine_grained_timing:
        for i, t in enumerate(timings):   # bucket names of kernel_wrapper.cu:1298-1307
            out.write("    Calculating field no. %d\n" % i)
            out.write("        Time to trace rays: %g ms\n" % t["raytracing_ms"])
            out.write("        Time preparing data for loop over energies: %g ms\n" % t["prepare_energy_loop_ms"])
            out.write("        Time depositing IDD and calculating sigma: %g ms\n" % t["fill_idd_sigma_ms"])
            out.write("        Time preparing for superposition: %g ms\n" % t["prepare_superp_ms"])
            out.write("        Time executing superposition: %g ms\n" % t["superp_ms"])
            out.write("        Kernel time to transform voxels: %g ms\n\n" % t["transforming_ms"])
    out.write("    Total global execution time (excluding GPU initialisation): %g ms.\n\n" % total)
    return timings
