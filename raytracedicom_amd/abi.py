"""ctypes image of include/rtd.h (the C ABI of the dose engine).

Each Structure mirrors one POD of include/rtd.h field for field; see that header for the reference
type each one replaces (BeamSettings src/beam_settings.h:101-109, EnergyStruct src/energy_struct.h:13-31,
Float3AffineTransform, Float3IdxTransform).
"""
import ctypes as C

RTD_ABI_VERSION = 3     # include/rtd.h

import numpy as np

RTD_OK = 0
RTD_ERR_INVALID_ARG = -1
RTD_ERR_HIP = -2
RTD_ERR_RADIUS_OVERFLOW = -3
RTD_ERR_NOT_READY = -4
RTD_ERR_IO = -5
RTD_ERR_NO_DEVICE = -6
RTD_ERR_OUT_OF_MEMORY = -7     # the LET block
RTD_NUC_OFF, RTD_NUC_SOUKUP, RTD_NUC_FLUKA, RTD_NUC_GAUSS_FIT = 0, 1, 2, 3
RTD_OBJ_SQ_DEVIATION, RTD_OBJ_SQ_OVERDOSE, RTD_OBJ_SQ_UNDERDOSE, RTD_OBJ_MEAN = 0, 1, 2, 3
RTD_OBJ_MAX_TERMS = 64
RTD_OPT_MAX_FIELDS = 16
RTD_OBJ_MAX_DVH, RTD_OBJ_MIN_DVH = 4, 5     # rtd_objective_add_dvh_term only
RTD_DVH_MAX_QUERIES = 64
RTD_OBJ_SQ_EUD, RTD_OBJ_SQ_MAX_EUD, RTD_OBJ_SQ_MIN_EUD = 6, 7, 8     # rtd_objective_add_eud_term only
RTD_EUD_MAX_QUERIES = 64
RTD_ROBUST_EXPECTED, RTD_ROBUST_WORST_CASE = 0, 1
RTD_ROBUST_MAX_SCENARIOS = 32
RTD_PLANSET_MAX_PLANS = 16     # plans of a plan set, and the largest plan_stride of the products with P right-hand sides

c_float_p = C.POINTER(C.c_float)


class RtdAffine(C.Structure):
    _fields_ = [("m", C.c_float * 9), ("v", C.c_float * 3)]


class RtdIdxTransform(C.Structure):
    _fields_ = [("delta", C.c_float * 3), ("offset", C.c_float * 3)]


class RtdBeam(C.Structure):
    _fields_ = [
        ("spot_weights", c_float_p),
        ("spot_nx", C.c_uint32), ("spot_ny", C.c_uint32), ("n_layers", C.c_uint32),
        ("energies", c_float_p),
        ("spot_sigmas", c_float_p),
        ("ray_spacing", C.c_float * 2),
        ("tracer_steps", C.c_uint32),
        ("source_dist", C.c_float * 2),
        ("spot_idx_to_gantry", RtdIdxTransform),
        ("gantry_to_im_idx", RtdAffine),
        ("gantry_to_dose_idx", RtdAffine),
    ]


class RtdLuts(C.Structure):
    _fields_ = [
        ("n_energy_samples", C.c_int32), ("n_energies", C.c_int32),
        ("energies_per_u", c_float_p), ("peak_depths", c_float_p), ("scale_facts", c_float_p),
        ("cidd_matrix", c_float_p),
        ("n_density_samples", C.c_int32), ("density_scale_fact", C.c_float), ("density_vector", c_float_p),
        ("n_sp_samples", C.c_int32), ("sp_scale_fact", C.c_float), ("sp_vector", c_float_p),
        ("n_rrl_samples", C.c_int32), ("rrl_scale_fact", C.c_float), ("rrl_vector", c_float_p),
        ("nuc_weight_matrix", c_float_p), ("nuc_sq_sigma_matrix", c_float_p),
    ]


class RtdOptions(C.Structure):
    _fields_ = [
        ("dose_to_water", C.c_int32), ("nozzle", C.c_int32),
        ("bp_depth_cutoff", C.c_float), ("conv_sigma_cutoff", C.c_float),
        ("ks_sigma_cutoff", C.c_float), ("ray_weight_cutoff", C.c_float),
        ("fine_grained_timing", C.c_int32), ("nuclear_corr", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


class RtdTiming(C.Structure):
    _fields_ = [
        ("raytracing_ms", C.c_float), ("prepare_energy_loop_ms", C.c_float), ("fill_idd_sigma_ms", C.c_float),
        ("prepare_superp_ms", C.c_float), ("superp_ms", C.c_float), ("transforming_ms", C.c_float),
        ("total_ms", C.c_float), ("superp_launches", C.c_int32), ("superp_kernel_ms", C.c_float),
        ("ray_dims", C.c_uint32 * 2), ("steps", C.c_uint32), ("n_layers", C.c_uint32), ("transfer_voxels", C.c_int64),
        ("reserved", C.c_int32 * 2),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["ray_dims"] = list(d["ray_dims"])
        return d


class RtdFieldInfo(C.Structure):
    _fields_ = [
        ("ray_dims", C.c_uint32 * 3), ("ray_offset", C.c_float * 3), ("ray_res", C.c_float * 3),
        ("beam_first_inside", C.c_int32), ("beam_first_outside", C.c_int32),
        ("beam_first_guaranteed_passive", C.c_int32), ("beam_first_calculated_passive", C.c_int32),
        ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3),
        ("live_steps", C.c_int64), ("max_radius", C.c_int32),
        ("dose_box_min", C.c_int32 * 3), ("dose_box_max", C.c_int32 * 3), ("uniform_sigma", C.c_int32),
    ]

    def as_dict(self):
        out = {}
        for k, _ in self._fields_:
            if k == "reserved":
                continue
            v = getattr(self, k)
            out[k] = list(v) if hasattr(v, "__len__") else v
        return out


class RtdPlanTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("upload_ms", C.c_float), ("bev_ms", C.c_float), ("exchange_ms", C.c_float),
                ("transfer_ms", C.c_float), ("download_ms", C.c_float), ("n_devices", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class RtdObjectiveTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("roi", C.c_int32), ("weight", C.c_double), ("dose_level", C.c_double)]


class RtdObjectiveDvhTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("roi", C.c_int32), ("weight", C.c_double), ("dose_level", C.c_double), ("volume_fraction", C.c_double)]


class RtdDvhQuery(C.Structure):
    _fields_ = [("roi", C.c_int32), ("reserved", C.c_int32), ("volume_fraction", C.c_double)]


class RtdObjectiveEudTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("roi", C.c_int32), ("weight", C.c_double), ("dose_level", C.c_double), ("exponent", C.c_double),
                ("reserved", C.c_double)]


class RtdEudQuery(C.Structure):
    _fields_ = [("roi", C.c_int32), ("reserved", C.c_int32), ("dose_level", C.c_double), ("exponent", C.c_double)]


class RtdOptimizerOptions(C.Structure):
    _fields_ = [("step_min", C.c_double), ("step_max", C.c_double), ("history_capacity", C.c_uint32), ("reserved", C.c_int32 * 3)]


class RtdOptimizerReport(C.Structure):
    _fields_ = [("f_last", C.c_double), ("f_best", C.c_double), ("step", C.c_double), ("best_iteration", C.c_int64),
                ("iterations", C.c_uint32), ("history_len", C.c_uint32), ("guarded", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class RtdRobustOptions(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_scenarios", C.c_uint32), ("probabilities", C.POINTER(C.c_double)), ("reserved", C.c_int32 * 4)]


class RtdRoiGrid(C.Structure):
    _fields_ = [("dims", C.c_uint32 * 3), ("world_to_idx", RtdAffine), ("plane_thickness_mm", C.c_float), ("reserved", C.c_int32 * 3)]


class RtdContourSet(C.Structure):
    _fields_ = [("points", c_float_p), ("offsets", C.POINTER(C.c_uint32)), ("n_contours", C.c_uint32), ("reserved", C.c_int32 * 3)]


class RtdRoiInfo(C.Structure):
    _fields_ = [("n_voxels", C.c_uint64), ("box_lo", C.c_uint32 * 3), ("box_hi", C.c_uint32 * 3), ("n_planes", C.c_uint32),
                ("n_slices_covered", C.c_uint32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {"n_voxels": int(self.n_voxels), "box_lo": list(self.box_lo), "box_hi": list(self.box_hi), "n_planes": int(self.n_planes),
                "n_slices_covered": int(self.n_slices_covered)}


class RtdTargetInfo(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("wepl_min", C.c_float), ("wepl_max", C.c_float), ("ray_lo", C.c_int32 * 2),
                ("ray_hi", C.c_int32 * 2), ("step_lo", C.c_int32), ("step_hi", C.c_int32), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {"n_samples": int(self.n_samples), "wepl_min": float(self.wepl_min), "wepl_max": float(self.wepl_max),
                "ray_lo": list(self.ray_lo), "ray_hi": list(self.ray_hi), "step_lo": int(self.step_lo), "step_hi": int(self.step_hi)}


class RtdTargetOptions(C.Structure):
    _fields_ = [("lateral_margin_mm", C.c_float), ("proximal_margin_mm", C.c_float), ("distal_margin_mm", C.c_float),
                ("reserved", C.c_int32 * 5)]


class RtdGammaOptions(C.Structure):
    _fields_ = [("dd_fraction", C.c_float), ("dta_mm", C.c_float), ("threshold_fraction", C.c_float), ("search_mult", C.c_float),
                ("norm_dose", C.c_float), ("local", C.c_uint32), ("interp", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class RtdGammaResult(C.Structure):
    _fields_ = [("n_evaluated", C.c_uint64), ("n_passed", C.c_uint64), ("max_gamma", C.c_float), ("norm_dose", C.c_float),
                ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return {"n_evaluated": int(self.n_evaluated), "n_passed": int(self.n_passed), "max_gamma": float(self.max_gamma),
                "norm_dose": float(self.norm_dose)}


RTD_GAMMA_MAX_RADIUS = 10

# rtd_roi_combine
RTD_ROI_OR, RTD_ROI_AND, RTD_ROI_ANDNOT, RTD_ROI_XOR = 0, 1, 2, 3


def default_gamma_options():
    """rtd_default_gamma_options: 1 % / 1 mm above 10 % of max(ref), global, node samples only."""
    o = RtdGammaOptions()
    o.dd_fraction = 0.01
    o.dta_mm = 1.0
    o.threshold_fraction = 0.10
    o.search_mult = 1.5
    o.interp = 1
    return o


class RtdResampleOptions(C.Structure):
    _fields_ = [("src_type", C.c_uint32), ("accumulate", C.c_uint32), ("scale", C.c_float), ("reserved0", C.c_uint32),
                ("src_scale", C.c_double), ("reserved", C.c_uint32 * 2)]


# rtd_resample_options.src_type
RTD_DOSE_F32, RTD_DOSE_U16, RTD_DOSE_U32 = 0, 1, 2


def default_resample_options():
    """rtd_default_resample_options: a float32 source, written (not accumulated), unscaled."""
    o = RtdResampleOptions()
    o.scale = 1.0
    o.src_scale = 1.0
    return o


class RtdWarp(C.Structure):
    """rtd_warp: the two index maps, k (displacement -> source-index units) and the field on the device (176 bytes)."""
    _fields_ = [("dst_idx_to_src_idx", RtdAffine), ("dst_idx_to_dvf_idx", RtdAffine), ("disp_to_src_idx", C.c_float * 9),
                ("reserved0", C.c_uint32), ("dev_dvf", C.c_void_p), ("dvf_dims", C.c_uint32 * 3), ("reserved", C.c_uint32 * 5)]


def make_warp(dst_idx_to_src_idx, dst_idx_to_dvf_idx, disp_to_src_idx, dev_dvf, dvf_dims):
    """rtd_warp from the pieces grids.warp_maps returns (each affine an RtdAffine or an (m, v) pair, k 3x3), the device pointer of
    the field [3][Z][Y][X] and its dims (x, y, z)."""
    w = RtdWarp()
    for name, a in (("dst_idx_to_src_idx", dst_idx_to_src_idx), ("dst_idx_to_dvf_idx", dst_idx_to_dvf_idx)):
        a = a if isinstance(a, RtdAffine) else make_affine(*a)
        C.memmove(C.byref(w, getattr(RtdWarp, name).offset), C.byref(a), C.sizeof(RtdAffine))
    k = np.asarray(disp_to_src_idx, dtype=np.float32).reshape(9)
    for i in range(9):
        w.disp_to_src_idx[i] = float(k[i])
    w.dev_dvf = int(dev_dvf) if dev_dvf else None
    for i in range(3):
        w.dvf_dims[i] = int(dvf_dims[i])
    return w


RTD_4D_MAX_PHASES = 16


class Rtd4dOptions(C.Structure):
    """rtd_4d_options: the phases of rtd_optimizer_create_4d — their warps (host rtd_warp[n_phases]) and weights (host float[n_phases]
    or NULL) (40 bytes)."""
    _fields_ = [("n_phases", C.c_uint32), ("reserved0", C.c_uint32), ("warps", C.POINTER(RtdWarp)), ("weights", c_float_p),
                ("reserved", C.c_int32 * 4)]


RTD_LBFGS_MAX_MEMORY, RTD_LBFGS_MAX_HALVINGS = 16, 7


class RtdLbfgsOptions(C.Structure):
    """rtd_lbfgs_options: memory m, max_halvings (K = 1 + max_halvings trial steps 2^-k), armijo_c1, initial_step (0: the spectral
    iteration's first rule), history_capacity (48 bytes)."""
    _fields_ = [("memory", C.c_uint32), ("max_halvings", C.c_uint32), ("armijo_c1", C.c_double), ("initial_step", C.c_double),
                ("history_capacity", C.c_uint32), ("reserved", C.c_int32 * 5)]


class RtdLbfgsReport(C.Structure):
    """rtd_lbfgs_report: what the line search and the memory of an L-BFGS optimiser did so far (144 bytes)."""
    _fields_ = [("pairs", C.c_uint32), ("unit_steps", C.c_uint32), ("backtracked_steps", C.c_uint32), ("halvings", C.c_uint32),
                ("resets", C.c_uint32), ("stalls", C.c_uint32), ("last_trial", C.c_int32), ("pair_admitted", C.c_int32),
                ("pair_slot", C.c_int32), ("ring_head", C.c_int32), ("last_step", C.c_double), ("last_gp", C.c_double),
                ("stall_factor", C.c_double), ("trial_values", C.c_double * 8), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["trial_values"] = list(d["trial_values"])
        return d


class RtdLbfgsBuffers(C.Structure):
    """rtd_lbfgs_buffers: the device arrays of an L-BFGS optimiser, for inspection (88 bytes)."""
    _fields_ = [("w", C.c_void_p), ("w_prev", C.c_void_p), ("grad", C.c_void_p), ("grad_prev", C.c_void_p), ("w_full", C.c_void_p),
                ("ring", C.c_void_p), ("trial_dose", C.c_void_p), ("gram", C.c_void_p), ("delta", C.c_void_p),
                ("n", C.c_uint32), ("memory", C.c_uint32), ("n_chunks", C.c_uint32), ("n_trials", C.c_uint32)]


RTD_LBFGS_COMPACT = 1


class RtdLbfgsLineBuffers(C.Structure):
    """rtd_lbfgs_line_buffers: what the line search of an L-BFGS optimiser reads and leaves, for inspection: d0, d1, the per-trial DVH
    thresholds float[n_trials][RTD_OBJ_MAX_TERMS] and EUD triples double[n_trials][RTD_OBJ_MAX_TERMS][3] (64 bytes)."""
    _fields_ = [("d0", C.c_void_p), ("d1", C.c_void_p), ("thresholds", C.c_void_p), ("eud", C.c_void_p),
                ("n_trials", C.c_uint32), ("n_terms", C.c_uint32), ("reserved", C.c_uint32 * 6)]


def default_lbfgs_options():
    """rtd_default_lbfgs_options: 8 pairs, 5 halvings (K = 6), c1 = 1e-4, the spectral iteration's first step rule."""
    o = RtdLbfgsOptions()
    o.memory = 8
    o.max_halvings = 5
    o.armijo_c1 = 1e-4
    o.initial_step = 0.0
    o.history_capacity = 4096
    return o


RTD_CON_MAX_DOSE, RTD_CON_MIN_DOSE, RTD_CON_MAX_MEAN, RTD_CON_MIN_MEAN = 0, 1, 2, 3
RTD_CON_MAX_CONSTRAINTS = 16


class RtdDoseConstraint(C.Structure):
    """rtd_dose_constraint: a hard bound on every voxel of a ROI (RTD_CON_MAX_DOSE / _MIN_DOSE) or on its mean dose (RTD_CON_MAX_MEAN /
    _MIN_MEAN) (32 bytes)."""
    _fields_ = [("kind", C.c_int32), ("roi", C.c_int32), ("dose_level", C.c_double), ("reserved", C.c_int32 * 4)]


class RtdConstraintLayout(C.Structure):
    """rtd_constraint_layout: the device tables of an objective's constraints: the union of the constrained ROIs and the CSR of the
    per-voxel constraints, one float multiplier per entry (56 bytes)."""
    _fields_ = [("union_voxels", C.c_void_p), ("entry_ptr", C.c_void_p), ("entry_constraint", C.c_void_p),
                ("n_union", C.c_uint32), ("n_entries", C.c_uint32), ("n_constraints", C.c_uint32), ("n_mean", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class RtdConstraintViolation(C.Structure):
    """rtd_constraint_violation: max(0, h) over a constraint's entries and the number of entries with h > tol (16 bytes)."""
    _fields_ = [("max_violation", C.c_double), ("n_violating", C.c_uint32), ("reserved", C.c_uint32)]


class RtdConstrainedOptions(C.Structure):
    """rtd_constrained_options: the penalty's start, growth and cap, the shrink the violation must show to keep the penalty, the
    feasibility tolerance, the multiplier cap, the inner block length and the outer history's capacity (72 bytes)."""
    _fields_ = [("rho0", C.c_double), ("rho_growth", C.c_double), ("rho_max", C.c_double), ("violation_shrink", C.c_double),
                ("feasibility_tol", C.c_double), ("lambda_max", C.c_double), ("inner_iterations", C.c_uint32),
                ("outer_capacity", C.c_uint32), ("reserved", C.c_int32 * 4)]


class RtdConstraintOuter(C.Structure):
    """rtd_constraint_outer: one outer update: its iteration, the penalty after its decision, the largest violation (24 bytes)."""
    _fields_ = [("iteration", C.c_uint64), ("rho", C.c_double), ("max_violation", C.c_double)]


class RtdConstraintReport(C.Structure):
    """rtd_constraint_report: what the outer updates of a constrained optimiser did so far (368 bytes)."""
    _fields_ = [("rho", C.c_double), ("f_objective", C.c_double), ("outer_updates", C.c_uint32), ("rho_increases", C.c_uint32),
                ("iterations_since_update", C.c_uint32), ("n_constraints", C.c_uint32), ("outer_history_len", C.c_uint32),
                ("reserved", C.c_uint32 * 3), ("psi", C.c_double * 16), ("max_violation", C.c_double * 16),
                ("n_violating", C.c_uint32 * 16)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        for k in ("psi", "max_violation", "n_violating"):
            d[k] = list(d[k])[:self.n_constraints]
        return d


class RtdConstraintBuffers(C.Structure):
    """rtd_constraint_buffers: the device arrays of a constrained optimiser, for inspection (64 bytes)."""
    _fields_ = [("lambda_", C.c_void_p), ("mu", C.c_void_p), ("rho", C.c_void_p), ("con_values", C.c_void_p), ("violations", C.c_void_p),
                ("outer_history", C.c_void_p), ("n_entries", C.c_uint32), ("n_constraints", C.c_uint32), ("n_mean", C.c_uint32),
                ("outer_capacity", C.c_uint32)]


def default_constrained_options():
    """rtd_default_constrained_options: rho0 1, growth 4, rho_max 1e8, shrink 0.5, tolerance 0, lambda_max 1e20, 20 inner iterations,
    256 outer history entries."""
    o = RtdConstrainedOptions()
    o.rho0, o.rho_growth, o.rho_max, o.violation_shrink, o.feasibility_tol, o.lambda_max = 1.0, 4.0, 1e8, 0.5, 0.0, 1e20
    o.inner_iterations, o.outer_capacity = 20, 256
    return o


class RtdLbfgsConstraintLineBuffers(C.Structure):
    """rtd_lbfgs_constraint_line_buffers: what the last line search of a constrained L-BFGS optimiser left about the constraints:
    con_trial double[n_trials][1 + RTD_CON_MAX_CONSTRAINTS] (the terms' value, then psi_c) and mean_trial
    double[n_trials][RTD_CON_MAX_CONSTRAINTS] (40 bytes)."""
    _fields_ = [("con_trial", C.c_void_p), ("mean_trial", C.c_void_p), ("n_trials", C.c_uint32), ("n_constraints", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class RtdDijCompactOptions(C.Structure):
    """rtd_dij_compact_options: release_plain (1: free the plain form's bulk once the compact form stands) (32 bytes)."""
    _fields_ = [("release_plain", C.c_uint32), ("reserved", C.c_int32 * 7)]


class RtdDijCompactInfo(C.Structure):
    """rtd_dij_compact_info: what rtd_field_dose_influence_compact built and the bytes the two forms keep (80 bytes)."""
    _fields_ = [("value_bits", C.c_uint32), ("col_bits", C.c_uint32), ("row_bits", C.c_uint32), ("lanes_per_row", C.c_uint32),
                ("entries_per_lane", C.c_uint32), ("plain_released", C.c_uint32), ("nnz", C.c_uint64), ("row_entries", C.c_uint64),
                ("compact_bytes", C.c_uint64), ("plain_bytes", C.c_uint64), ("released_bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class RtdDijCompactDevice(C.Structure):
    """rtd_dij_compact_device: the device arrays of a field's compact matrix, for inspection (128 bytes)."""
    _fields_ = [("scale", C.c_void_p), ("col_ptr", C.c_void_p), ("csc_code", C.c_void_p), ("csc_offset", C.c_void_p), ("csc_base", C.c_void_p),
                ("csc_rows", C.c_void_p), ("row_ptr", C.c_void_p), ("row_code", C.c_void_p), ("row_col", C.c_void_p),
                ("nnz", C.c_uint64), ("n_groups", C.c_uint64), ("n_rows", C.c_uint64), ("row_entries", C.c_uint64), ("box", C.c_int32 * 6)]


def default_dij_compact_options():
    """rtd_default_dij_compact_options: the plain form is kept."""
    return RtdDijCompactOptions()


class RtdRbeTissue(C.Structure):
    """rtd_rbe_tissue: photon alpha_x (1/Gy), beta_x (1/Gy^2) and the lines RBEmax / RBEmin = c[0] + c[1] * LETd (32 bytes)."""
    _fields_ = [("alpha_x", C.c_float), ("beta_x", C.c_float), ("rbe_max", C.c_float * 2), ("rbe_min", C.c_float * 2),
                ("reserved", C.c_uint32 * 2)]


# rtd_rbe_add_tissue: classes 0 (the default tissue) .. 255
RTD_RBE_MAX_CLASSES = 256


def default_optimizer_options():
    """rtd_default_optimizer_options: the step bounds only keep the Barzilai-Borwein step finite."""
    o = RtdOptimizerOptions()
    o.step_min = 1e-30
    o.step_max = 1e30
    o.history_capacity = 4096
    return o


def default_options():
    """Reference defaults of the compile-time switches (CMakeLists.txt:36-79)."""
    o = RtdOptions()
    o.dose_to_water = 1
    o.nozzle = 1
    o.bp_depth_cutoff = 1.05
    o.conv_sigma_cutoff = 3.0
    o.ks_sigma_cutoff = 3.0
    o.ray_weight_cutoff = 1.0
    o.fine_grained_timing = 0
    o.nuclear_corr = 0
    return o


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_float_p)


def make_affine(m, v):
    """Float3AffineTransform: m 3x3 row-major, v offset."""
    a = RtdAffine()
    mm = np.asarray(m, dtype=np.float32).reshape(9)
    vv = np.asarray(v, dtype=np.float32).reshape(3)
    for i in range(9):
        a.m[i] = float(mm[i])
    for i in range(3):
        a.v[i] = float(vv[i])
    return a


def make_idx_transform(delta, offset):
    t = RtdIdxTransform()
    for i in range(3):
        t.delta[i] = float(np.float32(delta[i]))
        t.offset[i] = float(np.float32(offset[i]))
    return t


def uint3(dims):
    return (C.c_uint32 * 3)(int(dims[0]), int(dims[1]), int(dims[2]))
