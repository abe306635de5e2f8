"""ctypes binding of librvseg.so (include/rvseg.h).

The HIP library is the product: there is no CPU fallback.  Importing this module without a built
librvseg.so raises; creating a context without a GPU raises RvsegError(NO_DEVICE).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RVSEG_LIBRARY: another build of the library (A/B timing of kernel variants on one GPU box); the product default is the
# in-tree librvseg.so
LIB_PATH = os.environ.get("RVSEG_LIBRARY") or os.path.join(_HERE, "librvseg.so")

RVSEG_MAX_LAYERS = 8

OK, ERR_INVALID_ARG, ERR_IO, ERR_FORMAT, ERR_NO_FOREST, ERR_HIP, ERR_NO_DEVICE, ERR_CAPACITY, NOT_READY = range(9)
LABEL_EVAL, LABEL_CRF, LABEL_NOCRF, LABEL_ARGMAX = range(4)
GT_LABELS, GT_RGB = range(2)
# rvseg_norm_kind / rvseg_kernel_kind / rvseg_compat_kind (the reference's NormalizationType / KernelType order, pairwise.h:32-42)
NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = range(4)
CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = range(3)
COMPAT_POTTS, COMPAT_DIAGONAL, COMPAT_MATRIX = range(3)
OBJECTIVE_LOGLIKELIHOOD, OBJECTIVE_HAMMING, OBJECTIVE_IOU = range(3)   # rvseg_objective_kind

# every symbol include/rvseg.h declares
SYMBOLS = [
    "rvseg_params_default", "rvseg_create", "rvseg_destroy", "rvseg_last_error",
    "rvseg_status_string", "rvseg_feature_length", "rvseg_forest_load", "rvseg_forest_load_mem",
    "rvseg_forest_info", "rvseg_forest_eval", "rvseg_extract_features", "rvseg_segment_frames",
    "rvseg_segment_frames_device", "rvseg_crf_infer", "rvseg_crf_infer_multi",
    "rvseg_lattice_build", "rvseg_lattice_filter", "rvseg_lattice_neighbours", "rvseg_last_timing",
    "rvseg_fuse_posteriors", "rvseg_label_values",
    "rvseg_forest_check", "rvseg_forest_write", "rvseg_forest_write_mem", "rvseg_forest_rewrite",
    "rvseg_poll_status",
    "rvseg_fuse_posteriors_device", "rvseg_cloud_features_device", "rvseg_crf_infer_device",
    "rvseg_label_values_device", "rvseg_process_map_device",
    "rvseg_crf_features_gaussian", "rvseg_crf_features_bilateral",
    "rvseg_train_params_default", "rvseg_forest_train",
    "rvseg_comm_unique_id", "rvseg_comm_init", "rvseg_comm_destroy", "rvseg_gather_frames",
    "rvseg_schedule_default", "rvseg_set_schedule", "rvseg_last_schedule",
    "rvseg_forest_train_result", "rvseg_forest_train_frames",
    "rvseg_host_register", "rvseg_host_unregister",
    "rvseg_color_coding_set", "rvseg_labels_from_rgb_device", "rvseg_labels_to_rgb_device",
    "rvseg_labels_from_rgb", "rvseg_labels_to_rgb", "rvseg_eval_reset", "rvseg_eval_accumulate_device",
    "rvseg_eval_accumulate", "rvseg_eval_confusion", "rvseg_eval_scores_from_counts",
    "rvseg_crf_terms_check", "rvseg_crf_infer_terms", "rvseg_crf_infer_terms_device",
    "rvseg_crf_logistic_unary", "rvseg_crf_logistic_unary_device",
    "rvseg_rectify_depth", "rvseg_rectify_depth_device", "rvseg_external_layers_set",
    "rvseg_segment_external", "rvseg_segment_external_device",
    "rvseg_project_cloud", "rvseg_project_cloud_device", "rvseg_process_map_poses_device", "rvseg_projection_matrix",
    "rvseg_crf_model_set", "rvseg_crf_model_set_device", "rvseg_crf_model_start", "rvseg_crf_model_start_device",
    "rvseg_crf_model_step", "rvseg_crf_model_step_device", "rvseg_crf_model_apply", "rvseg_crf_model_apply_device",
    "rvseg_crf_model_energy", "rvseg_crf_model_energy_device", "rvseg_crf_model_kl", "rvseg_crf_model_kl_device",
    "rvseg_crf_model_trace", "rvseg_crf_model_trace_device",
    "rvseg_crf_objective_check", "rvseg_crf_model_apply_transpose", "rvseg_crf_model_apply_transpose_device",
    "rvseg_crf_model_objective", "rvseg_crf_model_objective_device", "rvseg_crf_model_backward", "rvseg_crf_model_backward_device",
    "rvseg_crf_model_gradient", "rvseg_crf_model_gradient_device", "rvseg_crf_model_set_compat", "rvseg_crf_model_set_unary",
    "rvseg_crf_model_set_unary_device", "rvseg_crf_logistic_gradient", "rvseg_crf_logistic_gradient_device",
    "rvseg_crf_model_compat_apply", "rvseg_crf_model_compat_apply_device",
    "rvseg_crf_model_lattice_gradient", "rvseg_crf_model_lattice_gradient_device", "rvseg_crf_model_kernel_gradient",
    "rvseg_crf_model_kernel_gradient_device", "rvseg_crf_model_backward_kernel", "rvseg_crf_model_backward_kernel_device",
    "rvseg_crf_model_gradient_kernel", "rvseg_crf_model_gradient_kernel_device",
    "rvseg_crf_model_set_kernel", "rvseg_crf_model_set_logistic", "rvseg_crf_model_set_logistic_device",
    "rvseg_crf_model_set_logistic_params", "rvseg_crf_model_gradient_params", "rvseg_crf_model_gradient_params_device",
    "rvseg_crf_model_energy_gradient", "rvseg_lbfgs_params_default", "rvseg_minimize_lbfgs",
    "rvseg_crf_model_info",
    "rvseg_boosted_check", "rvseg_boosted_rewrite", "rvseg_boosted_load", "rvseg_boosted_load_mem", "rvseg_boosted_write",
    "rvseg_boosted_write_mem", "rvseg_boosted_weights", "rvseg_boosted_train", "rvseg_boosted_train_result", "rvseg_boosted_resample",
    "rvseg_forest_classify", "rvseg_forest_classify_trees", "rvseg_forest_measure", "rvseg_forest_tools_scores",
    "rvseg_forest_tools_correlation", "rvseg_forest_refit",
    "rvseg_prune_params_default", "rvseg_prune_schedule", "rvseg_forest_prune", "rvseg_forest_prune_energy", "rvseg_forest_prune_apply",
    "rvseg_forest_train_prior", "rvseg_boosted_train_prior",
]
PRIOR_NONE, PRIOR_INVERSE_FREQUENCY, PRIOR_GIVEN = range(3)   # rvseg_prior_mode
PRUNE_ERROR, PRUNE_COVER = 0, 1   # rvseg_prune_energy
PRUNE_MAX_STATE = 64
BOOSTED_WEIGHT_FIRST, BOOSTED_TREE_FIRST, BOOSTED_AS_LOADED = 0, 1, -1   # rvseg_boosted_order
# rvseg_lbfgs_status
LBFGS_CONVERGED, LBFGS_MAX_ITERATIONS, LBFGS_STOPPED, LBFGS_LINESEARCH_FAILED, LBFGS_NOT_FINITE, LBFGS_BAD_ARGUMENTS = 0, 1, 2, 3, -1, -2
LEARN_UNARY, LEARN_PAIRWISE, LEARN_KERNEL = 1, 2, 4   # learn_mask of rvseg_crf_model_energy_gradient


class RvsegParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
        ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("patch_size", C.c_int32), ("patch_size_reduce", C.c_int32),
        ("feature_color_patch", C.c_int32), ("feature_depth", C.c_int32),
        ("feature_height", C.c_int32), ("feature_normal", C.c_int32),
        ("fill_value", C.c_float),
        ("use_dense_crf", C.c_int32),
        ("dcrf_xyz_kernel", C.c_float), ("dcrf_rgb_kernel", C.c_float),
        ("dcrf_kernel_weight", C.c_float), ("dcrf_iterations", C.c_int32),
        ("multi_layer", C.c_int32), ("label_mode", C.c_int32),
        ("unknown_label", C.c_int32 * RVSEG_MAX_LAYERS),
        ("max_batch", C.c_int32), ("device", C.c_int32), ("lattice_capacity_log2", C.c_int32),
    ]


class RvsegTrainParams(C.Structure):
    _fields_ = [
        ("num_trees", C.c_int32), ("max_depth", C.c_int32), ("min_split_examples", C.c_int32),
        ("min_child_split_examples", C.c_int32), ("num_features", C.c_int32), ("use_bootstrap", C.c_int32),
        ("smoothing", C.c_float), ("seed", C.c_uint64),
    ]


class RvsegClassPrior(C.Structure):
    """rvseg_class_prior: the split objective of rvseg_forest_train_prior / rvseg_boosted_train_prior."""
    _fields_ = [("mode", C.c_int32), ("weights", C.c_float * 16)]


class RvsegPruneParams(C.Structure):
    """rvseg_prune_params: the schedule, the move probabilities and the energy of rvseg_forest_prune."""
    _fields_ = [
        ("start_temperature", C.c_float), ("end_temperature", C.c_float), ("alpha", C.c_float), ("inner_loops", C.c_int32),
        ("p_exchange", C.c_float), ("p_remove", C.c_float), ("p_add", C.c_float), ("energy", C.c_int32), ("seed", C.c_uint64),
    ]


class RvsegPruneTraceRow(C.Structure):
    """rvseg_prune_trace_row: what the reference's callback sees after every temperature iteration."""
    _fields_ = [("iteration", C.c_int32), ("temperature", C.c_float), ("energy", C.c_float), ("best_energy", C.c_float),
                ("state_size", C.c_int32)]


class RvsegSchedule(C.Structure):
    _fields_ = [(k, C.c_int32) for k in (
        "splat", "resident_blocks", "resident_band", "resident_chunk", "resident_window", "resident_cap_tiles",
        "group_vertices", "overlap_build", "overlap_layers", "build_priority_high", "trace", "serial_chains", "csr_block")]


class RvsegScheduleInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in (
        "splat", "planner_fallback", "csr_path", "n_frames", "points_per_frame", "vertices", "longest_list", "resident_blocks",
        "resident_band", "resident_chunk", "capacity_log2")]


class RvsegCrfTerm(C.Structure):
    """rvseg_crf_term: one pairwise term of a learned DenseCRF."""
    _fields_ = [
        ("d", C.c_int32), ("compat", C.c_int32), ("kernel_type", C.c_int32), ("normalization", C.c_int32),
        ("features", C.c_void_p), ("compat_params", C.c_void_p), ("kernel_params", C.c_void_p),
    ]


class RvsegCrfObjective(C.Structure):
    """rvseg_crf_objective: a learning objective of a DenseCRF kept on a context."""
    _fields_ = [("kind", C.c_int32), ("gt", C.c_void_p), ("robust", C.c_float), ("class_weight", C.c_void_p)]


class RvsegCrfModelInfo(C.Structure):
    """struct rvseg_crf_model_info: which model a context keeps, and its shape."""
    _fields_ = [("serial", C.c_uint64), ("N", C.c_int32), ("C", C.c_int32), ("n_terms", C.c_int32), ("K", C.c_int32),
                ("d", C.c_int32 * 8), ("compat_params", C.c_int32 * 8), ("kernel_params", C.c_int32 * 8),
                ("n_compat_params", C.c_int32), ("n_kernel_params", C.c_int32)]


class RvsegLbfgsParams(C.Structure):
    """rvseg_lbfgs_params"""
    _fields_ = [("m", C.c_int32), ("max_iterations", C.c_int32), ("max_linesearch", C.c_int32), ("reserved", C.c_int32),
                ("epsilon", C.c_double), ("ftol", C.c_double), ("min_step", C.c_double), ("max_step", C.c_double)]


class RvsegLbfgsReport(C.Structure):
    """rvseg_lbfgs_report"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("reserved", C.c_int32),
                ("gnorm", C.c_double), ("xnorm", C.c_double)]


ENERGY_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32)
PROGRESS_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double,
                          C.c_double, C.c_int32, C.c_int32, C.c_int32)

SPLAT_NAMES = {0: "none", 1: "list-major", 2: "resident"}


class RvsegError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("rvseg status %d: %s" % (status, message))
        self.status = status


_lib = None


def lib():
    """Loads librvseg.so.  torch (if it is going to be used in this process) must be imported
    first so that both share one HIP runtime (same soname libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "librvseg.so is not built (run `python __graft_entry__.py` or "
            "`make -C rovinasemanticsegmentation_amd/csrc`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    PP = C.POINTER(RvsegParams)
    L.rvseg_params_default.argtypes = [PP]
    L.rvseg_params_default.restype = None
    L.rvseg_create.argtypes = [PP, C.POINTER(vp)]
    L.rvseg_destroy.argtypes = [vp]
    L.rvseg_destroy.restype = None
    L.rvseg_last_error.argtypes = [vp]
    L.rvseg_last_error.restype = C.c_char_p
    L.rvseg_status_string.argtypes = [C.c_int]
    L.rvseg_status_string.restype = C.c_char_p
    L.rvseg_feature_length.argtypes = [vp]
    L.rvseg_forest_load.argtypes = [vp, C.c_char_p]
    L.rvseg_forest_load_mem.argtypes = [vp, vp, C.c_size_t]
    L.rvseg_forest_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                    C.POINTER(i32 * RVSEG_MAX_LAYERS)]
    L.rvseg_forest_eval.argtypes = [vp, vp, i32, i32, vp]
    L.rvseg_extract_features.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
    L.rvseg_segment_frames.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.rvseg_segment_frames_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rvseg_crf_infer.argtypes = [vp, i32, i32, i32, vp, vp, f32, i32, vp, vp, i32, i32]
    L.rvseg_crf_infer_multi.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, i32]
    L.rvseg_fuse_posteriors.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp]
    L.rvseg_label_values.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.rvseg_lattice_build.argtypes = [vp, vp, i32, i32, vp, vp, vp, i32, C.POINTER(i32)]
    L.rvseg_lattice_filter.argtypes = [vp, vp, i32, vp]
    L.rvseg_lattice_neighbours.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rvseg_last_timing.argtypes = [vp, C.c_char_p, C.c_size_t, vp, i32]
    L.rvseg_forest_check.argtypes = [vp, C.c_size_t, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.c_char_p, C.c_size_t]
    L.rvseg_forest_write.argtypes = [vp, C.c_char_p]
    L.rvseg_forest_write_mem.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_forest_rewrite.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_poll_status.argtypes = [vp, i32]
    L.rvseg_fuse_posteriors_device.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp]
    L.rvseg_cloud_features_device.argtypes = [vp, i32, vp, vp, vp, vp]
    L.rvseg_crf_infer_device.argtypes = [vp, i32, i32, i32, vp, i32, vp, f32, i32, vp, vp, i32, i32, vp]
    L.rvseg_label_values_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    L.rvseg_process_map_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.rvseg_train_params_default.argtypes = [C.POINTER(RvsegTrainParams)]
    L.rvseg_train_params_default.restype = None
    L.rvseg_forest_train.argtypes = [vp, vp, i32, i32, vp, i32, vp, C.POINTER(RvsegTrainParams), vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_forest_train_result.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_forest_train_frames.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, i32, C.POINTER(RvsegTrainParams), vp, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.POINTER(i32)]
    L.rvseg_boosted_check.argtypes = [vp, C.c_size_t, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.c_char_p, C.c_size_t]
    L.rvseg_boosted_rewrite.argtypes = [vp, C.c_size_t, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_boosted_load.argtypes = [vp, C.c_char_p, i32]
    L.rvseg_boosted_load_mem.argtypes = [vp, vp, C.c_size_t, i32]
    L.rvseg_boosted_write.argtypes = [vp, C.c_char_p, i32]
    L.rvseg_boosted_write_mem.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_boosted_weights.argtypes = [vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rvseg_boosted_train.argtypes = [vp, vp, i32, i32, vp, i32, C.POINTER(RvsegTrainParams), vp, C.c_size_t, C.POINTER(C.c_size_t),
                                      vp, vp, C.POINTER(i32)]
    L.rvseg_forest_train_prior.argtypes = [vp, vp, i32, i32, vp, i32, C.POINTER(RvsegTrainParams), C.POINTER(RvsegClassPrior), vp, C.c_size_t,
                                           C.POINTER(C.c_size_t)]
    L.rvseg_boosted_train_prior.argtypes = [vp, vp, i32, i32, vp, i32, C.POINTER(RvsegTrainParams), C.POINTER(RvsegClassPrior), vp, C.c_size_t,
                                            C.POINTER(C.c_size_t), vp, vp, C.POINTER(i32)]
    L.rvseg_boosted_train_result.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvseg_boosted_resample.argtypes = [vp, vp, vp, i32, f32, C.c_uint64, C.POINTER(f32), vp, vp, vp]
    L.rvseg_host_register.argtypes = [vp, C.c_size_t]
    L.rvseg_host_unregister.argtypes = [vp]
    L.rvseg_comm_unique_id.argtypes = [vp]
    L.rvseg_comm_init.argtypes = [vp, i32, i32, vp]
    L.rvseg_comm_destroy.argtypes = [vp]
    L.rvseg_comm_destroy.restype = None
    L.rvseg_gather_frames.argtypes = [vp, vp, C.c_size_t, vp, i32, vp]
    L.rvseg_crf_features_gaussian.argtypes = [i32, i32, f32, f32, vp]
    L.rvseg_crf_features_bilateral.argtypes = [i32, i32, f32, f32, f32, f32, f32, vp, vp]
    L.rvseg_schedule_default.argtypes = [C.POINTER(RvsegSchedule)]
    L.rvseg_schedule_default.restype = None
    L.rvseg_set_schedule.argtypes = [vp, C.POINTER(RvsegSchedule)]
    L.rvseg_last_schedule.argtypes = [vp, C.POINTER(RvsegScheduleInfo)]
    L.rvseg_color_coding_set.argtypes = [vp, i32, i32, vp, vp, C.c_int8]
    L.rvseg_labels_from_rgb_device.argtypes = [vp, i32, i32, vp, vp, vp]
    L.rvseg_labels_to_rgb_device.argtypes = [vp, i32, i32, vp, vp, vp]
    L.rvseg_labels_from_rgb.argtypes = [vp, i32, i32, vp, vp]
    L.rvseg_labels_to_rgb.argtypes = [vp, i32, i32, vp, vp]
    L.rvseg_eval_reset.argtypes = [vp]
    L.rvseg_eval_accumulate_device.argtypes = [vp, i32, vp, vp, i32, vp]
    L.rvseg_eval_accumulate.argtypes = [vp, i32, vp, vp, i32]
    L.rvseg_eval_confusion.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64)]
    L.rvseg_eval_scores_from_counts.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(f32), C.POINTER(f32), vp]
    TP = C.POINTER(RvsegCrfTerm)
    L.rvseg_crf_terms_check.argtypes = [i32, i32, i32, TP]
    L.rvseg_crf_infer_terms.argtypes = [vp, i32, i32, i32, TP, vp, i32, vp, vp, i32, i32]
    L.rvseg_crf_infer_terms_device.argtypes = [vp, i32, i32, i32, TP, vp, i32, i32, vp, vp, i32, i32, vp]
    L.rvseg_crf_logistic_unary.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.rvseg_crf_logistic_unary_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.rvseg_crf_model_set.argtypes = [vp, i32, i32, i32, TP, vp, i32]
    L.rvseg_crf_model_set_device.argtypes = [vp, i32, i32, i32, TP, vp, i32, vp]
    L.rvseg_crf_model_info.argtypes = [vp, C.POINTER(RvsegCrfModelInfo)]
    L.rvseg_crf_model_start.argtypes = [vp, vp]
    L.rvseg_crf_model_start_device.argtypes = [vp, vp, vp]
    L.rvseg_crf_model_step.argtypes = [vp, vp, i32]
    L.rvseg_crf_model_step_device.argtypes = [vp, vp, i32, vp]
    L.rvseg_crf_model_apply.argtypes = [vp, i32, vp, vp]
    L.rvseg_crf_model_apply_device.argtypes = [vp, i32, vp, vp, vp]
    L.rvseg_crf_model_energy.argtypes = [vp, vp, i32, vp, vp]
    L.rvseg_crf_model_energy_device.argtypes = [vp, vp, i32, vp, vp, vp]
    L.rvseg_crf_model_kl.argtypes = [vp, vp, vp]
    L.rvseg_crf_model_kl_device.argtypes = [vp, vp, vp, vp]
    L.rvseg_crf_model_trace.argtypes = [vp, i32, vp, vp, i32, i32, vp]
    L.rvseg_crf_model_trace_device.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp]
    OP = C.POINTER(RvsegCrfObjective)
    L.rvseg_crf_objective_check.argtypes = [OP]
    L.rvseg_crf_model_apply_transpose.argtypes = [vp, i32, vp, vp]
    L.rvseg_crf_model_apply_transpose_device.argtypes = [vp, i32, vp, vp, vp]
    L.rvseg_crf_model_objective.argtypes = [vp, OP, vp, vp, vp]
    L.rvseg_crf_model_objective_device.argtypes = [vp, OP, vp, vp, vp, vp]
    L.rvseg_crf_model_backward.argtypes = [vp, i32, vp, vp, vp, vp]
    L.rvseg_crf_model_backward_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_gradient.argtypes = [vp, i32, OP, vp, vp, vp, vp]
    L.rvseg_crf_model_gradient_device.argtypes = [vp, i32, OP, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_set_compat.argtypes = [vp, i32, vp]
    L.rvseg_crf_model_set_unary.argtypes = [vp, vp, i32]
    L.rvseg_crf_model_set_unary_device.argtypes = [vp, vp, i32, vp]
    L.rvseg_crf_logistic_gradient.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.rvseg_crf_logistic_gradient_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.rvseg_crf_model_compat_apply.argtypes = [vp, i32, vp, vp]
    L.rvseg_crf_model_compat_apply_device.argtypes = [vp, i32, vp, vp, vp]
    L.rvseg_crf_model_lattice_gradient.argtypes = [vp, i32, vp, vp, vp]
    L.rvseg_crf_model_lattice_gradient_device.argtypes = [vp, i32, vp, vp, vp, vp]
    L.rvseg_crf_model_kernel_gradient.argtypes = [vp, i32, vp, vp, vp, vp]
    L.rvseg_crf_model_kernel_gradient_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_backward_kernel.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_backward_kernel_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_gradient_kernel.argtypes = [vp, i32, OP, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_gradient_kernel_device.argtypes = [vp, i32, OP, vp, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_set_kernel.argtypes = [vp, i32, vp]
    L.rvseg_crf_model_set_logistic.argtypes = [vp, i32, vp, vp]
    L.rvseg_crf_model_set_logistic_device.argtypes = [vp, i32, vp, vp, vp]
    L.rvseg_crf_model_set_logistic_params.argtypes = [vp, vp]
    L.rvseg_crf_model_gradient_params.argtypes = [vp, i32, OP, vp, vp, vp, vp]
    L.rvseg_crf_model_gradient_params_device.argtypes = [vp, i32, OP, vp, vp, vp, vp, vp]
    L.rvseg_crf_model_energy_gradient.argtypes = [vp, i32, OP, i32, f32, vp, i32, vp, vp]
    L.rvseg_lbfgs_params_default.argtypes = [C.POINTER(RvsegLbfgsParams)]
    L.rvseg_lbfgs_params_default.restype = None
    L.rvseg_minimize_lbfgs.argtypes = [i32, vp, C.POINTER(C.c_double), ENERGY_FN, PROGRESS_FN, vp, C.POINTER(RvsegLbfgsParams),
                                       C.POINTER(RvsegLbfgsReport)]
    L.rvseg_rectify_depth.argtypes = [vp, i32, vp, vp, f32, f32, vp]
    L.rvseg_rectify_depth_device.argtypes = [vp, i32, vp, vp, f32, f32, vp, vp]
    L.rvseg_external_layers_set.argtypes = [vp, i32, vp]
    L.rvseg_segment_external.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp]
    L.rvseg_segment_external_device.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    L.rvseg_project_cloud.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.rvseg_project_cloud_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp]
    L.rvseg_process_map_poses_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.rvseg_projection_matrix.argtypes = [vp, vp, vp, vp]
    L.rvseg_forest_classify.argtypes = [vp, vp, i32, i32, i32, vp]
    L.rvseg_forest_classify_trees.argtypes = [vp, vp, i32, i32, i32, vp]
    L.rvseg_forest_measure.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp]
    L.rvseg_forest_tools_scores.argtypes = [vp, i32, C.POINTER(f32), vp]
    L.rvseg_forest_tools_correlation.argtypes = [vp, i32, C.c_uint64, vp]
    L.rvseg_forest_refit.argtypes = [vp, vp, i32, i32, vp, i32, vp, f32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.rvseg_prune_params_default.argtypes = [C.POINTER(RvsegPruneParams)]
    L.rvseg_prune_params_default.restype = None
    L.rvseg_prune_schedule.argtypes = [C.POINTER(RvsegPruneParams), C.POINTER(i32), C.POINTER(i32)]
    L.rvseg_forest_prune.argtypes = [vp, vp, i32, i32, vp, i32, C.POINTER(RvsegPruneParams), vp, C.POINTER(i32), C.POINTER(f32), vp, i32,
                                     C.POINTER(i32), vp]
    L.rvseg_forest_prune_energy.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp, i32, C.POINTER(f32)]
    L.rvseg_forest_prune_apply.argtypes = [vp, vp, i32]
    # debug entry point (not in include/rvseg.h, not in SYMBOLS): see debug_live_resources
    L.rvseg_debug_live_resources.argtypes = [C.POINTER(C.c_longlong)]
    L.rvseg_debug_live_resources.restype = None
    L.rvseg_debug_lattice_builds.argtypes = [vp, C.POINTER(C.c_longlong)]
    for name in SYMBOLS:
        getattr(L, name)  # raises AttributeError if the library does not export it
    _lib = L
    return L


def default_params(**kw):
    p = RvsegParams()
    lib().rvseg_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "unknown_label":
            for i, u in enumerate(v):
                p.unknown_label[i] = int(u)
        else:
            setattr(p, k, v)
    return p


def prune_params(**kw):
    """rvseg_prune_params with the reference's defaults (todos.txt:313-329), fields overridden by keyword."""
    p = RvsegPruneParams()
    lib().rvseg_prune_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("rvseg_prune_params has no field %r" % k)
        setattr(p, k, v)
    return p


def prune_schedule(params):
    """Host only: (temperature iterations, proposals) of a schedule; RvsegError where rvseg_forest_prune refuses it."""
    it, steps = C.c_int32(), C.c_int32()
    st = lib().rvseg_prune_schedule(C.byref(params), C.byref(it), C.byref(steps))
    if st != OK:
        raise RvsegError(st, "refused prune schedule")
    return it.value, steps.value


def check(ctx, status):
    if status != OK:
        msg = lib().rvseg_last_error(ctx)
        raise RvsegError(status, (msg or b"").decode("utf-8", "replace") or
                         lib().rvseg_status_string(status).decode())


def forest_check(blob, feature_length=0):
    """Host-only validation (no GPU): returns (status, message, info)."""
    blob = bytes(blob)
    nt, nn, md = C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(512)
    st = lib().rvseg_forest_check(blob, len(blob), feature_length, C.byref(nt), C.byref(nn), C.byref(md), err, 512)
    return st, err.value.decode("utf-8", "replace"), {"n_trees": nt.value, "n_nodes": nn.value, "max_depth": md.value}


def forest_rewrite(blob):
    """Host-only: parse a forest.dat image and serialise it again with the library's writer."""
    blob = bytes(blob)
    size = C.c_size_t()
    st = lib().rvseg_forest_rewrite(blob, len(blob), None, 0, C.byref(size))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    out = C.create_string_buffer(size.value)
    st = lib().rvseg_forest_rewrite(blob, len(blob), out, size.value, C.byref(size))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out.raw[:size.value]


def boosted_check(blob, order=BOOSTED_WEIGHT_FIRST, feature_length=0):
    """Host-only validation of a boosted-forest stream read in `order` (no GPU): returns (status, message, info)."""
    blob = bytes(blob)
    nt, nn, md = C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(512)
    st = lib().rvseg_boosted_check(blob, len(blob), order, feature_length, C.byref(nt), C.byref(nn), C.byref(md), err, 512)
    return st, err.value.decode("utf-8", "replace"), {"n_trees": nt.value, "n_nodes": nn.value, "max_depth": md.value}


def boosted_rewrite(blob, in_order=BOOSTED_WEIGHT_FIRST, out_order=None):
    """Host-only: parse a boosted-forest stream in in_order and serialise it in out_order (default: the same)."""
    blob = bytes(blob)
    out_order = in_order if out_order is None else out_order
    size = C.c_size_t()
    st = lib().rvseg_boosted_rewrite(blob, len(blob), in_order, out_order, None, 0, C.byref(size))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    out = C.create_string_buffer(size.value)
    st = lib().rvseg_boosted_rewrite(blob, len(blob), in_order, out_order, out, size.value, C.byref(size))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out.raw[:size.value]


def crf_features_gaussian(W, H, sx, sy):
    """DenseCRF2D::addPairwiseGaussian's feature matrix (densecrf.cpp:61-69), W*H x 2, host only."""
    import numpy as np
    out = np.empty((W * H, 2), np.float32)
    st = lib().rvseg_crf_features_gaussian(W, H, sx, sy, out.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out


def crf_features_bilateral(W, H, sx, sy, sr, sg, sb, im):
    """DenseCRF2D::addPairwiseBilateral's feature matrix (densecrf.cpp:70-81), W*H x 5, host only."""
    import numpy as np
    im = np.ascontiguousarray(im, np.uint8)
    assert im.size == W * H * 3
    out = np.empty((W * H, 5), np.float32)
    st = lib().rvseg_crf_features_bilateral(W, H, sx, sy, sr, sg, sb, im.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out


def projection_matrix(K, calib, pose):
    """rvseg_projection_matrix (host only): K (3 x 3), calib (the 21 floats of a calibration, or its last 12: R row-major
    then t, camera -> base link), pose (3 x 4, base link -> map) -> P (3 x 4 float32) of rvseg_project_cloud."""
    import numpy as np
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    calib = np.ascontiguousarray(calib, np.float32).reshape(-1)
    if calib.size == 21:
        calib = np.ascontiguousarray(calib[9:])
    pose = np.ascontiguousarray(pose, np.float32).reshape(-1)
    if calib.size != 12 or pose.size != 12:
        raise ValueError("calib: 21 or 12 floats, pose: 12 floats")
    out = np.empty((3, 4), np.float32)
    st = lib().rvseg_projection_matrix(K.ctypes.data_as(C.c_void_p), calib.ctypes.data_as(C.c_void_p), pose.ctypes.data_as(C.c_void_p),
                                       out.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out


def debug_live_resources():
    """Owning handles alive in this process, over all contexts: the library's own device buffers, pinned host buffers,
    events and streams.  A context that has been closed leaves all four where they were before it was created."""
    out = (C.c_longlong * 4)()
    lib().rvseg_debug_live_resources(out)
    return dict(zip(("device_buffers", "pinned_buffers", "events", "streams"), out))


def crf_terms_check(N, Cn, terms):
    """Host-only validation of rvseg_crf_term records (no GPU): returns the status."""
    arr = (RvsegCrfTerm * max(1, len(terms)))(*terms)
    return lib().rvseg_crf_terms_check(N, Cn, len(terms), arr)


def crf_objective_check(obj):
    """Host-only validation of an rvseg_crf_objective (no GPU): returns the status.  obj: RvsegCrfObjective or None."""
    return lib().rvseg_crf_objective_check(C.byref(obj) if obj is not None else None)


def eval_scores_from_counts(counts):
    """Host-only (no GPU): the scores of src/test.cpp:203-228 from a C x C uint64 count matrix (row = ground truth).
    Returns dict(global_acc, class_avg_acc, iou, row_pct) -- global_acc is NaN when the matrix is empty."""
    import numpy as np
    counts = np.ascontiguousarray(counts, np.uint64)
    Cn = counts.shape[0]
    assert counts.shape == (Cn, Cn)
    g, a, u = C.c_double(), C.c_float(), C.c_float()
    row = np.empty((Cn, Cn), np.float64)
    st = lib().rvseg_eval_scores_from_counts(counts.ctypes.data_as(C.c_void_p), Cn, C.byref(g), C.byref(a), C.byref(u),
                                             row.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return {"global_acc": g.value, "class_avg_acc": a.value, "iou": u.value, "row_pct": row}


def forest_tools_scores(confusion):
    """Host-only (no GPU): AccuracyTool's and ConfusionMatrixTool's floats (tools.cpp:77, 126-135) from C x C uint64
    counts [true][predicted].  Returns (accuracy float32, normalised matrix float32 C x C; a class without examples is a
    NaN row, as in the reference)."""
    import numpy as np
    counts = np.ascontiguousarray(confusion, np.uint64)
    Cn = counts.shape[0]
    assert counts.shape == (Cn, Cn)
    acc = C.c_float()
    norm = np.empty((Cn, Cn), np.float32)
    st = lib().rvseg_forest_tools_scores(counts.ctypes.data_as(C.c_void_p), Cn, C.byref(acc), norm.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return np.float32(acc.value), norm


def forest_tools_correlation(agree, P):
    """Host-only (no GPU): CorrelationTool's matrix (tools.cpp:226-228) from T x T uint64 agreement counts over P points."""
    import numpy as np
    agree = np.ascontiguousarray(agree, np.uint64)
    T = agree.shape[0]
    assert agree.shape == (T, T)
    out = np.empty((T, T), np.float32)
    st = lib().rvseg_forest_tools_correlation(agree.ctypes.data_as(C.c_void_p), T, int(P), out.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise RvsegError(st, lib().rvseg_status_string(st).decode())
    return out


def minimize_lbfgs(fun, x0, progress=None, **params):
    """rvseg_minimize_lbfgs (host only, no context): fun(x float64 array) -> (value, gradient); progress(x, g, fx, xnorm,
    gnorm, step, k, ls) -> non-zero stops.  params: fields of rvseg_lbfgs_params.  Returns (x, fx, report dict with status,
    iterations, evaluations, gnorm, xnorm and the call's rvseg_status as "rvseg_status").  An exception of a callback ends
    the run (the energy's as a value that is not finite) and is raised again here."""
    import numpy as np
    L = lib()
    p = RvsegLbfgsParams()
    L.rvseg_lbfgs_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_) or k == "reserved":
            raise TypeError("no such L-BFGS parameter: %s" % k)
        setattr(p, k, v)
    x = np.array(x0, np.float64).reshape(-1)
    n = x.shape[0]
    raised = []

    def energy(user, xp, gp, nn):
        try:
            value, grad = fun(np.ctypeslib.as_array(xp, (nn,)).copy())
            np.ctypeslib.as_array(gp, (nn,))[:] = np.asarray(grad, np.float64).reshape(nn)
            return float(value)
        except BaseException as e:   # never through the C frames
            raised.append(e)
            return float("nan")

    def report(user, xp, gp, fx, xnorm, gnorm, step, nn, k, ls):
        try:
            return int(progress(np.ctypeslib.as_array(xp, (nn,)).copy(), np.ctypeslib.as_array(gp, (nn,)).copy(), fx, xnorm, gnorm, step,
                                k, ls) or 0)
        except BaseException as e:
            raised.append(e)
            return 1

    fx = C.c_double(float("nan"))
    rep = RvsegLbfgsReport()
    st = L.rvseg_minimize_lbfgs(n, x.ctypes.data_as(C.c_void_p), C.byref(fx), ENERGY_FN(energy),
                                PROGRESS_FN(report) if progress is not None else C.cast(None, PROGRESS_FN), None, C.byref(p), C.byref(rep))
    if raised:
        raise raised[0]
    return x, fx.value, {"status": rep.status, "iterations": rep.iterations, "evaluations": rep.evaluations, "gnorm": rep.gnorm,
                         "xnorm": rep.xnorm, "rvseg_status": st}
