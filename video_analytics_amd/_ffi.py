"""ctypes binding of include/va.h (libva_hip.so).

PyTorch-ROCm tensors are only containers here: raw device pointers (``tensor.data_ptr()``) and
the current HIP stream cross the C ABI, nothing else.  There is no CPU fallback: if the HIP
library is missing or cannot be loaded, every entry point fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libva_hip.so")

VA_OK, VA_ERR_INVALID, VA_ERR_HIP, VA_ERR_WORKSPACE, VA_ERR_STOPPED = 0, 1, 2, 3, 4
VA_COLOR_JITTER_PARTIALS = 256  # include/va.h: uint32 partial sums per image in va_color_jitter_u8's workspace
VA_OPT_BF16_VARIANT, VA_OPT_F32_CONV_KERNEL, VA_OPT_TRAIN_STOP_AT, VA_OPT_BF16_FIRST_LAYER = 1, 2, 3, 4

# every symbol include/va.h declares (tests check that the library exports exactly these)
EXPORTS = [
    "va_version", "va_last_error", "va_ctx_create", "va_ctx_destroy",
    "va_vgg16_create", "va_vgg16_destroy", "va_vgg16_workspace_bytes", "va_vgg16_set_option", "va_vgg16_forward", "va_vgg16_classify",
    "va_copy_first_layer", "va_validate_batch",
    "va_tvl1_default_params", "va_tvl1_pyramid_sizes", "va_tvl1_tile_plan", "va_tvl1_workspace_bytes", "va_tvl1_flow",
    "va_flow_to_stack", "va_flow_to_stack_crop", "va_crop_images_u8",
    "va_flow_to_stack_views", "va_crop_images_u8_views", "va_view_mean", "va_flow_field_means", "va_flow_motion",
    "va_selftest_exact_math", "va_tvl1_profile_enable", "va_tvl1_profile_read", "va_tvl1_profile_levels",
    "va_flow_to_stack_snippets", "va_score_consensus", "va_fuse_scores",
    "va_meter_update", "va_meter_average", "va_linear_svm_predict",
    "va_vgg16_train_init", "va_vgg16_train_workspace_bytes", "va_vgg16_train_step",
    "va_vgg16_export_state", "va_vgg16_import_state", "va_vgg16_train_plan",
    "va_conv3x3_layer", "va_vgg16_first_layer",
    "va_flow_to_stack_resize", "va_resize_images_u8", "va_vgg16_train_step_consensus",
    "va_flow_homography", "va_flow_compensate", "va_frames_warp_pairs",
    "va_rgbdiff_to_stack", "va_fuse_scores_n",
    "va_train_conv_backward_layer", "va_train_fc_backward_layer", "va_train_pool_layer", "va_train_loss", "va_train_dropout",
    "va_vgg16_train_step_multitask", "va_train_loss_multitask",
    "va_linear_svm_fit_workspace_bytes", "va_linear_svm_fit", "va_linear_svm_fit_cg_steps",
    "va_linear_svm_fit_layout", "va_linear_svm_fit_phase",
    "va_vgg16_train_grad_floats", "va_vgg16_train_grad_layout", "va_vgg16_train_accumulate", "va_vgg16_train_apply_workspace_bytes",
    "va_vgg16_train_apply", "va_vgg16_unpack_grad", "va_train_conv_backward_layer_grad", "va_train_fc_backward_layer_grad",
    "va_color_jitter_u8",
    "va_frames_prepare_workspace_bytes", "va_frames_prepare",
    "va_flow_quantize_u8", "va_flowq_to_stack_snippets", "va_flowq_to_stack_resize",
    "va_solver_default", "va_vgg16_set_solver", "va_vgg16_get_solver", "va_train_dropout_p",
    "va_jpeg_decode_workspace_bytes", "va_jpeg_decode", "va_jpeg_idct", "va_jpeg_upsample",
    "va_jpeg_encode_workspace_bytes", "va_jpeg_encode", "va_jpeg_fdct", "va_jpeg_entropy_encode",
    "va_tvl1_workspace_bytes_opt", "va_tvl1_flow_opt", "va_flow_median", "va_tvl1_launch_plan",
    "va_brox_default_params", "va_brox_workspace_bytes", "va_brox_flow", "va_brox_inner_step",
    "va_farneback_default_params", "va_farneback_workspace_bytes", "va_farneback_flow", "va_farneback_polyexp", "va_farneback_pass",
    "va_dtraj_default_params", "va_dtraj_workspace_bytes", "va_dtraj_extract", "va_dtraj_state_layout",
    "va_dtraj_votes", "va_dtraj_integral", "va_dtraj_corner", "va_dtraj_sample", "va_dtraj_step", "va_dtraj_finish",
    "va_pca_workspace_bytes", "va_pca_chunk_rows", "va_pca_moments", "va_pca_transform",
    "va_gmm_default_params", "va_gmm_workspace_bytes", "va_gmm_stats", "va_gmm_posteriors", "va_gmm_mstep", "va_fisher_encode",
    "va_stip_default_params", "va_stip_workspace_bytes", "va_stip_extract", "va_stip_taps", "va_stip_smooth",
    "va_stip_gradient_products", "va_stip_response", "va_stip_maxima", "va_stip_votes", "va_stip_describe",
    "va_kmeans_default_params", "va_kmeans_workspace_bytes", "va_kmeans_tile_centres", "va_kmeans_assign", "va_kmeans_update",
    "va_kmeans_seed", "va_bow_histograms", "va_bow_encode",
]


# names of the slots of va_tvl1_params.tuning (csrc/va_internal.h, VA_TUNE_*): the library's own tuning
# switches, addressed by name from tests and tools (``default_tvl1_params(stream_levels=1)``)
TUNING_SLOTS = ("stream_levels", "stream_waves", "stream_chunks", "stream_slots", "rows_levels", "stream_ppl",
                "stream_queue", "rows_cfg")


class Tvl1Params(ctypes.Structure):
    """Mirror of ``va_tvl1_params`` (include/va.h).  ``median`` and ``median_every`` are plain Python attributes, not C
    fields: the options of ``va_tvl1_options``, which travel beside the structure (``tvl1_options``)."""
    median = 0
    median_every = 0
    _fields_ = [
        ("tau", ctypes.c_float),
        ("lambda_", ctypes.c_float),
        ("theta", ctypes.c_float),
        ("nscales", ctypes.c_int),
        ("warps", ctypes.c_int),
        ("epsilon", ctypes.c_float),
        ("iters", ctypes.c_int),
        ("scale_step", ctypes.c_float),
        ("block_iters", ctypes.c_int),
        ("fast_math", ctypes.c_int),
        ("tile_mask", ctypes.c_int),
        ("tuning", ctypes.c_int * 8),
    ]


def _tuning_property(i):
    return property(lambda self: self.tuning[i], lambda self, v: self.tuning.__setitem__(i, int(v)))


for _i, _name in enumerate(TUNING_SLOTS):
    setattr(Tvl1Params, _name, _tuning_property(_i))


class Tvl1Options(ctypes.Structure):
    """Mirror of ``va_tvl1_options`` (include/va.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("median", ctypes.c_int), ("median_every", ctypes.c_int)]


# va_tvl1_launch.family (include/va.h)
TVL1_LAUNCH_FAMILIES = ("tile", "stream", "median")


class Tvl1Launch(ctypes.Structure):
    """Mirror of ``va_tvl1_launch`` (include/va.h): one launch of ``va_tvl1_launch_plan``'s report."""
    _fields_ = [(name, ctypes.c_int) for name in (
        "level", "warp", "pair0", "npairs", "w", "h", "pitch", "family", "cfg", "waves", "levels", "eps", "fast", "median",
        "K", "it0", "grid_x", "grid_y", "strips", "row_chunks", "rows_per_chunk", "halo_x", "narrow", "rev")]


def tvl1_options(params):
    """The ``va_tvl1_options`` that the Python attributes of ``params`` ask for, or None when they ask for nothing."""
    median, every = int(getattr(params, "median", 0)), int(getattr(params, "median_every", 0))
    if median == 0 and every == 0:
        return None
    return Tvl1Options(ctypes.sizeof(Tvl1Options), median, every)


# names of the slots of va_brox_params.tuning (csrc/va_internal.h, VA_BROX_TUNE_*)
BROX_TUNING_SLOTS = ("whole_field", "tile_w", "tile_h", "sweeps_per_launch")


class BroxParams(ctypes.Structure):
    """Mirror of ``va_brox_params`` (include/va.h)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("alpha", ctypes.c_float),
        ("gamma", ctypes.c_float),
        ("scale_step", ctypes.c_float),
        ("omega", ctypes.c_float),
        ("epsilon", ctypes.c_float),
        ("nscales", ctypes.c_int),
        ("warps", ctypes.c_int),
        ("inner_iters", ctypes.c_int),
        ("solver_iters", ctypes.c_int),
        ("tuning", ctypes.c_int * 8),
    ]


for _i, _name in enumerate(BROX_TUNING_SLOTS):
    setattr(BroxParams, _name, _tuning_property(_i))


# names of the slots of va_farneback_params.tuning (csrc/va_internal.h, VA_FARNEBACK_TUNE_*)
FARNEBACK_TUNING_SLOTS = ("poly_tile_w", "poly_tile_h", "pass_tile_w", "pass_tile_h")


class FarnebackParams(ctypes.Structure):
    """Mirror of ``va_farneback_params`` (include/va.h)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("pyr_scale", ctypes.c_float),
        ("poly_sigma", ctypes.c_float),
        ("levels", ctypes.c_int),
        ("winsize", ctypes.c_int),
        ("iterations", ctypes.c_int),
        ("poly_n", ctypes.c_int),
        ("gaussian", ctypes.c_int),
        ("tuning", ctypes.c_int * 8),
    ]


for _i, _name in enumerate(FARNEBACK_TUNING_SLOTS):
    setattr(FarnebackParams, _name, _tuning_property(_i))


# names of the slots of va_dtraj_params.tuning (csrc/va_internal.h, VA_DTRAJ_TUNE_*)
DTRAJ_TUNING_SLOTS = ("chunk_frames", "votes_tile_w", "votes_tile_h")
# the regions of the track table, in the order of va_dtraj_state_layout's offsets (include/va.h)
DTRAJ_STATE_REGIONS = ("counts", "lists", "status", "start", "points", "sums", "occupancy", "pending")


class DenseTrajParams(ctypes.Structure):
    """Mirror of ``va_dtraj_params`` (include/va.h)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("step", ctypes.c_int),
        ("length", ctypes.c_int),
        ("patch", ctypes.c_int),
        ("nxy", ctypes.c_int),
        ("nt", ctypes.c_int),
        ("quality", ctypes.c_float),
        ("min_flow", ctypes.c_float),
        ("min_std", ctypes.c_float),
        ("max_std", ctypes.c_float),
        ("max_dis", ctypes.c_float),
        ("max_dis_share", ctypes.c_float),
        ("tuning", ctypes.c_int * 8),
    ]


for _i, _name in enumerate(DTRAJ_TUNING_SLOTS):
    setattr(DenseTrajParams, _name, _tuning_property(_i))


# names of the slots of va_stip_params.tuning (csrc/va_internal.h, VA_STIP_TUNE_*)
STIP_TUNING_SLOTS = ("row_tile_w", "col_tile_w", "col_tile_n")
STIP_MAX_SIGMAS, STIP_MAX_TAUS, STIP_MAX_RADIUS = 8, 4, 512


class StipParams(ctypes.Structure):
    """Mirror of ``va_stip_params`` (include/va.h).  ``sigma_list`` and ``tau_list`` read and write the
    scales in use together with their counts."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("n_sigmas", ctypes.c_int),
        ("n_taus", ctypes.c_int),
        ("sigmas", ctypes.c_float * STIP_MAX_SIGMAS),
        ("taus", ctypes.c_float * STIP_MAX_TAUS),
        ("integration", ctypes.c_float),
        ("k", ctypes.c_float),
        ("min_response", ctypes.c_float),
        ("cuboid", ctypes.c_float),
        ("neighbours", ctypes.c_int),
        ("nx", ctypes.c_int),
        ("ny", ctypes.c_int),
        ("nt", ctypes.c_int),
        ("bins", ctypes.c_int),
        ("tuning", ctypes.c_int * 8),
    ]


def _scale_list(field, count, limit):
    def get(self):
        return [float(v) for v in getattr(self, field)[:getattr(self, count)]]

    def put(self, values):
        values = [float(v) for v in values]
        if not 1 <= len(values) <= limit:
            raise ValueError("%s must hold 1 to %d scales, got %d" % (field, limit, len(values)))
        for i in range(limit):
            getattr(self, field)[i] = values[i] if i < len(values) else 0.0
        setattr(self, count, len(values))
    return property(get, put)


StipParams.sigma_list = _scale_list("sigmas", "n_sigmas", STIP_MAX_SIGMAS)
StipParams.tau_list = _scale_list("taus", "n_taus", STIP_MAX_TAUS)
for _i, _name in enumerate(STIP_TUNING_SLOTS):
    setattr(StipParams, _name, _tuning_property(_i))


VA_GMM_SOFT, VA_GMM_HARD = 0, 1  # include/va.h: va_gmm_stats' mode


class GmmParams(ctypes.Structure):
    """Mirror of ``va_gmm_params`` (include/va.h)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("chunk_rows", ctypes.c_int),
        ("batch_rows", ctypes.c_int),
        ("reserved", ctypes.c_int * 5),
    ]


VA_BOW_NONE, VA_BOW_L1, VA_BOW_L2 = 0, 1, 2  # include/va.h: va_bow_histograms' norm


class KmeansParams(ctypes.Structure):
    """Mirror of ``va_kmeans_params`` (include/va.h)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_int),
        ("chunk_rows", ctypes.c_int),
        ("reserved", ctypes.c_int * 6),
    ]


class SolverParams(ctypes.Structure):
    """Mirror of ``va_solver`` (include/va.h)."""
    _fields_ = [
        ("weight_decay", ctypes.c_float),
        ("bias_lr_mult", ctypes.c_float),
        ("bias_decay_mult", ctypes.c_float),
        ("dropout", ctypes.c_float * 3),
        ("frozen_layers", ctypes.c_int),
    ]


_lib = None


def lib():
    """Load libva_hip.so (built by ``__graft_entry__.build()`` / ``make -C video_analytics_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libva_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the hot path)" % LIB_PATH)
    # The library shares ONE HIP runtime with torch (streams and device pointers cross the ABI):
    # torch's bundled libamdhip64.so (SONAME libamdhip64.so.7) must be in the process before ours
    # is resolved, or the system copy under /opt/rocm would be loaded as a second runtime.
    import torch
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    pp = ctypes.POINTER(ctypes.c_void_p)
    fpp = ctypes.POINTER(ctypes.c_float)
    L.va_version.restype = ci
    L.va_last_error.restype = ctypes.c_char_p
    L.va_ctx_create.argtypes = [ci, pp]
    L.va_ctx_create.restype = ci
    L.va_ctx_destroy.argtypes = [vp]
    L.va_ctx_destroy.restype = None
    L.va_vgg16_create.argtypes = [vp, ci, ci, ci, ci, pp, pp, pp, pp, fpp, fpp, vp, pp]
    L.va_vgg16_create.restype = ci
    L.va_vgg16_destroy.argtypes = [vp]
    L.va_vgg16_destroy.restype = None
    L.va_vgg16_workspace_bytes.argtypes = [vp, ci]
    L.va_vgg16_workspace_bytes.restype = sz
    L.va_vgg16_set_option.argtypes = [vp, ci, ci]
    L.va_vgg16_set_option.restype = ci
    L.va_vgg16_forward.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, sz, vp]
    L.va_vgg16_forward.restype = ci
    L.va_vgg16_classify.argtypes = [vp, vp, ci, vp, vp, vp, sz, vp]
    L.va_vgg16_classify.restype = ci
    L.va_copy_first_layer.argtypes = [vp, vp, ci, ci, vp, vp]
    L.va_copy_first_layer.restype = ci
    L.va_validate_batch.argtypes = [vp, vp, vp, ci, ci, vp, vp]
    L.va_validate_batch.restype = ci
    L.va_tvl1_default_params.argtypes = [ctypes.POINTER(Tvl1Params)]
    L.va_tvl1_default_params.restype = None
    L.va_tvl1_pyramid_sizes.argtypes = [ci, ci, ctypes.POINTER(Tvl1Params), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.va_tvl1_pyramid_sizes.restype = ci
    L.va_tvl1_tile_plan.argtypes = [ci, ci, ctypes.POINTER(Tvl1Params), ctypes.POINTER(ci)]
    L.va_tvl1_tile_plan.restype = ci
    L.va_tvl1_workspace_bytes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(Tvl1Params)]
    L.va_tvl1_workspace_bytes.restype = sz
    L.va_tvl1_flow.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Tvl1Params), vp, vp, sz, vp]
    L.va_tvl1_flow.restype = ci
    L.va_tvl1_workspace_bytes_opt.argtypes = [ci, ci, ci, ci, ctypes.POINTER(Tvl1Params), ctypes.POINTER(Tvl1Options)]
    L.va_tvl1_workspace_bytes_opt.restype = sz
    L.va_tvl1_flow_opt.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Tvl1Params), ctypes.POINTER(Tvl1Options), vp, vp, sz, vp]
    L.va_tvl1_flow_opt.restype = ci
    L.va_tvl1_launch_plan.argtypes = [ci, ci, ci, ci, ctypes.POINTER(Tvl1Params), ctypes.POINTER(Tvl1Options),
                                      ctypes.POINTER(Tvl1Launch), ci]
    L.va_tvl1_launch_plan.restype = ci
    L.va_flow_median.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    L.va_flow_median.restype = ci
    L.va_brox_default_params.argtypes = [ctypes.POINTER(BroxParams)]
    L.va_brox_default_params.restype = None
    L.va_brox_workspace_bytes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(BroxParams)]
    L.va_brox_workspace_bytes.restype = sz
    L.va_brox_flow.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(BroxParams), vp, vp, sz, vp]
    L.va_brox_flow.restype = ci
    L.va_brox_inner_step.argtypes = [vp] + [vp] * 15 + [ci, ci, ci, ctypes.POINTER(BroxParams), vp, sz, vp]
    L.va_brox_inner_step.restype = ci
    L.va_farneback_default_params.argtypes = [ctypes.POINTER(FarnebackParams)]
    L.va_farneback_default_params.restype = None
    L.va_farneback_workspace_bytes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(FarnebackParams)]
    L.va_farneback_workspace_bytes.restype = sz
    L.va_farneback_flow.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(FarnebackParams), vp, vp, sz, vp]
    L.va_farneback_flow.restype = ci
    L.va_farneback_polyexp.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(FarnebackParams), vp, vp]
    L.va_farneback_polyexp.restype = ci
    L.va_farneback_pass.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(FarnebackParams), vp]
    L.va_farneback_pass.restype = ci
    pdt = ctypes.POINTER(DenseTrajParams)
    L.va_dtraj_default_params.argtypes = [pdt]
    L.va_dtraj_default_params.restype = None
    L.va_dtraj_workspace_bytes.argtypes = [ci, ci, ci, ci, pdt]
    L.va_dtraj_workspace_bytes.restype = sz
    L.va_dtraj_state_layout.argtypes = [ci, ci, pdt, ctypes.POINTER(sz), ci]
    L.va_dtraj_state_layout.restype = sz
    L.va_dtraj_extract.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, pdt, vp, vp, vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), vp, sz, vp]
    L.va_dtraj_extract.restype = ci
    L.va_dtraj_votes.argtypes = [vp, vp, ci, vp, ci, ci, ci, pdt, vp, vp]
    L.va_dtraj_votes.restype = ci
    L.va_dtraj_integral.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.va_dtraj_integral.restype = ci
    L.va_dtraj_corner.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.va_dtraj_corner.restype = ci
    L.va_dtraj_sample.argtypes = [vp, vp, vp, ci, ci, ci, pdt, vp, vp]
    L.va_dtraj_sample.restype = ci
    L.va_dtraj_step.argtypes = [vp, vp, vp, ci, ci, ci, pdt, vp, vp]
    L.va_dtraj_step.restype = ci
    L.va_dtraj_finish.argtypes = [vp, ci, ci, pdt, vp, vp, vp, vp, ci, vp]
    L.va_dtraj_finish.restype = ci
    pgp, cdb = ctypes.POINTER(GmmParams), ctypes.c_double
    psp = ctypes.POINTER(StipParams)
    L.va_stip_default_params.argtypes = [psp]
    L.va_stip_default_params.restype = None
    L.va_stip_workspace_bytes.argtypes = [ci, ci, ci, ci, psp]
    L.va_stip_workspace_bytes.restype = sz
    L.va_stip_extract.argtypes = [vp, vp, ci, vp, ci, ci, ci, psp, vp, vp, vp, ci, ctypes.POINTER(ci), vp, sz, vp]
    L.va_stip_extract.restype = ci
    L.va_stip_taps.argtypes = [cdb, ctypes.POINTER(cf), ci]
    L.va_stip_taps.restype = ci
    L.va_stip_smooth.argtypes = [vp, vp, ci, ci, ci, ci, cdb, cdb, psp, vp, vp, sz, vp]
    L.va_stip_smooth.restype = ci
    L.va_stip_gradient_products.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.va_stip_gradient_products.restype = ci
    L.va_stip_response.argtypes = [vp, vp, ci, ci, ci, cf, vp, vp]
    L.va_stip_response.restype = ci
    L.va_stip_maxima.argtypes = [vp, vp, ci, ci, ci, cf, ci, ci, ci, vp, vp, ci, vp, vp, vp]
    L.va_stip_maxima.restype = ci
    L.va_stip_votes.argtypes = [vp, vp, vp, ci, ci, ci, psp, vp, vp, vp]
    L.va_stip_votes.restype = ci
    L.va_stip_describe.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, psp, vp, vp]
    L.va_stip_describe.restype = ci
    L.va_pca_workspace_bytes.argtypes = [ci, ci]
    L.va_pca_workspace_bytes.restype = sz
    L.va_pca_chunk_rows.argtypes = [ci, ci]
    L.va_pca_chunk_rows.restype = ci
    L.va_pca_moments.argtypes = [vp, vp, ci, ci, ci, vp, vp, sz, vp]
    L.va_pca_moments.restype = ci
    L.va_pca_transform.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, vp]
    L.va_pca_transform.restype = ci
    L.va_gmm_default_params.argtypes = [pgp]
    L.va_gmm_default_params.restype = None
    L.va_gmm_workspace_bytes.argtypes = [ci, ci, ci, ci, pgp]
    L.va_gmm_workspace_bytes.restype = sz
    L.va_gmm_stats.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, pgp, vp, vp, vp, sz, vp]
    L.va_gmm_stats.restype = ci
    L.va_gmm_posteriors.argtypes = [vp, vp, ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, sz, vp]
    L.va_gmm_posteriors.restype = ci
    L.va_gmm_mstep.argtypes = [vp, vp, ci, ci, ci, cdb, vp, vp, vp, vp]
    L.va_gmm_mstep.restype = ci
    L.va_fisher_encode.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, cdb, vp, vp]
    L.va_fisher_encode.restype = ci
    pkp = ctypes.POINTER(KmeansParams)
    L.va_kmeans_default_params.argtypes = [pkp]
    L.va_kmeans_default_params.restype = None
    L.va_kmeans_workspace_bytes.argtypes = [ci, ci, ci, ci, pkp]
    L.va_kmeans_workspace_bytes.restype = sz
    L.va_kmeans_tile_centres.argtypes = []
    L.va_kmeans_tile_centres.restype = ci
    L.va_kmeans_assign.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]
    L.va_kmeans_assign.restype = ci
    L.va_kmeans_update.argtypes = [vp, vp, ci, ci, vp, vp, ci, pkp, vp, vp, vp, vp, sz, vp]
    L.va_kmeans_update.restype = ci
    L.va_kmeans_seed.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, sz, vp]
    L.va_kmeans_seed.restype = ci
    L.va_bow_histograms.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp]
    L.va_bow_histograms.restype = ci
    L.va_bow_encode.argtypes = [vp, vp, ci, ci, vp, ci, vp, ci, ci, vp, vp, sz, vp]
    L.va_bow_encode.restype = ci
    L.va_flow_to_stack.argtypes = [vp, vp, ci, ci, ci, cf, cf, cf, vp, vp]
    L.va_flow_to_stack.restype = ci
    L.va_flow_to_stack_crop.argtypes = [vp, vp, ci, ci, ci, cf, cf, cf, vp, ci, ci, vp, vp]
    L.va_flow_to_stack_crop.restype = ci
    L.va_crop_images_u8.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp]
    L.va_crop_images_u8.restype = ci
    L.va_flow_to_stack_views.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, ci, ci, ci, vp, vp]
    L.va_flow_to_stack_views.restype = ci
    L.va_crop_images_u8_views.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp]
    L.va_crop_images_u8_views.restype = ci
    L.va_flow_to_stack_snippets.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, ci, ci, ci, vp, vp]
    L.va_flow_to_stack_snippets.restype = ci
    L.va_flow_to_stack_resize.argtypes = [vp, vp, ci, ci, ci, cf, cf, cf, vp, ci, ci, vp, vp]
    L.va_flow_to_stack_resize.restype = ci
    L.va_flow_quantize_u8.argtypes = [vp, vp, ci, ci, ci, cf, vp, vp]
    L.va_flow_quantize_u8.restype = ci
    L.va_flowq_to_stack_snippets.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, cf, cf, vp, ci, ci, ci, vp, vp]
    L.va_flowq_to_stack_snippets.restype = ci
    L.va_flowq_to_stack_resize.argtypes = [vp, vp, ci, ci, ci, cf, cf, vp, ci, ci, vp, vp]
    L.va_flowq_to_stack_resize.restype = ci
    L.va_resize_images_u8.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp]
    L.va_resize_images_u8.restype = ci
    L.va_rgbdiff_to_stack.argtypes = [vp, vp, ci, ci, ci, ci, ci, fpp, vp, ci, vp, vp]
    L.va_rgbdiff_to_stack.restype = ci
    L.va_color_jitter_u8.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.va_color_jitter_u8.restype = ci
    L.va_frames_prepare_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
    L.va_frames_prepare_workspace_bytes.restype = sz
    L.va_frames_prepare.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.va_frames_prepare.restype = ci
    L.va_score_consensus.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    L.va_score_consensus.restype = ci
    L.va_fuse_scores.argtypes = [vp, vp, vp, ci, ci, cf, cf, vp, vp, vp]
    L.va_fuse_scores.restype = ci
    L.va_fuse_scores_n.argtypes = [vp, pp, fpp, ci, ci, ci, vp, vp, vp]
    L.va_fuse_scores_n.restype = ci
    L.va_view_mean.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.va_view_mean.restype = ci
    L.va_flow_field_means.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.va_flow_field_means.restype = ci
    L.va_flow_motion.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
    L.va_flow_motion.restype = ci
    L.va_flow_homography.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp]
    L.va_flow_homography.restype = ci
    L.va_flow_compensate.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp]
    L.va_flow_compensate.restype = ci
    L.va_frames_warp_pairs.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
    L.va_frames_warp_pairs.restype = ci
    L.va_selftest_exact_math.argtypes = [vp, cf, cf, vp, vp]
    L.va_selftest_exact_math.restype = ci
    L.va_tvl1_profile_enable.argtypes = [vp, ci]
    L.va_tvl1_profile_enable.restype = ci
    L.va_tvl1_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ci]
    L.va_tvl1_profile_read.restype = ci
    L.va_tvl1_profile_levels.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ci, ci]
    L.va_tvl1_profile_levels.restype = ci
    L.va_meter_update.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, vp]
    L.va_meter_update.restype = ci
    L.va_meter_average.argtypes = [vp, vp, vp, ci, ci, vp, vp]
    L.va_meter_average.restype = ci
    L.va_linear_svm_predict.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, vp, vp]
    L.va_linear_svm_predict.restype = ci
    L.va_vgg16_train_init.argtypes = [vp, vp]
    L.va_vgg16_train_init.restype = ci
    L.va_vgg16_train_workspace_bytes.argtypes = [vp, ci]
    L.va_vgg16_train_workspace_bytes.restype = sz
    L.va_vgg16_train_step.argtypes = [vp, vp, ci, vp, ci, cf, cf, ctypes.c_ulonglong, vp, vp, vp, sz, vp]
    L.va_vgg16_train_step.restype = ci
    L.va_vgg16_train_step_consensus.argtypes = [vp, vp, ci, vp, ci, ci, cf, cf, ctypes.c_ulonglong, vp, vp, vp, sz, vp]
    L.va_vgg16_train_step_consensus.restype = ci
    L.va_vgg16_train_plan.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_ulonglong)]
    L.va_vgg16_train_plan.restype = ci
    L.va_vgg16_export_state.argtypes = [vp, ci, pp, pp, pp, pp, vp]
    L.va_vgg16_export_state.restype = ci
    L.va_vgg16_import_state.argtypes = [vp, ci, pp, pp, pp, pp, vp]
    L.va_vgg16_import_state.restype = ci
    L.va_conv3x3_layer.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ctypes.c_char_p, ci, vp]
    L.va_conv3x3_layer.restype = ci
    L.va_vgg16_first_layer.argtypes = [vp, vp, ci, ci, vp, vp, ctypes.c_char_p, ci, vp]
    L.va_vgg16_first_layer.restype = ci
    L.va_train_conv_backward_layer.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, vp,
                                               ctypes.POINTER(sz), ctypes.c_char_p, ci, vp]
    L.va_train_conv_backward_layer.restype = ci
    L.va_train_fc_backward_layer.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, cf, ctypes.c_char_p, ci, vp]
    L.va_train_fc_backward_layer.restype = ci
    L.va_train_pool_layer.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.va_train_pool_layer.restype = ci
    L.va_train_loss.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
    L.va_train_loss.restype = ci
    L.va_train_dropout.argtypes = [vp, vp, sz, ctypes.c_ulonglong, ci, vp]
    L.va_train_dropout.restype = ci
    pi = ctypes.POINTER(ci)
    L.va_vgg16_train_step_multitask.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, pi, cf, cf, ctypes.c_ulonglong, vp, vp, vp, sz, vp]
    L.va_vgg16_train_step_multitask.restype = ci
    L.va_train_loss_multitask.argtypes = [vp, vp, vp, vp, ci, ci, ci, pi, vp, vp, vp]
    L.va_train_loss_multitask.restype = ci
    cd = ctypes.c_double
    L.va_linear_svm_fit_workspace_bytes.argtypes = [ci, ci, ci]
    L.va_linear_svm_fit_workspace_bytes.restype = sz
    L.va_linear_svm_fit.argtypes = [vp, vp, vp, ci, ci, ci, cd, cd, cd, ci, ci, vp, vp, vp, vp, sz, vp]
    L.va_linear_svm_fit.restype = ci
    L.va_linear_svm_fit_cg_steps.argtypes = [vp, ci, ci, ci, vp, sz, vp, vp]
    L.va_linear_svm_fit_cg_steps.restype = ci
    psz = ctypes.POINTER(sz)
    L.va_linear_svm_fit_layout.argtypes = [ci, ci, ci, psz, ci]
    L.va_linear_svm_fit_layout.restype = sz
    L.va_linear_svm_fit_phase.argtypes = [vp, vp, vp, ci, ci, ci, cd, cd, cd, ci, ci, vp, sz, vp]
    L.va_linear_svm_fit_phase.restype = ci
    L.va_vgg16_train_grad_floats.argtypes = [vp]
    L.va_vgg16_train_grad_floats.restype = sz
    L.va_vgg16_train_grad_layout.argtypes = [vp, psz, psz]
    L.va_vgg16_train_grad_layout.restype = ci
    L.va_vgg16_train_accumulate.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, pi, fpp, ci, ctypes.c_ulonglong, vp, vp, vp, sz, vp, sz, vp]
    L.va_vgg16_train_accumulate.restype = ci
    L.va_vgg16_train_apply_workspace_bytes.argtypes = []
    L.va_vgg16_train_apply_workspace_bytes.restype = sz
    L.va_vgg16_train_apply.argtypes = [vp, vp, sz, cf, cf, cf, vp, vp, sz, vp]
    L.va_vgg16_train_apply.restype = ci
    L.va_vgg16_unpack_grad.argtypes = [vp, vp, pp, pp, pp, pp, vp]
    L.va_vgg16_unpack_grad.restype = ci
    L.va_train_conv_backward_layer_grad.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                                    psz, ctypes.c_char_p, ci, vp]
    L.va_train_conv_backward_layer_grad.restype = ci
    L.va_train_fc_backward_layer_grad.argtypes = [vp, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, cf, ctypes.c_char_p, ci, vp]
    L.va_train_fc_backward_layer_grad.restype = ci
    L.va_solver_default.argtypes = [ctypes.POINTER(SolverParams)]
    L.va_solver_default.restype = None
    L.va_vgg16_set_solver.argtypes = [vp, ctypes.POINTER(SolverParams)]
    L.va_vgg16_set_solver.restype = ci
    L.va_vgg16_get_solver.argtypes = [vp, ctypes.POINTER(SolverParams)]
    L.va_vgg16_get_solver.restype = ci
    L.va_train_dropout_p.argtypes = [vp, vp, sz, ctypes.c_ulonglong, ci, cf, vp]
    L.va_train_dropout_p.restype = ci
    L.va_jpeg_decode_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
    L.va_jpeg_decode_workspace_bytes.restype = sz
    L.va_jpeg_decode.argtypes = [vp, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]
    L.va_jpeg_decode.restype = ci
    L.va_jpeg_idct.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.va_jpeg_idct.restype = ci
    L.va_jpeg_upsample.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp]
    L.va_jpeg_upsample.restype = ci
    L.va_jpeg_encode_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci, ci]
    L.va_jpeg_encode_workspace_bytes.restype = sz
    L.va_jpeg_encode.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, sz, vp, vp, vp, sz, vp]
    L.va_jpeg_encode.restype = ci
    L.va_jpeg_fdct.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.va_jpeg_fdct.restype = ci
    L.va_jpeg_entropy_encode.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, sz, vp, vp, vp, sz, vp]
    L.va_jpeg_entropy_encode.restype = ci
    _lib = L
    return L


def check(rc):
    """Map a C return code to the exception the reference's Python surface would raise
    (ValueError for bad arguments -- Sheet03/spatialModel.py:46, Sheet03/utils.py:56)."""
    if rc == VA_OK:
        return
    msg = lib().va_last_error().decode("utf-8", "replace")
    if rc in (VA_ERR_INVALID, VA_ERR_WORKSPACE):
        raise ValueError(msg)
    raise RuntimeError(msg)


def _default_params(cls, fill, label, over, alias=None):
    """``cls()`` filled by the library's ``fill``, then the keyword overrides; an unknown name raises ValueError."""
    p = cls()
    getattr(lib(), fill)(ctypes.byref(p))
    for k, v in over.items():
        if k == alias:
            k += "_"
        if k == "struct_bytes" or not hasattr(p, k):
            raise ValueError("unknown %s parameter %r" % (label, k))
        setattr(p, k, v)
    return p


def default_tvl1_params(**over):
    return _default_params(Tvl1Params, "va_tvl1_default_params", "TV-L1", over, alias="lambda")


def default_brox_params(**over):
    """``va_brox_default_params`` with keyword overrides: alpha, gamma, scale_step, omega, epsilon, nscales, warps,
    inner_iters, solver_iters and the tuning slots ``BROX_TUNING_SLOTS``.  An unknown name raises ValueError."""
    return _default_params(BroxParams, "va_brox_default_params", "Brox", over)


def default_farneback_params(**over):
    """``va_farneback_default_params`` with keyword overrides: pyr_scale, poly_sigma, levels, winsize, iterations, poly_n,
    gaussian and the tuning slots ``FARNEBACK_TUNING_SLOTS``.  An unknown name raises ValueError, and so does a value out of
    range (the text is ``va_farneback_workspace_bytes``', which names the field)."""
    p = _default_params(FarnebackParams, "va_farneback_default_params", "Farneback", over)
    if lib().va_farneback_workspace_bytes(64, 64, 1, 2, ctypes.byref(p)) == 0:
        raise ValueError(lib().va_last_error().decode())
    return p


def default_dense_traj_params(**over):
    """``va_dtraj_default_params`` with keyword overrides: step, length, patch, nxy, nt, quality, min_flow, min_std, max_std,
    max_dis, max_dis_share and the tuning slots ``DTRAJ_TUNING_SLOTS``.  An unknown name raises ValueError, and so does a value
    out of range (the text is ``va_dtraj_workspace_bytes``', which names the field)."""
    p = _default_params(DenseTrajParams, "va_dtraj_default_params", "dense-trajectory", over)
    if lib().va_dtraj_state_layout(64, 64, ctypes.byref(p), None, 0) == 0:
        raise ValueError(lib().va_last_error().decode())
    return p


def default_stip_params(**over):
    """``va_stip_default_params`` with keyword overrides: sigmas and taus (lists of 1..8 and 1..4 scales), integration, k,
    min_response, cuboid, neighbours, nx, ny, nt, bins and the tuning slots ``STIP_TUNING_SLOTS``.  An unknown name raises
    ValueError, and so does a value out of range (the text is ``va_stip_workspace_bytes``', which names the field)."""
    over = dict(over)
    lists = {k: over.pop(k) for k in ("sigmas", "taus") if k in over}
    p = _default_params(StipParams, "va_stip_default_params", "space-time interest point", over)
    if "sigmas" in lists:
        p.sigma_list = lists["sigmas"]
    if "taus" in lists:
        p.tau_list = lists["taus"]
    if lib().va_stip_workspace_bytes(64, 64, 8, 1, ctypes.byref(p)) == 0:
        raise ValueError(lib().va_last_error().decode())
    return p


def stip_taps(sigma):
    """``va_stip_taps``: the float32 taps g[0..r] of ``sigma`` as the device uses them (numpy array of r + 1 values)."""
    import numpy as np
    buf = (ctypes.c_float * (STIP_MAX_RADIUS + 1))()
    r = lib().va_stip_taps(float(sigma), buf, STIP_MAX_RADIUS + 1)
    if r < 0:
        raise ValueError("stip_taps: sigma must be > 0 with a radius int(4 sigma + 0.5) <= %d, got %r" % (STIP_MAX_RADIUS, sigma))
    return np.frombuffer(buf, dtype=np.float32, count=r + 1).copy()


def default_gmm_params(**over):
    """``va_gmm_default_params`` with keyword overrides: chunk_rows (rows summed serially before the chunks are added, 16 ..
    65536, default 1024) and batch_rows (rows whose responsibilities exist at once, chunk_rows .. 65536, default 65536).  An
    unknown name raises ValueError, and so does a value out of range (the text is ``va_gmm_workspace_bytes``', which names the
    field)."""
    p = _default_params(GmmParams, "va_gmm_default_params", "GMM", over)
    if lib().va_gmm_workspace_bytes(1, 1, 1, 1, ctypes.byref(p)) == 0:
        raise ValueError(lib().va_last_error().decode())
    return p


def default_kmeans_params(**over):
    """``va_kmeans_default_params`` with keyword overrides: chunk_rows (rows per chunk of the update's counting sort, 64 ..
    2^20, default 8192; no result depends on it).  An unknown name raises ValueError, and so does a value out of range (the
    text is ``va_kmeans_workspace_bytes``', which names the field)."""
    p = _default_params(KmeansParams, "va_kmeans_default_params", "k-means", over)
    if lib().va_kmeans_workspace_bytes(1, 1, 1, 1, ctypes.byref(p)) == 0:
        raise ValueError(lib().va_last_error().decode())
    return p


def dtraj_state_layout(w, h, params):
    """``va_dtraj_state_layout``: (bytes of the track table, {region name: byte offset}) -- see include/va.h."""
    off = (ctypes.c_size_t * len(DTRAJ_STATE_REGIONS))()
    n = lib().va_dtraj_state_layout(int(w), int(h), ctypes.byref(params), off, len(DTRAJ_STATE_REGIONS))
    if n == 0:
        raise ValueError(lib().va_last_error().decode())
    return n, dict(zip(DTRAJ_STATE_REGIONS, (int(o) for o in off)))


_ctx = {}


def ctx(device=None):
    """One va_ctx per (process, device)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("video_analytics_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                           "and there is no CPU fallback for the hot path")
    if device is None:
        device = torch.cuda.current_device()
    device = int(device)
    if device not in _ctx:
        h = ctypes.c_void_p()
        check(lib().va_ctx_create(device, ctypes.byref(h)))
        _ctx[device] = h
    return _ctx[device]


def stream_ptr(device=None):
    """The CURRENT stream of ``device`` (a tensor's device or index; default: the current device): every binding
    passes the device of the tensors it hands over, so that a tensor on cuda:1 never travels with cuda:0's stream."""
    import torch
    if isinstance(device, torch.Tensor):
        device = device.device
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
