"""ctypes binding of include/va.h (libva_hip.so).

PyTorch-ROCm tensors are only containers here: raw device pointers (``tensor.data_ptr()``) and
the current HIP stream cross the C ABI, nothing else.  There is no CPU fallback: if the HIP
library is missing or cannot be loaded, every entry point fails loudly.

To add an entry point, write its prototype in include/va.h and one row in ``SIGNATURES`` below, at the same place in
the order: nothing else.  ``lib()`` binds what the table says and ``EXPORTS`` is its keys.  A new parameter struct also gets
a ``ctypes.Structure`` mirror and a pointer alias above the table.  tests/test_abi.py holds the table, the mirrors' layout
and the constants restated here to the header.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libva_hip.so")

VA_OK, VA_ERR_INVALID, VA_ERR_HIP, VA_ERR_WORKSPACE, VA_ERR_STOPPED = 0, 1, 2, 3, 4
VA_COLOR_JITTER_PARTIALS = 256  # include/va.h: uint32 partial sums per image in va_color_jitter_u8's workspace
VA_OPT_BF16_VARIANT, VA_OPT_F32_CONV_KERNEL, VA_OPT_TRAIN_STOP_AT, VA_OPT_BF16_FIRST_LAYER = 1, 2, 3, 4


def _tuning_slots(names):
    """Class decorator: slot ``i`` of the mirror's ``tuning`` array becomes the attribute ``names[i]``."""
    def slot(i):
        return property(lambda self: self.tuning[i], lambda self, v: self.tuning.__setitem__(i, int(v)))

    def name_them(cls):
        for i, name in enumerate(names):
            setattr(cls, name, slot(i))
        return cls
    return name_them


# names of the slots of va_tvl1_params.tuning (csrc/va_internal.h, VA_TUNE_*): the library's own tuning
# switches, addressed by name from tests and tools (``default_tvl1_params(stream_levels=1)``)
TUNING_SLOTS = ("stream_levels", "stream_waves", "stream_chunks", "stream_slots", "rows_levels", "stream_ppl",
                "stream_queue", "rows_cfg")


@_tuning_slots(TUNING_SLOTS)
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


@_tuning_slots(BROX_TUNING_SLOTS)
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


# names of the slots of va_farneback_params.tuning (csrc/va_internal.h, VA_FARNEBACK_TUNE_*)
FARNEBACK_TUNING_SLOTS = ("poly_tile_w", "poly_tile_h", "pass_tile_w", "pass_tile_h")


@_tuning_slots(FARNEBACK_TUNING_SLOTS)
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


# names of the slots of va_dtraj_params.tuning (csrc/va_internal.h, VA_DTRAJ_TUNE_*)
DTRAJ_TUNING_SLOTS = ("chunk_frames", "votes_tile_w", "votes_tile_h")
# the regions of the track table, in the order of va_dtraj_state_layout's offsets (include/va.h)
DTRAJ_STATE_REGIONS = ("counts", "lists", "status", "start", "points", "sums", "occupancy", "pending")


@_tuning_slots(DTRAJ_TUNING_SLOTS)
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


# names of the slots of va_stip_params.tuning (csrc/va_internal.h, VA_STIP_TUNE_*)
STIP_TUNING_SLOTS = ("row_tile_w", "col_tile_w", "col_tile_n")
STIP_MAX_SIGMAS, STIP_MAX_TAUS, STIP_MAX_RADIUS = 8, 4, 512


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


@_tuning_slots(STIP_TUNING_SLOTS)
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
    sigma_list = _scale_list("sigmas", "n_sigmas", STIP_MAX_SIGMAS)
    tau_list = _scale_list("taus", "n_taus", STIP_MAX_TAUS)


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
HMM_MAX_STATES, HMM_MAX_DIM = 1024, 512  # include/va.h: the limits of va_hmm_viterbi's models and va_hmm_emissions' columns


# include/va.h: the channels of va_chi2_combine, the fields of va_kernel_svm_fit_layout in its order, the phases of
# va_kernel_svm_fit_phase
CHI2_MAX_CHANNELS = 16
KSVM_FIT_FIELDS = ("B", "HB", "BC", "Z", "X", "R", "P", "HP", "Q", "free", "q", "pgn", "nsv", "steps", "rr", "cgtol", "cgs", "ref",
                   "live", "notdone", "tight")
KSVM_PHASES = ("init", "eval", "cg", "line_search")


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


# The types of the table.  vp is a handle, a stream or a DEVICE buffer, whatever scalar the header types it as; the p*
# aliases are HOST arrays and structs.
vp, cs, pp = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)
ci, cf, cd, sz, u64 = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_ulonglong
pi, pf, pd, psz, pu64 = (ctypes.POINTER(t) for t in (ci, cf, cd, sz, u64))
p_tvl1, p_tvl1_opt, p_tvl1_launch, p_brox, p_farneback, p_dtraj, p_stip, p_gmm, p_kmeans, p_solver = (
    ctypes.POINTER(t) for t in (Tvl1Params, Tvl1Options, Tvl1Launch, BroxParams, FarnebackParams, DenseTrajParams, StipParams,
                                GmmParams, KmeansParams, SolverParams))

# name: (return type, argument types) of every function include/va.h declares, in the header's order
SIGNATURES = {
    "va_version": (ci, []),
    "va_last_error": (cs, []),
    "va_ctx_create": (ci, [ci, pp]),
    "va_ctx_destroy": (None, [vp]),
    "va_vgg16_create": (ci, [vp, ci, ci, ci, ci, pp, pp, pp, pp, pf, pf, vp, pp]),
    "va_vgg16_destroy": (None, [vp]),
    "va_vgg16_workspace_bytes": (sz, [vp, ci]),
    "va_vgg16_set_option": (ci, [vp, ci, ci]),
    "va_vgg16_forward": (ci, [vp, vp, ci, ci, vp, vp, vp, vp, sz, vp]),
    "va_vgg16_classify": (ci, [vp, vp, ci, vp, vp, vp, sz, vp]),
    "va_copy_first_layer": (ci, [vp, vp, ci, ci, vp, vp]),
    "va_validate_batch": (ci, [vp, vp, vp, ci, ci, vp, vp]),
    "va_tvl1_default_params": (None, [p_tvl1]),
    "va_tvl1_pyramid_sizes": (ci, [ci, ci, p_tvl1, pi, pi]),
    "va_tvl1_tile_plan": (ci, [ci, ci, p_tvl1, pi]),
    "va_tvl1_workspace_bytes": (sz, [ci, ci, ci, ci, p_tvl1]),
    "va_tvl1_flow": (ci, [vp, vp, ci, ci, ci, ci, ci, p_tvl1, vp, vp, sz, vp]),
    "va_tvl1_workspace_bytes_opt": (sz, [ci, ci, ci, ci, p_tvl1, p_tvl1_opt]),
    "va_tvl1_flow_opt": (ci, [vp, vp, ci, ci, ci, ci, ci, p_tvl1, p_tvl1_opt, vp, vp, sz, vp]),
    "va_tvl1_launch_plan": (ci, [ci, ci, ci, ci, p_tvl1, p_tvl1_opt, p_tvl1_launch, ci]),
    "va_flow_median": (ci, [vp, vp, ci, ci, ci, ci, vp, vp]),
    "va_brox_default_params": (None, [p_brox]),
    "va_brox_workspace_bytes": (sz, [ci, ci, ci, ci, p_brox]),
    "va_brox_flow": (ci, [vp, vp, ci, ci, ci, ci, ci, p_brox, vp, vp, sz, vp]),
    "va_brox_inner_step": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, p_brox, vp, sz, vp]),
    "va_farneback_default_params": (None, [p_farneback]),
    "va_farneback_workspace_bytes": (sz, [ci, ci, ci, ci, p_farneback]),
    "va_farneback_flow": (ci, [vp, vp, ci, ci, ci, ci, ci, p_farneback, vp, vp, sz, vp]),
    "va_farneback_polyexp": (ci, [vp, vp, ci, ci, ci, p_farneback, vp, vp]),
    "va_farneback_pass": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, p_farneback, vp]),
    "va_dtraj_default_params": (None, [p_dtraj]),
    "va_dtraj_workspace_bytes": (sz, [ci, ci, ci, ci, p_dtraj]),
    "va_dtraj_extract": (ci, [vp, vp, ci, vp, vp, ci, ci, ci, p_dtraj, vp, vp, vp, ci, pi, pi, vp, sz, vp]),
    "va_dtraj_state_layout": (sz, [ci, ci, p_dtraj, psz, ci]),
    "va_dtraj_votes": (ci, [vp, vp, ci, vp, ci, ci, ci, p_dtraj, vp, vp]),
    "va_dtraj_integral": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "va_dtraj_corner": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "va_dtraj_sample": (ci, [vp, vp, vp, ci, ci, ci, p_dtraj, vp, vp]),
    "va_dtraj_step": (ci, [vp, vp, vp, ci, ci, ci, p_dtraj, vp, vp]),
    "va_dtraj_finish": (ci, [vp, ci, ci, p_dtraj, vp, vp, vp, vp, ci, vp]),
    "va_stip_default_params": (None, [p_stip]),
    "va_stip_workspace_bytes": (sz, [ci, ci, ci, ci, p_stip]),
    "va_stip_extract": (ci, [vp, vp, ci, vp, ci, ci, ci, p_stip, vp, vp, vp, ci, pi, vp, sz, vp]),
    "va_stip_taps": (ci, [cd, pf, ci]),
    "va_stip_smooth": (ci, [vp, vp, ci, ci, ci, ci, cd, cd, p_stip, vp, vp, sz, vp]),
    "va_stip_gradient_products": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "va_stip_response": (ci, [vp, vp, ci, ci, ci, cf, vp, vp]),
    "va_stip_maxima": (ci, [vp, vp, ci, ci, ci, cf, ci, ci, ci, vp, vp, ci, vp, vp, vp]),
    "va_stip_votes": (ci, [vp, vp, vp, ci, ci, ci, p_stip, vp, vp, vp]),
    "va_stip_describe": (ci, [vp, vp, ci, vp, vp, ci, ci, ci, p_stip, vp, vp]),
    "va_flow_to_stack": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp, vp]),
    "va_flow_to_stack_crop": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp, ci, ci, vp, vp]),
    "va_crop_images_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp]),
    "va_flow_to_stack_views": (ci, [vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, ci, ci, ci, vp, vp]),
    "va_crop_images_u8_views": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp]),
    "va_view_mean": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "va_flow_to_stack_snippets": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, ci, ci, ci, vp, vp]),
    "va_flow_to_stack_resize": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp, ci, ci, vp, vp]),
    "va_resize_images_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp]),
    "va_flow_quantize_u8": (ci, [vp, vp, ci, ci, ci, cf, vp, vp]),
    "va_flowq_to_stack_snippets": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ci, cf, cf, vp, ci, ci, ci, vp, vp]),
    "va_flowq_to_stack_resize": (ci, [vp, vp, ci, ci, ci, cf, cf, vp, ci, ci, vp, vp]),
    "va_rgbdiff_to_stack": (ci, [vp, vp, ci, ci, ci, ci, ci, pf, vp, ci, vp, vp]),
    "va_color_jitter_u8": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "va_frames_prepare_workspace_bytes": (sz, [ci, ci, ci, ci, ci]),
    "va_frames_prepare": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "va_jpeg_decode_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
    "va_jpeg_decode": (ci, [vp, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]),
    "va_jpeg_idct": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "va_jpeg_upsample": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp]),
    "va_jpeg_encode_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci, ci]),
    "va_jpeg_encode": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, sz, vp, vp, vp, sz, vp]),
    "va_jpeg_fdct": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "va_jpeg_entropy_encode": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, sz, vp, vp, vp, sz, vp]),
    "va_flow_field_means": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "va_flow_motion": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "va_flow_homography": (ci, [vp, vp, ci, ci, ci, ci, cd, cd, vp, vp, vp]),
    "va_flow_compensate": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
    "va_frames_warp_pairs": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "va_selftest_exact_math": (ci, [vp, cf, cf, vp, vp]),
    "va_conv3x3_layer": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, cs, ci, vp]),
    "va_vgg16_first_layer": (ci, [vp, vp, ci, ci, vp, vp, cs, ci, vp]),
    "va_train_conv_backward_layer": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, vp, psz, cs, ci, vp]),
    "va_train_fc_backward_layer": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, cf, cs, ci, vp]),
    "va_train_conv_backward_layer_grad": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, psz, cs, ci, vp]),
    "va_train_fc_backward_layer_grad": (ci, [vp, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, cf, cs, ci, vp]),
    "va_train_pool_layer": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "va_train_loss": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp]),
    "va_train_loss_multitask": (ci, [vp, vp, vp, vp, ci, ci, ci, pi, vp, vp, vp]),
    "va_train_dropout": (ci, [vp, vp, sz, u64, ci, vp]),
    "va_linear_svm_fit_layout": (sz, [ci, ci, ci, psz, ci]),
    "va_linear_svm_fit_phase": (ci, [vp, vp, vp, ci, ci, ci, cd, cd, cd, ci, ci, vp, sz, vp]),
    "va_tvl1_profile_enable": (ci, [vp, ci]),
    "va_tvl1_profile_read": (ci, [vp, pd, ci]),
    "va_tvl1_profile_levels": (ci, [vp, pd, ci, ci]),
    "va_meter_update": (ci, [vp, vp, vp, ci, ci, vp, vp, ci, vp]),
    "va_meter_average": (ci, [vp, vp, vp, ci, ci, vp, vp]),
    "va_linear_svm_predict": (ci, [vp, vp, ci, ci, vp, vp, ci, vp, vp, vp]),
    "va_linear_svm_fit_workspace_bytes": (sz, [ci, ci, ci]),
    "va_linear_svm_fit": (ci, [vp, vp, vp, ci, ci, ci, cd, cd, cd, ci, ci, vp, vp, vp, vp, sz, vp]),
    "va_linear_svm_fit_cg_steps": (ci, [vp, ci, ci, ci, vp, sz, vp, vp]),
    "va_score_consensus": (ci, [vp, vp, ci, ci, ci, ci, vp, vp]),
    "va_fuse_scores": (ci, [vp, vp, vp, ci, ci, cf, cf, vp, vp, vp]),
    "va_fuse_scores_n": (ci, [vp, pp, pf, ci, ci, ci, vp, vp, vp]),
    "va_vgg16_train_init": (ci, [vp, vp]),
    "va_vgg16_train_workspace_bytes": (sz, [vp, ci]),
    "va_vgg16_train_step": (ci, [vp, vp, ci, vp, ci, cf, cf, u64, vp, vp, vp, sz, vp]),
    "va_vgg16_train_step_consensus": (ci, [vp, vp, ci, vp, ci, ci, cf, cf, u64, vp, vp, vp, sz, vp]),
    "va_vgg16_train_step_multitask": (ci, [vp, vp, ci, vp, vp, ci, ci, ci, pi, cf, cf, u64, vp, vp, vp, sz, vp]),
    "va_vgg16_train_grad_floats": (sz, [vp]),
    "va_vgg16_train_grad_layout": (ci, [vp, psz, psz]),
    "va_vgg16_train_accumulate": (ci, [vp, vp, ci, vp, vp, ci, ci, ci, pi, pf, ci, u64, vp, vp, vp, sz, vp, sz, vp]),
    "va_vgg16_train_apply_workspace_bytes": (sz, []),
    "va_vgg16_train_apply": (ci, [vp, vp, sz, cf, cf, cf, vp, vp, sz, vp]),
    "va_vgg16_unpack_grad": (ci, [vp, vp, pp, pp, pp, pp, vp]),
    "va_solver_default": (None, [p_solver]),
    "va_vgg16_set_solver": (ci, [vp, p_solver]),
    "va_vgg16_get_solver": (ci, [vp, p_solver]),
    "va_train_dropout_p": (ci, [vp, vp, sz, u64, ci, cf, vp]),
    "va_vgg16_train_plan": (ci, [vp, ci, pu64]),
    "va_vgg16_export_state": (ci, [vp, ci, pp, pp, pp, pp, vp]),
    "va_vgg16_import_state": (ci, [vp, ci, pp, pp, pp, pp, vp]),
    "va_pca_workspace_bytes": (sz, [ci, ci]),
    "va_pca_chunk_rows": (ci, [ci, ci]),
    "va_pca_moments": (ci, [vp, vp, ci, ci, ci, vp, vp, sz, vp]),
    "va_pca_transform": (ci, [vp, vp, ci, ci, vp, vp, ci, vp, vp]),
    "va_gmm_default_params": (None, [p_gmm]),
    "va_gmm_workspace_bytes": (sz, [ci, ci, ci, ci, p_gmm]),
    "va_gmm_stats": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, p_gmm, vp, vp, vp, sz, vp]),
    "va_gmm_posteriors": (ci, [vp, vp, ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, sz, vp]),
    "va_gmm_mstep": (ci, [vp, vp, ci, ci, ci, cd, vp, vp, vp, vp]),
    "va_fisher_encode": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, cd, vp, vp]),
    "va_kmeans_default_params": (None, [p_kmeans]),
    "va_kmeans_workspace_bytes": (sz, [ci, ci, ci, ci, p_kmeans]),
    "va_kmeans_tile_centres": (ci, []),
    "va_kmeans_assign": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "va_kmeans_update": (ci, [vp, vp, ci, ci, vp, vp, ci, p_kmeans, vp, vp, vp, vp, sz, vp]),
    "va_kmeans_seed": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, sz, vp]),
    "va_bow_histograms": (ci, [vp, vp, ci, vp, ci, ci, ci, vp, vp]),
    "va_bow_encode": (ci, [vp, vp, ci, ci, vp, ci, vp, ci, ci, vp, vp, sz, vp]),
    "va_hmm_wave_states": (ci, []),
    "va_hmm_wave_edges": (ci, []),
    "va_hmm_backtrack_block": (ci, []),
    "va_hmm_emissions": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, ci, vp, vp]),
    "va_hmm_viterbi": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, sz, sz, vp, sz, vp]),
    "va_hmm_fb_workspace_bytes": (sz, [ci, ci, sz]),
    "va_hmm_forward_backward": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, sz, vp,
                                     sz, sz, vp, vp, vp, sz, vp]),
    "va_hmm_gauss_stats": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, sz, vp, vp, vp, ci, vp, vp, vp]),
    "va_chi2_distance": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "va_linear_gram": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "va_upper_mean": (ci, [vp, vp, ci, vp, vp, vp]),
    "va_chi2_combine": (ci, [vp, pp, pd, ci, sz, vp, vp]),
    "va_kernel_svm_fit_workspace_bytes": (sz, [ci, ci]),
    "va_kernel_svm_fit": (ci, [vp, vp, vp, ci, ci, cd, cd, cd, ci, ci, vp, vp, vp, vp, sz, vp]),
    "va_kernel_svm_fit_layout": (sz, [ci, ci, psz, ci]),
    "va_kernel_svm_fit_phase": (ci, [vp, vp, vp, ci, ci, cd, cd, cd, ci, ci, vp, sz, vp]),
}

# every symbol include/va.h declares (tests check that the library exports exactly these)
EXPORTS = list(SIGNATURES)

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
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


def last_error():
    """``va_last_error``: the library's text for the last call of this thread that failed."""
    return lib().va_last_error().decode("utf-8", "replace")


def check(rc):
    """Map a C return code to the exception the reference's Python surface would raise
    (ValueError for bad arguments -- Sheet03/spatialModel.py:46, Sheet03/utils.py:56)."""
    if rc == VA_OK:
        return
    if rc in (VA_ERR_INVALID, VA_ERR_WORKSPACE):
        raise ValueError(last_error())
    raise RuntimeError(last_error())


def _default_params(cls, fill, label, over, alias=None, probe=None):
    """``cls()`` filled by the library's ``fill``, then the keyword overrides; an unknown name raises ValueError.  ``probe``
    (library, reference to the structure) is a ``*_workspace_bytes`` or ``*_state_layout`` call on a legal shape: where it
    answers 0 a value is out of range, and ``va_last_error``'s text is raised as ValueError."""
    p = cls()
    getattr(lib(), fill)(ctypes.byref(p))
    for k, v in over.items():
        if k == alias:
            k += "_"
        if k == "struct_bytes" or not hasattr(p, k):
            raise ValueError("unknown %s parameter %r" % (label, k))
        setattr(p, k, v)
    if probe is not None and probe(lib(), ctypes.byref(p)) == 0:
        raise ValueError(last_error())
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
    return _default_params(FarnebackParams, "va_farneback_default_params", "Farneback", over,
                           probe=lambda L, p: L.va_farneback_workspace_bytes(64, 64, 1, 2, p))


def default_dense_traj_params(**over):
    """``va_dtraj_default_params`` with keyword overrides: step, length, patch, nxy, nt, quality, min_flow, min_std, max_std,
    max_dis, max_dis_share and the tuning slots ``DTRAJ_TUNING_SLOTS``.  An unknown name raises ValueError, and so does a value
    out of range (the text is ``va_dtraj_workspace_bytes``', which names the field)."""
    return _default_params(DenseTrajParams, "va_dtraj_default_params", "dense-trajectory", over,
                           probe=lambda L, p: L.va_dtraj_state_layout(64, 64, p, None, 0))


def default_stip_params(**over):
    """``va_stip_default_params`` with keyword overrides: sigmas and taus (lists of 1..8 and 1..4 scales), integration, k,
    min_response, cuboid, neighbours, nx, ny, nt, bins and the tuning slots ``STIP_TUNING_SLOTS``.  An unknown name raises
    ValueError, and so does a value out of range (the text is ``va_stip_workspace_bytes``', which names the field)."""
    over = dict(over)
    for k in ("sigmas", "taus"):  # after the other fields, through the property that keeps the count with the scales
        if k in over:
            over[k[:-1] + "_list"] = over.pop(k)
    return _default_params(StipParams, "va_stip_default_params", "space-time interest point", over,
                           probe=lambda L, p: L.va_stip_workspace_bytes(64, 64, 8, 1, p))


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
    return _default_params(GmmParams, "va_gmm_default_params", "GMM", over,
                           probe=lambda L, p: L.va_gmm_workspace_bytes(1, 1, 1, 1, p))


def default_kmeans_params(**over):
    """``va_kmeans_default_params`` with keyword overrides: chunk_rows (rows per chunk of the update's counting sort, 64 ..
    2^20, default 8192; no result depends on it).  An unknown name raises ValueError, and so does a value out of range (the
    text is ``va_kmeans_workspace_bytes``', which names the field)."""
    return _default_params(KmeansParams, "va_kmeans_default_params", "k-means", over,
                           probe=lambda L, p: L.va_kmeans_workspace_bytes(1, 1, 1, 1, p))


def dtraj_state_layout(w, h, params):
    """``va_dtraj_state_layout``: (bytes of the track table, {region name: byte offset}) -- see include/va.h."""
    off = (ctypes.c_size_t * len(DTRAJ_STATE_REGIONS))()
    n = lib().va_dtraj_state_layout(int(w), int(h), ctypes.byref(params), off, len(DTRAJ_STATE_REGIONS))
    if n == 0:
        raise ValueError(last_error())
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
