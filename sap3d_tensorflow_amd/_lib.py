"""ctypes binding of libp3dhip.so (include/p3d_hip.h).  There is no CPU fallback: a missing or
unloadable library, or a box without a HIP device, raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3D_LIB: another build of the same library (same-box A/Bs against an older round's, tools/ab/); every declared symbol must
# still bind, so it cannot be anything else
LIB_PATH = os.environ.get("P3D_LIB") or os.path.join(_HERE, "libp3dhip.so")

P3D_COMM_ID_BYTES = 128
# p3d_set_loss kinds (include/p3d_hip.h P3D_LOSS_*)
LOSSES = {"smooth_l1": 0, "bce": 1, "l1": 2}
# the per-map loss P3D_LOSS_KLD_CC under its names: (kld_weight, cc_weight) of p3d_set_loss_weights
P3D_LOSS_KLD_CC = 3
MAP_LOSSES = {"kld": (1.0, 0.0), "kld_cc": (1.0, 1.0)}
# the per-map loss with a fixation map, P3D_LOSS_SALIENCY: (kld, cc, nss, sim) of p3d_set_saliency_weights
P3D_LOSS_SALIENCY = 4
SALIENCY_LOSSES = {"kld_cc_nss": (1.0, 1.0, 1.0, 0.0), "kld_cc_nss_sim": (1.0, 1.0, 1.0, 1.0)}
# p3d_set_regularization terms (include/p3d_hip.h P3D_REG_*)
REGULARIZATION = {"weightdecay": 1, "l2": 2}
# p3d_set_optimizer kinds (include/p3d_hip.h P3D_OPT_*) and the TF slot names of each kind's slots 0, 1 (<var>/<suffix>)
OPTIMIZERS = {"adam": 0, "momentum": 1, "sgd": 2}
SLOT_NAMES = {"adam": ("Adam", "Adam_1"), "momentum": ("Momentum",), "sgd": ()}


class P3dConfig(C.Structure):
    _fields_ = [("structure", C.c_int), ("batch", C.c_int), ("frames", C.c_int), ("height", C.c_int),
                ("width", C.c_int), ("base", C.c_int), ("blocks", C.c_int * 3), ("device", C.c_int),
                ("world_size", C.c_int), ("rank", C.c_int)]


class P3dOpTime(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("kernel", C.c_char * 48), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("phase", C.c_int)]


class P3dAugment(C.Structure):
    _fields_ = [("p_flip", C.c_float), ("p_reverse", C.c_float), ("min_scale", C.c_float), ("contrast", C.c_float),
                ("brightness", C.c_float)]


class P3dPostprocess(C.Structure):
    _fields_ = [("sigma", C.c_float), ("radius", C.c_int), ("norm", C.c_int)]


class P3dRender(C.Structure):
    """p3d_render: table[v] = b | g << 8 | r << 16 | o << 24; contour level 0 is off."""
    _fields_ = [("table", C.c_uint32 * 256), ("contour_level", C.c_int), ("contour_thickness", C.c_int), ("contour_bgr", C.c_ubyte * 3)]


class P3dReframe(C.Structure):
    """p3d_reframe: the window, the gate level (0 .. 255) and the smoothing radius in frames (0 .. 255)."""
    _fields_ = [("crop_h", C.c_int), ("crop_w", C.c_int), ("gate", C.c_int), ("smooth_radius", C.c_int)]


class P3dVideoTemporal(C.Structure):
    _fields_ = [("kind", C.c_int), ("sigma", C.c_float), ("radius", C.c_int), ("alpha", C.c_float)]


# p3d_set_postprocess normalisations (include/p3d_hip.h P3D_NORM_*)
NORMS = {"none": 0, "max": 1, "range": 2}
P3D_BLUR_MAX_RADIUS = 255


class P3dHistMatch(C.Structure):
    _fields_ = [("mode", C.c_int), ("nbins", C.c_int), ("nt", C.c_int), ("cdf", C.POINTER(C.c_double)), ("centres", C.POINTER(C.c_double))]


# p3d_set_hist_match modes (include/p3d_hip.h P3D_MATCH_*)
MATCH_MODES = {"off": 0, "table": 1, "density": 2}
P3D_HIST_MAX_BINS = 1024
# p3d_set_eval_extra flags (include/p3d_hip.h P3D_EVAL_*)
EVAL_EXTRA = {"kldiv": 1, "info_gain": 2}
# p3d_video_open modes (include/p3d_hip.h P3D_VIDEO_*)
VIDEO_MODES = {"newest": 0, "mean": 1}
# p3d_trainset_open frame formats and flags (include/p3d_hip.h P3D_TRAINSET_*)
# p3d_video_score / p3d_score_maps_u8: the columns' flags (also their order in a row of scores) and the AUC-Judd ties laws
SCORE_COLUMNS = {"cc": 1, "sim": 2, "judd": 4, "kl": 8, "nss": 16}
SCORE_MATLAB = ("cc", "sim", "judd")
SCORE_TIES = {"reference": 0, "expected": 1}
TRAINSET_FORMATS = {"u8": 0, "f32": 1}
P3D_TRAINSET_FIXATIONS = 1
# dataflow.render_table: this project's own colour maps and the two opacity laws
RENDER_COLORMAPS = ("grey", "hot", "jet")
RENDER_OPACITIES = ("constant", "ramp")
# p3d_set_video_temporal kinds (include/p3d_hip.h P3D_TEMPORAL_*)
TEMPORAL_KINDS = {"off": 0, "gauss": 1, "ema": 2}
P3D_TEMPORAL_MAX_RADIUS = 24
# P3D_PRIOR_* of include/p3d_hip.h: what a map adds to the accumulator, and how the stage combines a map with the prior
PRIOR_KINDS = {"fixations": 0, "bytes": 1}
PRIOR_MODES = {"off": 0, "mul": 1, "mix": 2}
P3D_PRIOR_MAX_MAPS = 16000000


# the descriptors of p3d_debug_fused_conv (include/p3d_hip.h)
_FP = C.POINTER(C.c_float)


class P3dFusedBn(C.Structure):
    _fields_ = [("y", _FP), ("ld", C.c_int), ("off", C.c_int), ("gamma", _FP), ("beta", _FP), ("partials", _FP), ("nparts", C.c_int),
                ("rows", C.c_int64), ("publish", C.c_int), ("update_moving", C.c_int), ("scale", _FP), ("shift", _FP), ("mean", _FP),
                ("invstd", _FP), ("moving_mean", _FP), ("moving_var", _FP)]


class P3dFusedBnGrad(C.Structure):
    _fields_ = [("y", _FP), ("ld", C.c_int), ("off", C.c_int), ("gamma", _FP), ("mean", _FP), ("invstd", _FP), ("partials", _FP),
                ("nparts", C.c_int), ("rows", C.c_int64), ("publish", C.c_int), ("coef", _FP), ("dgamma", _FP), ("dbeta", _FP)]


class P3dFusedGate(C.Structure):
    _fields_ = [("y", _FP), ("ld_y", C.c_int), ("off_y", C.c_int), ("scale", _FP), ("shift", _FP), ("mean", _FP), ("invstd", _FP),
                ("out", _FP), ("ld_out", C.c_int), ("off_out", C.c_int), ("part", _FP), ("part_rows", C.c_int)]


class P3dFusedConv(C.Structure):
    _fields_ = [("kind", C.c_int), ("xshape", C.c_int64 * 5), ("wshape", C.c_int64 * 5), ("stride", C.c_int * 3), ("w", _FP),
                ("bias", _FP), ("f16", C.c_int), ("at", C.c_int), ("src", P3dFusedBn * 2), ("g", _FP), ("ld_g", C.c_int),
                ("off_g", C.c_int), ("grad", C.c_int), ("gbn", P3dFusedBnGrad), ("ngate", C.c_int), ("gate", P3dFusedGate * 2),
                ("raw_store", C.c_int), ("accum", C.c_int), ("out", _FP), ("ld_out", C.c_int), ("off_out", C.c_int),
                ("gpart_rows", C.c_int)]


class P3dError(RuntimeError):
    pass


_lib = None
_fp = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_ubyte)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)

# every symbol include/p3d_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "p3d_default_config": (None, [C.POINTER(P3dConfig)]),
    "p3d_create": (C.c_int, [C.POINTER(P3dConfig), C.POINTER(C.c_void_p)]),
    "p3d_destroy": (None, [C.c_void_p]),
    "p3d_last_error": (C.c_char_p, []),
    "p3d_num_params": (C.c_int, [C.c_void_p]),
    "p3d_param_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), _ip, _i64p, _ip]),
    "p3d_set_param": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_get_param": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_get_grad": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_init_params": (C.c_int, [C.c_void_p, C.c_uint64]),
    "p3d_forward": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_float, C.c_uint64, _fp]),
    "p3d_predict_windows": (C.c_int, [C.c_void_p, _fp, _fp]),
    "p3d_block_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "p3d_block_forward": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int64, _fp, C.c_int64]),
    "p3d_block_backward": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int64, _fp, C.c_int64, _fp]),
    "p3d_set_pointwise_fp16": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_set_bn_fusion": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_set_attention_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_set_loss": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_set_loss_weights": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "p3d_set_saliency_weights": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "p3d_upload_fixations": (C.c_int, [C.c_void_p, _u8p]),
    "p3d_last_loss_terms": (C.c_int, [C.c_void_p, _dp, _i64p]),
    "p3d_set_regularization": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "p3d_last_regularization": (C.c_int, [C.c_void_p, _dp]),
    "p3d_param_regularization": (C.c_int, [C.c_void_p, C.c_char_p, _fp, _fp]),
    "p3d_debug_dirty_counters": (C.c_int64, []),
    "p3d_debug_force_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "p3d_debug_schedule": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_char_p, C.c_int64, _i64p]),
    "p3d_debug_perturb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "p3d_debug_perturb_count": (C.c_int, [C.c_void_p, _i64p, _i64p]),
    "p3d_debug_perturb_selftest": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_debug_decision_count": (C.c_int, [C.c_void_p]),
    "p3d_debug_decision_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), _i64p]),
    "p3d_debug_decision_get": (C.c_int, [C.c_void_p, C.c_int, _fp, _fp, C.c_int64]),
    "p3d_train_step": (C.c_int, [C.c_void_p, _fp, _fp, C.c_float, C.c_uint64, _fp]),
    "p3d_backward": (C.c_int, [C.c_void_p, _fp, _fp, C.c_float, C.c_uint64, _fp, _fp]),
    "p3d_set_adam": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "p3d_set_optimizer": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]),
    "p3d_get_slot": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _fp, C.c_int64]),
    "p3d_set_slot": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _fp, C.c_int64]),
    "p3d_get_optimizer_step": (C.c_int, [C.c_void_p, _i64p]),
    "p3d_set_optimizer_step": (C.c_int, [C.c_void_p, C.c_int64]),
    "p3d_activation_info": (C.c_int, [C.c_void_p, C.c_char_p, _i64p]),
    "p3d_get_activation": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_upload_inputs": (C.c_int, [C.c_void_p, _fp, _fp]),
    "p3d_train_step_device": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64]),
    "p3d_forward_device": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint64]),
    "p3d_last_loss": (C.c_int, [C.c_void_p, _fp]),
    "p3d_synchronize": (C.c_int, [C.c_void_p]),
    "p3d_profile_step": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.POINTER(P3dOpTime), C.c_int]),
    "p3d_comm_unique_id": (C.c_int, [C.c_void_p]),
    "p3d_comm_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "p3d_debug_stem_wgrad_through_bn": (C.c_int, [C.c_int, _fp, C.POINTER(C.c_int64), _fp, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "p3d_debug_install_abort_trace": (C.c_int, []),
    "p3d_device_count": (C.c_int, []),
    "p3d_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "p3d_debug_bucket_audit": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_int64, _i64p, _i64p, C.POINTER(C.c_int32), C.c_int,
                                         _i64p, _i64p]),
    "p3d_op_conv3d": (C.c_int, [C.c_int, _fp, _i64p, _fp, _i64p, _ip, _fp, _fp]),
    "p3d_debug_conv_bn_stats": (C.c_int, [C.c_int, _fp, _i64p, _fp, _fp, _i64p, _ip, _fp, C.c_int, _fp, _fp, _fp, _fp, _ip,
                                          C.POINTER(C.c_char_p)]),
    "p3d_debug_bn_pass": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int,
                                    C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_int, _fp, C.c_int, C.c_int,
                                    _fp, _fp, _fp, _fp, _ip]),
    "p3d_debug_gn_pass": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _fp, C.c_int, _fp, C.c_int,
                                    C.c_int, _fp, _fp, _fp, _fp, C.c_int, C.c_float, C.c_uint64, C.c_int, _fp, _fp, _fp, _fp, _fp,
                                    _ip]),
    "p3d_debug_cbam": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, _fp, _fp, _fp,
                                 C.c_int, _fp, C.c_int, _fp, _fp, _fp, _fp, _fp, _ip]),
    "p3d_debug_head": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, C.c_int, _fp,
                                 C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _ip]),
    "p3d_debug_smooth_l1": (C.c_int, [C.c_int, _fp, _fp, C.c_int64, C.c_int, C.c_int, _dp, _fp, _ip]),
    "p3d_debug_loss": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, C.c_int64, C.c_int, C.c_int, _dp, _fp, _ip]),
    "p3d_debug_map_loss": (C.c_int, [C.c_int, _fp, _fp, _fp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, _dp,
                                     _fp, _dp, _ip]),
    "p3d_debug_saliency_loss": (C.c_int, [C.c_int, _fp, _fp, _fp, _u8p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float,
                                          C.c_float, C.c_float, _dp, _fp, _dp, _ip]),
    "p3d_debug_adam_decay": (C.c_int, [C.c_int, _fp, _fp, _fp, _fp, C.c_int64, C.c_int, _i64p, _i64p, _fp, C.c_int, C.c_float,
                                       C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _dp, _fp]),
    "p3d_debug_optimizer": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]),
    "p3d_debug_optimizer_decay": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, C.c_int64, C.c_int, _i64p, _i64p, _fp, C.c_int, C.c_float,
                                            C.c_float, C.c_int, C.c_int, C.c_int, _dp]),
    "p3d_debug_adam": (C.c_int, [C.c_int, _fp, _fp, _fp, _fp, C.c_int64, C.c_int, C.c_float, C.c_int64, C.c_float, C.c_float,
                                 C.c_float, C.c_int, _fp]),
    "p3d_debug_opt_scaled": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int64, C.c_int, _i64p, _i64p, _fp, C.c_int, C.c_float,
                                       C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, _dp, _fp]),
    "p3d_debug_grad_norm": (C.c_int, [C.c_int, _fp, _fp, C.c_int64, C.c_int, _i64p, _i64p, _fp, C.c_int, _i64p, _i64p, C.c_int,
                                      C.c_float, C.c_int, _dp, _dp, _fp]),
    "p3d_set_grad_clip": (C.c_int, [C.c_void_p, C.c_float]),
    "p3d_get_grad_norm": (C.c_int, [C.c_void_p, _dp, _dp, _fp]),
    "p3d_set_ema": (C.c_int, [C.c_void_p, C.c_double, C.c_int]),
    "p3d_get_ema": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_set_ema_var": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.c_int64]),
    "p3d_ema_swap": (C.c_int, [C.c_void_p]),
    "p3d_ema_swapped": (C.c_int, [C.c_void_p]),
    "p3d_set_grad_accum": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_get_grad_accum": (C.c_int, [C.c_void_p, _ip, _ip]),
    "p3d_debug_grad_accum": (C.c_int, [C.c_int, C.c_int, _fp, _fp, C.c_int64, C.c_int]),
    "p3d_debug_ema": (C.c_int, [C.c_int, _fp, _fp, C.c_int64, C.c_int, C.c_float, C.c_int]),
    "p3d_set_augment": (C.c_int, [C.c_void_p, C.POINTER(P3dAugment)]),
    "p3d_get_augment": (C.c_int, [C.c_void_p, C.POINTER(P3dAugment), _ip]),
    "p3d_augment_inputs": (C.c_int, [C.c_void_p, C.c_uint64]),
    "p3d_last_augment": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), _fp]),
    "p3d_last_augment_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_debug_augment": (C.c_int, [C.c_int, _fp, _fp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _fp, C.c_int,
                                    _fp, _fp, _u8p]),
    "p3d_debug_augment_draw": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(P3dAugment), C.POINTER(C.c_int32), _fp]),
    "p3d_debug_stat_parts": (C.c_int, [_i64p, _i64p, _ip, C.c_int, _ip, _ip]),
    "p3d_debug_igemm_groupable": (C.c_int, [_i64p, _i64p, _ip]),
    "p3d_op_conv3d_backprop_input": (C.c_int, [C.c_int, _fp, _fp, _i64p, _ip, _i64p, _fp]),
    "p3d_op_conv3d_backprop_filter": (C.c_int, [C.c_int, _fp, _i64p, _fp, _i64p, _ip, _fp, _fp]),
    "p3d_op_conv3d_transpose": (C.c_int, [C.c_int, _fp, _i64p, _fp, _i64p, _ip, _fp, _fp]),
    "p3d_op_max_pool3d": (C.c_int, [C.c_int, _fp, _i64p, _ip, _ip, _fp]),
    "p3d_op_max_pool3d_grad": (C.c_int, [C.c_int, _fp, _i64p, _ip, _ip, _fp, _fp]),
    "p3d_op_bias_add_grad": (C.c_int, [C.c_int, _fp, C.c_int64, C.c_int, _fp]),
    "p3d_debug_conv_launch": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int, C.c_int, _i64p, _fp, _i64p, _ip, _fp, C.c_int, C.c_int, _fp,
                                        C.c_int, C.c_int, C.c_char_p, C.c_int, _ip]),
    "p3d_debug_fused_conv": (C.c_int, [C.c_int, C.POINTER(P3dFusedConv), C.c_char_p, C.c_int, _ip]),
    "p3d_debug_fused_wgrad": (C.c_int, [C.c_int, C.c_int, C.POINTER(_fp), _ip, _ip, _i64p, C.POINTER(_fp), _ip, _ip, _i64p, _ip,
                                        _ip, C.POINTER(_fp), _ip, _ip, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), _ip,
                                        C.POINTER(_fp), _ip, _ip, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.c_char_p, C.c_int, _ip,
                                        _ip]),
    "p3d_debug_fused_reject": (C.c_int, [C.c_int, C.c_int, _ip, _ip]),
    "p3d_debug_wgrad_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(_fp), _ip, _ip, _i64p, C.POINTER(_fp), _ip, _ip, _i64p, _ip, _ip,
                                        C.POINTER(_fp), C.POINTER(_fp), C.c_int, C.c_int, C.c_char_p, C.c_int, _ip, _ip]),
    "p3d_debug_max_pool3d": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, _i64p, _ip, _ip, _fp, C.c_int, C.c_int]),
    "p3d_debug_max_pool3d_grad": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, _i64p, _ip, _ip, _fp, C.c_int, C.c_int, C.c_int, _fp,
                                            C.POINTER(C.c_char_p)]),
    "p3d_debug_bias_add_grad": (C.c_int, [C.c_int, _fp, C.c_int64, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_op_attention_core": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "p3d_debug_attention_core": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "p3d_debug_attention_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "p3d_debug_softmax_rows": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _fp, _fp, C.c_int]),
    "p3d_debug_attn_mix": (C.c_int, [C.c_int, C.c_int64, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_uint64, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, _fp]),
    "p3d_metric_cc": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_metric_sim": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_metric_nss": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_metric_auc_judd": (C.c_int, [C.c_int, _fp, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_metric_auc_borji": (C.c_int, [C.c_int, _fp, _fp, _ip, C.c_int, C.c_int, C.c_int, C.c_double, _dp]),
    "p3d_mapf_frames": (C.c_int, [C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp]),
    "p3d_mapf_density": (C.c_int, [C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_resize_linear": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_metric_auc_shuffled": (C.c_int, [C.c_int, _fp, _fp, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _dp]),
    "p3d_eval_last_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                       _dp, _ip, _ip, C.c_int, C.c_double, _dp, _dp]),
    "p3d_debug_eval_maps": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                      C.POINTER(C.c_ubyte), C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, C.c_double, _dp]),
    "p3d_resize_linear_u8": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]),
    "p3d_pred_maps_u8": (C.c_int, [C.c_void_p, _ip, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_ubyte), _dp]),
    "p3d_set_postprocess": (C.c_int, [C.c_void_p, C.POINTER(P3dPostprocess)]),
    "p3d_get_postprocess": (C.c_int, [C.c_void_p, C.POINTER(P3dPostprocess), _ip]),
    "p3d_blur_taps": (C.c_int, [C.c_float, C.c_int, _fp, C.c_int, _ip]),
    "p3d_debug_blur_strip": (C.c_int, [C.c_int, _ip, _ip, _ip]),
    "p3d_gaussian_blur": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _fp]),
    "p3d_postprocess_maps": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P3dPostprocess),
                                       C.c_float, _fp, _u8p]),
    "p3d_debug_eval_maps_post": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                           C.POINTER(C.c_ubyte), C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, C.c_double, _dp,
                                           C.POINTER(P3dPostprocess)]),
    "p3d_cumulative_distribution": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _i64p, _dp, _dp]),
    "p3d_match_hist": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _fp]),
    "p3d_match_hist_maps": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_set_hist_match": (C.c_int, [C.c_void_p, C.POINTER(P3dHistMatch)]),
    "p3d_get_hist_match": (C.c_int, [C.c_void_p, C.POINTER(P3dHistMatch)]),
    "p3d_postprocess_maps_match": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P3dPostprocess),
                                             C.POINTER(P3dHistMatch), C.c_float, _fp, _u8p]),
    "p3d_debug_eval_maps_match": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                            C.POINTER(C.c_ubyte), C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, C.c_double, _dp,
                                            C.POINTER(P3dPostprocess), C.POINTER(P3dHistMatch)]),
    "p3d_set_eval_extra": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int, C.c_int]),
    "p3d_get_eval_extra": (C.c_int, [C.c_void_p, _ip, C.POINTER(_fp), _ip, _ip]),
    "p3d_last_eval_extra": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "p3d_debug_eval_maps_extra": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                            C.POINTER(C.c_ubyte), C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, C.c_double, _dp,
                                            C.POINTER(P3dPostprocess), C.POINTER(P3dHistMatch), C.c_int, _fp, _dp]),
    "p3d_metric_kldiv": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_metric_info_gain": (C.c_int, [C.c_int, _fp, _fp, _fp, C.c_int, C.c_int, _dp]),
    "p3d_prior_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "p3d_prior_add": (C.c_int, [C.c_void_p, _u8p, C.c_int64, C.c_int]),
    "p3d_prior_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), _i64p]),
    "p3d_prior_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _i64p]),
    "p3d_prior_finish": (C.c_int, [C.c_void_p, C.c_float, C.c_int, _fp]),
    "p3d_prior_close": (C.c_int, [C.c_void_p]),
    "p3d_prior_last_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_set_prior_map": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int]),
    "p3d_get_prior_map": (C.c_int, [C.c_void_p, _fp, C.c_int64, _ip, _ip]),
    "p3d_set_prior_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "p3d_get_prior_stage": (C.c_int, [C.c_void_p, _ip, _fp]),
    "p3d_set_eval_extra_prior": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_debug_prior_count": (C.c_int, [C.c_int, C.c_int, _u8p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int,
                                        C.POINTER(C.c_uint32), _ip]),
    "p3d_debug_prior_count_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, _i64p, _i64p, _ip]),
    "p3d_debug_prior_apply": (C.c_int, [C.c_int, C.c_int, C.c_float, _fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp]),
    "p3d_postprocess_maps_prior": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P3dPostprocess),
                                             C.POINTER(P3dHistMatch), _fp, C.c_int, C.c_float, C.c_float, _fp, _u8p]),
    "p3d_debug_eval_maps_prior": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                            C.POINTER(C.c_ubyte), C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, C.c_double, _dp,
                                            C.POINTER(P3dPostprocess), C.POINTER(P3dHistMatch), C.c_int, _fp, _dp, _fp, C.c_int, C.c_float]),
    "p3d_fixpool_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64]),
    "p3d_fixpool_put": (C.c_int, [C.c_void_p, C.c_int64, _u8p, C.c_int64]),
    "p3d_fixpool_info": (C.c_int, [C.c_void_p, _ip, _ip, _i64p, _i64p, _i64p]),
    "p3d_fixpool_get": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_uint64)]),
    "p3d_fixpool_close": (C.c_int, [C.c_void_p]),
    "p3d_fixpool_last_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_eval_shuffled_begin": (C.c_int, [C.c_void_p, _ip, C.c_int, C.POINTER(C.c_uint32)]),
    "p3d_eval_shuffled_draws": (C.c_int, [C.c_void_p, _ip, _ip, C.c_int, C.c_double]),
    "p3d_last_eval_shuffled": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "p3d_debug_fix_pack": (C.c_int, [C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "p3d_debug_fix_union": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "p3d_debug_fix_select": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, _ip, _ip, C.c_int, _ip]),
    "p3d_debug_eval_maps_shuffled": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int,
                                               _dp, _ip, _ip, C.c_int, C.c_double, _dp, C.POINTER(P3dPostprocess), C.POINTER(P3dHistMatch),
                                               C.c_int, _fp, _dp, _fp, C.c_int, C.c_float, _u8p, C.c_int, _ip, C.c_int, _ip, _ip, C.c_int,
                                               C.c_double, C.POINTER(C.c_uint32), _dp]),
    "p3d_video_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "p3d_video_close": (C.c_int, [C.c_void_p]),
    "p3d_video_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip]),
    "p3d_video_put_frames": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int]),
    "p3d_video_put_frames_u8": (C.c_int, [C.c_void_p, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_video_predict": (C.c_int, [C.c_void_p, _ip, C.c_int]),
    "p3d_video_get_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp, C.POINTER(C.c_int32)]),
    "p3d_video_maps_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, _dp]),
    "p3d_video_last_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_debug_video_gather": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, C.c_int64, _ip, C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_debug_video_scatter": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_int64, C.c_int, _ip, C.c_int, C.c_int, C.c_int,
                                          _fp, C.POINTER(C.c_int32), C.c_int]),
    "p3d_debug_video_mean": (C.c_int, [C.c_int, _fp, C.POINTER(C.c_int32), C.c_int, C.c_int64, C.c_int, _fp]),
    "p3d_debug_video_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _ip, C.c_int,
                                       C.POINTER(C.c_int32)]),
    "p3d_set_video_temporal": (C.c_int, [C.c_void_p, C.POINTER(P3dVideoTemporal)]),
    "p3d_get_video_temporal": (C.c_int, [C.c_void_p, C.POINTER(P3dVideoTemporal), _ip]),
    "p3d_video_temporal_last_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_temporal_filter": (C.c_int, [C.c_int, C.POINTER(P3dVideoTemporal), _fp, C.c_int, C.c_int64, C.c_int, C.c_int, _fp]),
    "p3d_debug_video_temporal": (C.c_int, [C.c_int, C.c_int, C.POINTER(P3dVideoTemporal), _fp, C.POINTER(C.c_int32), C.c_int, C.c_int64,
                                           C.c_int, C.c_int, C.c_int, _fp]),
    "p3d_debug_video_temporal_plan": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, _ip, _ip, _ip]),
    "p3d_debug_video_temporal_desc": (C.c_int, [C.c_int, C.POINTER(P3dVideoTemporal), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                                _dp, _dp]),
    "p3d_trainset_open": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int, C.c_int, _fp]),
    "p3d_trainset_close": (C.c_int, [C.c_void_p]),
    "p3d_trainset_info": (C.c_int, [C.c_void_p, _ip, _i64p, _ip, _ip, _i64p]),
    "p3d_trainset_video_info": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip, _ip]),
    "p3d_trainset_put_frames_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_int]),
    "p3d_trainset_put_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp, C.c_int]),
    "p3d_trainset_put_density_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_int]),
    "p3d_trainset_put_fixations": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p, C.c_int]),
    "p3d_trainset_stage": (C.c_int, [C.c_void_p, _ip, _ip, C.c_int]),
    "p3d_trainset_step": (C.c_int, [C.c_void_p, _ip, _ip, C.c_int, C.c_float, C.c_uint64, _fp]),
    "p3d_trainset_forward": (C.c_int, [C.c_void_p, _ip, _ip, C.c_int, _fp]),
    "p3d_trainset_get_staged": (C.c_int, [C.c_void_p, _fp, _fp, _u8p]),
    "p3d_trainset_last_ms": (C.c_int, [C.c_void_p, _dp]),
    "p3d_debug_trainset_gather": (C.c_int, [C.c_int, C.c_int, C.c_void_p, _u8p, _u8p, C.c_int, _ip, C.c_int, C.c_int64, _fp, _ip, _ip, _ip,
                                            C.c_int, C.c_int, _fp, _fp, _u8p]),
    "p3d_video_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, _u8p, C.c_int, C.c_int, _dp, _u8p, _dp]),
    "p3d_score_maps_u8": (C.c_int, [C.c_int, _u8p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]),
    "p3d_debug_score_u8": (C.c_int, [C.c_int, _u8p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _dp]),
    "p3d_debug_score_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, _ip, _ip, _i64p]),
    "p3d_score_sweep_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_double, _dp]),
    "p3d_debug_score_sweep_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_double, C.c_int, _ip, _ip, _dp]),
    "p3d_video_shuffled_begin": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int, C.POINTER(C.c_uint32)]),
    "p3d_video_score_auc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, _u8p, C.c_int, C.c_int, _dp, _ip, _ip, _ip,
                                      C.c_int, C.c_double, _dp, _dp, _dp]),
    "p3d_render_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(P3dRender), _u8p]),
    "p3d_video_keep_source": (C.c_int, [C.c_void_p, C.c_int]),
    "p3d_video_source_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _i64p]),
    "p3d_video_render": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, C.POINTER(P3dRender), _u8p, _u8p, _dp]),
    "p3d_debug_render_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(P3dRender), C.c_int, _u8p]),
    "p3d_debug_render_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _i64p]),
    "p3d_reframe_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(P3dReframe), _i32p, _i32p, _u32p, _u8p]),
    "p3d_video_reframe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, C.POINTER(P3dReframe), _i32p, _i32p, _u32p,
                                    _u8p, _u8p, _dp]),
    "p3d_debug_reframe_u8": (C.c_int, [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(P3dReframe), C.c_int, _i32p, _i32p, _u32p, _u8p]),
    "p3d_debug_reframe_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _i64p]),
    "p3d_crc32c": (C.c_uint32, [C.c_void_p, C.c_size_t, C.c_uint32]),
    "p3d_shutdown": (C.c_int, []),
}


def _torch_lib_dir():
    """Directory of the ROCm libraries a PyTorch-ROCm wheel bundles (torch/lib), or None.  Does not import torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        return None
    if spec is None or not spec.origin:
        return None
    d = os.path.join(os.path.dirname(spec.origin), "lib")
    return d if os.path.exists(os.path.join(d, "libamdhip64.so")) else None


def _one_rocm_runtime_per_process():
    """One HIP runtime per process, whatever the import order.  PyTorch-ROCm wheels bundle their own libamdhip64 /
    libhsa-runtime64 / librccl (torch/lib) under the same sonames as /opt/rocm's.  If libp3dhip.so were loaded first it
    would bind to /opt/rocm's copies, a later `import torch` would map the bundled ones next to them: two HIP runtimes
    in one process (tools/dupe_probe.py).  So when such a wheel is installed and torch is not loaded yet, its bundled runtime is mapped
    here BY PATH, without importing torch (a first `import torch` costs a minute or two on a fresh box): libp3dhip then
    binds to it by soname, and so does torch whenever it is imported.  With torch already imported nothing is needed."""
    import sys
    if "torch" in sys.modules:
        return
    if mapped_rocm_runtimes():
        return          # a runtime is already mapped (e.g. rocprofv3 preloads /opt/rocm's): bind to that one
    d = _torch_lib_dir()
    if d is None:
        return
    for name in ("libhsa-runtime64.so", "libamdhip64.so", "librccl.so"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            C.CDLL(p)        # RTLD_LOCAL: see lib()


def mapped_rocm_runtimes():
    """{library stem: sorted list of distinct files mapped into this process} for the HIP / HSA / RCCL runtimes."""
    import re
    found = {}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                m = re.search(r"(/\S*/(libamdhip64|libhsa-runtime64|librccl)\.so[^\s/]*)", line)
                if m:
                    found.setdefault(m.group(2), set()).add(os.path.realpath(m.group(1)))
    except OSError:
        pass
    return dict((k, sorted(v)) for k, v in found.items())


def _refuse_two_runtimes():
    dup = dict((k, v) for k, v in mapped_rocm_runtimes().items() if len(v) > 1)
    if dup:
        raise P3dError("two copies of a ROCm runtime library are mapped into this process (%s): it would crash at exit. "
                       "Load sap3d_tensorflow_amd (or torch) before anything else that pulls in a HIP runtime; see "
                       "INTEGRATION.md, 'One HIP runtime per process'." % dup)


_sessions = None


def register_session(s):
    """Sessions are closed, and the library's process-wide device resources released, from a Python atexit hook -- i.e.
    before interpreter finalisation and before any C++ static destructor -- so teardown never depends on the order in
    which libraries were loaded."""
    global _sessions
    if _sessions is None:
        import weakref
        _sessions = weakref.WeakSet()
    _sessions.add(s)


def _shutdown():
    if _sessions is not None:
        for s in list(_sessions):
            try:
                s.close()
            except Exception:
                pass
    if _lib is not None:
        try:
            _lib.p3d_shutdown()
        except Exception:
            pass


def lib():
    """Load libp3dhip.so once.  Raises if it has not been built (python -m sap3d_tensorflow_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P3dError("libp3dhip.so is not built (%s); run `python sap3d_tensorflow_amd/build.py`. "
                           "There is no CPU fallback." % LIB_PATH)
        _one_rocm_runtime_per_process()
        # RTLD_LOCAL (ctypes' default), never RTLD_GLOBAL: with its symbols in the global scope a later `import torch`
        # binds some of torch's C++ runtime symbols to this library's copies and the process dies at interpreter exit
        # (`double free or corruption`), even with a single HIP runtime mapped (tests/test_load_order.py)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _refuse_two_runtimes()
        _lib = l
        import atexit
        atexit.register(_shutdown)
    return _lib


def check(rc):
    if rc != 0:
        raise P3dError(lib().p3d_last_error().decode("utf-8", "replace"))


def fptr(a):
    return a.ctypes.data_as(_fp) if a is not None else None
