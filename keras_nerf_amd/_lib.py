"""ctypes binding of libknerf_hip.so (include/knerf.h).  There is no CPU fallback: a missing library or a missing
gfx950 device is an error, never a silent detour."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KNERF_LIB") or os.path.join(_HERE, "libknerf_hip.so")   # KNERF_LIB: A/B builds (tools/kbench.py)

KNERF_OK, KNERF_ERR_INVALID, KNERF_ERR_HIP, KNERF_ERR_NONFINITE, KNERF_ERR_NODEVICE = 0, -1, -2, -3, -4
COARSE, FINE = 0, 1


class KnerfConfig(C.Structure):
    _fields_ = [("n_coarse", C.c_int32), ("n_fine", C.c_int32), ("pos_emb_xyz", C.c_int32), ("pos_emb_dir", C.c_int32),
                ("n_layers", C.c_int32), ("dense_units", C.c_int32), ("skip_layer", C.c_int32),
                ("white_background", C.c_int32), ("oob_clamp", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("flags", C.c_int32)]


class KnerfOptimizer(C.Structure):
    """struct knerf_optimizer (include/knerf.h): schedule kind and parameters, clip kind and argument, weight decay"""
    _fields_ = [("schedule", C.c_int32), ("staircase", C.c_int32), ("n_values", C.c_int32), ("clip", C.c_int32),
                ("lr", C.c_double), ("decay_steps", C.c_double), ("decay_rate", C.c_double), ("alpha", C.c_double),
                ("clip_arg", C.c_double), ("weight_decay", C.c_double),
                ("boundaries", C.c_int64 * 15), ("values", C.c_double * 16)]


class KnerfObjective(C.Structure):
    """struct knerf_objective (include/knerf.h): loss kind, Huber's delta, the two regularisers' weights and the nets they apply to"""
    _fields_ = [("loss_kind", C.c_int32), ("huber_delta", C.c_float), ("distortion", C.c_float), ("opacity_entropy", C.c_float),
                ("nets", C.c_int32)]


class KnerfRayModel(C.Structure):
    """struct knerf_ray_model (include/knerf.h): NDC rays or pinhole rays, sample spacing, the NDC near plane"""
    _fields_ = [("ndc", C.c_int32), ("spacing", C.c_int32), ("ndc_near", C.c_float)]


class KnerfCameraModel(C.Structure):
    """struct knerf_camera_model (include/knerf.h): the camera model of a launch and the offset added to integer pixel coordinates"""
    _fields_ = [("model", C.c_int32), ("pixel_offset", C.c_float)]


class KnerfBakedField(C.Structure):
    """struct knerf_baked_field (include/knerf.h): device records and occupancy bits, lattice resolution, SH degree, the box"""
    _fields_ = [("records", C.c_void_p), ("bits", C.c_void_p), ("resolution", C.c_int32 * 3), ("sh_degree", C.c_int32),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class KnerfBakedTrain(C.Structure):
    """struct knerf_baked_train (include/knerf.h): the field (bits = the support), the slot table, the gradient rows, their count"""
    _fields_ = [("field", KnerfBakedField), ("slot_of", C.c_void_p), ("grad", C.c_void_p), ("n_slots", C.c_uint64)]


class KnerfBakedBricks(C.Structure):
    """struct knerf_baked_bricks (include/knerf.h): device brick records, brick table and occupancy bits, the lattice, log2 of the brick
    edge, the number of stored bricks"""
    _fields_ = [("records", C.c_void_p), ("brick_of", C.c_void_p), ("bits", C.c_void_p), ("resolution", C.c_int32 * 3),
                ("sh_degree", C.c_int32), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("brick_log2", C.c_int32),
                ("n_bricks", C.c_uint64)]


class KnerfBakedQBricks(C.Structure):
    """struct knerf_baked_qbricks (include/knerf.h): a brick set whose records are the quantised ones, and the exponent word per brick"""
    _fields_ = [("bricks", KnerfBakedBricks), ("exponents", C.c_void_p)]


class KnerfBakedQuerySpec(C.Structure):
    """struct knerf_baked_query_spec (include/knerf.h): the points (a device list, or a grid given on the host), the directions, the lane
    choice and the three outputs"""
    _fields_ = [("points", C.c_void_p), ("n", C.c_uint64), ("grid_resolution", C.POINTER(C.c_int32)), ("grid_lo", C.POINTER(C.c_float)),
                ("grid_hi", C.POINTER(C.c_float)), ("directions", C.c_void_p), ("per_point", C.c_int32), ("flags", C.c_int32),
                ("sigma", C.c_void_p), ("rgb", C.c_void_p), ("gradient", C.c_void_p)]


class KnerfBakedBricksTrain(C.Structure):
    """struct knerf_baked_bricks_train (include/knerf.h): the optimiser's brick field (bits = the support) and the gradient rows, one
    per stored record"""
    _fields_ = [("field", KnerfBakedBricks), ("grad", C.c_void_p)]


class KnerfBakedRgba(C.Structure):
    """struct knerf_baked_rgba (include/knerf.h): device backgrounds [n,3] and alphas [n] (either may be NULL), what the target's rgb is
    stored over (0 or 1), the opacity loss's weight"""
    _fields_ = [("background", C.c_void_p), ("alpha", C.c_void_p), ("stored_background", C.c_float), ("opacity", C.c_float)]


class KnerfBakedDepth(C.Structure):
    """struct knerf_baked_depth (include/knerf.h): device depth targets [n] in ray-parameter units, weights [n] (may be NULL: every ray
    1), the depth loss's weight"""
    _fields_ = [("target", C.c_void_p), ("weight", C.c_void_p), ("depth", C.c_float)]


BAKED_WHITE_BACKGROUND, BAKED_SKIP_EMPTY, BAKED_LANES_SHIFT = 1, 2, 8
SPACING_LINEAR, SPACING_DISPARITY = 0, 1
SPACINGS = {"linear": SPACING_LINEAR, "disparity": SPACING_DISPARITY}
CAMERA_PINHOLE, CAMERA_OPENCV, CAMERA_FISHEYE = 0, 1, 2
CAMERA_MODELS = {"pinhole": CAMERA_PINHOLE, "opencv": CAMERA_OPENCV, "fisheye": CAMERA_FISHEYE}
CAMERA_ROW = 12             # floats per intrinsics row: fx, fy, cx, cy, six coefficients, two zeros
LOSS_MSE, LOSS_MAE, LOSS_HUBER, LOSS_LOG_COSH = 0, 1, 2, 3
SCHEDULE_CONSTANT, SCHEDULE_EXPONENTIAL, SCHEDULE_COSINE, SCHEDULE_PIECEWISE = 0, 1, 2, 3
CLIP_NONE, CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = 0, 1, 2, 4
SCHEDULE_MAX_VALUES = 16

FLAG_FORCE_GENERIC = 1
FLAG_ENCODED_WIDTHS = 2      # pos_emb_xyz / pos_emb_dir hold the two encoded input widths of a stand-alone NeRFMLP (include/knerf.h)


_P = C.c_void_p
_F = C.c_void_p  # device float* passed as integers (tensor.data_ptr())
# name -> (restype, argtypes): exactly the declarations of include/knerf.h
SIGNATURES = {
    "knerf_param_count": (C.c_size_t, []),
    "knerf_param_count_for": (C.c_size_t, [_P]),
    "knerf_create": (C.c_int, [C.POINTER(KnerfConfig), C.POINTER(_P)]),
    "knerf_destroy": (C.c_int, [_P]),
    "knerf_last_error": (C.c_char_p, [_P]),
    "knerf_set_weights": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_size_t]),
    "knerf_get_weights": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_size_t]),
    "knerf_weights_device": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "knerf_grads_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "knerf_refresh_weights": (C.c_int, [_P, _P]),
    "knerf_forward_chunk": (C.c_int, [_P, _P, C.c_int, _F, _F, _F, C.c_int, C.c_int, _F, _F, _F]),
    "knerf_sample_fine": (C.c_int, [_P, _P, _F, _F, _F, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _F]),
    "knerf_render_chunk": (C.c_int, [_P, _P, _F, _F, _F, _F, C.c_uint64, C.c_uint64, C.c_int, _F, _F, _F, _F, _F, _F, _F]),
    "knerf_train_chunk": (C.c_int, [_P, _P, _F, _F, _F, _F, _F, C.c_uint64, C.c_uint64, C.c_int, C.c_float, _F, _F, _F]),
    "knerf_train_batch": (C.c_int, [_P, _P, _F, _F, _F, _F, _F, C.c_uint64, C.c_int, C.c_int, _F, _F, _F]),
    "knerf_apply_adam": (C.c_int, [_P, _P]),
    "knerf_poll_nonfinite": (C.c_int, [_P, _P, C.c_int]),
    "knerf_zero_grads": (C.c_int, [_P, _P]),
    "knerf_set_option": (C.c_int, [_P, C.c_char_p, C.c_double]),
    "knerf_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "knerf_tile_stats": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "knerf_tile_stats_net": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "knerf_grad_diagnostics": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int64)]),
    "knerf_render_batch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "knerf_ray_points": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "knerf_image_metrics": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "knerf_metrics_update": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "knerf_mlp_call": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_uint64, _P]),
    "knerf_step_count": (C.c_int, [_P]),
    "knerf_set_step_count": (C.c_int, [_P, C.c_int]),
    "knerf_set_optimizer": (C.c_int, [_P, _P, C.POINTER(KnerfOptimizer)]),
    "knerf_get_optimizer": (C.c_int, [_P, C.POINTER(KnerfOptimizer)]),
    "knerf_set_objective": (C.c_int, [_P, _P, C.POINTER(KnerfObjective)]),
    "knerf_get_objective": (C.c_int, [_P, C.POINTER(KnerfObjective)]),
    "knerf_objective_terms": (C.c_int, [_P, _P, _F]),
    "knerf_get_adam_state": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]),
    "knerf_set_adam_state": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]),
    "knerf_generate_rays": (C.c_int, [_P, _P, _F, _F, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_float, C.c_float, C.c_float, _F, _F, _F]),
    "knerf_draw_ray_batch": (C.c_int, [_P, _P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int,
                                       C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _F, C.c_uint64, _F, _F, _F, _F, _P]),
    "knerf_generate_rays_ext": (C.c_int, [_P, _P, _F, _F, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_float, C.c_float, C.c_float, _F, _F, _F, C.POINTER(KnerfRayModel)]),
    "knerf_draw_ray_batch_ext": (C.c_int, [_P, _P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int,
                                           C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _F, C.c_uint64, _F, _F, _F, _F, _P,
                                           C.POINTER(KnerfRayModel)]),
    "knerf_generate_rays_cam": (C.c_int, [_P, _P, _F, _F, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _F, C.c_int, C.POINTER(KnerfCameraModel), C.c_float, C.c_float, _F, _F, _F,
                                          C.POINTER(KnerfRayModel)]),
    "knerf_draw_ray_batch_cam": (C.c_int, [_P, _P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int,
                                           C.POINTER(KnerfCameraModel), C.c_float, C.c_float, C.c_int,
                                           C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _F, C.c_uint64, _F, _F, _F, _F, _P,
                                           C.POINTER(KnerfRayModel)]),
    "knerf_project_points": (C.c_int, [_P, _F, _P, _F, _F, C.c_int, C.POINTER(KnerfCameraModel), C.c_uint64, _F, _F, _P]),
    "knerf_positional_encoding": (C.c_int, [_P, _F, C.c_longlong, C.c_int, _F]),
    "knerf_composite": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, _F, _F, _F]),
    "knerf_inverse_cdf": (C.c_int, [_P, _F, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    "knerf_profile_enable": (C.c_int, [_P, C.c_int]),
    "knerf_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "knerf_query_points": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_uint64, _P, _P, _P]),
    "knerf_query_grid": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _P, _P]),
    "knerf_marching_cubes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _P,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_int64), _P, _P, _P]),
    "knerf_set_occupancy": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "knerf_occupancy_from_grid": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "knerf_occupancy_stats": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "knerf_occupancy_train_stats": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "knerf_occupancy_decay_max": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_float]),
    "knerf_termination_stats": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "knerf_baked_project": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_uint64, _F, _F]),
    "knerf_baked_pack": (C.c_int, [_P, _F, _F, _F, _P, C.c_uint64, C.c_uint64, C.c_int, _P]),
    "knerf_baked_render": (C.c_int, [_P, C.POINTER(KnerfBakedField), _F, _F, _F, _F, C.c_float, C.c_float, C.c_uint64, C.c_float,
                                     C.c_float, C.c_int, _F, _F, _F, _P]),
    "knerf_baked_train_rays": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64, C.c_uint64,
                                         C.c_float, C.c_float, C.c_int, _F]),
    "knerf_baked_train_rays_ext": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                             C.c_uint64, C.c_float, C.c_float, C.c_int, _F, C.POINTER(KnerfObjective), _F]),
    "knerf_baked_train_rays_rgba": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                              C.c_uint64, C.c_float, C.c_float, C.c_int, _F, C.POINTER(KnerfObjective), _F,
                                              C.POINTER(KnerfBakedRgba)]),
    "knerf_baked_train_rays_depth": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                               C.c_uint64, C.c_float, C.c_float, C.c_int, _F, C.POINTER(KnerfObjective), _F,
                                               C.POINTER(KnerfBakedRgba), C.POINTER(KnerfBakedDepth)]),
    "knerf_baked_train_apply": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _P, _P, _F, _F, _F, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float]),
    "knerf_baked_train_tv": (C.c_int, [_P, C.POINTER(KnerfBakedTrain), _P, _F, C.c_float, C.c_float, C.c_float, _F]),
    "knerf_baked_resample": (C.c_int, [_P, C.POINTER(KnerfBakedField), C.POINTER(C.c_int32), C.c_float, _P]),
    "knerf_baked_render_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), _F, _F, _F, _F, C.c_float, C.c_float, C.c_uint64, C.c_float,
                                            C.c_float, C.c_int, _F, _F, _F, _P]),
    "knerf_baked_bricks_train_rays": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                                C.c_uint64, C.c_float, C.c_float, C.c_int, _F]),
    "knerf_baked_bricks_train_rays_ext": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F,
                                                    C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_int, _F,
                                                    C.POINTER(KnerfObjective), _F]),
    "knerf_baked_bricks_train_rays_rgba": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F,
                                                     C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_int, _F,
                                                     C.POINTER(KnerfObjective), _F, C.POINTER(KnerfBakedRgba)]),
    "knerf_baked_bricks_train_rays_depth": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _F, _F, _F, _F, C.c_float, C.c_float, _F,
                                                      C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_int, _F,
                                                      C.POINTER(KnerfObjective), _F, C.POINTER(KnerfBakedRgba),
                                                      C.POINTER(KnerfBakedDepth)]),
    "knerf_baked_bricks_train_apply": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _P, _F, _F, _F, C.c_float, C.c_float, C.c_float,
                                                 C.c_float, C.c_float]),
    "knerf_baked_resample_bricks_sigma": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), C.POINTER(C.c_int32), C.c_float, _F]),
    "knerf_baked_resample_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), C.POINTER(KnerfBakedBricks), _P, C.c_float, _P]),
    "knerf_baked_bricks_train_tv": (C.c_int, [_P, C.POINTER(KnerfBakedBricksTrain), _P, _P, _F, C.c_float, C.c_float, C.c_float, _F]),
    "knerf_baked_ray_gradients": (C.c_int, [_P, C.POINTER(KnerfBakedField), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                            C.c_uint64, C.c_float, C.c_float, C.c_int, _F, _F, _F]),
    "knerf_baked_ray_gradients_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), _F, _F, _F, _F, C.c_float, C.c_float, _F, C.c_uint64,
                                                   C.c_uint64, C.c_float, C.c_float, C.c_int, _F, _F, _F]),
    "knerf_pose_gradients": (C.c_int, [_P, _F, _F, _F, _P, C.c_uint64, C.c_uint64, _P]),
    "knerf_baked_quantize_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), _P, _P]),
    "knerf_baked_dequantize_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedQBricks), _P]),
    "knerf_baked_render_qbricks": (C.c_int, [_P, C.POINTER(KnerfBakedQBricks), _F, _F, _F, _F, C.c_float, C.c_float, C.c_uint64, C.c_float,
                                             C.c_float, C.c_int, _F, _F, _F, _P]),
    "knerf_baked_query": (C.c_int, [_P, C.POINTER(KnerfBakedField), C.POINTER(KnerfBakedQuerySpec)]),
    "knerf_baked_query_bricks": (C.c_int, [_P, C.POINTER(KnerfBakedBricks), C.POINTER(KnerfBakedQuerySpec)]),
    "knerf_baked_query_qbricks": (C.c_int, [_P, C.POINTER(KnerfBakedQBricks), C.POINTER(KnerfBakedQuerySpec)]),
}

_lib = None


class KnerfError(RuntimeError):
    pass


_by_path = {}


def load_path(path: str) -> C.CDLL:
    """A library of this ABI by path (bound once per path): the product library, or a build with further fused shapes
    (build.py --add-shape / KNERF_AUTO_BUILD in runtime.py).  Raises (never falls back) when the file is missing."""
    path = os.path.abspath(path)
    lib = _by_path.get(path)
    if lib is None:
        if not os.path.exists(path):
            raise KnerfError(f"{path} is missing: run `python keras_nerf_amd/build.py` (hipcc, gfx950). "
                             "keras_nerf_amd has no CPU path.")
        # torch first: its bundled HIP runtime must be the one already mapped when libknerf_hip.so resolves
        # libamdhip64, otherwise two runtimes coexist and the second one sees no device / foreign pointers
        import torch  # noqa: F401
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _by_path[path] = lib
    return lib


def build_info(path: str = None) -> dict:
    """What is inside the library at `path` (default: the one load() binds): {"lib_path", "lib_sha16", "kernel_digest",
    "git_head_at_build"}.  kernel_digest (build.py: the source of the three big kernels + flags) comes from the record build.py
    writes beside the library and is None when that record is missing or describes ANOTHER file (its lib_sha16 differs from the
    file's): a digest is only as good as its tie to the binary."""
    import json
    from .build import file_sha16
    path = os.path.abspath(path or LIB_PATH)
    out = {"lib_path": os.path.relpath(path, os.path.dirname(_HERE)), "lib_sha16": file_sha16(path) if os.path.exists(path) else None,
           "kernel_digest": None, "git_head_at_build": None}
    try:
        info = json.load(open(path + ".info.json"))
    except (OSError, ValueError):
        return out
    if info.get("lib_sha16") == out["lib_sha16"]:
        out["kernel_digest"] = info.get("kernel_digest"); out["git_head_at_build"] = info.get("git_head_at_build")
    return out


def load() -> C.CDLL:
    """Load the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if os.environ.get("KNERF_LIB"):          # an A/B build takes the product library's place: never silently
            import logging
            logging.warning("KNERF_LIB is set: keras_nerf_amd runs on %s instead of the product library %s", LIB_PATH,
                            os.path.join(_HERE, "libknerf_hip.so"))
        _lib = load_path(LIB_PATH)
    return _lib
