"""ctypes binding of the C ABI in include/stainlib_hip.h.

The HIP library is the product: if ``libstainlib_hip.so`` is missing or a call fails this
module raises -- there is no CPU fallback anywhere in ``stainlib_amd``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# STAINLIB_HIP_LIB: development override (tools/ load the -DSL_DEVTOOLS build, libstainlib_hip_dev.so, through it)
LIB_PATH = os.environ.get("STAINLIB_HIP_LIB") or os.path.join(_HERE, "csrc", "libstainlib_hip.so")


class SlProfile(C.Structure):
    _fields_ = [
        ("events", C.POINTER(C.c_void_p)),
        ("tags", C.POINTER(C.c_int32)),
        ("tiles", C.POINTER(C.c_int32)),
        ("capacity", C.c_int32),
        ("used", C.c_int32),
        ("mask", C.c_int32),
        ("reserved", C.c_int32),
    ]


PROF_MOMENTS, PROF_SELECT_ANGLE, PROF_SELECT_CONC, PROF_FINISH, PROF_APPLY, PROF_DICT = 1, 2, 4, 8, 16, 32
PROF_FUSED_FIT, PROF_FUSED_TRANSFORM = 64, 128
PROF_NAMES = {1: "k_moments", 2: "k_select<merged>", 4: "k_select<conc>", 8: "k_finish_*", 16: "k_apply", 32: "k_dict",
              64: "k_macenko_fused<fit>", 128: "k_macenko_fused<transform>"}


class SlParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("luminosity_threshold", C.c_double),
        ("angular_percentile", C.c_double),
        ("lasso_lambda", C.c_double),
        ("dl_lambda", C.c_double),
        ("dl_max_sweeps", C.c_int32),
        ("schedule", C.c_int32),
        ("dl_tol", C.c_double),
        ("profile", C.POINTER(SlProfile)),
        ("fallbacks_out", C.c_void_p),
        ("resweeps_out", C.c_void_p),
        ("fused_min_tiles", C.c_int32),
        ("prefilter", C.c_int32),
        ("prefilter_out", C.c_void_p),
        ("two_sweep", C.c_int32),
        ("reserved1", C.c_int32),
        ("twosweep_out", C.c_void_p),
    ]


class SlTensorFormat(C.Structure):
    """The model-ready output of sl_to_tensor / sl_normalize_apply_tensor (a HOST struct, like SlParams)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32),
        ("layout", C.c_int32),
        ("reserved", C.c_int32),
        ("mean", C.c_double * 3),
        ("std", C.c_double * 3),
    ]


class SlSeparateOut(C.Structure):
    """The outputs of sl_stain_separate (a HOST struct; the pointers in it are DEVICE pointers, NULL = not wanted)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("conc_dtype", C.c_int32),
        ("norm", C.c_void_p),
        ("stain", C.c_void_p * 2),
        ("conc", C.c_void_p),
    ]


class SlViewStages(C.Structure):
    """The stages of the one-pass recipe (sl_normalize_stages_view*; a HOST struct, the pointers in it are DEVICE pointers, NULL = absent)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("hed_sigma", C.c_void_p),
        ("hed_bias", C.c_void_p),
        ("hed_applied", C.c_void_p),
        ("skimage_mode", C.c_int),
        ("hsb_codes", C.c_void_p),
        ("tone_tables", C.c_void_p),
        ("noise_codes", C.c_void_p),
    ]


DTYPE_F32, DTYPE_F16, DTYPE_BF16 = range(3)
LAYOUT_NCHW, LAYOUT_NHWC = range(2)


class StainlibHipError(RuntimeError):
    pass


# ops (sl_workspace_bytes)
(OP_MACENKO_FIT, OP_MACENKO_TRANSFORM, OP_VAHADANE_FIT, OP_VAHADANE_TRANSFORM, OP_HED_AUGMENT, OP_STAIN_AUGMENT, OP_TILE_MOMENTS,
 OP_LAB_STATS) = range(1, 9)
# skimage semantics of sl_hed_augment (only 0.18 is golden-pinned)
HED_SKIMAGE_018, HED_SKIMAGE_019, HED_SKIMAGE_017, HED_EXPERIMENTAL_LOG10 = range(4)
# selection key sets of the pooled slide-level mode (two targets each)
KEYSET_ANGLE, KEYSET_CONC = range(2)
# per-tile status
TILE_OK, TILE_EMPTY_MASK, TILE_DEGENERATE_COV, TILE_ZERO_MAXC = range(4)

_P = C.c_void_p
_SIGNATURES = {
    "sl_version": (C.c_int, []),
    "sl_error_string": (C.c_char_p, [C.c_int]),
    "sl_default_params": (None, [C.POINTER(SlParams)]),
    "sl_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sl_workspace_bytes_for": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams)]),
    "sl_macenko_fit": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), _P, _P, _P, _P, C.c_size_t, _P]),
    "sl_vahadane_fit": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "sl_normalize_apply": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P]),
    "sl_macenko_transform": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "sl_vahadane_transform": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "sl_hed_augment": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_double, C.c_double, C.c_int, _P, _P, C.c_size_t, _P]),
    "sl_hed_augment_f64": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_double, C.c_double, C.c_int, _P, _P, C.c_size_t, _P]),
    "sl_rgb_to_od": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "sl_stain_augment": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(SlParams), _P]),
    "sl_tissue_mask": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    "sl_concentrations": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_double, _P, _P]),
    "sl_grayscale_augment": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "sl_od_to_rgb": (C.c_int, [_P, C.c_size_t, _P, _P, _P]),
    "sl_rgb_to_lab8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "sl_lab8_to_rgb": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "sl_lab_split": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "sl_lab_merge": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "sl_standardize_brightness": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "sl_reinhard_stats": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "sl_reinhard_transform": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_double, _P, _P, C.c_size_t, _P]),
    "sl_luminosity_standardize": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, C.c_size_t, _P]),
    "sl_tile_moments": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), _P, _P, C.c_size_t, _P]),
    "sl_slide_key_histogram": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_uint32), C.c_int, _P, _P]),
    "sl_slide_key_next_above": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, C.POINTER(C.c_double),
                                           C.POINTER(C.c_uint32), _P, _P]),
    "sl_slide_key_histogram16": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, C.POINTER(C.c_double),
                                            C.POINTER(C.c_uint32), _P, _P]),
    "sl_slide_key_histogram_sampled": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_uint32), C.c_int, C.c_int, _P, _P]),
    "sl_slide_key_window": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, C.POINTER(C.c_double),
                                       C.POINTER(C.c_uint32), _P, _P]),
    # device-driven pooled statistics (state: SL_POOL_STATE_DOUBLES doubles on the device)
    "sl_pool_begin": (C.c_int, [_P, C.POINTER(SlParams), _P, _P]),
    "sl_pool_histogram": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "sl_pool_pick": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "sl_pool_window": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, _P, _P]),
    "sl_pool_resolve": (C.c_int, [_P, C.c_int, _P, C.POINTER(SlParams), _P]),
    # the pooled statistics in one full sweep (state: SL_POOL2_STATE_DOUBLES doubles; workspace: sl_pool2_workspace_bytes)
    "sl_pool2_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sl_pool2_sample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, C.c_size_t, _P, _P]),
    "sl_pool2_begin": (C.c_int, [_P, C.POINTER(SlParams), C.c_int, _P, _P]),
    "sl_pool2_hist": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, _P, C.c_size_t, _P, _P]),
    "sl_pool2_bands": (C.c_int, [_P, C.c_int, _P, _P]),
    "sl_pool2_sweep": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, _P, C.c_size_t, _P, _P]),
    "sl_pool2_exact": (C.c_int, [_P, _P, _P]),
    "sl_pool2_step": (C.c_int, [_P, C.c_int, _P, _P]),
    "sl_pool2_local": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, C.c_size_t, _P, _P]),
    # the pooled slide-level Vahadane dictionary (state: SDICT_STATE_DOUBLES doubles; workspace: sl_sdict_workspace_bytes)
    "sl_sdict_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sl_sdict_begin": (C.c_int, [C.POINTER(SlParams), C.c_int, _P, _P]),
    "sl_sdict_sweep": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(SlParams), C.c_int, _P, _P, C.c_size_t, _P, _P]),
    "sl_sdict_step": (C.c_int, [_P, _P, C.POINTER(SlParams), _P]),
    # the pooled slide-level Reinhard / luminosity statistics (state: SLAB_STATE_DOUBLES doubles; workspace: sl_slab_workspace_bytes)
    "sl_slab_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sl_slab_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P]),
    "sl_slab_begin": (C.c_int, [_P, _P, C.c_int, _P]),
    "sl_slab_lab": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_double, _P, C.c_size_t, _P, _P]),
    "sl_slab_finish": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_double, C.c_int, _P]),
    "sl_slab_map": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, _P]),
    # model-ready tensor output (SlTensorFormat: a host struct)
    "sl_default_tensor_format": (None, [C.POINTER(SlTensorFormat)]),
    "sl_to_tensor": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(SlTensorFormat), _P]),
    "sl_normalize_apply_tensor": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, C.POINTER(SlTensorFormat), _P]),
    # stain separation (SlSeparateOut: a host struct of device pointers)
    "sl_default_separate_out": (None, [C.POINTER(SlSeparateOut)]),
    "sl_stain_separate": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, C.POINTER(SlSeparateOut), _P]),
    # stain jitter in the apply pass (SlParams and SlTensorFormat: host structs, either may be NULL)
    "sl_normalize_jitter": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.POINTER(SlParams),
                                      C.POINTER(SlTensorFormat), _P]),
    # crop / flip / rot90 in the apply pass (windows: n x 3 int32 on the device; M_src, alpha_beta, SlParams, SlTensorFormat may be NULL)
    "sl_normalize_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int,
                                    C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P]),
    # HED augmentation behind the apply pass: the byte sums of the image a route would write (sums: n uint64, applied: n int32 or NULL, both
    # on the device), and the view pass with the HED stage (sl_normalize_view's parameters, then sigma, bias, applied, skimage_mode)
    "sl_normalize_sums": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.POINTER(SlParams), C.c_double, C.c_double,
                                    _P, _P, _P]),
    "sl_normalize_hed_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int,
                                        C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P, _P, _P, C.c_int, _P]),
    # the Lab family behind the view (rgb, out, n, h, w, oh, ow, windows, d_mask, <the existing call's arguments>, fmt, stream)
    "sl_reinhard_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_double, _P, _P,
                                   C.c_size_t, C.POINTER(SlTensorFormat), _P]),
    "sl_luminosity_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_double, _P, _P, C.c_size_t,
                                     C.POINTER(SlTensorFormat), _P]),
    "sl_slab_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_double,
                               C.POINTER(SlTensorFormat), _P]),
}
# the 2x / 4x box shrink of the view passes: each parent's parameters with `int shrink` behind d_mask (the ninth)
for _name in ("sl_normalize_view", "sl_normalize_hed_view", "sl_reinhard_view", "sl_luminosity_view", "sl_slab_view"):
    _res, _args = _SIGNATURES[_name]
    _SIGNATURES[_name + "_shrink"] = (_res, _args[:9] + [C.c_int] + _args[9:])
# the resizing views (windows: n x 5 int32): each parent's parameters with `int max_wh, int max_ww` behind d_mask
for _name in ("sl_normalize_view", "sl_normalize_hed_view"):
    _res, _args = _SIGNATURES[_name]
    _SIGNATURES[_name + "_resize"] = (_res, _args[:9] + [C.c_int, C.c_int] + _args[9:])
del _name, _res, _args
# stain separation in the view pass (rgb, n, h, w, oh, ow, windows, d_mask, shrink, <sl_stain_separate's statistics, lambda and outs>, fmt, stream)
_SIGNATURES["sl_stain_separate_view"] = (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P,
                                                   C.c_double, C.POINTER(SlSeparateOut), C.POINTER(SlTensorFormat), _P])
# companion planes through the windows of a view (planes, out, n, c, h, w, elem_bytes, oh, ow, windows, d_mask, shrink, max_wh, max_ww, mode, stream)
_SIGNATURES["sl_view_planes"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, _P])
# the affine views (windows: n x 6 int32 on the device): rgb, out, n, h, w, oh, ow, windows, max_r, fill_rgb, <sl_normalize_view's statistics,
# params, fmt>, stream -- and planes, out, n, c, h, w, elem_bytes, oh, ow, windows, max_r, fill_bits, stream
_SIGNATURES["sl_normalize_view_affine"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_uint32, _P, _P, _P, _P,
                                                     _P, C.c_int, C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P])
_SIGNATURES["sl_view_planes_affine"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_uint64,
                                                  _P])
# the elastic views (field: n x gh x gw x 2 int32 on the device): the affine views' parameters with `const int32_t* field, int cell_log2,
# int max_d` behind max_r
for _name in ("sl_normalize_view", "sl_view_planes"):
    _res, _args = _SIGNATURES[_name + "_affine"]
    _i = 9 if _name == "sl_normalize_view" else 11
    _SIGNATURES[_name + "_elastic"] = (_res, _args[:_i] + [_P, C.c_int, C.c_int] + _args[_i:])
del _name, _res, _args, _i
# hue / saturation / brightness augmentation (codes: n x 3 int32 on the device): rgb, out, n, h, w, codes, fmt, stream -- and the view pass
# with the HSB stage: rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, max_wh, max_ww, <sl_normalize_view's statistics, params, fmt>, codes, stream
_SIGNATURES["sl_hsb_augment"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(SlTensorFormat), _P])
_SIGNATURES["sl_normalize_hsb_view"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                                  _P, _P, _P, C.c_int, C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P, _P])
# the blurred view (codes: n x 9 int32 on the device): rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, max_r, <sl_normalize_view's statistics,
# params, fmt>, codes, stream
_SIGNATURES["sl_normalize_blur_view"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P,
                                                   _P, _P, C.c_int, C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P, _P])
# the post stage (tables: n x 256 bytes, codes: n x 4 int32, on the device; each may be null, not both): rgb, out, n, h, w, tables, codes, fmt,
# stream -- and the view pass with the stage on its write side: sl_normalize_hsb_view's arguments with tables, codes in place of its codes
_SIGNATURES["sl_post_augment"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(SlTensorFormat), _P])
_SIGNATURES["sl_normalize_post_view"] = (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                                   _P, _P, _P, C.c_int, C.POINTER(SlParams), C.POINTER(SlTensorFormat), _P, _P, _P])
# the one-pass recipe: the parent's arguments (sl_normalize_post_view's without tables, codes; sl_normalize_view_affine's; _view_elastic's) with
# `const SlViewStages* stages` in front of the stream
_SIGNATURES["sl_normalize_stages_view"] = (C.c_int, _SIGNATURES["sl_normalize_post_view"][1][:-3] + [C.POINTER(SlViewStages), _P])
for _name in ("affine", "elastic"):
    _SIGNATURES["sl_normalize_stages_view_" + _name] = (C.c_int, _SIGNATURES["sl_normalize_view_" + _name][1][:-1] + [C.POINTER(SlViewStages), _P])
del _name
PLANES_NEAREST, PLANES_AREA = range(2)
POOL_STATE_DOUBLES, POOL_M, POOL_MAXC, POOL_STATUS, POOL_MISS = 64, 0, 6, 8, 9
POOL2_STATE_DOUBLES, POOL2_HIST_WORDS, POOL2_WHY = 256, 2 * 8192 + 8 * 32, 33
SDICT_STATE_DOUBLES, SDICT_SUMS, SDICT_M, SDICT_STATUS, SDICT_SWEEPS, SDICT_ROUNDS, SDICT_MODE, SDICT_D, SDICT_NPX = 64, 32, 0, 6, 7, 8, 9, 10, 16
SLAB_STATE_DOUBLES, SLAB_SUMS_A, SLAB_SUMS_B, SLAB_TABLES = 512, 256, 262, 32
SLAB_P90, SLAB_MEANS, SLAB_STDS, SLAB_LPCT, SLAB_TISSUE, SLAB_NPX, SLAB_STATUS = 0, 1, 4, 7, 8, 9, 10
EXPECTED_VERSION = 600     # the SL_VERSION this binding (SlParams, signatures) was written for
EXPORTS = tuple(_SIGNATURES)

_lib = None


def lib() -> C.CDLL:
    """Load libstainlib_hip.so (once).  torch is imported first so that the library binds to
    the same HIP runtime (libamdhip64.so.7) torch already has in the process."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StainlibHipError(
                f"{LIB_PATH} not found: build it with `make -C stainlib_amd/csrc` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        import torch  # noqa: F401  (loads the HIP runtime)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(h, name)   # AttributeError here == a symbol the header declares is missing
            fn.restype = res
            fn.argtypes = args
        if h.sl_version() != EXPECTED_VERSION:      # a stale .so would read SlParams at other offsets (round-5 advisor finding)
            raise StainlibHipError(f"{LIB_PATH} is ABI {h.sl_version()}, this package binds ABI {EXPECTED_VERSION}: rebuild it "
                                   "(make -C stainlib_amd/csrc)")
        _lib = h
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        raise StainlibHipError(f"{what} failed: {lib().sl_error_string(code).decode()} (code {code})")


def default_tensor_format() -> SlTensorFormat:
    f = SlTensorFormat()
    lib().sl_default_tensor_format(C.byref(f))
    return f


def default_separate_out() -> SlSeparateOut:
    o = SlSeparateOut()
    lib().sl_default_separate_out(C.byref(o))
    return o


def default_params() -> SlParams:
    p = SlParams()
    lib().sl_default_params(C.byref(p))
    return p
