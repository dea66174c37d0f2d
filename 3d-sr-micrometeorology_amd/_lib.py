"""ctypes binding of libsr3d.so (the C ABI declared in include/sr3d.h).

There is NO fallback: if the shared library is missing or a symbol cannot be
resolved the import of the engine fails, and every wrapper raises
``RuntimeError`` with ``sr3d_last_error()`` when a call returns non-zero.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SR3D_LIBRARY: developer hook for A/B timing of two builds of the library (tools/layer_bench.py); never a fallback
LIB_PATH = os.environ.get("SR3D_LIBRARY") or os.path.join(_HERE, "libsr3d.so")

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
ACT_UNSHUFFLE = 0x400  # flag OR-ed to `act` of sr3d_conv3d_bwd_data_act: the fused slice is an unshuffle layer's output
ACT_FROM_Y = 0x200    # flag OR-ed to `act` of sr3d_gated_act_bwd: its second operand is the layer output y
ACT_OUT_F32 = 0x100   # flag OR-ed to `act` of sr3d_conv3d_fwd (include/sr3d.h): fp32 output of a bf16-storage layer
DTYPE_F32, DTYPE_BF16 = 0, 1
DTYPE_CODE = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16}
PACK_FWD, PACK_FWD_GATED, PACK_BWD, PACK_BWD_GATED, PACK_FWD_UNSHUFFLE = 0, 1, 2, 3, 4
ACT_CODE = {None: ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU}
# indices into the output of sr3d_eval_metrics (include/sr3d.h: SR3D_EVAL_*)
EVAL_INDEX = {"L1": 0, "L2": 1, "MaskedL1": 2, "MaskedL2": 3, "MaskedL1NearWall": 4, "MaskedL2NearWall": 5,
              "ResidualContinuity": 6, "ResidualContinuityTarget": 7, "AbsDiffTemperature": 8, "DiffVelocityNorm": 9,
              "AbsDiffTemperatureLev": 10, "DiffVelocityNormLev": 11, "AbsDiffDivergence": 12, "DiffOmegaNorm": 13}
EVAL_SUMS = {"abs": 14, "mask_abs": 15, "sq": 16, "mask_sq": 17, "mask": 18}
EVAL_COUNT = 19
# rows of the outputs of sr3d_eval_level_profiles (include/sr3d.h: SR3D_PROFILE_*, SR3D_PROFILE_SUM_*)
PROFILE_INDEX = {"L1": 0, "L2": 1, "MaskedL1": 2, "MaskedL2": 3, "MaskedL1NearWall": 4, "MaskedL2NearWall": 5,
                 "ResidualContinuity": 6, "ResidualContinuityTarget": 7, "AbsDiffTemperature": 8,
                 "DiffVelocityNorm": 9, "AbsDiffDivergence": 10, "DiffOmegaNorm": 11, "ChannelwiseMseT": 12,
                 "ChannelwiseMseU": 13, "ChannelwiseMseV": 14, "ChannelwiseMseW": 15}
PROFILE_COUNT = 16
PROFILE_SUM_INDEX = {"abs": 0, "sq": 1, "sq_T": 2, "sq_U": 3, "sq_V": 4, "sq_W": 5, "mask": 6, "mask_abs": 7,
                     "mask_sq": 8, "near": 9, "near_abs": 10, "near_sq": 11, "mask_dT": 12, "mask_dV": 13,
                     "mask_int": 14, "near_int": 15, "res_p": 16, "res_t": 17, "ddiv": 18, "omega": 19}
PROFILE_SUM_COUNT = 20
# rows of the outputs of sr3d_eval_wall_distance_profiles (include/sr3d.h: SR3D_WALLDIST_*, SR3D_WALLDIST_SUM_*): the
# per-level names; the NEAR sums are POS ([b > 0]) here, and the cell count of a bin follows
WALLDIST_INDEX = dict(PROFILE_INDEX)
WALLDIST_COUNT = 16
WALLDIST_SUM_INDEX = {**{{"near": "pos", "near_abs": "pos_abs", "near_sq": "pos_sq"}.get(k, k): v
                         for k, v in PROFILE_SUM_INDEX.items()}, "cells": 20}
WALLDIST_SUM_COUNT = 21
WALLDIST_MAX_D = 30     # SR3D_WALLDIST_MAX_D
WALL_DISTANCE_MAX_CAP = 254
# sr3d_eval_distributions (include/sr3d.h: SR3D_DIST_*): the series (first axis of its outputs), classes and slots
DIST_SERIES_INDEX = {"ERR_T": 0, "ERR_U": 1, "ERR_V": 2, "ERR_W": 3, "ERR_VEL_NORM": 4, "PRED_T": 5, "PRED_U": 6,
                     "PRED_V": 7, "PRED_W": 8, "TRUTH_T": 9, "TRUTH_U": 10, "TRUTH_V": 11, "TRUTH_W": 12}
DIST_SERIES = 13
DIST_CLASSES = 2        # 0: fluid cells within near_width of a wall, 1: the other fluid cells
DIST_BINS = 256
DIST_SLOTS = 259        # underflow, the bins, overflow, NaN
# sr3d_eval_scale_statistics (include/sr3d.h: SR3D_SCALE_*): the series and moments (last two axes of its sums)
SCALE_SERIES_INDEX = {"PRED_T": 0, "PRED_U": 1, "PRED_V": 2, "PRED_W": 3, "TRUTH_T": 4, "TRUTH_U": 5, "TRUTH_V": 6,
                      "TRUTH_W": 7, "ERR_T": 8, "ERR_U": 9, "ERR_V": 10, "ERR_W": 11}
SCALE_MOMENT_INDEX = {"D1": 0, "D2": 1, "D3": 2, "D4": 3, "F0": 4, "F1": 5, "FF0": 6, "FF1": 7}
SCALE_DIRS = ("x", "y", "z")
SCALE_SERIES, SCALE_MOMENTS = 12, 8
SCALE_MAX_LAG = 64      # SR3D_SCALE_MAX_LAG
ROTATE_COEF_READY, ROTATE_PHYSICAL = 1, 2   # flags of the rotation calls (include/sr3d.h: SR3D_ROTATE_*)


class Slice(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("channels", C.c_int32)]


class SurfaceSrc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("C", C.c_int32), ("Zs", C.c_int32), ("channel", C.c_int32),
                ("levels", C.c_int32), ("affine", C.c_int32), ("scale", C.c_float), ("mean", C.c_float)]


class LrDataParams(C.Structure):
    _fields_ = [("raw", C.c_void_p), ("channel_stride", C.c_longlong), ("C", C.c_int32), ("Z", C.c_int32),
                ("Y", C.c_int32), ("X", C.c_int32), ("scale", C.c_int32), ("hr_margin", C.c_int32),
                ("align_nan", C.c_int32), ("hr_mask", C.c_void_p), ("lr_tops", C.c_void_p), ("lat", C.c_void_p),
                ("lon", C.c_void_p), ("lev", C.c_void_p), ("hr_out", C.c_void_p), ("lr_out", C.c_void_p)]


class GradsParams(C.Structure):
    _fields_ = [("X", C.c_int32), ("Y", C.c_int32), ("Z", C.c_int32), ("byteswap", C.c_int32), ("yrev", C.c_int32),
                ("zrev", C.c_int32), ("align_nan", C.c_int32), ("level_offset", C.c_longlong * 4),
                ("level_pitch", C.c_longlong * 4), ("src_bytes", C.c_longlong * 4), ("undef", C.c_double * 4),
                ("out", C.c_void_p), ("tm_is_nan", C.c_void_p)]


class ConvDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("Z", C.c_int32), ("Y", C.c_int32),
                ("X", C.c_int32), ("stride", C.c_int32), ("dtype", C.c_int32)]


# every symbol include/sr3d.h declares: name -> (restype, argtypes)
_P, _I, _LL, _F, _D, _SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double, C.c_size_t
_DESC, _SL = C.POINTER(ConvDesc), C.POINTER(Slice)
SYMBOLS = {
    "sr3d_version": (_I, []),
    "sr3d_last_error": (C.c_char_p, []),
    "sr3d_packed_weight_bytes": (_SZ, [_DESC, _I]),
    "sr3d_pack_weights": (_I, [_DESC, _I, _P, _P, _P, _P]),
    "sr3d_conv3d_fwd": (_I, [_DESC, _SL, _I, _P, _P, _P, _I, _I, _P, _P]),
    "sr3d_conv3d_fwd_exports_absmax": (_I, [_DESC, _I]),
    "sr3d_gated_conv3d_fwd": (_I, [_DESC, _SL, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "sr3d_conv3d_bwd_data_workspace_bytes": (_SZ, [_DESC, _I]),
    "sr3d_conv3d_bwd_data": (_I, [_DESC, _SL, _I, _P, _P, _SL, _I, _P, _SZ, _P]),
    "sr3d_conv3d_bwd_data_fuses_act": (_I, [_DESC, _I, _SL, _I, _I, _I]),
    "sr3d_conv3d_bwd_data_act": (_I, [_DESC, _SL, _I, _P, _P, _SL, _I, _I, _P, _I, _P, _P, _SZ, _P]),
    "sr3d_conv3d_bwd_weight_workspace_bytes": (_SZ, [_DESC, _I]),
    "sr3d_conv3d_bwd_weight": (_I, [_DESC, _SL, _I, _SL, _I, _P, _P, _SZ, _P, _P, _P]),
    "sr3d_bias_grad_workspace_bytes": (_SZ, [_I, _I, _LL]),
    "sr3d_bias_grad": (_I, [_P, _I, _I, _LL, _P, _P, _I, _P]),
    "sr3d_gated_act_bwd": (_I, [_P, _P, _P, _P, _P, _LL, _I, _I, _P, _P]),
    "sr3d_gated_act_bwd_sum": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _P, _P]),
    "sr3d_lrelu_bwd": (_I, [_P, _P, _P, _LL, _I, _P, _P]),
    "sr3d_unshuffle_lrelu_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "sr3d_upsample_cat": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sr3d_avgpool2": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sr3d_near_wall": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sr3d_pconv_mask_update": (_I, [_P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "sr3d_mul_mask": (_I, [_P, _P, _P, _I, _I, _LL, _I, _I, _P]),
    "sr3d_pconv_scale": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _LL, _I, _I, _P]),
    "sr3d_preprocess": (_I, [_P, _P, _I, _I, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _F, _I, _F, _I, _P]),
    "sr3d_loss_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sr3d_l1_fwd_bwd": (_I, [_P, _P, _LL, _P, _P, _P, _P]),
    "sr3d_mixed_div_grad_l2_fwd_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, C.POINTER(_F), _F, _F, _F, _P, _P, _P, _P]),
    "sr3d_mixed_div_grad_l2_bwd": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(_F), _F, _F, _F, _P, _P, _P, _P]),
    "sr3d_weighted_lp_bwd": (_I, [_P, _P, _P, _I, _I, _LL, _I, _P, _P, _P]),
    "sr3d_eval_metrics_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sr3d_eval_metrics": (_I, [_P, _P, _P, _I, _I, _I, _I, C.POINTER(_F), _F, _I, _P, _P, _P]),
    "sr3d_eval_level_profiles_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sr3d_eval_level_profiles": (_I, [_P, _P, _P, _I, _I, _I, _I, C.POINTER(_F), _F, _I, _P, _P, _P, _P]),
    "sr3d_wall_distance_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sr3d_wall_distance": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "sr3d_eval_wall_distance_profiles_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "sr3d_eval_wall_distance_profiles": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(_F), _F, _I, _P, _P, _P, _P]),
    "sr3d_eval_distributions_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sr3d_eval_distributions": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _I, _I,
                                     _P, _P, _P, _P, _P]),
    "sr3d_eval_scale_statistics_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "sr3d_eval_scale_statistics": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sr3d_rotate_workspace_bytes":(_SZ, [_I, _I, _I, _I, _I]),
    "sr3d_rotate_fields": (_I, [_P, _P, _I, _I, _I, _I, _I, C.POINTER(_D), C.POINTER(_D), _D, _I, _P, _SZ, _P]),
    "sr3d_rotate_building": (_I, [_P, _P, _I, _I, _I, _I, _I, _D, _D, _I, _P, _SZ, _P]),
    "sr3d_equivariance_errors": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(_D), C.POINTER(_D), _D, _I, _I, _I, _I, _I, _P,
                                      _P, _SZ, _P]),
    "sr3d_surface_temperature": (_I, [C.POINTER(SurfaceSrc), _I, _I, _I, _P, C.POINTER(_D), _I, _P, _P]),
    "sr3d_surface_temperature_workspace_bytes": (_SZ, [_I, _I, _I]),
    "sr3d_surface_temperature_errors": (_I, [C.POINTER(SurfaceSrc), C.POINTER(SurfaceSrc), _I, _I, _I, _P,
                                             C.POINTER(_D), _I, _P, _P, _P, _P, _SZ, _P]),
    "sr3d_lrdata_workspace_bytes": (_SZ, [_I, _I, _I]),
    "sr3d_lrdata": (_I, [C.POINTER(LrDataParams), _P, _SZ, _P]),
    "sr3d_grads_decode": (_I, [C.POINTER(C.c_void_p), C.POINTER(GradsParams), _P]),
    "sr3d_interp_baseline_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I, _I]),
    "sr3d_interp_baseline": (_I, [_P, _LL, _LL, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "sr3d_ssim3d_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "sr3d_ssim3d": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_F), _I, _F, _F, _P, _P, _P, _P]),
    "sr3d_adam_step": (_I, [_P, _P, _P, _P, _LL, _D, _D, _D, _D, _I, _D, _P]),
    "sr3d_adam_step_device_counter": (_I, [_P, _P, _P, _P, _LL, _D, _D, _D, _D, _P, _P, _D, _P]),
    "sr3d_profile_enable": (_I, [_I]),
    "sr3d_profile_read": (_I, [_I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libsr3d.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C 3d-sr-micrometeorology_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing -> loud failure
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()


PROFILING = False   # per-kernel HIP-event timing is on (bench.py): ops then keeps every launch on ONE stream


def profile_enable(on) -> None:
    """sr3d_profile_enable (0 off, 1 every family, 2 only the stride-1 convolution families) + the flag `ops` reads:
    kernels overlapped on two streams cannot be timed one by one"""
    global PROFILING
    check(lib.sr3d_profile_enable(int(on)), "sr3d_profile_enable")
    PROFILING = bool(on)


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {lib.sr3d_last_error().decode()}")


def stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_ptr(t: torch.Tensor, what: str = "tensor", dtype: torch.dtype = torch.float32) -> C.c_void_p:
    """device pointer of a dense GPU tensor of the expected element type (None -> NULL)"""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU: the sr3d engine has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    return C.c_void_p(t.data_ptr())


def slices(tensors, what="srcs", dtype: torch.dtype = torch.float32):
    """(B,C,Z,Y,X) tensors (or (channels, None) pairs for 'no gradient wanted') -> Slice array"""
    arr = (Slice * len(tensors))()
    for i, t in enumerate(tensors):
        if isinstance(t, tuple):
            arr[i].ptr, arr[i].channels = None, int(t[0])
        else:
            arr[i].ptr, arr[i].channels = dev_ptr(t, f"{what}[{i}]", dtype).value, int(t.shape[1])
    return arr


def conv_desc(B, Cin, Cout, Z, Y, X, stride, dtype: torch.dtype = torch.float32) -> ConvDesc:
    if dtype not in DTYPE_CODE:
        raise TypeError(f"the sr3d engine stores activations as float32 or bfloat16 (got {dtype})")
    return ConvDesc(int(B), int(Cin), int(Cout), int(Z), int(Y), int(X), int(stride), DTYPE_CODE[dtype])


def torch_dtype(desc: ConvDesc) -> torch.dtype:
    return torch.bfloat16 if desc.dtype == DTYPE_BF16 else torch.float32
