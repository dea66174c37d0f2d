"""Rotation-equivariance errors of the trained model (reference src/equivariance_error_calculator.py) on the GPU.

The reference rotates the LR input, the building mask and the prediction about the vertical axis with
scipy.ndimage.rotate (order-3 splines, float64, one 2-D plane at a time on the host), runs the model on the original
and on the rotated input, and reports the window means of |dT|, |dw| and ||(du, dv)|| (keys ``tm``, ``vr``,
``vl_vp``).  Here the rotations are HIP kernels (csrc/sr3d_rotate.hip) and the last rotation is fused with the error
reduction, so the rotated prediction is never materialised.

The public names and keyword signatures are the reference's.  numpy arrays and CPU tensors are accepted and moved to
``device`` (which must be a GPU: there is no CPU path); results come back in the reference's types (numpy arrays,
a dict of numpy float64).  Device tensors stay on the device: nothing goes to the host between the two forwards.
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from .. import ops

KEYS = ("tm", "vr", "vl_vp")


def _device_of(a, device=None) -> torch.device:
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a.device
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"device {dev}: the rotations run on the GPU only (the sr3d engine has no CPU path)")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU available: the sr3d engine has no CPU path")
    return dev


def _on_device(a, dev: torch.device) -> torch.Tensor:
    """numpy array / tensor -> contiguous fp32 tensor on dev"""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _is_host(a) -> bool:
    return not (isinstance(a, torch.Tensor) and a.is_cuda)


def rotate_temperature_velocity(Xs, means: list, scales: list, angle: float, rescaled: bool = True):
    """(B, 4, Z, Y, X) normalised (T, u, v, w) rotated by ``angle`` degrees about z, velocity rotated as a vector,
    re-normalised and clipped to [0, 1] (``rescaled=False``: the physical field).  numpy / CPU input -> float64 numpy
    (the reference's type; the values carry fp32 resolution); device input -> fp32 device tensor."""
    dev = _device_of(Xs)
    y = ops.rotate_fields(_on_device(Xs, dev), means, scales, angle, rescaled=rescaled)
    return y.cpu().numpy().astype(np.float64) if _is_host(Xs) else y


def rotate_building_height(bs, angle: float, th: float = 0.1):
    """building mask rotated by ``angle`` degrees about z and thresholded (``> th``) to {0, 1}.
    numpy / CPU input -> numpy of the input's float dtype; device input -> fp32 device tensor."""
    if bs.ndim != 5:
        raise ValueError("rotate_building_height expects (batch, channel, z, y, x)")
    dev = _device_of(bs)
    y = ops.rotate_building(_on_device(bs, dev), angle, th)
    if not _is_host(bs):
        return y
    dt = bs.dtype if isinstance(bs, np.ndarray) else torch.empty((), dtype=bs.dtype).numpy().dtype
    return y.cpu().numpy().astype(dt if np.issubdtype(dt, np.floating) else np.float32)


def calc_error_ratio(diff, sx: int, ex: int, sy: int, ey: int):
    """mean of |diff|[..., sy:ey, sx:ex] over (batch, z, y, x) (the reference's helper, plain array arithmetic)"""
    assert diff.ndim == 4
    if isinstance(diff, torch.Tensor):
        return diff.abs()[..., sy:ey, sx:ex].double().mean()
    return np.mean(np.abs(diff)[..., sy:ey, sx:ex])


def _forward(model: torch.nn.Module, x: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        y = model(x, b)
    return y if y.dtype == torch.float32 else y.float()


def _preds_pair(Xs, bs, model, means, scales, angle, device):
    """the reference's two forwards with the LR input and the mask rotated on the GPU; returns (preds, preds_after_rot)
    as fp32 device tensors"""
    dev = _device_of(Xs, device)
    x, b = _on_device(Xs, dev), _on_device(bs, dev)
    preds = _forward(model, x, b)
    rx, rb = ops.rotate_fields(x, means, scales, angle), ops.rotate_building(b, angle)
    return preds, _forward(model, rx, rb)


def calc_preds_for_equivariance_errors(*, Xs, bs, model: torch.nn.Module, means: list, scales: list, angle: float,
                                       device: str, dtype: torch.dtype = torch.float32):
    """(rotated_preds, preds_after_rot), both dimensionalised (scales * v + means), float64 -- numpy for numpy / CPU
    input as in the reference, device tensors for device input.  (``dtype``: kept for the reference's signature; the
    engine's model takes fp32 inputs.)"""
    preds, par = _preds_pair(Xs, bs, model, means, scales, angle, device)
    rot = ops.rotate_fields(preds, means, scales, angle)
    m = torch.tensor(means, dtype=torch.float64, device=preds.device).view(1, 4, 1, 1, 1)
    s = torch.tensor(scales, dtype=torch.float64, device=preds.device).view(1, 4, 1, 1, 1)
    rot, par = s * rot.double() + m, s * par.double() + m
    if _is_host(Xs):
        return rot.cpu().numpy(), par.cpu().numpy()
    return rot, par


def _as_dict(err: torch.Tensor) -> typing.Dict[str, np.float64]:
    v = err.cpu().numpy()
    return {k: np.float64(v[i]) for i, k in enumerate(KEYS)}


def calc_equivariance_errors(*, Xs, bs, model: torch.nn.Module, means: list, scales: list, angle: float, sx: int,
                             ex: int, sy: int, ey: int, device: str, dtype: torch.dtype = torch.float32):
    """{'tm', 'vr', 'vl_vp'}: window means of |dT|, |dw| and ||(du, dv)|| between the rotated prediction and the
    prediction on the rotated input (dimensional units).  Both forwards run under no_grad on ``model``; the last
    rotation and the reduction are one fused kernel."""
    preds, par = _preds_pair(Xs, bs, model, means, scales, angle, device)
    return _as_dict(ops.equivariance_errors(preds, par, means, scales, angle, sx, ex, sy, ey))


def calc_equivariance_errors_over_angles(*, Xs, bs, model: torch.nn.Module, means: list, scales: list,
                                         angles: typing.Sequence[float], sx: int, ex: int, sy: int, ey: int,
                                         device: str, dtype: torch.dtype = torch.float32) -> typing.List[dict]:
    """calc_equivariance_errors at every angle of ``angles`` (one dict per angle, in order; each equal to the
    single-angle call bit for bit).  The prediction on the original input is computed once, and so are the spline
    coefficients of the LR input, the mask and that prediction: each later angle pays only the gathers, the second
    forward and the fused error."""
    dev = _device_of(Xs, device)
    x, b = _on_device(Xs, dev), _on_device(bs, dev)
    preds = _forward(model, x, b)
    ws = (ops.rotate_workspace(x), ops.rotate_workspace(b))
    wp = ops.rotate_workspace(preds)
    errs = []
    for i, angle in enumerate(angles):
        ready = i > 0
        rx = ops.rotate_fields(x, means, scales, angle, workspace=ws[0], coef_ready=ready)
        rb = ops.rotate_building(b, angle, workspace=ws[1], coef_ready=ready)
        par = _forward(model, rx, rb)
        errs.append(ops.equivariance_errors(preds, par, means, scales, angle, sx, ex, sy, ey, workspace=wp,
                                            coef_ready=ready))
    return [_as_dict(e) for e in errs]
