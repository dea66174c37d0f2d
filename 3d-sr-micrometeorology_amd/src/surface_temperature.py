"""Near-surface (2 m) temperature among buildings (the reference's make_inference + make_2m_temperature notebooks).

The reference dimensionalises each prediction on the host, writes it to disk, reads it back with the raw HR truth and
extrapolates temperature in a Python double loop over every (x, y) column to the building / ground top height.  Here
the extrapolation is one HIP kernel (csrc/sr3d_surface.hip) that reads the model output or the HR volume in place;
the fused form also reduces the error sums on the device (ops.surface_temperature_errors).

Arrays follow the notebook's axis order: temperature (N, Z, X, Y), building heights (X, Y) as read_building_height
returns them, 2 m maps (N, X, Y).  The kernels take the engine's (Y, X) layout.
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from .. import ops

Z0, DZ = 17.5, 5.0
HEIGHT_LEVELS = np.arange(32) * 5 + 17.5  # meters


def dimensionalize(data, means, scales):
    """physical units from normalised ones (numpy arrays or tensors with broadcastable means / scales)"""
    assert data.ndim == means.ndim == scales.ndim
    assert data.shape[1] == 4
    return data * scales + means


def _device(device=None) -> torch.device:
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"device {dev}: the 2 m temperature runs on the GPU only (the sr3d engine has no CPU path)")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU available: the sr3d engine has no CPU path")
    return dev


def building_map(building: np.ndarray, device=None) -> torch.Tensor:
    """read_building_height's (X, Y) array -> the kernels' (Y, X) fp64 map on the device"""
    assert building.ndim == 2
    return torch.from_numpy(np.ascontiguousarray(np.asarray(building, dtype=np.float64).T)).to(_device(device))


def infer_2m_height_temperature(temperature: np.ndarray, building: np.ndarray, device=None) -> np.ndarray:
    """the notebook's contract: temperature (N, Z, X, Y) float32 on the levels HEIGHT_LEVELS[:Z] (Z <= 32: the notebook
    takes all 32), building (X, Y) -> (N, X, Y) float32, NaN where the building tops the highest level -- computed on
    the GPU"""
    assert temperature.ndim == 4  # batch, z, x, y dims
    assert building.ndim == 2  # x and y dims
    assert building.shape == temperature.shape[2:]
    assert 1 <= temperature.shape[1] <= len(HEIGHT_LEVELS)
    dev = _device(device)
    t = torch.from_numpy(np.ascontiguousarray(temperature, dtype=np.float32)).to(dev)
    src = t.transpose(2, 3).contiguous().unsqueeze(1)             # (N, 1, Z, Y, X)
    out = ops.surface_temperature(src, building_map(building, dev), channel=0, levels=temperature.shape[1], z0=Z0,
                                  dz=DZ)
    return np.ascontiguousarray(out.transpose(1, 2).cpu().numpy())


def calc_2m_temperature_errors(acc) -> typing.Dict[str, float]:
    """RMSE and MAE from the accumulator of ops.surface_temperature_errors (sum (p - t)^2, sum |p - t|, count): the
    notebook's sqrt(nanmean((pred - true) ** 2)) and nanmean(|pred - true|), in fp64; NaN when nothing was counted"""
    a = acc.detach().cpu().double().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc, dtype=np.float64)
    sq, ab, n = (float(v) for v in a.reshape(3))
    if n == 0:
        return {"RMSE": float("nan"), "MAE": float("nan")}
    return {"RMSE": float(np.sqrt(sq / n)), "MAE": ab / n}
