"""LR training data from HR fields, building-aware (reference datascience/src/training_data_maker.py, the "outside LR
buildings" variant that script/make_dl_data_using_outside_lr_builds.py uses).

The reference masks the HR buildings, fills the masked cells with xarray's nearest ``interpolate_na`` along lev, lat
and lon, masks the LR buildings resized to the HR grid and average-pools 4x4x4 blocks with masked weights.  Here one
HIP call does it per time step for all channels (ops.coarse_grain_outside_buildings, csrc/sr3d_lrdata.hip), without
xarray, and the building maps become per-LR-column level counts (``lr_building_tops``).

What the reference's pooling computes: a masked cell holds NaN, and NaN * 0 = NaN, so a block with any masked or
still-NaN cell is NaN and every other block is the plain mean of its 64 cells.  ``avg_pooling_weights`` is accepted
for the reference's interface but the result does not depend on it.  The reference's output dtype follows how the
installed xarray promotes ``xr.where(mask, np.nan, float32)``; these functions return float32, the dtype the training
Datasets convert to.  Arrays replace DataArrays: ``da`` is (lev, lat, lon), ``levs`` / ``lats`` / ``lons`` its
coordinates (None: index coordinates; they must increase strictly, as xarray requires).
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from .. import ops

SCALE = ops.LRDATA_SCALE


def _device(device=None) -> torch.device:
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"device {dev}: the LR data maker runs on the GPU only (the sr3d engine has no CPU path)")
    return dev


def _level_counts(tz: np.ndarray, ez: np.ndarray, levs: np.ndarray) -> np.ndarray:
    """calc_is_in_building as a count per column: the levels before the first one >= tz where tz > ez, else 0 (a NaN
    top, or one above every level, marks nothing -- argmin of an all-equal row is 0)"""
    levs = np.asarray(levs, dtype=np.float64)
    top = (levs[:, None, None] < tz[None]).argmin(axis=0)
    return np.where(~(tz <= ez), top, 0).astype(np.int32)


def lr_building_tops(lr_tz: np.ndarray, lr_ez: np.ndarray, hr_levs, scale: int = SCALE) -> np.ndarray:
    """(2, Y/s, X/s) int32 from the LR building tops / ground heights (y, x): per LR column the number of masked HR
    levels of the resized LR buildings (make_resized_lr_tz's mask: every HR column of the LR cell has it) and the
    number of masked LR levels (calc_is_in_building at hr_levs[::scale])"""
    lr_tz, lr_ez = np.asarray(lr_tz, dtype=np.float64), np.asarray(lr_ez, dtype=np.float64)
    assert lr_tz.ndim == 2 and lr_tz.shape == lr_ez.shape
    levs = np.asarray(hr_levs, dtype=np.float64)
    return np.stack([_level_counts(lr_tz, lr_ez, levs), _level_counts(lr_tz, lr_ez, levs[::scale])])


def _tops_from_resized_mask(mask: np.ndarray, scale: int) -> np.ndarray:
    """make_resized_lr_tz's (z, y, x) mask -> lr_building_tops[0:1] with no LR-level mask; raises if the mask is not
    a per-LR-cell prefix of levels"""
    m = np.asarray(mask) == 1
    Z, Y, X = m.shape
    count = m.sum(axis=0)
    lr = count[::scale, ::scale]
    if not (np.array_equal(m, np.arange(Z)[:, None, None] < count[None])
            and np.array_equal(count, np.repeat(np.repeat(lr, scale, 0), scale, 1))):
        raise ValueError("lr_is_in_build must be make_resized_lr_tz's mask: the lowest levels of whole LR cells")
    return np.stack([lr, np.zeros_like(lr)]).astype(np.int32)


def _check_widths(lev_window_width: int, lat_window_width: int, lon_window_width: int) -> int:
    if not lev_window_width == lat_window_width == lon_window_width == SCALE:
        raise ValueError(f"window widths {(lev_window_width, lat_window_width, lon_window_width)}: only "
                         f"{SCALE} x {SCALE} x {SCALE} is implemented (the reference asserts SR_SCALE == 4)")
    return SCALE


def _coarse_grain(stack: np.ndarray, lr_is_in_build, hr_is_in_build, levs, lats, lons, scale, device):
    dev = _device(device)
    lr_mask = lr_is_in_build.detach().cpu().numpy() if isinstance(lr_is_in_build, torch.Tensor) else lr_is_in_build
    hr_mask = torch.as_tensor(np.asarray(hr_is_in_build) == 1 if not isinstance(hr_is_in_build, torch.Tensor)
                              else hr_is_in_build == 1).to(dev)
    tops = torch.from_numpy(_tops_from_resized_mask(lr_mask, scale)).to(dev)
    raw = torch.as_tensor(stack).to(device=dev, dtype=torch.float32).contiguous()
    _, lr = ops.coarse_grain_outside_buildings(raw, hr_mask, tops, scale=scale, hr_margin=0, lat=lats, lon=lons,
                                               lev=levs, align_nan=False)
    return lr.cpu().numpy()


def make_coarse_grained_dataarray_with_outside_lr_buildings(
        *, da, lr_is_in_build, hr_is_in_build, avg_pooling_weights=None, lev_window_width: int,
        lat_window_width: int, lon_window_width: int, levs=None, lats=None, lons=None, device=None) -> np.ndarray:
    """the reference's function for one variable ``da`` (lev, lat, lon): ``hr_is_in_build`` (z, y, x) is the HR mask,
    ``lr_is_in_build`` (z, y, x) the resized LR buildings (make_resized_lr_tz(...)[0]); returns the LR array
    (Z/4, Y/4, X/4) float32.  ``avg_pooling_weights`` is unused (module docstring)."""
    s = _check_widths(lev_window_width, lat_window_width, lon_window_width)
    a = da.detach().cpu().numpy() if isinstance(da, torch.Tensor) else np.asarray(da)
    assert a.ndim == 3 and np.shape(lr_is_in_build) == np.shape(hr_is_in_build) == a.shape  # z, y, x
    return _coarse_grain(a[None], lr_is_in_build, hr_is_in_build, levs, lats, lons, s, device)[0]


def make_coarse_grained_dataset_with_outside_lr_buildings(
        *, hr_ds, lr_is_in_build, hr_is_in_build, avg_pooling_weights=None, lev_window_width: int,
        lat_window_width: int, lon_window_width: int, levs=None, lats=None, lons=None,
        device=None) -> typing.Union[typing.Dict[str, np.ndarray], np.ndarray]:
    """every variable of ``hr_ds`` -- a mapping name -> (lev, lat, lon) array, or one (C, lev, lat, lon) array --
    in ONE GPU call; returns the same structure of LR arrays (float32)"""
    s = _check_widths(lev_window_width, lat_window_width, lon_window_width)
    if isinstance(hr_ds, typing.Mapping):
        names = list(hr_ds)
        stack = np.stack([v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                          for v in hr_ds.values()])
    else:
        names = None
        stack = hr_ds.detach().cpu().numpy() if isinstance(hr_ds, torch.Tensor) else np.asarray(hr_ds)
    assert stack.ndim == 4 and np.shape(lr_is_in_build) == np.shape(hr_is_in_build) == stack.shape[1:]
    lr = _coarse_grain(stack, lr_is_in_build, hr_is_in_build, levs, lats, lons, s, device)
    return lr if names is None else {n: lr[i] for i, n in enumerate(names)}
