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

``load_atmos_data`` / ``_load_atmos_data`` read the LES's GrADS output (src/io_grads.py) with the reference's asserts
and return an ``AtmosData``: lazy, memory-mapped, and decoded per time step on the GPU (ops.grads_decode,
csrc/sr3d_grads.hip) instead of an xr.Dataset.
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


# ---------------------------------------------------------------- the LES's GrADS output as device tensors
class AtmosData:
    """the four variables of one GrADS output directory (reference: the xr.Dataset of load_atmos_data), lazy: nothing
    is read until a time step is asked for.  Unpacks as the reference's tuple (vl, vp, vr, tm); ``lev`` / ``lat`` /
    ``lon`` / ``time`` are tm's coordinates.  ``step(i)`` decodes time index i on the GPU (ops.grads_decode): the four
    level-window byte ranges go to the device as they lie in the files, and vl, vp, vr come out NaN wherever tm is
    (align_nan_grids).  ``stage`` / ``decode`` are the two halves of ``step`` for callers that pipeline them."""

    NAMES = ("tm", "vl", "vp", "vr")           # the channel order of step()
    ALIGN = 256                                # every variable's bytes start on a multiple of it in a staging buffer

    def __init__(self, vl, vp, vr, tm):
        self.vl, self.vp, self.vr, self.tm = vl, vp, vr, tm
        self._vars = (tm, vl, vp, vr)
        sizes = [v.step_range(0)[1] - v.step_range(0)[0] if v.shape[0] else 0 for v in self._vars]
        self._starts = np.concatenate([[0], np.cumsum([-(-s // self.ALIGN) * self.ALIGN for s in sizes])]).tolist()
        self._sizes = sizes

    def __iter__(self):
        return iter((self.vl, self.vp, self.vr, self.tm))

    lev = property(lambda self: self.tm.lev)
    lat = property(lambda self: self.tm.lat)
    lon = property(lambda self: self.tm.lon)
    time = property(lambda self: self.tm.time)
    shape = property(lambda self: self.tm.shape)

    @property
    def staging_bytes(self) -> int:
        """size of the buffer ``stage`` fills"""
        return self._starts[-1]

    def stage(self, i: int, out: torch.Tensor) -> torch.Tensor:
        """copy the four byte ranges of time index i from the files into the host uint8 tensor ``out`` (pinned, for an
        asynchronous copy to the device)"""
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.numel() >= self.staging_bytes and not out.is_cuda
        host = out.numpy()
        for v, s, n in zip(self._vars, self._starts, self._sizes):
            host[s:s + n] = v.step_bytes(i)
        return out

    def decode(self, staged: torch.Tensor, want_tm_mask: bool = False):
        """the device copy of a staged buffer -> (4, Z, Y, X) fp32 (channels tm, vl, vp, vr), on the current stream;
        with ``want_tm_mask`` also isnan(tm) as (Z, Y, X) uint8"""
        tm = self.tm
        same = all((v.byteswap, v.yrev, v.zrev, v.shape, v.full_plane_shape, v.window)
                   == (tm.byteswap, tm.yrev, tm.zrev, tm.shape, tm.full_plane_shape, tm.window) for v in self._vars)
        if not same:
            raise ValueError("the four variables differ in shape, window or layout options")
        Y, X = tm.full_plane_shape
        res = ops.grads_decode([staged[s:s + n] for s, n in zip(self._starts, self._sizes)],
                               shape=(tm.shape[1], Y, X), level_offset=[v.level_offset for v in self._vars],
                               level_pitch=[v.level_pitch for v in self._vars], undef=[v.undef for v in self._vars],
                               byteswap=tm.byteswap, yrev=tm.yrev, zrev=tm.zrev, align_nan=True,
                               want_tm_mask=want_tm_mask)
        if tm.window == (slice(0, Y), slice(0, X)):
            return res
        wy, wx = tm.window                       # a margin was cut (read_array's margin > 0)
        if want_tm_mask:
            return res[0][..., wy, wx].contiguous(), res[1][..., wy, wx].contiguous()
        return res[..., wy, wx].contiguous()

    def steps(self, indices, device=None, overlap: bool = True):
        """yields (i, decoded (4, Z, Y, X) tensor) for every time index of ``indices``.  With ``overlap`` the copy to
        the device and the decode of the NEXT index run on a side stream while the caller works on the tensor it was
        handed: two staging sets (pinned host buffer, device buffer), reused in event order.  The caller queues its
        GPU work on the tensor on the current stream before it asks for the next one."""
        dev = _device(device)
        indices = list(indices)
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream()
            side = torch.cuda.Stream() if overlap else main
            sets = [dict(pin=torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory(),
                         dev=torch.empty(self.staging_bytes, dtype=torch.uint8, device=dev),
                         copied=torch.cuda.Event(), ready=torch.cuda.Event(), consumed=torch.cuda.Event(), raw=None)
                    for _ in range(2 if overlap else 1)]
            side.wait_stream(main)

            def launch(k):
                s = sets[k % len(sets)]
                s["copied"].synchronize()            # the pinned buffer's last copy has left it
                self.stage(indices[k], s["pin"])
                with torch.cuda.stream(side):
                    side.wait_event(s["consumed"])   # the caller's work on this set's last tensor is done
                    s["dev"].copy_(s["pin"], non_blocking=True)
                    s["copied"].record(side)
                    s["raw"] = self.decode(s["dev"])
                    s["ready"].record(side)

            if overlap and indices:
                launch(0)
            for k, i in enumerate(indices):
                if not overlap:
                    launch(k)
                elif k + 1 < len(indices):
                    launch(k + 1)                    # one step ahead of the step the caller is about to work on
                s = sets[k % len(sets)]
                main.wait_event(s["ready"])
                raw, s["raw"] = s["raw"], None
                raw.record_stream(main)
                yield i, raw
                del raw
                s["consumed"].record(main)

    def step(self, i: int, device=None, want_tm_mask: bool = False):
        """time index i as a (4, Z, Y, X) fp32 tensor on ``device``"""
        dev = _device(device)
        host = self.stage(i, torch.empty(self.staging_bytes, dtype=torch.uint8))
        with torch.cuda.device(dev):
            return self.decode(host.to(dev), want_tm_mask)


def _load_atmos_data(grads_dir, min_index_height: int = 4, max_index_height: int = 101, margin: int = 20,
                     discarded_initial_period: int = 10, nest_level: str = "0n") -> AtmosData:
    """the reference's function: the four variables of ``grads_dir`` with the level window and margin cut; unpacks as
    (vl, vp, vr, tm).  The NaN alignment to tm happens when a time step is decoded (AtmosData.step)."""
    from .io_grads import read_array
    kw = dict(margin=margin, min_index_height=min_index_height, max_index_height=max_index_height,
              discarded_initial_period=discarded_initial_period, nest_level=nest_level)
    vl = read_array(grads_dir, "vl", **kw)
    vp = read_array(grads_dir, "vp", **kw)
    vr = read_array(grads_dir, "vr", **kw)
    tm = read_array(grads_dir, "tm", **kw)
    return AtmosData(vl, vp, vr, tm)


def load_atmos_data(grads_dir, data_shape: tuple = (50, 96, 400, 400)) -> AtmosData:
    """the reference's function with its asserts: four variables of ``data_shape`` (t, z, y, x) from level index 4
    (lev = 17.5 m, the ground level around Tokyo station) on a unique vertical spacing of 5 m"""
    assert data_shape[-2] == data_shape[-1], "x and y grid numbers are not equal"
    max_index_height = 4 + data_shape[1]
    data = _load_atmos_data(grads_dir, max_index_height=max_index_height, margin=0)
    vl, vp, vr, tm = data
    assert vl.shape == tuple(data_shape)  # t,z,y,x
    assert vl.shape == vp.shape == vr.shape == tm.shape
    assert vl.dims == ("time", "lev", "lat", "lon")  # t,z,y,x
    assert vl.dims == vp.dims == vr.dims == tm.dims

    vertical_grid_spaces = np.unique(np.diff(tm.lev))
    assert len(vertical_grid_spaces) == 1, "Vertical grid spacing is not unique"
    assert vertical_grid_spaces[0] == 5.0, "Vertical grid spacing is not equal to 5 meters"
    return data
