"""numpy restatement of the reference's LR training data (datascience/: make_coarse_grained_dataarray_with_outside_lr_
buildings and the per-time-step part of make_dl_data_using_outside_lr_builds), in two forms.

- literal (small sizes): xarray's interpolate_na(method="nearest", fill_value="extrapolate") line by line with
  scipy interp1d's rule, then the reference's sliding_window_view pooling with its weights;
- block (any size): the fill as a choice of source column, and the pooling as non-overlapping 4x4x4 blocks summed in
  numpy's pairwise order for 64 contiguous elements.

tests/test_lr_data_host.py pins the literal fill to scipy (tests/golden/lr_data.npz) and the two forms to each other;
the GPU tests pin the kernel to the block form."""
import numpy as np

S = 4


def calc_is_in_building(tz, ez, levs):
    """the reference's loop, verbatim in effect: (z, y, x) float64"""
    out = np.zeros((len(levs),) + tz.shape)
    for j in range(tz.shape[0]):
        for i in range(tz.shape[1]):
            t, e = tz[j, i], ez[j, i]
            if t <= e:
                continue
            out[:(np.asarray(levs) < t).argmin(), j, i] = 1
    return out


# ---------------------------------------------------------------- literal form
def nearest_fill_line(y, x):
    """xarray's func_interpolate_na with scipy interp1d(kind="nearest", fill_value="extrapolate"): midpoints
    x[i]/2 + x[i+1]/2, searchsorted side="left" (ties to the lower coordinate), edge values past the ends"""
    nans = np.isnan(y)
    if nans.sum() == 0 or nans.sum() == len(y):
        return y
    xv, yv = x[~nans], y[~nans]
    bds = xv / 2.0
    bds = bds[1:] + bds[:-1]
    idx = np.searchsorted(bds, x[nans], side="left").clip(0, len(xv) - 1)
    out = y.copy()
    out[nans] = yv[idx]
    return out


def interpolate_na(a, axis, coord):
    coord = np.arange(a.shape[axis], dtype=np.float64) if coord is None else np.asarray(coord, dtype=np.float64)
    return np.apply_along_axis(nearest_fill_line, axis, a, coord)


def pooling_weights(mask):
    w = np.where(mask == 1, 0.0, 1.0)
    w = np.lib.stride_tricks.sliding_window_view(w, (S, S, S), axis=(0, 1, 2))
    sw = np.broadcast_to(np.sum(w, axis=(-3, -2, -1), keepdims=True), w.shape)
    with np.errstate(invalid="ignore"):
        return np.where(sw != 0, w / sw, np.nan)


def coarse_grain_literal(da, hr_is_in_build, lr_is_in_build, levs=None, lats=None, lons=None):
    """the reference function for one (z, y, x) float32 variable; lr_is_in_build = the resized LR buildings"""
    hr = np.where(hr_is_in_build == 1, np.nan, da)
    hr = interpolate_na(hr, 0, levs)
    if np.sum(np.isnan(hr)) > 0:
        hr = interpolate_na(hr, 1, lats)
        hr = interpolate_na(hr, 2, lons)
    hr = np.where(lr_is_in_build == 1, np.nan, hr)
    v = np.lib.stride_tricks.sliding_window_view(hr, (S, S, S), axis=(0, 1, 2))
    s = np.sum(v * pooling_weights(lr_is_in_build), axis=(-3, -2, -1))
    lr = np.full(hr.shape, np.nan, dtype=hr.dtype)
    lr[S // 2:-S // 2 + 1, S // 2:-S // 2 + 1, S // 2:-S // 2 + 1] = s
    return lr[S // 2::S, S // 2::S, S // 2::S]


# ---------------------------------------------------------------- block form
def nearest_index(valid, coord, axis):
    """per position along `axis`: the index of the valid position interp1d(kind="nearest") picks (itself if valid),
    -1 where the line has none"""
    n = valid.shape[axis]
    coord = np.arange(n, dtype=np.float64) if coord is None else np.asarray(coord, dtype=np.float64)
    shape = [1] * valid.ndim
    shape[axis] = n
    idx = np.arange(n).reshape(shape)
    lo = np.maximum.accumulate(np.where(valid, idx, -1), axis=axis)
    hi = np.flip(np.minimum.accumulate(np.flip(np.where(valid, idx, n), axis), axis=axis), axis)
    c = coord.reshape(shape)
    clo, chi = coord[np.clip(lo, 0, n - 1)], coord[np.clip(hi, 0, n - 1)]
    pick = np.where(c <= clo / 2.0 + chi / 2.0, lo, hi)
    pick = np.where(lo < 0, hi, np.where(hi >= n, lo, pick))
    return np.where((lo < 0) & (hi >= n), -1, pick)


def fill_block(hr, levs=None, lats=None, lons=None):
    """the lev / lat / lon nearest fill of a (z, y, x) volume with NaN, as a source column per (y, x)"""
    Z, Y, X = hr.shape
    k = nearest_index(~np.isnan(hr), levs, 0)
    filled = np.take_along_axis(hr, np.maximum(k, 0), axis=0)
    filled[k < 0] = np.nan
    live = k[0] >= 0                                  # (y, x)
    ysrc = nearest_index(live, lats, 0)               # (y, x): -1 where x has no live column
    xlive = live.any(axis=0)
    xsrc = nearest_index(xlive, lons, 0)              # (x,)
    yy = np.broadcast_to(np.arange(Y)[:, None], (Y, X))
    xx = np.broadcast_to(np.arange(X)[None, :], (Y, X))
    sx = np.where(xlive[None, :], xx, xsrc[None, :])
    sy = np.where(sx >= 0, ysrc[yy, np.maximum(sx, 0)], -1)
    out = filled[:, np.maximum(sy, 0), np.maximum(sx, 0)]
    out[:, sy < 0] = np.nan
    return out


def block_mean(v):
    """(Z, Y, X) -> (Z/4, Y/4, X/4): numpy's pairwise sum of the 64 products x * (1/64) of each block, float64"""
    Z, Y, X = v.shape
    b = v.reshape(Z // S, S, Y // S, S, X // S, S).transpose(0, 2, 4, 1, 3, 5)
    b = b.reshape(Z // S, Y // S, X // S, 8, 8).astype(np.float64) * (1.0 / 64.0)
    r = b[..., 0, :].copy()
    for i in range(1, 8):
        r = r + b[..., i, :]
    return ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))


def coarse_grain_block(da, hr_is_in_build, lr_is_in_build, levs=None, lats=None, lons=None):
    hr = np.where(hr_is_in_build == 1, np.nan, da)
    hr = fill_block(hr, levs, lats, lons)
    hr = np.where(lr_is_in_build == 1, np.nan, hr)
    return block_mean(hr).astype(np.float32)


# ---------------------------------------------------------------- fixtures
def make_case(seed, C=4, Z=8, Y=24, X=28, coords=False):
    """one time step over every rule: a tm NaN in mid-column, a fully-NaN column in one channel, a fully-NaN x line
    in another, HR buildings of several heights, LR tops on the ground, between levels, in (lev[Z-4], lev[Z-1]],
    above every level and NaN, and optionally non-index lat / lon coordinates"""
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((C, Z, Y, X)) * np.exp2(rng.integers(-24, 6, (C, Z, Y, X)))).astype(np.float32)
    raw[0, 3, 5, 6] = np.nan
    raw[min(2, C - 1), :, 7, 9] = np.nan
    raw[min(1, C - 1), :, :, 3] = np.nan
    hm = np.zeros((Z, Y, X), bool)
    hm[:5, 2:4, 2:5] = True
    hm[:, 10:12, 10] = True
    levs = 17.5 + 5.0 * np.arange(Z)
    lr_tz = rng.choice([0.0, 20.0, 30.0, levs[Z - 3], levs[Z - 1], np.nan, 1000.0], (Y // S, X // S))
    lr_ez = np.where(rng.random((Y // S, X // S)) < 0.1, 40.0, 0.0)
    lats = np.cumsum(rng.uniform(0.5, 1.5, Y)) if coords else None
    lons = np.cumsum(rng.uniform(0.5, 1.5, X)) if coords else None
    return raw, hm, lr_tz, lr_ez, levs, lats, lons


# ---------------------------------------------------------------- one time step of the script
def resized_lr_mask(lr_tz, lr_ez, levs):
    f = S
    return calc_is_in_building(np.repeat(np.repeat(lr_tz, f, 0), f, 1), np.repeat(np.repeat(lr_ez, f, 0), f, 1),
                               np.asarray(levs))


def lr_data_ref(raw, hr_mask, lr_tz, lr_ez, levs, lats=None, lons=None, margin=40, align_nan=True, form="block"):
    """raw (C, Z, Y, X) float32, hr_mask (Z, Y, X) -> (HR output, LR output) float32, margins cut"""
    raw = np.array(raw, dtype=np.float32)
    if align_nan:
        raw[1:] = np.where(np.isnan(raw[0])[None], np.nan, raw[1:])
    hm = np.asarray(hr_mask).astype(bool)
    hr = np.where(hm[None], np.nan, raw)
    rz = resized_lr_mask(lr_tz, lr_ez, levs)
    lz = calc_is_in_building(lr_tz, lr_ez, np.asarray(levs)[::S])
    cg = coarse_grain_literal if form == "literal" else coarse_grain_block
    lr = np.stack([cg(raw[c], hm, rz, levs, lats, lons) for c in range(raw.shape[0])]).astype(np.float32)
    lr = np.where(lz[None] == 1, np.nan, lr).astype(np.float32)
    m, ml = margin, margin // S
    if m:
        hr, lr = hr[..., m:-m, m:-m], lr[..., ml:-ml, ml:-ml]
    return np.ascontiguousarray(hr), np.ascontiguousarray(lr)
