#!/usr/bin/env python3
"""Writes tests/golden/lr_data.npz: the nearest fill of the reference's LR data maker recorded from scipy, called the
way xarray's DataArray.interpolate_na(dim, method="nearest", fill_value="extrapolate") calls it -- per line, a line
with no NaN or only NaN unchanged, otherwise interp1d(x[valid], y[valid], kind="nearest", fill_value="extrapolate",
bounds_error=False) evaluated at the NaN positions (xarray.core.missing: func_interpolate_na, ScipyInterpolator).

  lines/<i>/{y,x,out}   hand-built lines: ties, extrapolation at both ends, all-NaN, no NaN, one valid point,
                        non-index coordinates with near-ties
  vol_a/*, vol_b/*      small volumes filled along lev, then lat, then lon (lat / lon only if NaN is left, as the
                        reference's guard does): a tm NaN in mid-column, fully-NaN columns filled along lat (vol_a)
                        and a fully-NaN x line filled along lon (vol_b)
  step/*                one time step of the script on a (4, 8, 24, 24) domain with margin 4: the HR output and the
                        LR output, pooled with sliding windows and the masked weights as the reference does

Needs scipy (a tool, not a test dependency).  usage: python tools/make_golden_lr_data.py"""
import os
import sys

import numpy as np
from scipy.interpolate import interp1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lr_data.npz")
S = 4


def xr_fill_line(y, x):
    nans = np.isnan(y)
    if nans.sum() == 0 or nans.sum() == len(y):
        return y
    f = interp1d(x[~nans], y[~nans], kind="nearest", fill_value="extrapolate", bounds_error=False)
    out = y.copy()
    out[nans] = f(x[nans])
    return out


def xr_fill(a, axis, coord):
    return np.apply_along_axis(xr_fill_line, axis, a, np.asarray(coord, dtype=np.float64))


def fill_3d(v, lev, lat, lon):
    out = xr_fill(v, 0, lev)
    if np.sum(np.isnan(out)) > 0:
        out = xr_fill(xr_fill(out, 1, lat), 2, lon)
    return out


def in_building(tz, ez, levs):
    """1 below the first level >= tz where tz > ez (argmin of an all-True or all-False comparison is 0: nothing)"""
    out = np.zeros((len(levs),) + tz.shape)
    for j in range(tz.shape[0]):
        for i in range(tz.shape[1]):
            if not tz[j, i] <= ez[j, i]:
                out[:int(np.argmin(levs < tz[j, i])), j, i] = 1
    return out


def pool(hr, mask):
    w = np.where(mask == 1, 0.0, 1.0)
    w = np.lib.stride_tricks.sliding_window_view(w, (S, S, S), axis=(0, 1, 2))
    sw = np.broadcast_to(w.sum(axis=(-3, -2, -1), keepdims=True), w.shape)
    with np.errstate(invalid="ignore"):
        w = np.where(sw != 0, w / sw, np.nan)
    s = np.sum(np.lib.stride_tricks.sliding_window_view(hr, (S, S, S), axis=(0, 1, 2)) * w, axis=(-3, -2, -1))
    lr = np.full(hr.shape, np.nan, dtype=hr.dtype)
    lr[S // 2:-S // 2 + 1, S // 2:-S // 2 + 1, S // 2:-S // 2 + 1] = s
    return lr[S // 2::S, S // 2::S, S // 2::S]


def lines(rng):
    nan = np.nan

    def f(*v):
        return np.array(v, dtype=np.float32)

    def idx(n):
        return np.arange(n, dtype=np.float64)

    out = [
        (f(1, nan, 3), idx(3)),                                      # tie: the lower coordinate
        (f(nan, nan, 2, nan, nan, nan, 5, nan), idx(8)),             # both ends, an odd gap
        (f(nan, 7, nan, nan, 9, nan, nan), idx(7)),                  # an even gap
        (f(nan, nan, nan, nan), idx(4)),                             # all NaN: unchanged
        (f(1, 2, 3, 4), idx(4)),                                     # no NaN
        (f(nan, nan, 4, nan, nan), idx(5)),                          # one valid point
        (f(1, nan, 3), np.array([0.1, 0.2, 0.30000000000000004])),   # near-ties in fp64
        (f(1, nan, 3), np.array([0.1, 0.2, 0.3])),
        (f(1, nan, nan, 3), np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0])),
        (f(5, nan, 6), np.array([17.5, 22.5, 27.5])),                # levels: the tie goes down
    ]
    for _ in range(6):
        n = 12
        x = np.cumsum(rng.choice([0.5, 1.0, 1.0 + 2.0 ** -40, 1.5], n))
        y = rng.standard_normal(n).astype(np.float32)
        y[rng.random(n) < 0.5] = np.nan
        out.append((y, x))
    return out


def main():
    rng = np.random.default_rng(20261016)
    d = {}
    ls = lines(rng)
    d["lines/n"] = np.array(len(ls))
    for i, (y, x) in enumerate(ls):
        d[f"lines/{i}/y"], d[f"lines/{i}/x"], d[f"lines/{i}/out"] = y, x, xr_fill_line(y, x)

    Z, Y, X = 8, 6, 5
    for name in ("vol_a", "vol_b"):
        v = rng.standard_normal((Z, Y, X)).astype(np.float32)
        v[:3, 0, 0] = np.nan
        v[4, 2, 1] = np.nan                                      # mid-column NaN
        v[:, 3, 2] = np.nan                                      # fully-NaN columns: lat fill
        v[:, 4, 2] = np.nan
        if name == "vol_b":
            v[:, :, 3] = np.nan                                  # a fully-NaN x line: lon fill
        lev = 17.5 + 5.0 * np.arange(Z)
        lat = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.5])
        lon = np.array([0.0, 1.0, 2.0, 3.5, 5.0])
        after_lev = xr_fill(v, 0, lev)
        dead = np.isnan(after_lev).all(axis=0)
        d[f"{name}/in"], d[f"{name}/filled"] = v, fill_3d(v, lev, lat, lon)
        d[f"{name}/lev"], d[f"{name}/lat"], d[f"{name}/lon"] = lev, lat, lon
        d[f"{name}/lat_filled_columns"] = np.array(int((dead & ~dead.all(axis=0)[None]).sum()))
        d[f"{name}/lon_filled_columns"] = np.array(int((dead & dead.all(axis=0)[None]).sum()))

    C, Z, Y, X, m = 4, 8, 24, 24, 4
    levs = 17.5 + 5.0 * np.arange(Z)
    lats = np.cumsum(rng.choice([1.0, 1.0, 0.75, 1.25], Y))
    lons = np.cumsum(rng.choice([1.0, 1.0, 0.75, 1.25], X))
    raw = np.empty((C, Z, Y, X), np.float32)
    raw[0] = 290 + 10 * rng.standard_normal((Z, Y, X))
    raw[1:] = 5 * rng.standard_normal((C - 1, Z, Y, X)) * np.exp2(rng.integers(-20, 2, (C - 1, Z, Y, X)))
    raw[0, 5, 9, 9] = np.nan                                     # a tm NaN in mid-column (aligned into vl, vp, vr)
    raw[0, :, 12, 12] = np.nan                                   # a fully-NaN column
    raw[2, :, 6, 15] = np.nan                                    # ... and one in one channel only
    hr_tz = np.where(rng.random((Y, X)) < 0.2, rng.uniform(18, 45, (Y, X)), 10.0)
    hr_ez = np.full((Y, X), 15.0)
    lr_tz = rng.choice([0.0, 25.0, 33.0, levs[Z - 2], 1000.0], (Y // S, X // S))
    lr_tz[1, 2] = np.nan
    lr_tz[2, 3] = levs[Z - 3] + 1.0                              # in (lev[Z-4], lev[Z-1]]
    lr_ez = np.full((Y // S, X // S), 15.0)
    al = raw.copy()
    al[1:] = np.where(np.isnan(al[0])[None], np.nan, al[1:])
    hm = (in_building(hr_tz, hr_ez, levs) + np.isnan(al[0])) > 0
    hr = np.where(hm[None], np.nan, al)
    rz = in_building(np.repeat(np.repeat(lr_tz, S, 0), S, 1), np.repeat(np.repeat(lr_ez, S, 0), S, 1), levs)
    lz = in_building(lr_tz, lr_ez, levs[::S])
    lr = []
    for c in range(C):
        h = fill_3d(np.where(hm, np.nan, al[c]), levs, lats, lons)
        lr.append(pool(np.where(rz == 1, np.nan, h), rz))
    lr = np.where(lz[None] == 1, np.nan, np.stack(lr)).astype(np.float32)
    ml = m // S
    d.update({"step/raw": raw, "step/hr_mask": hm, "step/lr_tz": lr_tz, "step/lr_ez": lr_ez, "step/levs": levs,
              "step/lats": lats, "step/lons": lons, "step/margin": np.array(m),
              "step/hr": np.ascontiguousarray(hr[..., m:-m, m:-m]),
              "step/lr": np.ascontiguousarray(lr[..., ml:-ml, ml:-ml])})
    np.savez_compressed(OUT, **d)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(d)} arrays)", file=sys.stderr)


if __name__ == "__main__":
    main()
