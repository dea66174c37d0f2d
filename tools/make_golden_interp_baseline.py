#!/usr/bin/env python3
"""Writes tests/golden/interp_baseline.npz: the interpolation baseline (the reference notebooks' ``fill_na``) recorded
from CPU torch and scipy.  The trilinear step is ``F.interpolate(scale_factor=s, mode="trilinear")``; the fill calls
scipy the way xarray's DataArray.interpolate_na(dim, method="linear", fill_value="extrapolate") does on a dimension
without coordinate -- per line, a line with no NaN or with fewer than two valid cells unchanged, otherwise
interp1d(x[valid], y[valid], kind="linear", fill_value="extrapolate", bounds_error=False) evaluated at the NaN positions,
x the fp64 index (xarray.core.missing: func_interpolate_na, ScipyInterpolator) -- along z, then y, then x, each result
stored back as fp32.

Two deliberate differences from the notebook.  It upsamples ``xs[:, None]``, a batch of one-channel volumes, which
ATen's CPU code treats as channels-last and sums as eight weight-product terms; here the variables are the channels of
one sample (``xs[None]``), the contiguous layout whose nested sum include/sr3d.h states.  And y[valid] is promoted to
fp64 first, as include/sr3d.h states the rule.  Given fp32 values, interp1d forms y_hi - y_lo in fp32 before it divides
in fp64, which moves about a quarter of the filled cells by one fp32 rounding of that difference; xarray hands scipy
the fp32 values, so this is one of the ways in which parity with xarray itself stays unpinned.

  lines/<i>/{y,out}              hand-built lines: both ends, gaps, all NaN, no NaN, one valid cell, two valid cells
  <case>_x<s>/{blank,values,checksum}
                                 every rule case of tests/interp_baseline_ref.py at both scales (inputs regenerated
                                 there from the seed): the cells that were NaN before the fill (packed bits), what they
                                 hold after it, and the xor of the bit patterns of all other cells, which are torch's
                                 own upsample

Needs scipy (a tool, not a test dependency).  usage: python tools/make_golden_interp_baseline.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.interpolate import interp1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "interp_baseline.npz")


def xr_fill_line(y):
    x = np.arange(len(y), dtype=np.float64)
    nans = np.isnan(y)
    n_nans = nans.sum()
    if n_nans == 0 or n_nans >= len(y) - 1:
        return y
    f = interp1d(x[~nans], y[~nans].astype(np.float64), kind="linear", fill_value="extrapolate", bounds_error=False)
    out = y.copy()
    out[nans] = f(x[nans])
    return out


def fill_na(lr, mask, scale):
    up = F.interpolate(torch.from_numpy(lr)[None], scale_factor=scale, mode="trilinear")[0].numpy()
    build = F.interpolate(torch.from_numpy(mask.astype(np.float32))[None, None], scale_factor=scale,
                          mode="nearest")[0, 0].numpy()
    a = np.where(build[None] == 0, up, np.float32(np.nan))
    for axis in (1, 2, 3):
        a = np.apply_along_axis(xr_fill_line, axis, a)
    assert a.dtype == np.float32
    return a


def lines():
    nan = np.nan

    def f(*v):
        return np.array(v, dtype=np.float32)

    return [f(nan, nan, 2, nan, nan, nan, 5.5, nan), f(1, nan, 3), f(nan, 7, nan, nan, 9.25, nan, nan),
            f(nan, nan, nan, nan), f(1, 2, 3, 4), f(nan, nan, 4, nan, nan), f(nan, 4, nan, 0.1, nan),
            f(0.1, nan, nan, 0.7, nan, -3e-5, nan, nan, nan, 1e6), f(nan, 3), f(nan, nan, nan, 1.1, 1.3)]


def main():
    import interp_baseline_ref as R
    d = {}
    ls = lines()
    d["lines/n"] = np.array(len(ls))
    for i, y in enumerate(ls):
        d[f"lines/{i}/y"], d[f"lines/{i}/out"] = y, xr_fill_line(y)
    for scale in sorted(R.RULE_SHAPES):
        for name in sorted(R.RULE_CASES):
            lr, mask = R.rule_case(name, scale)
            k = f"{name}_x{scale}"
            out = fill_na(lr, mask, scale)
            blank = F.interpolate(torch.from_numpy(mask.astype(np.float32))[None, None], scale_factor=scale,
                                  mode="nearest")[0, 0].numpy() != 0
            blank = blank[None] | np.isnan(F.interpolate(torch.from_numpy(lr)[None], scale_factor=scale,
                                                         mode="trilinear")[0].numpy())
            d[f"{k}/blank"], d[f"{k}/values"] = np.packbits(blank), out[blank]
            d[f"{k}/checksum"] = np.bitwise_xor.reduce(out[~blank].view(np.uint32))
    np.savez_compressed(OUT, **d)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(d)} arrays)", file=sys.stderr)


if __name__ == "__main__":
    main()
