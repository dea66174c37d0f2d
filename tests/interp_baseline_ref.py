"""Numpy restatement of the interpolation baseline (the reference notebooks' ``fill_na``; include/sr3d.h:
sr3d_interp_baseline), pinned to scipy by tests/golden/interp_baseline.npz (tools/make_golden_interp_baseline.py).

  1. trilinear upsample: torch's CPU ``F.interpolate(mode="trilinear")`` on a contiguous multi-channel tensor;
  2. NaN where the nearest-upsampled LR building mask is set;
  3. along z, y, x: a line with k NaN out of n is unchanged if k == 0 or k >= n - 1, else every NaN cell i takes
     (y_hi - y_lo) / (hi - lo) * (i - lo) + y_lo with j = clip(searchsorted(v, i), 1, m), lo = v[j-1], hi = v[j] over the
     valid indices v, evaluated in fp64 and (dtype float32) rounded once to fp32.

``dtype=np.float64`` runs the same code in fp64 throughout (the inputs promoted): the yardstick for tolerances.
"""
import numpy as np
import torch
import torch.nn.functional as F


def trilinear(lr, scale, dtype=np.float32):
    """(..., z, y, x) -> (..., s*z, s*y, s*x), align_corners=False, the scale factor passed as it is"""
    t = torch.from_numpy(np.ascontiguousarray(lr, dtype=dtype))
    lead = t.shape[:-3]
    t = t.reshape((1, -1) + tuple(t.shape[-3:]))
    # the volumes as CHANNELS of one sample, and never a single channel: a one-channel tensor is also channels-last
    # contiguous, and ATen's kernel for that layout sums eight weight-product terms instead of the nested form
    if t.shape[1] == 1:
        t = t.expand(1, 2, *t.shape[2:]).contiguous()
    out = F.interpolate(t, scale_factor=scale, mode="trilinear")[0, :int(np.prod(lead, dtype=np.int64))]
    return out.reshape(tuple(lead) + tuple(out.shape[-3:])).numpy()


def upsampled_mask(mask, scale):
    m = np.asarray(mask) != 0
    return m.repeat(scale, 0).repeat(scale, 1).repeat(scale, 2)


def fill_axis(a, axis):
    """one pass of step 3 along `axis`; a new array of a's dtype"""
    moved = np.moveaxis(a, axis, -1)
    lines = np.ascontiguousarray(moved).reshape(-1, moved.shape[-1])
    n = lines.shape[1]
    nan = np.isnan(lines)
    k = nan.sum(axis=1)
    for l in np.nonzero((k > 0) & (k < n - 1))[0]:
        v = np.nonzero(~nan[l])[0]
        i = np.nonzero(nan[l])[0]
        j = np.clip(np.searchsorted(v, i), 1, len(v) - 1)
        lo, hi = v[j - 1], v[j]
        y_lo, y_hi = lines[l, lo].astype(np.float64), lines[l, hi].astype(np.float64)
        lines[l, i] = ((y_hi - y_lo) / (hi - lo) * (i - lo) + y_lo).astype(lines.dtype)
    return np.moveaxis(lines.reshape(moved.shape), -1, axis)


def fill(masked):
    """step 3 on a (..., Z, Y, X) volume -> (filled, [NaN count after z, after y, after x])"""
    a, counts = masked, []
    for axis in (-3, -2, -1):
        a = fill_axis(a, axis)
        counts.append(int(np.isnan(a).sum()))
    return np.ascontiguousarray(a), counts


def interp_baseline_ref(lr, lr_is_in_build, scale=4, dtype=np.float32):
    """-> dict(out, masked = the volume after step 2, n_nan = NaN counts after step 2 and after each pass)"""
    up = trilinear(lr, scale, dtype)
    masked = np.where(upsampled_mask(lr_is_in_build, scale), np.asarray(np.nan, dtype), up)
    out, counts = fill(masked)
    return dict(out=out, masked=masked, n_nan=[int(np.isnan(masked).sum())] + counts)


# ---------------------------------------------------------------- the rule cases (shared by the host and GPU tests)
RULE_SHAPES = {4: (4, 3, 5, 7), 2: (4, 4, 6, 5)}       # LR (C, z, y, x) per scale
# name -> the pass after which no NaN is left ("never": some stay)
RULE_CASES = {"ground": "z", "top": "z", "floating": "z", "one_valid_level": "z", "lr_nan": "z", "column": "y",
              "two_columns": "y", "column_on_y_edge": "y", "y_line": "x", "everything": "never"}


def rule_case(name, scale):
    """(lr (C, z, y, x) fp32, mask (z, y, x) uint8) built to hit one rule"""
    C, z, y, x = RULE_SHAPES[scale]
    rng = np.random.default_rng(sorted(RULE_CASES).index(name) * 10 + scale)
    lr = rng.random((C, z, y, x), dtype=np.float32)
    m = np.zeros((z, y, x), np.uint8)
    if name == "ground":                # a building rising from the ground: extrapolation downwards
        m[:z - 1, 1, 2] = 1
    elif name == "top":                 # a masked top level: extrapolation upwards
        m[z - 1, 2, 3] = 1
    elif name == "floating":            # interior interpolation
        m[1, 3, 1] = 1
    elif name == "one_valid_level":     # one valid LR level = s valid HR levels: still filled in z
        m[1:, 1, 4] = 1
    elif name == "lr_nan":              # a NaN of the LR input itself, outside the mask
        m[0, 1, 2] = 1
        lr[1, 1, 3, 3] = np.nan
        lr[2, z - 1, 0, 0] = np.nan
    elif name == "column":              # a fully masked column: the y pass
        m[:, 2, 2] = 1
    elif name == "two_columns":         # two fully masked columns, adjacent along y and along x
        m[:, 2:4, 3] = 1
        m[:, 1, 0:2] = 1
    elif name == "column_on_y_edge":    # y extrapolation, at both edges
        m[:, 0, 3] = 1
        m[:, y - 1, 1] = 1
    elif name == "y_line":              # a whole y line of fully masked columns: left to the x pass
        m[:, :, 4] = 1
        m[:, :, 0] = 1
    elif name == "everything":          # every (y, x) plane masked at every level: nothing to fill from
        m[:] = 1
    else:
        raise KeyError(name)
    return lr, m


def tower_case(seed=3, shape=(1, 4, 8, 20, 24), built=0.2):
    """LR (B, C, z, y, x) and a random 'tower' mask: about `built` of the columns hold a building from the ground up to
    a random level, some through the whole depth"""
    rng = np.random.default_rng(seed)
    B, C, z, y, x = shape
    lr = rng.standard_normal(shape).astype(np.float32)
    top = np.where(rng.random((y, x)) < built, rng.integers(1, z + 2, (y, x)), 0)    # z + 1: the whole column
    m = (np.arange(z)[:, None, None] < top[None]).astype(np.uint8)
    return lr, m
