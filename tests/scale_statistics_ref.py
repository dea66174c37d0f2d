"""Restatement of the scale-resolved evaluation (include/sr3d.h: sr3d_eval_scale_statistics) in numpy, fp64, one slice
pair per direction and lag:

    first = f[..., : n - r], second = f[..., r :]        along the direction's axis
    valid = fluid(first) & fluid(second)                 fluid: b > 0
            & fluid at every cell between them           (unobstructed rule)
    delta = second - first;  D1 .. D4 = sum delta^k;  F0, F1 = sum first, second;  FF0, FF1 = sum first^2, second^2

over the valid pairs, per sample and per level of the FIRST cell, for f = p_c, t_c and p_c - t_c (in fp64).  Values of
cells outside every valid pair are selected out (``np.where``), never multiplied by 0.  ``abs_sums`` holds sum |term|
of every entry: the scale of the rounding-error bound of a sum of that many terms in any order."""
import numpy as np
import torch

SERIES = ("PRED_T", "PRED_U", "PRED_V", "PRED_W", "TRUTH_T", "TRUTH_U", "TRUTH_V", "TRUTH_W", "ERR_T", "ERR_U", "ERR_V",
          "ERR_W")
MOMENTS = ("D1", "D2", "D3", "D4", "F0", "F1", "FF0", "FF1")
DIRS = ("x", "y", "z")
NSERIES, NMOMENTS, NDIRS, MAX_LAG = 12, 8, 3, 64
AXIS = {0: 3, 1: 2, 2: 1}          # direction -> axis of a (B, Z, Y, X) array
M = {n: i for i, n in enumerate(MOMENTS)}


def quantise(x, q=256):
    """floor to multiples of 1 / q (fp32 in, fp32 out; exact)"""
    return torch.floor(x * q) / q


def _sl(a, axis, lo, hi):
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(lo, hi)
    return a[tuple(idx)]


def scale_statistics_ref(p, t, b, R, unobstructed=False, per_sample=False):
    """(sums fp64 ([B,] Z, 3, R, 12, 8), pairs int64 ([B,] Z, 3, R), abs_sums fp64 like sums) as numpy arrays"""
    pn, tn = p.numpy().astype(np.float64), t.numpy().astype(np.float64)
    B, _, Z, Y, X = pn.shape
    with np.errstate(invalid="ignore"):
        f = np.concatenate([pn, tn, pn - tn], axis=1)                  # (B, 12, Z, Y, X)
    fluid = (b[:, 0] > 0).numpy()                                      # (B, Z, Y, X)
    sums = np.zeros((B, Z, NDIRS, R, NSERIES, NMOMENTS))
    abs_sums = np.zeros_like(sums)
    pairs = np.zeros((B, Z, NDIRS, R), dtype=np.int64)
    for d in range(NDIRS):
        ax = AXIS[d]
        n = fluid.shape[ax]
        for r in range(1, min(R, n - 1) + 1):
            valid = _sl(fluid, ax, 0, n - r) & _sl(fluid, ax, r, n)
            if unobstructed:
                for k in range(1, r):
                    valid = valid & _sl(fluid, ax, k, n - r + k)
            zs = valid.shape[1]                                         # levels that have a first cell (d = z: Z - r)
            pairs[:, :zs, d, r - 1] = valid.sum(axis=(2, 3))
            f0, f1 = _sl(f, ax + 1, 0, n - r), _sl(f, ax + 1, r, n)
            with np.errstate(invalid="ignore", over="ignore"):
                delta = f1 - f0
                d2 = delta * delta
                terms = (delta, d2, d2 * delta, d2 * d2, f0, f1, f0 * f0, f1 * f1)
                for m, term in enumerate(terms):
                    sel = np.where(valid[:, None], term, 0.0)           # (B, 12, zs, Y', X')
                    sums[:, :zs, d, r - 1, :, m] = sel.sum(axis=(3, 4)).transpose(0, 2, 1)
                    abs_sums[:, :zs, d, r - 1, :, m] = np.abs(sel).sum(axis=(3, 4)).transpose(0, 2, 1)
    if per_sample:
        return sums, pairs, abs_sums
    return sums.sum(axis=0), pairs.sum(axis=0), abs_sums.sum(axis=0)
