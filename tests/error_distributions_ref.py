"""Restatement of the error-distribution evaluation (include/sr3d.h: sr3d_eval_distributions) in numpy, written from
the binning rule in ``np.float32`` arithmetic:

    inv = float32(256.0 / (float64(hi) - float64(lo)))
    k   = floor(float32(float32(v - lo) * inv))

k < 0 or -inf: underflow (slot 0); k >= 256 or +inf: overflow (slot 257); NaN: slot 258; else slot 1 + k.  This is the
definition, not ``np.histogram``: in float64 that differs on values within rounding of an edge.  Only fluid cells
(b > 0) are binned; class 0 holds those with ``wall_distance_ref(b, near_width) <= near_width``, class 1 the others;
``near_width == 0``: every fluid cell is class 1."""
import numpy as np
import torch

from wall_distance_ref import wall_distance_ref

SERIES = ("ERR_T", "ERR_U", "ERR_V", "ERR_W", "ERR_VEL_NORM", "PRED_T", "PRED_U", "PRED_V", "PRED_W", "TRUTH_T",
          "TRUTH_U", "TRUTH_V", "TRUTH_W")
NSERIES, NCLASSES, NBINS, NSLOTS = 13, 2, 256, 259
UNDER, OVER, NAN = 0, 257, 258
DEFAULT_RANGES = dict(err_range=(-0.5, 0.5), field_range=(-0.5, 1.5), vel_norm_range=(0.0, 8.0))


def ranges(err_range=(-0.5, 0.5), field_range=(-0.5, 1.5), vel_norm_range=(0.0, 8.0)):
    """(lo, hi) float32 arrays of the 13 series; err_range / field_range: one pair or one per channel"""
    def four(r):
        r = np.asarray(r, dtype=np.float64)
        return np.broadcast_to(r, (4, 2))
    pairs = np.concatenate([four(err_range), np.asarray(vel_norm_range, dtype=np.float64)[None], four(field_range),
                            four(field_range)])
    return pairs[:, 0].astype(np.float32), pairs[:, 1].astype(np.float32)


def slots(v, lo, hi):
    """slot of every value of the float32 array v for the range (lo, hi)"""
    v = np.asarray(v, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    inv = np.float32(256.0 / (np.float64(hi) - np.float64(lo)))
    with np.errstate(invalid="ignore", over="ignore"):
        s = v - lo
        assert s.dtype == np.float32
        k = np.floor(s * inv)
        assert k.dtype == np.float32
    out = np.empty(v.shape, dtype=np.int64)
    nan = np.isnan(v)
    under = ~nan & ((k < 0) | (v == -np.inf))
    over = ~nan & ~under & ((k >= NBINS) | (v == np.inf))
    mid = ~(nan | under | over)
    out[nan], out[under], out[over] = NAN, UNDER, OVER
    out[mid] = 1 + k[mid].astype(np.int64)
    return out


def series_values(p, t, stds):
    """(13, B, Z, Y, X) float32: the value of every series at every voxel"""
    p, t = p.numpy().astype(np.float32), t.numpy().astype(np.float32)
    s = [np.float32(x) for x in stds]
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - t
        a, b, c = s[1] * d[:, 1], s[2] * d[:, 2], s[3] * d[:, 3]
        vel = np.sqrt((a * a + b * b) + c * c)
    assert d.dtype == np.float32 and vel.dtype == np.float32
    return np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 3], vel, *(p[:, c] for c in range(4)), *(t[:, c] for c in range(4))])


def classes(b, near_width):
    """(B, Z, Y, X) int array: -1 built (not b > 0), 0 near the walls, 1 far"""
    fluid = (b[:, 0] > 0).numpy()
    if near_width > 0:
        near = (wall_distance_ref(b, near_width)[:, 0] <= near_width).numpy()
    else:
        near = np.zeros_like(fluid)
    return np.where(fluid, np.where(near, 0, 1), -1)


def distributions_ref(p, t, b, stds, near_width=1, per_sample=False, **rng):
    """(counts int64 ([B,] 13, 2, 259), minmax float32 ([B,] 13, 2, 2), cells int64 ([B,] 3)) as torch tensors"""
    lo, hi = ranges(**rng)
    vals = series_values(p, t, stds)
    cls = classes(b, near_width)
    B = p.shape[0]
    groups = [slice(i, i + 1) for i in range(B)] if per_sample else [slice(0, B)]
    counts = np.zeros((len(groups), NSERIES, NCLASSES, NSLOTS), dtype=np.int64)
    minmax = np.empty((len(groups), NSERIES, NCLASSES, 2), dtype=np.float32)
    minmax[..., 0], minmax[..., 1] = np.inf, -np.inf
    cells = np.zeros((len(groups), 3), dtype=np.int64)
    for g, sl in enumerate(groups):
        c = cls[sl]
        cells[g] = [(c == -1).sum(), (c == 0).sum(), (c == 1).sum()]
        for s in range(NSERIES):
            v = vals[s, sl]
            sl_s = slots(v, lo[s], hi[s])
            for k in range(NCLASSES):
                sel = c == k
                counts[g, s, k] = np.bincount(sl_s[sel], minlength=NSLOTS)
                w = v[sel]
                w = w[~np.isnan(w)]
                if w.size:
                    minmax[g, s, k] = [w.min(), w.max()]
    out = [torch.from_numpy(x) for x in (counts, minmax, cells)]
    return tuple(out) if per_sample else tuple(x[0] for x in out)
