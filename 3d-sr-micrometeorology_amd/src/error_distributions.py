"""Error-distribution evaluation (engine extension; the reference's evaluation reports means only): how large the
worst cells' errors are, whether the error is biased, and whether the super-resolved field reproduces the DISTRIBUTION
of the truth.  One fused pass per batch (``ops.eval_distributions``, csrc/sr3d_eval_dist.hip) gives 256-bin histograms of
the signed normalised errors, the velocity-error norm and the predicted and true fields over the fluid cells, near the
walls and away from them, with the exact min and max.  Histogram counts are integers: ``DistributionMeter`` adds them
over a loader (or over ranks) exactly, so its result IS the histogram of the pooled test set, and every quantile and
PDF distance here is a function of the counts alone.

A quantile read off a histogram lies within one bin width of the quantile of the raw values (every order statistic is
placed inside the bin that holds it), provided the under- and overflow slots are empty; where a quantile falls into one
of them it is clamped to the range and flagged."""
import typing
from logging import getLogger

import numpy as np
import torch

from .. import ops
from .._lib import DIST_BINS, DIST_CLASSES, DIST_SERIES, DIST_SERIES_INDEX, DIST_SLOTS

logger = getLogger()

SERIES_NAMES: typing.Tuple[str, ...] = tuple(sorted(DIST_SERIES_INDEX, key=DIST_SERIES_INDEX.get))
CLASS_NAMES = ("near_wall", "far", "fluid")          # fluid = both classes added
QUANTILES = (0.1, 1, 5, 25, 50, 75, 95, 99, 99.9)    # percent: columns q0.1 .. q99.9
ABS_QUANTILES = (50, 90, 99, 99.9)                   # percent of |error|: columns abs_q50 .. abs_q99.9
UNDER, OVER, NAN = 0, DIST_SLOTS - 2, DIST_SLOTS - 1


def _name(prefix: str, q: float) -> str:
    return f"{prefix}{q:g}"


def bin_edges(lo: float, hi: float, bins: int = DIST_BINS) -> np.ndarray:
    """the ``bins + 1`` edges of a series' bins (fp64); bin k is [edge k, edge k + 1) up to the rule's fp32 rounding"""
    return float(lo) + (float(hi) - float(lo)) * np.arange(bins + 1, dtype=np.float64) / bins


def _quantiles(under: int, bins: np.ndarray, over: int, lo: float, hi: float, qs: np.ndarray):
    """quantiles (fractions ``qs``) of one histogram: numpy's linear rule, (1 - f) x[i] + f x[i + 1] at i + f =
    q (n - 1), on order statistics placed linearly inside their bins (the j-th of c values of a bin at (j + 1/2) / c of
    its width); an order statistic in the under- / overflow slot is lo / hi and sets the flag"""
    nb = len(bins)
    c = np.concatenate([[under], bins, [over]]).astype(np.int64)
    n = int(c.sum())
    if n == 0:
        return np.full(len(qs), np.nan), np.zeros(len(qs), dtype=bool)
    cum = np.cumsum(c)
    w = (float(hi) - float(lo)) / nb

    def order_stat(i):      # i: integer ranks 0 .. n - 1
        slot = np.searchsorted(cum, i, side="right")            # first slot with cum > i
        before = cum[slot] - c[slot]
        x = float(lo) + (slot - 1 + (i - before + 0.5) / c[slot]) * w
        clamped = (slot == 0) | (slot == nb + 1)
        return np.where(slot == 0, float(lo), np.where(slot == nb + 1, float(hi), x)), clamped

    r = qs * (n - 1)
    i0 = np.floor(r).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    f = r - i0
    (x0, c0), (x1, c1) = order_stat(i0), order_stat(i1)
    return (1.0 - f) * x0 + f * x1, c0 | (c1 & (f > 0))


def quantiles_from_counts(counts, lo: float, hi: float, qs: typing.Sequence[float]):
    """``counts``: (..., DIST_SLOTS) of one series (any leading dimensions), ``qs``: fractions in [0, 1].  Returns
    ``(values, clamped)`` shaped (..., len(qs)): the quantiles of the non-NaN values, linear inside the bin; NaN for
    an empty histogram; where a quantile falls into the under- or overflow slot it is clamped to ``lo`` / ``hi`` and
    ``clamped`` is set.  With both slots empty the value is within one bin width of the quantile of the raw values."""
    c = np.asarray(counts, dtype=np.int64)
    if c.shape[-1] != DIST_SLOTS:
        raise ValueError(f"quantiles_from_counts expects (..., {DIST_SLOTS}) counts")
    qs = np.asarray(qs, dtype=np.float64)
    if qs.ndim != 1 or bool(((qs < 0) | (qs > 1)).any()):
        raise ValueError("quantiles are fractions in [0, 1]")
    flat = c.reshape(-1, DIST_SLOTS)
    vals, flags = zip(*[_quantiles(r[UNDER], r[1:OVER], r[OVER], lo, hi, qs) for r in flat]) if len(flat) else ((), ())
    return (np.array(vals, dtype=np.float64).reshape(c.shape[:-1] + qs.shape),
            np.array(flags, dtype=bool).reshape(c.shape[:-1] + qs.shape))


def fold_counts(counts, lo: float, hi: float) -> typing.Tuple[int, np.ndarray, int]:
    """the histogram of |v| from the histogram of a signed series whose range is symmetric (lo == -hi): (0, bins
    (DIST_BINS / 2) over [0, hi), overflow) -- bin j of |v| is bin 128 + j plus its mirror image 127 - j, and both
    outer slots are overflow"""
    if float(lo) != -float(hi):
        raise ValueError(f"folding about 0 needs a symmetric range (got {lo} .. {hi})")
    c = np.asarray(counts, dtype=np.int64)
    half = DIST_BINS // 2
    bins = c[1:OVER]
    return 0, bins[half:] + bins[:half][::-1], int(c[UNDER] + c[OVER])


def abs_quantiles_from_counts(counts, lo: float, hi: float, qs: typing.Sequence[float]):
    """as ``quantiles_from_counts`` for |v|: the signed bins folded about 0 (``fold_counts``); (..., DIST_SLOTS) in,
    ``(values, clamped)`` (..., len(qs)) out"""
    c = np.asarray(counts, dtype=np.int64)
    qs = np.asarray(qs, dtype=np.float64)
    flat = c.reshape(-1, DIST_SLOTS)
    out = [_quantiles(*fold_counts(r, lo, hi), 0.0, hi, qs) for r in flat]
    return (np.array([v for v, _ in out], dtype=np.float64).reshape(c.shape[:-1] + qs.shape),
            np.array([f for _, f in out], dtype=bool).reshape(c.shape[:-1] + qs.shape))


def wasserstein1(counts_a, counts_b, lo: float, hi: float) -> float:
    """the 1-Wasserstein distance between two histograms over the same range: bin width x sum |CDF_a - CDF_b| on the
    normalised counts, the under- and overflow slots taken as one more bin on either side; NaN slots are left out.
    NaN when either histogram is empty."""
    a, b = (np.asarray(c, dtype=np.int64)[..., :NAN].astype(np.float64) for c in (counts_a, counts_b))
    na, nb = a.sum(), b.sum()
    if na == 0 or nb == 0:
        return float("nan")
    w = (float(hi) - float(lo)) / DIST_BINS
    return float(w * np.abs(np.cumsum(a) / na - np.cumsum(b) / nb)[:-1].sum())


class DistributionMeter:
    """running histograms over a loader.  Counts and cells are added as int64 on the device, min of mins and max of
    maxes taken there; ``result()`` makes the one device -> host copy.  Integer adds are exact: the result over a
    loader is exactly the histogram of the pooled test set (one call on the concatenation of all batches)."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.counts, self.minmax, self.cells = None, None, None

    def update(self, counts: torch.Tensor, minmax: torch.Tensor, cells: torch.Tensor) -> None:
        """what ``ops.eval_distributions`` returned for a batch (whole-batch form)"""
        if tuple(counts.shape) != (DIST_SERIES, DIST_CLASSES, DIST_SLOTS) or tuple(minmax.shape) != (
                DIST_SERIES, DIST_CLASSES, 2) or tuple(cells.shape) != (3,) or counts.dtype != torch.int64:
            raise ValueError("DistributionMeter takes the outputs of ops.eval_distributions (per_sample=False)")
        if self.counts is None:
            self.counts, self.minmax, self.cells = counts.clone(), minmax.clone(), cells.clone()
            return
        self.counts += counts
        self.cells += cells
        self.minmax[..., 0] = torch.minimum(self.minmax[..., 0], minmax[..., 0])
        self.minmax[..., 1] = torch.maximum(self.minmax[..., 1], minmax[..., 1])

    def result(self) -> typing.Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(counts int64 (DIST_SERIES, DIST_CLASSES, DIST_SLOTS), minmax fp32 (DIST_SERIES, DIST_CLASSES, 2), cells
        int64 (3): built, near, far) as host arrays"""
        if self.counts is None:
            raise RuntimeError("DistributionMeter.result() before any update()")
        packed = torch.cat([self.counts.flatten(), self.cells.flatten(),
                            self.minmax.contiguous().flatten().view(torch.int32).to(torch.int64)]).cpu().numpy()
        n = self.counts.numel()
        counts, cells = packed[:n].reshape(tuple(self.counts.shape)), packed[n:n + 3]
        minmax = packed[n + 3:].astype(np.int32).view(np.float32).reshape(tuple(self.minmax.shape))
        return counts, minmax, cells


def distribution_table(counts: np.ndarray, minmax: np.ndarray, lo: typing.Sequence[float], hi: typing.Sequence[float],
                       means: typing.Sequence[float], stds: typing.Sequence[float]):
    """the DataFrame of ``evaluate_error_distributions`` from pooled counts and min / max"""
    import pandas as pd

    counts = np.asarray(counts, dtype=np.int64)
    counts3 = np.concatenate([counts, counts.sum(axis=1, keepdims=True)], axis=1)              # + fluid
    mm = np.asarray(minmax, dtype=np.float64)
    mm3 = np.concatenate([mm, np.stack([mm[:, :, 0].min(axis=1), mm[:, :, 1].max(axis=1)], axis=-1)[:, None]], axis=1)
    qs, aqs = np.array(QUANTILES) / 100.0, np.array(ABS_QUANTILES) / 100.0
    rows = []
    for name in SERIES_NAMES:
        s = DIST_SERIES_INDEX[name]
        is_err, is_field = name.startswith("ERR_") and name != "ERR_VEL_NORM", not name.startswith("ERR_")
        ch = "TUVW".index(name[-1]) if name != "ERR_VEL_NORM" else None
        # physical units: errors scale with the channel's std, fields also shift by its mean, the norm already is
        scale = 1.0 if ch is None else float(stds[ch])
        shift = float(means[ch]) if is_field else 0.0
        for k, cls in enumerate(CLASS_NAMES):
            c = counts3[s, k]
            row = {"series": name, "class": cls, "cells": int(c.sum()), "underflow": int(c[UNDER]),
                   "overflow": int(c[OVER]), "nan": int(c[NAN]), "min": mm3[s, k, 0], "max": mm3[s, k, 1]}
            q, flag = quantiles_from_counts(c, lo[s], hi[s], qs)
            row.update({_name("q", p): v for p, v in zip(QUANTILES, q)})
            row["clamped"] = bool(flag.any())
            if is_err and float(lo[s]) == -float(hi[s]):
                aq, aflag = abs_quantiles_from_counts(c, lo[s], hi[s], aqs)
                row.update({_name("abs_q", p): v for p, v in zip(ABS_QUANTILES, aq)})
                row["clamped"] = row["clamped"] or bool(aflag.any())
            if name.startswith("TRUTH_"):
                row["w1_to_pred"] = wasserstein1(c, counts3[DIST_SERIES_INDEX["PRED_" + name[-1]], k], lo[s], hi[s])
            phys = {}
            for key, v in row.items():
                if key in ("min", "max") or key.startswith("q"):
                    phys[key + "_phys"] = v * scale + shift
                elif key.startswith("abs_q") or key == "w1_to_pred":
                    phys[key + "_phys"] = v * scale
            row.update(phys)
            rows.append(row)
    df = pd.DataFrame(rows)
    lead = ["series", "class", "cells", "underflow", "overflow", "nan", "min", "max"]
    lead += [_name("q", p) for p in QUANTILES] + [_name("abs_q", p) for p in ABS_QUANTILES] + ["w1_to_pred", "clamped"]
    lead = [c for c in lead if c in df.columns]
    return df[lead + [c for c in df.columns if c not in lead]]


def out_of_range_series(counts: np.ndarray) -> typing.List[str]:
    """names of the series with a non-zero under- plus overflow count (either class)"""
    c = np.asarray(counts)
    return [n for n in SERIES_NAMES if int(c[DIST_SERIES_INDEX[n], :, [UNDER, OVER]].sum()) > 0]


def evaluate_error_distributions(model, loader, config: dict, *, device: str = "cuda:0", near_width: int = 1,
                                 err_range=(-0.5, 0.5), field_range=(-0.5, 1.5), vel_norm_range=(0.0, 8.0),
                                 return_histograms: bool = False):
    """``optim_helper.evaluate`` for distributions: a pandas.DataFrame with one row per (series, class in near_wall,
    far, fluid): ``cells`` (values binned, NaN included), ``underflow``, ``overflow``, ``nan``, ``min``, ``max``, the
    quantiles ``q0.1 .. q99.9``, for the four signed error series ``abs_q50 .. abs_q99.9`` (of |error|), for the TRUTH
    rows ``w1_to_pred`` (1-Wasserstein distance to the PRED histogram of the channel), ``clamped`` (a quantile fell
    outside the range) and every value column again in physical units (``*_phys``: x std of the channel, + its mean
    for the fields; ERR_VEL_NORM is physical already).  ``config['data']`` gives ``stds`` and ``means``.
    ``return_histograms``: also the dict ``script/evaluate_error_distributions.py --save_histograms`` stores."""
    from .optim_helper import _device_batches
    stds = list(config["data"]["stds"])
    means = list(config["data"].get("means", [0.0] * 4))
    lo, hi = ops.distribution_ranges(err_range, field_range, vel_norm_range)
    meter = DistributionMeter()
    n = 0
    with torch.no_grad():
        for Xs, bs, ys in _device_batches(loader, device):
            preds = model(Xs, bs)
            meter.update(*ops.eval_distributions(preds, ys, bs, stds, err_range=err_range, field_range=field_range,
                                                 vel_norm_range=vel_norm_range, near_width=near_width))
            n += len(Xs)
    counts, minmax, cells = meter.result()
    for name in out_of_range_series(counts):
        s = DIST_SERIES_INDEX[name]
        logger.warning(f"{name}: {int(counts[s, :, UNDER].sum())} values below and {int(counts[s, :, OVER].sum())} above "
                       f"the range {lo[s]:g} .. {hi[s]:g} (exact min {float(minmax[s, :, 0].min()):g}, max "
                       f"{float(minmax[s, :, 1].max()):g}): widen the range")
    logger.info(f"error distributions over {n} samples: {int(cells[1])} near-wall and {int(cells[2])} far fluid cells, "
                f"{int(cells[0])} built")
    df = distribution_table(counts, minmax, lo, hi, means, stds)
    if return_histograms:
        return df, {"counts": counts, "minmax": minmax, "cells": cells, "lo": np.array(lo), "hi": np.array(hi),
                    "near_width": np.array(int(near_width)), "series": np.array(SERIES_NAMES),
                    "stds": np.array(stds, dtype=np.float64), "means": np.array(means, dtype=np.float64)}
    return df
