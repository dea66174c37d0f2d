"""Scale-resolved evaluation (engine extension; every other evaluation pass is a one-point statistic): at which length
scales the super-resolved detail is real, at which it is blurred and at which it is invented.  The domain is full of
buildings, so a spectrum of the masked planes means nothing; the building-aware equivalent is the two-point statistic
over the valid fluid pairs (x, x + r e_d).  One fused pass per batch (``ops.eval_scale_statistics``,
csrc/sr3d_eval_scale.hip) gives, per level, direction and lag, the fp64 sums D1 .. D4 of the increment's powers and F0,
F1, FF0, FF1 of the two ends' values and squares, for the prediction, the truth and the error, with the pair counts.
``ScaleStatisticsMeter`` pools them over a loader; every quantity here is a function of the pooled sums alone:

* structure functions S_k(r) = <delta^k>, increment skewness S3 / S2^1.5 and flatness S4 / S2^2;
* the two-point correlation rho(r), centred with the pair set's own means and variances;
* S2_pred / S2_truth (how much small-scale variance is recovered), the correlation of the increments of prediction and
  truth (whether the recovered detail is in the right place), S2_err / S2_truth (from which scale the model can be
  trusted), the integral length scale of the error.

The sums are of the normalised fields; the functions take the channel ``stds`` and answer in K and m/s (dimensionless
quantities do not depend on them).  Arrays are shaped (..., 3, R, 12, 8) / (..., 3, R) with any leading axes (levels).
A quotient with zero pairs or a zero denominator is NaN, never an exception."""
import typing
from logging import getLogger

import numpy as np
import torch

from .. import ops
from .._lib import SCALE_DIRS, SCALE_MOMENT_INDEX, SCALE_MOMENTS, SCALE_SERIES, SCALE_SERIES_INDEX

logger = getLogger()

SERIES_NAMES: typing.Tuple[str, ...] = tuple(sorted(SCALE_SERIES_INDEX, key=SCALE_SERIES_INDEX.get))
CHANNELS = ("T", "u", "v", "w")
KINDS = ("pred", "truth", "err")                      # series index = 4 * kind + channel
LONGITUDINAL = {"u": "x", "v": "y", "w": "z"}         # the velocity component along the separation
_M = SCALE_MOMENT_INDEX


def _check(sums, pairs):
    s, n = np.asarray(sums, dtype=np.float64), np.asarray(pairs, dtype=np.int64)
    if s.ndim < 4 or s.shape[-4] != len(SCALE_DIRS) or s.shape[-2:] != (SCALE_SERIES, SCALE_MOMENTS) or n.shape != s.shape[:-2]:
        raise ValueError(f"expected sums (..., 3, R, {SCALE_SERIES}, {SCALE_MOMENTS}) and pairs (..., 3, R)")
    return s, n


def _div(a, b):
    """a / b, NaN where b == 0 (or where either is NaN)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    out = np.full(a.shape, np.nan)
    np.divide(a, b, out=out, where=(b != 0) & ~np.isnan(b))
    return out


def _series_stds(stds) -> np.ndarray:
    s = np.asarray([float(v) for v in stds], dtype=np.float64)
    if s.shape != (4,):
        raise ValueError("stds = (std_T, std_u, std_v, std_w)")
    return np.tile(s, 3)                               # pred, truth, err of each channel


def pool_levels(sums, pairs):
    """sums and pairs added over every leading axis: (3, R, 12, 8) and (3, R)"""
    s, n = _check(sums, pairs)
    lead = tuple(range(s.ndim - 4))
    return s.sum(axis=lead), n.sum(axis=lead)


def structure_function(sums, pairs, stds, order: int = 2) -> np.ndarray:
    """S_order(r) = <delta^order> over the valid pairs, in (K or m/s)^order: (..., 3, R, 12)"""
    if order not in (1, 2, 3, 4):
        raise ValueError("structure functions of order 1 .. 4 are stored")
    s, n = _check(sums, pairs)
    return _div(s[..., order - 1], n[..., None]) * _series_stds(stds) ** order


def increment_skewness(sums, pairs, stds=None) -> np.ndarray:
    """S3 / S2^1.5 (dimensionless: ``stds`` cancels): (..., 3, R, 12)"""
    s, n = _check(sums, pairs)
    s2, s3 = _div(s[..., _M["D2"]], n[..., None]), _div(s[..., _M["D3"]], n[..., None])
    return _div(s3, np.where(s2 > 0, s2, np.nan) ** 1.5)


def increment_flatness(sums, pairs, stds=None) -> np.ndarray:
    """S4 / S2^2 (dimensionless; 3 for Gaussian increments): (..., 3, R, 12)"""
    s, n = _check(sums, pairs)
    s2, s4 = _div(s[..., _M["D2"]], n[..., None]), _div(s[..., _M["D4"]], n[..., None])
    return _div(s4, s2 ** 2)


def autocorrelation(sums, pairs, stds=None) -> np.ndarray:
    """rho(r) = (<f f'> - <f> <f'>) / sqrt(var f var f'), every average over the lag's own pair set (the first cells
    and the second cells of a masked domain are different sets: each end has its own mean and variance), with
    sum f f' = (FF0 + FF1 - D2) / 2.  Dimensionless: (..., 3, R, 12)"""
    s, n = _check(sums, pairs)
    n = n[..., None]
    m0, m1 = _div(s[..., _M["F0"]], n), _div(s[..., _M["F1"]], n)
    cross = _div((s[..., _M["FF0"]] + s[..., _M["FF1"]] - s[..., _M["D2"]]) / 2, n)
    v0, v1 = _div(s[..., _M["FF0"]], n) - m0 ** 2, _div(s[..., _M["FF1"]], n) - m1 ** 2
    prod = v0 * v1
    return _div(cross - m0 * m1, np.sqrt(np.where(prod > 0, prod, np.nan)))


def _d2(s):
    """D2 of pred, truth, err per channel: three (..., 3, R, 4) arrays"""
    d2 = s[..., _M["D2"]]
    return d2[..., 0:4], d2[..., 4:8], d2[..., 8:12]


def variance_ratio(sums, pairs, stds=None) -> np.ndarray:
    """S2_pred / S2_truth per channel: the share of the truth's variance at that scale the prediction has (1: all of
    it, < 1: blurred, > 1: more than there is).  (..., 3, R, 4)"""
    s, _ = _check(sums, pairs)
    dp, dt, _ = _d2(s)
    return _div(dp, dt)


def increment_correlation(sums, pairs, stds=None) -> np.ndarray:
    """the correlation of the increments of prediction and truth, (S2_p + S2_t - S2_e) / (2 sqrt(S2_p S2_t)): whether
    the detail at that scale is in the right place.  (..., 3, R, 4)"""
    s, _ = _check(sums, pairs)
    dp, dt, de = _d2(s)
    prod = dp * dt
    return _div(dp + dt - de, 2 * np.sqrt(np.where(prod > 0, prod, np.nan)))


def relative_error(sums, pairs, stds=None) -> np.ndarray:
    """S2_err / S2_truth per channel (0: exact at that scale; 2: as wrong as an independent field).  (..., 3, R, 4)"""
    s, _ = _check(sums, pairs)
    _, dt, de = _d2(s)
    return _div(de, dt)


def integral_length_scale_of(rho, delta_meter: float):
    """delta x (1/2 + sum rho(r)) over r = 1, 2, .. up to, not including, the first lag with rho <= 0 (trapezoid of rho
    from rho(0) = 1).  ``rho``: (..., R), lags along the last axis.  Returns ``(scale, truncated)``, each (...):
    ``truncated`` where no lag with rho <= 0 lies within R (a lag without pairs ends the sum too, and counts as
    truncated); NaN where lag 1 has no pairs."""
    rho = np.asarray(rho, dtype=np.float64)
    stop = ~(rho > 0)                                        # rho <= 0 or NaN
    before = np.cumsum(stop, axis=-1) == 0                   # lags before the first stop
    scale = float(delta_meter) * (0.5 + np.where(before, rho, 0.0).sum(axis=-1))
    first = np.argmax(stop, axis=-1)
    ended = stop.any(axis=-1)
    at_stop = np.take_along_axis(rho, first[..., None], axis=-1)[..., 0]
    truncated = ~ended | np.isnan(at_stop)
    return np.where(np.isnan(rho[..., 0]), np.nan, scale), truncated


def integral_length_scale(sums, pairs, stds=None, delta_meter: float = 5.0):
    """``integral_length_scale_of`` the autocorrelation of every series: ``(scale_m, truncated)``, each (..., 3, 12)"""
    rho = autocorrelation(sums, pairs)
    return integral_length_scale_of(np.moveaxis(rho, -2, -1), delta_meter)


def resolved_lag_of(rel, threshold: float = 0.5) -> np.ndarray:
    """the smallest lag r from which ``rel`` (..., R) stays <= threshold at every larger lag that has pairs (NaN lags
    are skipped); NaN where it never does, or nothing has pairs.  (...), as floats"""
    rel = np.asarray(rel, dtype=np.float64)
    R = rel.shape[-1]
    bad = ~np.isnan(rel) & ~(rel <= threshold)
    last_bad = np.where(bad.any(axis=-1), R - np.argmax(bad[..., ::-1], axis=-1), 0)     # lag (1-based) of the last bad one
    seen = ~np.isnan(rel)
    last_seen = np.where(seen.any(axis=-1), R - np.argmax(seen[..., ::-1], axis=-1), 0)
    return np.where(last_bad < last_seen, last_bad + 1.0, np.nan)


def resolved_lag(sums, pairs, stds=None, threshold: float = 0.5) -> np.ndarray:
    """``resolved_lag_of`` the relative error of every channel: (..., 3, 4)"""
    return resolved_lag_of(np.moveaxis(relative_error(sums, pairs), -2, -1), threshold)


class ScaleStatisticsMeter:
    """running sums over a loader: what ``ops.eval_scale_statistics`` returns for a batch (whole-batch form) is copied
    to the host and added there in fp64 (pairs in int64)."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.sums, self.pairs = None, None

    def update(self, sums, pairs) -> None:
        s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
        n = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
        if s.ndim != 5 or s.dtype != np.float64 or n.dtype != np.int64 or s.shape[1] != len(SCALE_DIRS) or \
                s.shape[3:] != (SCALE_SERIES, SCALE_MOMENTS) or n.shape != s.shape[:3]:
            raise ValueError("ScaleStatisticsMeter takes the outputs of ops.eval_scale_statistics (per_sample=False)")
        if self.sums is None:
            self.sums, self.pairs = s.copy(), n.copy()
            return
        if s.shape != self.sums.shape:
            raise ValueError(f"batch of another shape: {s.shape} after {self.sums.shape}")
        self.sums += s
        self.pairs += n

    def result(self) -> typing.Tuple[np.ndarray, np.ndarray]:
        """(sums fp64 (Z, 3, R, 12, 8), pairs int64 (Z, 3, R))"""
        if self.sums is None:
            raise RuntimeError("ScaleStatisticsMeter.result() before any update()")
        return self.sums.copy(), self.pairs.copy()


def scale_statistics_table(sums, pairs, stds, delta_meter: float = 5.0, per_level: bool = False,
                           threshold: float = 0.5):
    """the DataFrame of ``evaluate_scale_statistics`` from pooled sums (Z, 3, R, 12, 8) and pairs (Z, 3, R): one row
    per (channel, direction, lag), the levels pooled -- or, with ``per_level``, one such block per level with a
    leading ``level`` column."""
    import pandas as pd

    s, n = _check(sums, pairs)
    if s.ndim != 5:
        raise ValueError("scale_statistics_table expects sums (Z, 3, R, 12, 8)")
    if per_level:
        blocks = [(z, s[z], n[z]) for z in range(s.shape[0])]
    else:
        blocks = [(None,) + pool_levels(s, n)]
    rows = []
    for level, bs, bn in blocks:
        S = {k: structure_function(bs, bn, stds, k) for k in (2, 3, 4)}
        skew, flat, rho = increment_skewness(bs, bn), increment_flatness(bs, bn), autocorrelation(bs, bn)
        ratio, corr, rel = variance_ratio(bs, bn), increment_correlation(bs, bn), relative_error(bs, bn)
        scale, trunc = integral_length_scale(bs, bn, delta_meter=delta_meter)
        res = resolved_lag(bs, bn, threshold=threshold)
        R = bn.shape[-1]
        for c, ch in enumerate(CHANNELS):
            for d, dname in enumerate(SCALE_DIRS):
                for r in range(1, R + 1):
                    row = {} if level is None else {"level": level}
                    row.update({"channel": ch, "direction": dname, "lag": r, "distance_m": r * float(delta_meter),
                                "pairs": int(bn[d, r - 1]), "longitudinal": LONGITUDINAL.get(ch) == dname})
                    for k, kind in enumerate(KINDS):
                        i = 4 * k + c
                        row[f"S2_{kind}"], row[f"S3_{kind}"], row[f"S4_{kind}"] = (S[o][d, r - 1, i] for o in (2, 3, 4))
                        row[f"skewness_{kind}"], row[f"flatness_{kind}"] = skew[d, r - 1, i], flat[d, r - 1, i]
                        row[f"rho_{kind}"] = rho[d, r - 1, i]
                    row["variance_ratio"], row["increment_correlation"] = ratio[d, r - 1, c], corr[d, r - 1, c]
                    row["relative_error"] = rel[d, r - 1, c]
                    # per (channel, direction): repeated on every lag's row
                    for k, kind in enumerate(KINDS):
                        row[f"integral_scale_{kind}_m"] = scale[d, 4 * k + c]
                        row[f"integral_scale_{kind}_truncated"] = bool(trunc[d, 4 * k + c])
                    row["resolved_lag"] = res[d, c]
                    row["resolved_distance_m"] = res[d, c] * float(delta_meter)
                    rows.append(row)
    return pd.DataFrame(rows)


def evaluate_scale_statistics(model, loader, config: dict, *, device: str = "cuda:0", max_lag: int = 32,
                              unobstructed: bool = False, per_level: bool = False, delta_meter: float = 5.0,
                              threshold: float = 0.5, return_sums: bool = False):
    """``optim_helper.evaluate`` for two-point statistics: a pandas.DataFrame with one row per (channel, direction,
    lag) -- ``distance_m``, ``pairs``, ``longitudinal`` (u along x, v along y, w along z), and for pred, truth and err
    ``S2_* .. S4_*`` (K or m/s to that power), ``skewness_*``, ``flatness_*``, ``rho_*``; ``variance_ratio`` (S2_pred /
    S2_truth), ``increment_correlation``, ``relative_error`` (S2_err / S2_truth); per (channel, direction), repeated on
    its rows, ``integral_scale_*_m`` with ``*_truncated`` and ``resolved_lag`` / ``resolved_distance_m`` (the smallest
    lag from which ``relative_error`` stays <= ``threshold``).  Levels are pooled, or one block per level with
    ``per_level``.  ``config['data']['stds']`` gives the units.  ``return_sums``: also the dict
    ``script/evaluate_scale_statistics.py --save_sums`` stores."""
    from .optim_helper import _device_batches
    stds = list(config["data"]["stds"])
    meter = ScaleStatisticsMeter()
    n = 0
    with torch.no_grad():
        for Xs, bs, ys in _device_batches(loader, device):
            preds = model(Xs, bs)
            meter.update(*ops.eval_scale_statistics(preds, ys, bs, max_lag=max_lag, unobstructed=unobstructed))
            n += len(Xs)
    sums, pairs = meter.result()
    logger.info(f"scale statistics over {n} samples: lags 1 .. {int(max_lag)}, "
                f"{'unobstructed pairs only' if unobstructed else 'pairs with both ends in the fluid'}, "
                f"{int(pairs[:, :, 0].sum())} pairs at lag 1")
    df = scale_statistics_table(sums, pairs, stds, delta_meter=delta_meter, per_level=per_level, threshold=threshold)
    if return_sums:
        return df, {"sums": sums, "pairs": pairs, "series": np.array(SERIES_NAMES),
                    "moments": np.array(sorted(_M, key=_M.get)), "directions": np.array(SCALE_DIRS),
                    "unobstructed": np.array(bool(unobstructed)), "delta_meter": np.array(float(delta_meter)),
                    "stds": np.array(stds, dtype=np.float64)}
    return df
