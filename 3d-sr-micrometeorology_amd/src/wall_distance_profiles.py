"""Wall-distance-resolved evaluation (engine extension; the reference offers the near-wall modules at one width per
pass).  Every metric of the final evaluation per class of Chebyshev distance from the nearest building, from ONE fused
pass per batch (``ops.eval_wall_distance_profiles``, csrc/sr3d_walldist.hip): bin 0 holds the built cells, bin k the
cells k cells away from a building, bin D + 1 everything farther than D = ``max_distance``.  The modules' formulas are
restricted to the bin in numerator and denominator alike; ``MaskedL1NearWall`` / ``MaskedL2NearWall`` are cumulative
over the bins 0 .. k, which makes them the reference's modules with ``num_filter_applications=k``.

``WallDistanceProfileMeter`` averages over a loader exactly as ``optim_helper.AverageMeter`` does per metric; the
``pooled`` variant divides the summed numerators by the summed denominators instead (the cumulative rows re-derived
from the summed sums), which stays finite where a single batch had an empty bin."""
import typing
from logging import getLogger

import numpy as np
import torch

from .. import ops
from .._lib import WALLDIST_COUNT, WALLDIST_INDEX, WALLDIST_SUM_COUNT, WALLDIST_SUM_INDEX

logger = getLogger()

WALL_DISTANCE_PROFILE_NAMES: typing.Tuple[str, ...] = tuple(sorted(WALLDIST_INDEX, key=WALLDIST_INDEX.get))
COUNT_COLUMNS = ("Cells", "FluidCells", "InteriorCells")
EPS = 1e-30     # the modules' default


def calc_wall_distance_profiles(predicts: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor,
                                stds: typing.Sequence[typing.Optional[float]], delta_meter: float = 5.0,
                                max_distance: int = 8, dist: typing.Optional[torch.Tensor] = None
                                ) -> typing.Dict[str, torch.Tensor]:
    """{profile name: (max_distance + 2,) tensor on the device} over the whole batch"""
    values, _ = ops.eval_wall_distance_profiles(predicts, targets, masks, stds, delta_meter, max_distance, dist)
    return {name: values[i] for name, i in WALLDIST_INDEX.items()}


def pooled_profiles(sums: np.ndarray) -> np.ndarray:
    """the ratios of ``sr3d_eval_wall_distance_profiles`` from summed raw sums ((WALLDIST_SUM_COUNT, D + 2), fp64):
    (WALLDIST_COUNT, D + 2)"""
    s = {k: np.asarray(sums[i], dtype=np.float64) for k, i in WALLDIST_SUM_INDEX.items()}
    out = np.empty((WALLDIST_COUNT, sums.shape[-1]), dtype=np.float64)
    P = WALLDIST_INDEX
    with np.errstate(divide="ignore", invalid="ignore"):
        out[P["L1"]], out[P["L2"]] = s["abs"] / (4.0 * s["cells"]), s["sq"] / (4.0 * s["cells"])
        out[P["MaskedL1"]], out[P["MaskedL2"]] = s["mask_abs"] / (4.0 * s["mask"] + EPS), s["mask_sq"] / (4.0 * s["mask"] + EPS)
        pos = np.cumsum(s["pos"])
        out[P["MaskedL1NearWall"]] = np.cumsum(s["pos_abs"]) / (4.0 * pos + EPS)
        out[P["MaskedL2NearWall"]] = np.cumsum(s["pos_sq"]) / (4.0 * pos + EPS)
        n_grid = s["mask_int"] - s["near_int"]
        for name, key in (("ResidualContinuity", "res_p"), ("ResidualContinuityTarget", "res_t"),
                          ("AbsDiffDivergence", "ddiv"), ("DiffOmegaNorm", "omega")):
            out[P[name]] = s[key] / n_grid
        out[P["AbsDiffTemperature"]] = s["mask_dT"] / (s["mask"] + EPS)
        out[P["DiffVelocityNorm"]] = s["mask_dV"] / (s["mask"] + EPS)
        for c in "TUVW":
            out[P[f"ChannelwiseMse{c}"]] = s[f"sq_{c}"] / s["cells"]
    return out


class WallDistanceProfileMeter:
    """running per-distance profiles over a loader; everything stays on the device until ``result()``'s one copy"""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.weighted, self.sums = None, None    # fp64 on the device: sum of values * n, sum of the raw sums
        self.count = 0                           # samples

    def update(self, values: torch.Tensor, sums: torch.Tensor, n: int) -> None:
        """``values``, ``sums``: what ``ops.eval_wall_distance_profiles`` returned for a batch of ``n`` samples"""
        if tuple(values.shape[:-1]) != (WALLDIST_COUNT,) or tuple(sums.shape[:-1]) != (WALLDIST_SUM_COUNT,):
            raise ValueError("WallDistanceProfileMeter takes the outputs of ops.eval_wall_distance_profiles")
        if self.weighted is None:
            self.weighted, self.sums = torch.zeros_like(values, dtype=torch.float64), torch.zeros_like(sums, dtype=torch.float64)
        elif self.weighted.shape != values.shape:
            raise ValueError(f"the number of bins changed: {self.weighted.shape[-1]} -> {values.shape[-1]}")
        self.weighted += values.double() * n
        self.sums += sums.double()
        self.count += int(n)

    def result(self, pooled: bool = False) -> typing.Tuple[np.ndarray, np.ndarray]:
        """(profiles (WALLDIST_COUNT, D + 2), raw sums (WALLDIST_SUM_COUNT, D + 2)) as fp64 host arrays.
        ``pooled=False``: the sample-weighted mean of the per-batch values (``AverageMeter``; NaN where any batch had
        an empty bin); ``pooled=True``: ratio of the summed sums"""
        if self.weighted is None:
            raise RuntimeError("WallDistanceProfileMeter.result() before any update()")
        both = torch.cat([self.weighted, self.sums], dim=0).cpu().numpy()      # the one device -> host copy
        weighted, sums = both[:WALLDIST_COUNT], both[WALLDIST_COUNT:]
        return (pooled_profiles(sums) if pooled else weighted / self.count), sums


def evaluate_wall_distance_profiles(*, dataloader, model, stds: typing.Sequence[typing.Optional[float]], device: str,
                                    max_distance: int = 8, delta_meter: float = 5.0, pooled: bool = False):
    """``optim_helper.evaluate`` per distance class: a pandas.DataFrame with one row per bin and one column per
    profile (``WALL_DISTANCE_PROFILE_NAMES``), plus ``distance_cells``, ``distance_m`` (= k * delta_meter; ``inf`` for
    the last bin, the cells farther than ``max_distance``) and the cell counts ``Cells``, ``FluidCells``,
    ``InteriorCells`` (interior cells that are fluid and not next to a wall: the denominator of the divergence /
    vorticity profiles) summed over the loader"""
    import pandas as pd

    from .optim_helper import _device_batches
    meter = WallDistanceProfileMeter()
    with torch.no_grad():
        for Xs, bs, ys in _device_batches(dataloader, device):
            preds = model(Xs, bs)
            values, sums = ops.eval_wall_distance_profiles(preds, ys, bs, stds, delta_meter, max_distance)
            meter.update(values, sums, n=len(Xs))
    profiles, sums = meter.result(pooled=pooled)
    nb = profiles.shape[-1]
    S = WALLDIST_SUM_INDEX
    meters = np.arange(nb, dtype=np.float64) * float(delta_meter)
    meters[-1] = np.inf
    cols = {"distance_cells": np.arange(nb), "distance_m": meters}
    cols.update({name: profiles[WALLDIST_INDEX[name]] for name in WALL_DISTANCE_PROFILE_NAMES})
    cols.update(Cells=sums[S["cells"]], FluidCells=sums[S["mask"]], InteriorCells=sums[S["mask_int"]] - sums[S["near_int"]])
    logger.info(f"wall-distance profiles over {meter.count} samples, {nb} bins ({'pooled' if pooled else 'batch-averaged'})")
    return pd.DataFrame(cols)
