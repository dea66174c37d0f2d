"""Height-resolved evaluation (engine extension; the reference offers ``AbsDiffTemperature(lev=k)`` and
``DiffVelocityVectorNorm(lev=k)`` only: one level and two metrics per pass).  Every metric of the final evaluation as
a vertical profile, from ONE fused pass per batch (``ops.eval_level_profiles``, csrc/sr3d_eval_profile.hip): the
modules' formulas restricted to z == k in numerator and denominator alike.

``LevelProfileMeter`` averages over a loader exactly as ``optim_helper.AverageMeter`` does per metric (sum of value *
batch size over the number of samples), so its ``AbsDiffTemperature`` at level k is what ``optim_helper.evaluate``
reports for ``AbsDiffTemperature(lev=k)``; the ``pooled`` variant divides the summed numerators by the summed
denominators instead, which stays finite where a single batch had an empty level."""
import typing
from logging import getLogger

import numpy as np
import torch

from .. import ops
from .._lib import PROFILE_COUNT, PROFILE_INDEX, PROFILE_SUM_COUNT, PROFILE_SUM_INDEX

logger = getLogger()

LEVEL_PROFILE_NAMES: typing.Tuple[str, ...] = tuple(sorted(PROFILE_INDEX, key=PROFILE_INDEX.get))
COUNT_COLUMNS = ("FluidCells", "NearWallCells", "InteriorCells")
EPS = 1e-30     # the modules' default


def calc_level_profiles(predicts: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor,
                        stds: typing.Sequence[typing.Optional[float]], delta_meter: float = 5.0
                        ) -> typing.Dict[str, torch.Tensor]:
    """{profile name: (Z,) tensor on the device} over the whole batch, as the reference's modules would see it"""
    values, _ = ops.eval_level_profiles(predicts, targets, masks, stds, delta_meter)
    return {name: values[i] for name, i in PROFILE_INDEX.items()}


def pooled_profiles(sums: np.ndarray, cells_per_level: float) -> np.ndarray:
    """the ratios of ``sr3d_eval_level_profiles`` from summed raw sums ((PROFILE_SUM_COUNT, Z), fp64) and the number
    of (sample, y, x) cells per level: (PROFILE_COUNT, Z)"""
    s = {k: np.asarray(sums[i], dtype=np.float64) for k, i in PROFILE_SUM_INDEX.items()}
    out = np.empty((PROFILE_COUNT, sums.shape[-1]), dtype=np.float64)
    P = PROFILE_INDEX
    with np.errstate(divide="ignore", invalid="ignore"):
        out[P["L1"]], out[P["L2"]] = s["abs"] / (4.0 * cells_per_level), s["sq"] / (4.0 * cells_per_level)
        out[P["MaskedL1"]], out[P["MaskedL2"]] = s["mask_abs"] / (4.0 * s["mask"] + EPS), s["mask_sq"] / (4.0 * s["mask"] + EPS)
        out[P["MaskedL1NearWall"]] = s["near_abs"] / (4.0 * s["near"] + EPS)
        out[P["MaskedL2NearWall"]] = s["near_sq"] / (4.0 * s["near"] + EPS)
        n_grid = s["mask_int"] - s["near_int"]
        for name, key in (("ResidualContinuity", "res_p"), ("ResidualContinuityTarget", "res_t"),
                          ("AbsDiffDivergence", "ddiv"), ("DiffOmegaNorm", "omega")):
            out[P[name]] = s[key] / n_grid
        out[P["AbsDiffTemperature"]] = s["mask_dT"] / (s["mask"] + EPS)
        out[P["DiffVelocityNorm"]] = s["mask_dV"] / (s["mask"] + EPS)
        for c in "TUVW":
            out[P[f"ChannelwiseMse{c}"]] = s[f"sq_{c}"] / cells_per_level
    return out


class LevelProfileMeter:
    """running vertical profiles over a loader; everything stays on the device until ``result()``'s one copy"""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.weighted, self.sums = None, None    # fp64 on the device: sum of values * n, sum of the raw sums
        self.count, self.cells = 0, 0            # samples, (sample, y, x) cells per level: known on the host

    def update(self, values: torch.Tensor, sums: torch.Tensor, n: int, cells: int) -> None:
        """``values``, ``sums``: what ``ops.eval_level_profiles`` returned for a batch of ``n`` samples with ``cells``
        = n * Y * X cells per level"""
        if tuple(values.shape[:-1]) != (PROFILE_COUNT,) or tuple(sums.shape[:-1]) != (PROFILE_SUM_COUNT,):
            raise ValueError("LevelProfileMeter takes the whole-batch outputs of ops.eval_level_profiles")
        if self.weighted is None:
            self.weighted, self.sums = torch.zeros_like(values, dtype=torch.float64), torch.zeros_like(sums, dtype=torch.float64)
        elif self.weighted.shape != values.shape:
            raise ValueError(f"the number of levels changed: {self.weighted.shape[-1]} -> {values.shape[-1]}")
        self.weighted += values.double() * n
        self.sums += sums.double()
        self.count += int(n)
        self.cells += int(cells)

    def result(self, pooled: bool = False) -> typing.Tuple[np.ndarray, np.ndarray]:
        """(profiles (PROFILE_COUNT, Z), raw sums (PROFILE_SUM_COUNT, Z)) as fp64 host arrays.  ``pooled=False``: the
        sample-weighted mean of the per-batch values (``AverageMeter``); ``pooled=True``: ratio of the summed sums"""
        if self.weighted is None:
            raise RuntimeError("LevelProfileMeter.result() before any update()")
        both = torch.cat([self.weighted, self.sums], dim=0).cpu().numpy()      # the one device -> host copy
        weighted, sums = both[:PROFILE_COUNT], both[PROFILE_COUNT:]
        return (pooled_profiles(sums, float(self.cells)) if pooled else weighted / self.count), sums


def evaluate_level_profiles(*, dataloader, model, stds: typing.Sequence[typing.Optional[float]], device: str,
                            delta_meter: float = 5.0, pooled: bool = False):
    """``optim_helper.evaluate`` for vertical profiles: a pandas.DataFrame with one row per level and one column per
    profile (``LEVEL_PROFILE_NAMES``), plus ``level``, ``height_m`` (``ops.surface_heights``) and the cell counts
    ``FluidCells``, ``NearWallCells``, ``InteriorCells`` (interior cells that are fluid and not next to a wall: the
    denominator of the divergence / vorticity profiles) summed over the loader"""
    import pandas as pd

    from .optim_helper import _device_batches
    meter = LevelProfileMeter()
    with torch.no_grad():
        for Xs, bs, ys in _device_batches(dataloader, device):
            preds = model(Xs, bs)
            values, sums = ops.eval_level_profiles(preds, ys, bs, stds, delta_meter)
            meter.update(values, sums, n=len(Xs), cells=len(Xs) * ys.shape[-2] * ys.shape[-1])
    profiles, sums = meter.result(pooled=pooled)
    Z = profiles.shape[-1]
    S = PROFILE_SUM_INDEX
    cols = {"level": np.arange(Z), "height_m": np.array(list(ops.surface_heights(Z)), dtype=np.float64)}
    cols.update({name: profiles[PROFILE_INDEX[name]] for name in LEVEL_PROFILE_NAMES})
    cols.update(FluidCells=sums[S["mask"]], NearWallCells=sums[S["near"]],
                InteriorCells=sums[S["mask_int"]] - sums[S["near_int"]])
    logger.info(f"vertical profiles over {meter.count} samples, {Z} levels ({'pooled' if pooled else 'batch-averaged'})")
    return pd.DataFrame(cols)
