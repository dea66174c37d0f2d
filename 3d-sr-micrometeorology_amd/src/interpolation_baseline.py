"""The interpolation baseline the evaluation metrics are compared against: ``fill_na`` of the reference's plotting
notebooks (pytorch/notebook/plot_horizontal_sections_at_various_locations.ipynb and
plot_horizontal_vertical_section_at_fixed_location.ipynb, cell "Define methods").

The notebook upsamples the LR field trilinearly x4, blanks the cells of the nearest-upsampled LR building mask and fills
them with xarray's ``interpolate_na(method="linear", fill_value="extrapolate")`` along z, then y, then x.  Here all of
that is one call of the HIP kernels in csrc/sr3d_interp.hip (``ops.interp_baseline``).  The fill is pinned to scipy's
``interp1d`` on index coordinates with the values promoted to fp64, which is what xarray dispatches to; xarray itself
is not a dependency and parity with it is not pinned.

``InterpolationBaseline`` has the model's ``forward(Xs, bs)``, so ``optim_helper.evaluate``, ``write_out_inferences``
and script/make_2m_temperature.py take it in place of the network.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import ops


def _mask_tensor(lr_is_in_build) -> torch.Tensor:
    m = lr_is_in_build if isinstance(lr_is_in_build, torch.Tensor) else torch.from_numpy(np.asarray(lr_is_in_build))
    if m.dim() != 3:
        raise ValueError(f"lr_is_in_build must be (z, y, x) (got {tuple(m.shape)}): of the (4, Z, y, x) file the "
                         "LR-data script writes, pass [0, :z]")
    return (m != 0).to(torch.uint8)


def fill_na(xs: torch.Tensor, lr_is_in_build, scale: int = 4) -> torch.Tensor:
    """the notebook's function: ``xs`` (C, z, y, x) -> (C, scale*z, scale*y, scale*x) on the GPU, with the notebook's
    two asserts (some NaN before the fill, none after it)"""
    if xs.dim() != 4:
        raise ValueError(f"fill_na: xs must be (C, z, y, x) (got {tuple(xs.shape)})")
    dev = xs.device if xs.is_cuda else torch.device("cuda")
    mask = _mask_tensor(lr_is_in_build).to(dev)
    x = xs.detach().to(dev, torch.float32)
    assert bool(mask.any()) or bool(torch.isnan(x).any()), "No Nan values"
    with torch.no_grad():
        hr, n_unfilled = ops.interp_baseline(x[None], mask, scale)
    assert int(n_unfilled) == 0
    return hr[0]


class InterpolationBaseline(nn.Module):
    """``fill_na`` behind the network's signature: ``forward(Xs, bs)`` -> (B, C, Z, Y, X), ``bs`` unused.  No parameters;
    the mask travels with ``.to(device)``.  ``n_unfilled`` is the last call's count of cells still NaN, on the device
    (reading it synchronises; a forward does not)."""

    def __init__(self, lr_is_in_build, scale: int = 4):
        super().__init__()
        if scale not in ops.INTERP_SCALES:
            raise ValueError(f"scale {scale}: only {ops.INTERP_SCALES} are implemented")
        self.scale = int(scale)
        self.register_buffer("lr_is_in_build", _mask_tensor(lr_is_in_build), persistent=False)
        self.n_unfilled = None

    def forward(self, Xs: torch.Tensor, bs: torch.Tensor = None) -> torch.Tensor:
        with torch.no_grad():
            hr, self.n_unfilled = ops.interp_baseline(Xs, self.lr_is_in_build, self.scale)
        return hr
