"""Restatement of the height-resolved evaluation (include/sr3d.h: sr3d_eval_level_profiles) in plain torch, built from
the oracle's own pieces (oracle.ref_cpu: near_wall_mask, divergence, vorticity, _interior_masked, central_diff): the
field of every metric is summed over (batch, channel, y, x) per level, the interior fields (voxels 1 .. n-2) map to
levels 1 .. Z-2, and the ratios are the modules' formulas with numerator and denominator restricted to one level.
Runs in the dtype of its inputs: fp64 inputs give the reference values the GPU tests compare against."""
import numpy as np
import torch

from helpers import tower_mask
from oracle import ref_cpu as R

STDS = [8.4, 14.4, 21.6, 7.0]
RAGGED = (2, 19, 11, 67)              # B, Z, Y, X: one full and one partial 8 x 62 x 16 tile on every axis
QUANT = 4096                          # the golden file stores the U[0,1) fields as uint16 multiples of 1 / 4096
PROFILES = ("L1", "L2", "MaskedL1", "MaskedL2", "MaskedL1NearWall", "MaskedL2NearWall", "ResidualContinuity",
            "ResidualContinuityTarget", "AbsDiffTemperature", "DiffVelocityNorm", "AbsDiffDivergence", "DiffOmegaNorm",
            "ChannelwiseMseT", "ChannelwiseMseU", "ChannelwiseMseV", "ChannelwiseMseW")
INTERIOR = ("ResidualContinuity", "ResidualContinuityTarget", "AbsDiffDivergence", "DiffOmegaNorm")
SUMS = ("abs", "sq", "sq_T", "sq_U", "sq_V", "sq_W", "mask", "mask_abs", "mask_sq", "near", "near_abs", "near_sq",
        "mask_dT", "mask_dV", "mask_int", "near_int", "res_p", "res_t", "ddiv", "omega")


def _per_level(f):
    return f.sum(dim=(0, 1, 3, 4))


def _interior_per_level(f, Z):
    """f lives on z = 1 .. Z-2 (empty when an axis has no interior)"""
    out = torch.zeros(Z, dtype=f.dtype)
    if Z > 2:
        out[1:Z - 1] = _per_level(f)
    return out


def level_sums(p, t, b, stds, delta=5.0):
    """{name in SUMS: (Z,) tensor}"""
    Z = p.shape[2]
    d = p - t
    ad, sq = d.abs(), d ** 2
    near = R.near_wall_mask(b)
    S = {"abs": _per_level(ad), "sq": _per_level(sq), "mask": _per_level(b), "near": _per_level(near),
         "mask_abs": _per_level(b * ad), "mask_sq": _per_level(b * sq),
         "near_abs": _per_level(near * ad), "near_sq": _per_level(near * sq)}
    for c, n in enumerate("TUVW"):
        S[f"sq_{n}"] = _per_level(sq[:, c:c + 1])
    sc = torch.tensor(list(stds[1:]), dtype=torch.float32)[None, :, None, None, None]
    dv = torch.linalg.norm(p[:, 1:] * sc - t[:, 1:] * sc, dim=1, keepdim=True)
    dT = (p[:, 0:1] - t[:, 0:1]).abs() * stds[0]
    S["mask_dT"], S["mask_dV"] = _per_level(b * dT), _per_level(b * dv)
    S["mask_int"] = _interior_per_level(b[..., 1:-1, 1:-1, 1:-1], Z)
    S["near_int"] = _interior_per_level(near[..., 1:-1, 1:-1, 1:-1], Z)
    rp, _ = R._interior_masked(R.divergence, b, p, stds[1:], delta)
    rt, _ = R._interior_masked(R.divergence, b, t, stds[1:], delta)
    op, _ = R._interior_masked(R.vorticity, b, p, stds[1:], delta)
    ot, _ = R._interior_masked(R.vorticity, b, t, stds[1:], delta)
    S["res_p"], S["res_t"] = _interior_per_level(rp.abs(), Z), _interior_per_level(rt.abs(), Z)
    S["ddiv"] = _interior_per_level((rp - rt).abs(), Z)
    S["omega"] = _interior_per_level(torch.linalg.norm(op - ot, dim=1, keepdim=True), Z)
    assert set(S) == set(SUMS)
    return S


def ratios(S, cells, eps=1e-30):
    """{name in PROFILES: (Z,) tensor} from the per-level sums and the number of (sample, y, x) cells of a level"""
    n_grid = S["mask_int"] - S["near_int"]
    V = {"L1": S["abs"] / (4 * cells), "L2": S["sq"] / (4 * cells),
         "MaskedL1": S["mask_abs"] / (4 * S["mask"] + eps), "MaskedL2": S["mask_sq"] / (4 * S["mask"] + eps),
         "MaskedL1NearWall": S["near_abs"] / (4 * S["near"] + eps),
         "MaskedL2NearWall": S["near_sq"] / (4 * S["near"] + eps),
         "ResidualContinuity": S["res_p"] / n_grid, "ResidualContinuityTarget": S["res_t"] / n_grid,
         "AbsDiffDivergence": S["ddiv"] / n_grid, "DiffOmegaNorm": S["omega"] / n_grid,
         "AbsDiffTemperature": S["mask_dT"] / (S["mask"] + eps), "DiffVelocityNorm": S["mask_dV"] / (S["mask"] + eps)}
    for n in "TUVW":
        V[f"ChannelwiseMse{n}"] = S[f"sq_{n}"] / cells
    assert set(V) == set(PROFILES)
    return V


def level_profiles_ref(p, t, b, stds, delta=5.0):
    """(values, sums) over the whole batch: {name: (Z,) tensor} each"""
    S = level_sums(p, t, b, stds, delta)
    return ratios(S, p.shape[0] * p.shape[3] * p.shape[4]), S


# ---- the ragged case of the golden file --------------------------------------------------------------------------
def make_ragged_inputs(seed=20261017):
    """what tests/make_level_profiles_golden.py stores: two U[0,1) fields as uint16 multiples of 1 / QUANT and an iid
    mask with 20 % of the cells built, packed to bits"""
    B, Z, Y, X = RAGGED
    rng = np.random.default_rng(seed)
    p = rng.integers(0, QUANT, size=(B, 4, Z, Y, X), dtype=np.uint16)
    t = rng.integers(0, QUANT, size=(B, 4, Z, Y, X), dtype=np.uint16)
    fluid = rng.random((B, 1, Z, Y, X)) > 0.2
    return p, t, np.packbits(fluid)


def ragged_case(gold, kind):
    """(p, t, b) fp32 CPU tensors of the ragged case with the golden file's iid mask or the tower mask"""
    B, Z, Y, X = RAGGED
    p = torch.from_numpy(gold["ragged/p_u16"].astype(np.float32) / QUANT)
    t = torch.from_numpy(gold["ragged/t_u16"].astype(np.float32) / QUANT)
    if kind == "iid":
        n = B * Z * Y * X
        b = torch.from_numpy(np.unpackbits(gold["ragged/fluid_bits"])[:n].reshape(B, 1, Z, Y, X).astype(np.float32))
    else:
        b = tower_mask(Z, Y, X).repeat(B, 1, 1, 1, 1)
    return p, t, b
