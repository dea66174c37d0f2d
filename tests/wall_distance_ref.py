"""Restatement of the wall-distance-resolved evaluation (include/sr3d.h: sr3d_wall_distance,
sr3d_eval_wall_distance_profiles) in plain torch.  The distance is the number of 3 x 3 x 3 max-pools of the built cells
(``1 - b > 0``, zero padding) it takes to reach a cell, capped at cap + 1; the per-voxel terms are built from the
oracle's own pieces exactly as tests/level_profiles_ref.py takes them, then summed per distance bin instead of per
level.  Runs in the dtype of its inputs: fp64 inputs give the reference values the GPU tests compare against.

It also makes the cases, on B = 2 and (Z, Y, X) = (19, 23, 67): one full and one partial 8 x 62 x 16 tile or more on
every axis, and distances that cross tile edges."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import tower_mask
from level_profiles_ref import INTERIOR, PROFILES, QUANT, STDS
from oracle import ref_cpu as R

SHAPE = (2, 19, 23, 67)               # B, Z, Y, X
CASES = ("tower", "sparse", "fractional", "mixed", "iid", "one_cell", "all_fluid")
GOLDEN_CASES = ("tower", "sparse", "fractional")      # the reference's own masks and module values are stored for these
GOLDEN_WIDTHS = (1, 2, 3, 5, 8, 12)
SUMS = ("abs", "sq", "sq_T", "sq_U", "sq_V", "sq_W", "mask", "mask_abs", "mask_sq", "pos", "pos_abs", "pos_sq",
        "mask_dT", "mask_dV", "mask_int", "near_int", "res_p", "res_t", "ddiv", "omega", "cells")
COUNTS = ("cells", "pos", "mask", "mask_int", "near_int")
assert PROFILES[4:6] == ("MaskedL1NearWall", "MaskedL2NearWall")


def wall_distance_ref(b, cap):
    """uint8 tensor shaped like b: 0 where 1 - b > 0, else min(Chebyshev distance to the nearest such cell, cap + 1)"""
    reach = (1.0 - b.float() > 0).float()
    dist = torch.full(b.shape, cap + 1, dtype=torch.uint8)
    dist[reach > 0] = 0
    for k in range(1, cap + 1):
        grown = F.max_pool3d(reach, 3, 1, 1)
        dist[(grown > 0) & (reach == 0)] = k
        if bool((grown == reach).all()):
            break
        reach = grown
    return dist


def near_wall_ref(b, n):
    """calc_mask_near_build_wall(b, num_filter_applications=n) as the Chebyshev dilation"""
    cap = min(n, 254)
    return ((wall_distance_ref(b, cap) <= cap) & (b > 0)).float()


def voxel_terms(p, t, b, stds, delta=5.0):
    """{name in SUMS: (B, Z, Y, X) tensor}: what a voxel adds to every sum (channels already added up)"""
    d = p - t
    ad, sq = d.abs(), d ** 2
    pos = (b > 0).to(p.dtype)
    ch = lambda f: f.sum(dim=1)     # noqa: E731
    T = {"abs": ch(ad), "sq": ch(sq), "mask": ch(b), "pos": ch(pos), "mask_abs": ch(b * ad), "mask_sq": ch(b * sq),
         "pos_abs": ch(pos * ad), "pos_sq": ch(pos * sq), "cells": torch.ones_like(b[:, 0])}
    for c, n in enumerate("TUVW"):
        T[f"sq_{n}"] = sq[:, c]
    sc = torch.tensor(list(stds[1:]), dtype=torch.float32)[None, :, None, None, None]
    T["mask_dV"] = ch(b * torch.linalg.norm(p[:, 1:] * sc - t[:, 1:] * sc, dim=1, keepdim=True))
    T["mask_dT"] = ch(b * (p[:, 0:1] - t[:, 0:1]).abs() * stds[0])

    def whole(f):       # an interior field (voxels 1 .. n-2) on the whole grid; empty when an axis has no interior
        out = torch.zeros_like(b[:, 0])
        if min(b.shape[2:]) > 2:
            out[:, 1:-1, 1:-1, 1:-1] = ch(f)
        return out

    near = R.near_wall_mask(b)
    T["mask_int"], T["near_int"] = whole(b[..., 1:-1, 1:-1, 1:-1]), whole(near[..., 1:-1, 1:-1, 1:-1])
    if min(b.shape[2:]) > 2:
        rp, _ = R._interior_masked(R.divergence, b, p, stds[1:], delta)
        rt, _ = R._interior_masked(R.divergence, b, t, stds[1:], delta)
        op, _ = R._interior_masked(R.vorticity, b, p, stds[1:], delta)
        ot, _ = R._interior_masked(R.vorticity, b, t, stds[1:], delta)
        T["res_p"], T["res_t"], T["ddiv"] = whole(rp.abs()), whole(rt.abs()), whole((rp - rt).abs())
        T["omega"] = whole(torch.linalg.norm(op - ot, dim=1, keepdim=True))
    else:
        for k in ("res_p", "res_t", "ddiv", "omega"):
            T[k] = torch.zeros_like(b[:, 0])
    assert set(T) == set(SUMS)
    return T


def bin_sums(terms, dist, D):
    """{name: (D + 2,) tensor}: bin 0 is dist == 0, k is dist == k, D + 1 is dist > D"""
    bins = dist[:, 0].long().clamp(max=D + 1).flatten()
    return {k: torch.zeros(D + 2, dtype=f.dtype).index_add_(0, bins, f.flatten()) for k, f in terms.items()}


def ratios(S, eps=1e-30):
    """{name in PROFILES: (D + 2,) tensor} from the per-bin sums; the near-wall rows are cumulative"""
    n_grid = S["mask_int"] - S["near_int"]
    cum = {k: torch.cumsum(S[k], 0) for k in ("pos", "pos_abs", "pos_sq")}
    V = {"L1": S["abs"] / (4 * S["cells"]), "L2": S["sq"] / (4 * S["cells"]),
         "MaskedL1": S["mask_abs"] / (4 * S["mask"] + eps), "MaskedL2": S["mask_sq"] / (4 * S["mask"] + eps),
         "MaskedL1NearWall": cum["pos_abs"] / (4 * cum["pos"] + eps),
         "MaskedL2NearWall": cum["pos_sq"] / (4 * cum["pos"] + eps),
         "ResidualContinuity": S["res_p"] / n_grid, "ResidualContinuityTarget": S["res_t"] / n_grid,
         "AbsDiffDivergence": S["ddiv"] / n_grid, "DiffOmegaNorm": S["omega"] / n_grid,
         "AbsDiffTemperature": S["mask_dT"] / (S["mask"] + eps), "DiffVelocityNorm": S["mask_dV"] / (S["mask"] + eps)}
    for n in "TUVW":
        V[f"ChannelwiseMse{n}"] = S[f"sq_{n}"] / S["cells"]
    assert set(V) == set(PROFILES)
    return V


def wall_distance_profiles_ref(p, t, b, stds, delta=5.0, D=8, dist=None):
    """(values, sums) over the whole batch: {name: (D + 2,) tensor} each"""
    dist = wall_distance_ref(b, D) if dist is None else dist
    S = bin_sums(voxel_terms(p, t, b, stds, delta), dist, D)
    return ratios(S), S


# ---- the cases ----------------------------------------------------------------------------------------------------
def make_inputs(seed=20261018):
    """what tests/make_wall_distance_golden.py stores: two U[0,1) fields as uint16 multiples of 1 / QUANT, the sparse
    mask (0.2 % built), the cells of it that the fractional case sets to 0.5 (about 0.1 %) and the iid mask (20 %
    built), the masks packed to bits"""
    B, Z, Y, X = SHAPE
    rng = np.random.default_rng(seed)
    p = rng.integers(0, QUANT, size=(B, 4, Z, Y, X), dtype=np.uint16)
    t = rng.integers(0, QUANT, size=(B, 4, Z, Y, X), dtype=np.uint16)
    sparse = rng.random((B, 1, Z, Y, X)) > 0.002
    half = rng.random((B, 1, Z, Y, X)) < 0.001
    iid = rng.random((B, 1, Z, Y, X)) > 0.2
    return {"p_u16": p, "t_u16": t, "mask/sparse_bits": np.packbits(sparse), "mask/half_bits": np.packbits(half),
            "mask/iid_bits": np.packbits(iid)}


def unpack(bits, shape=None):
    shape = (SHAPE[0], 1) + SHAPE[1:] if shape is None else shape
    return torch.from_numpy(np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(np.float32))


def case(gold, kind):
    """(p, t, b) fp32 CPU tensors"""
    B, Z, Y, X = SHAPE
    p = torch.from_numpy(gold["p_u16"].astype(np.float32) / QUANT)
    t = torch.from_numpy(gold["t_u16"].astype(np.float32) / QUANT)
    tower = tower_mask(Z, Y, X).repeat(B, 1, 1, 1, 1)
    sparse = unpack(gold["mask/sparse_bits"])
    if kind == "tower":
        b = tower
    elif kind == "sparse":
        b = sparse
    elif kind == "fractional":
        b = torch.where(unpack(gold["mask/half_bits"]) > 0, torch.tensor(0.5), sparse)
    elif kind == "mixed":           # a per-sample indexing slip in dist shows here
        b = torch.cat([tower[:1], sparse[1:]])
    elif kind == "iid":             # only bins 0 .. 2 are populated
        b = unpack(gold["mask/iid_bits"])
    elif kind == "one_cell":
        b = torch.ones(B, 1, Z, Y, X)
        b[:, :, 0, 11, 33] = 0
    elif kind == "all_fluid":
        b = torch.ones(B, 1, Z, Y, X)
    else:
        raise KeyError(kind)
    return p, t, b
