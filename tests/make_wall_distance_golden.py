"""Generate tests/golden/wall_distance.npz (build machine only; never run on the GPU box, never collected by pytest).

    python tests/make_wall_distance_golden.py

It imports the reference's own ``calc_mask_near_build_wall``, ``MaskedL1LossNearWall`` and ``MaskedL2LossNearWall``
(read-only, no bytecode written; ``SR3D_REFERENCE`` names the reference's pytorch directory) and evaluates them with
``num_filter_applications = n`` for n in 1, 2, 3, 5, 8, 12 on the tower, sparse and fractional cases of
tests/wall_distance_ref.py (B = 2, (Z, Y, X) = (19, 23, 67)).  Only data is stored:
    p_u16, t_u16                       the two U[0,1) fields as uint16 multiples of 1 / 4096 (exact in fp32)
    mask/sparse_bits, half_bits, iid_bits      the seeded masks, packed to bits (1 = fluid; half: the 0.5 cells)
    near/<kind>/<n>                    calc_mask_near_build_wall(b, n), packed to bits
    module/<kind>/<n>                  [MaskedL1LossNearWall(n), MaskedL2LossNearWall(n)](p, t, b), float32
    stds                               the scales of the restatement
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SR3D_REFERENCE", "/root/reference/pytorch")
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.loss_maker import MaskedL1LossNearWall, MaskedL2LossNearWall, calc_mask_near_build_wall  # noqa: E402  (the reference's)

import wall_distance_ref as WR  # noqa: E402


def main():
    g = WR.make_inputs()
    g["stds"] = np.asarray(WR.STDS, dtype=np.float64)
    for kind in WR.GOLDEN_CASES:
        p, t, b = WR.case(g, kind)
        for n in WR.GOLDEN_WIDTHS:
            with torch.no_grad():
                near = calc_mask_near_build_wall(b, n)
                assert set(near.unique().tolist()) <= {0.0, 1.0}
                g[f"near/{kind}/{n}"] = np.packbits(near.numpy() > 0)
                g[f"module/{kind}/{n}"] = np.array([float(MaskedL1LossNearWall(num_filter_applications=n)(p, t, b)),
                                                    float(MaskedL2LossNearWall(num_filter_applications=n)(p, t, b))],
                                                   dtype=np.float32)
    # what the GPU tests rely on: at D = 8 every bin of tower and sparse is populated, and every bin where M = b (1 -
    # near_1) can be non-zero (2 .. 9) holds interior cells with M = 1
    for kind in ("tower", "sparse"):
        p, t, b = WR.case(g, kind)
        _, S = WR.wall_distance_profiles_ref(p.double(), t.double(), b.double(), WR.STDS, D=8)
        assert bool((S["cells"] > 0).all()), (kind, S["cells"])
        n_grid = S["mask_int"] - S["near_int"]
        assert bool((n_grid[:2] == 0).all()) and bool((n_grid[2:] > 0).all()), (kind, n_grid)
        print(kind, "cells per bin", S["cells"].long().tolist(), "interior M cells", n_grid.long().tolist())
    for kind, lo in (("tower", 14), ("sparse", 12)):
        cells = torch.bincount(WR.wall_distance_ref(WR.case(g, kind)[2], 12).flatten().long(), minlength=14)
        assert bool((cells[:lo] > 0).all()), (kind, cells)
        print(kind, "cells per distance at cap 12", cells.tolist())
    out = os.path.join(HERE, "golden", "wall_distance.npz")
    np.savez_compressed(out, **g)
    print("wrote", out, os.path.getsize(out), "bytes")
    for k, v in g.items():
        if k.startswith("module/"):
            print(k, v)


if __name__ == "__main__":
    main()
