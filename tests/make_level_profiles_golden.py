"""Generate tests/golden/level_profiles.npz (build machine only; never run on the GPU box, never collected by pytest).

    python tests/make_level_profiles_golden.py

It imports the reference's own ``AbsDiffTemperature`` and ``DiffVelocityVectorNorm`` (read-only, no bytecode written;
``SR3D_REFERENCE`` names the reference's pytorch directory) and evaluates them with ``lev=k`` for every level k of the
ragged case of tests/level_profiles_ref.py (B = 2, (Z, Y, X) = (19, 11, 67)), once with the iid mask and once with
the tower mask.  Only data is stored:
    ragged/p_u16, ragged/t_u16   the two U[0,1) fields as uint16 multiples of 1 / 4096 (exact in fp32)
    ragged/fluid_bits            the iid mask (1 = fluid, 20 % built), packed to bits
    ragged/<kind>/AbsDiffTemperature, ragged/<kind>/DiffVelocityNorm     (Z,) float32: the modules' values, lev = 0 .. Z-1
    stds                         the scales the modules were built with
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

from src.loss_maker import AbsDiffTemperature, DiffVelocityVectorNorm  # noqa: E402  (the reference's)

import level_profiles_ref as LR  # noqa: E402


def main():
    p16, t16, bits = LR.make_ragged_inputs()
    g = {"ragged/p_u16": p16, "ragged/t_u16": t16, "ragged/fluid_bits": bits,
         "stds": np.asarray(LR.STDS, dtype=np.float64)}
    Z = LR.RAGGED[1]
    for kind in ("iid", "tower"):
        p, t, b = LR.ragged_case(g, kind)
        with torch.no_grad():
            g[f"ragged/{kind}/AbsDiffTemperature"] = np.array(
                [float(AbsDiffTemperature(LR.STDS[0], lev=k)(p, t, b)) for k in range(Z)], dtype=np.float32)
            g[f"ragged/{kind}/DiffVelocityNorm"] = np.array(
                [float(DiffVelocityVectorNorm(LR.STDS[1:], lev=k)(p, t, b)) for k in range(Z)], dtype=np.float32)
        assert 0.15 < 1.0 - float(b.mean()) < 0.25 or kind == "tower"
    out = os.path.join(HERE, "golden", "level_profiles.npz")
    np.savez_compressed(out, **g)
    print("wrote", out, os.path.getsize(out), "bytes")
    for k, v in g.items():
        if k.count("/") == 2:
            print(k, v[:4], "...")


if __name__ == "__main__":
    main()
