"""Generate tests/golden/equivariance*.npz from the reference's equivariance_error_calculator (build machine only).

Run from anywhere:   python tools/make_golden_equivariance.py
Like oracle/make_golden.py it puts the reference's pytorch/ directory on sys.path (read-only import, no bytecode
written) and runs the reference's own functions -- scipy.ndimage.rotate in float64 on the CPU -- on seeded inputs.
Only data is stored:
  equivariance.npz        rotations: inputs fp32, scipy outputs fp64 (fields) / fp32 (mask, before the threshold)
      fa/x                (2, 4, 3, 37, 53) normalised fields; fa/<angle>: 4 (b, c, z) planes of the rotated fields
                          (planes fa/planes), every angle -- whole-tensor outputs at 7 angles would exceed the size
                          limit of a committed file
      fb/seed             (1, 4, 8, 80, 80) LR-shape fields, regenerated from torch.Generator().manual_seed(seed)
                          (fb/sum checks the regeneration); fb/<angle>: planes fb/planes of the rotated fields
      mk/b                (1, 1, 16, 64, 64) building mask; mk/<angle>: the reference's rotated mask before the
                          threshold (float32, as scipy returns it for a float32 input)
  equivariance_model.npz  one end-to-end sample through the reference's tiny-width UNetSR with the weights of
                          model_tiny_a.npz (not stored twice): x (1, 4, 4, 8, 12), b (1, 1, 16, 32, 48), preds,
                          preds_after_rot (normalised, fp32: the model's outputs) and dict_err at ANGLE over WINDOW
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("SR3D_REFERENCE", "/root/reference/pytorch")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import scipy.ndimage  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from src import equivariance_error_calculator as eq  # noqa: E402
from src.model_maker import make_model  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
ANGLES = (90.0, 180.0, -90.0, 30.0, 45.0, 17.5, -63.0)
ANGLE = 30.0
WINDOW = dict(sx=5, ex=-7, sy=3, ey=29)   # non-trivial: both ends, a negative bound
torch.set_num_threads(8)


def key(a):
    return f"{a:+.1f}"


def boxes_mask(Z, Y, X, seed):
    """1 = fluid, 0 = building: seeded boxes rising from z = 0"""
    rng = np.random.default_rng(seed)
    b = np.ones((1, 1, Z, Y, X), np.float32)
    for _ in range(6):
        y0, x0 = rng.integers(0, Y - 8), rng.integers(0, X - 8)
        h, dy, dx = rng.integers(2, Z), rng.integers(3, Y // 5), rng.integers(3, X // 5)
        b[..., :h, y0:y0 + dy, x0:x0 + dx] = 0
    return b


def main():
    cfg = yaml.safe_load(open(os.path.join(REF, "config", "default.yml")))
    means, scales = cfg["data"]["means"], cfg["data"]["stds"]
    rot = {"means": np.array(means), "scales": np.array(scales), "angles": np.array(ANGLES)}

    g = torch.Generator().manual_seed(11)
    xa = torch.rand(2, 4, 3, 37, 53, generator=g).numpy()
    rot["fa/x"] = xa
    rot["fa/planes"] = pa = np.array([[0, 0, 0], [0, 1, 1], [1, 2, 2], [1, 3, 0]])
    rot["fb/seed"] = np.array(12)
    xb = torch.rand(1, 4, 8, 80, 80, generator=torch.Generator().manual_seed(12)).numpy()
    rot["fb/sum"] = np.array(xb.astype(np.float64).sum())
    rot["fb/planes"] = pb = np.array([[0, 1, 3], [0, 2, 6]])
    rot["mk/b"] = bm = boxes_mask(16, 64, 64, 13)
    for a in ANGLES:
        ya = eq.rotate_temperature_velocity(xa, means, scales, a)
        rot[f"fa/{key(a)}"] = np.stack([ya[b, c, z] for b, c, z in pa])
        yb = eq.rotate_temperature_velocity(xb, means, scales, a)
        rot[f"fb/{key(a)}"] = np.stack([yb[b, c, z] for b, c, z in pb])
        rot[f"mk/{key(a)}"] = scipy.ndimage.rotate(bm, angle=a, axes=(-2, -1), reshape=False)
        assert rot[f"mk/{key(a)}"].dtype == np.float32
    np.savez_compressed(os.path.join(OUT, "equivariance.npz"), **rot)

    tiny = np.load(os.path.join(OUT, "model_tiny_a.npz"))
    model = make_model(json.loads(str(tiny["config_json"]))).eval()
    model.load_state_dict({k[3:]: torch.from_numpy(tiny[k]) for k in tiny.files if k.startswith("sd/")})
    g = torch.Generator().manual_seed(15)
    x = torch.rand(1, 4, 4, 8, 12, generator=g)
    b = torch.from_numpy(boxes_mask(16, 32, 48, 16))
    _, preds_after_rot = eq.calc_preds_for_equivariance_errors(
        Xs=x, bs=b, model=model, means=means, scales=scales, angle=ANGLE, device="cpu")
    err = eq.calc_equivariance_errors(Xs=x, bs=b, model=model, means=means, scales=scales, angle=ANGLE, device="cpu",
                                      **WINDOW)
    with torch.no_grad():
        preds = model(x, b).numpy()
    m = np.array(means)[None, :, None, None, None]
    s = np.array(scales)[None, :, None, None, None]
    out = {"x": x.numpy(), "b": b.numpy(), "preds": preds,
           "preds_after_rot": ((preds_after_rot - m) / s).astype(np.float32), "angle": np.array(ANGLE),
           "window": np.array([WINDOW[k] for k in ("sx", "ex", "sy", "ey")]), "means": np.array(means),
           "scales": np.array(scales)}
    assert np.allclose(out["preds_after_rot"] * s + m, preds_after_rot, rtol=0, atol=1e-9)
    for k in ("tm", "vr", "vl_vp"):
        out[f"err/{k}"] = np.array(err[k], np.float64)
    np.savez_compressed(os.path.join(OUT, "equivariance_model.npz"), **out)
    print({k: float(v) for k, v in err.items()})


if __name__ == "__main__":
    main()
