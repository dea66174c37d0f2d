#!/usr/bin/env python3
"""Near-surface (2 m) temperature at the test-set shape: prediction (1, 4, 32, 320, 320), raw HR truth
(1, 4, 40, 320, 320), default.yml widths, seeded building tops over every branch of the extrapolation.

GPU (default): device-event times of the map-only kernel, of the fused call (both maps + error sums, one launch), of
the model forward and of the forward plus the fused call per sample; bytes are ALGORITHMIC per column (tz 8 B, two
levels of each source 8 B, each map 4 B: 20 B for one map, 32 B fused).
--host: the reference's host loop on the CPU -- the notebook's infer_2m_height_temperature, loaded from the reference
checkout given by --reference (not part of this repository; skipped when absent) -- and the vectorised numpy
restatement of tests/surface_ref.py, per sample.
usage: python tools/surface_temperature_bench.py [--iters 50] [--host [--reference DIR] [--samples 1]]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PEAK = 8.0e12   # MI355X HBM3E peak, B/s
Y = X = 320
H = np.arange(32) * 5 + 17.5
MEAN_T = 302.0   # the reference's config/default.yml data.means[0]


def building(seed=0):
    """(X, Y) building tops: ground below H[0], on levels, between levels, above the top, NaN"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 10, (X, Y))
    b = rng.uniform(0.0, H[0], (X, Y))
    b = np.where(k >= 6, rng.uniform(H[0], H[-1], (X, Y)), b)
    b = np.where(k == 5, H[rng.integers(0, 32, (X, Y))], b)
    b = np.where(k == 4, H[-1] + 10.0, b)
    b[0, 0] = np.nan
    return b


def host(args):
    import surface_ref as sr
    rng = np.random.default_rng(1)
    t = (295 + 5 * rng.standard_normal((args.samples, 32, X, Y))).astype(np.float32)
    b = building()
    t0 = time.perf_counter()
    sr.t2m_ref(t, b, H)
    t_vec = (time.perf_counter() - t0) / args.samples
    print(f"numpy restatement (tests/surface_ref.py), host CPU   {t_vec * 1e3:9.1f} ms per sample")
    nb = os.path.join(args.reference, "notebook", "make_2m_temperature.ipynb")
    if not os.path.exists(nb):
        print(f"reference host loop: not measured ({nb} not found)")
        return
    cells = ["".join(c["source"]) for c in json.load(open(nb))["cells"] if c["cell_type"] == "code"]
    ns = {"np": np, "tqdm": lambda it, **kw: it}
    for src in cells:
        if src.startswith("HEIGHT_LEVELS =") or "def infer_2m_height_temperature" in src:
            exec(compile(src, nb, "exec"), ns)
    t0 = time.perf_counter()
    ns["infer_2m_height_temperature"](t, b)
    t_ref = (time.perf_counter() - t0) / args.samples
    print(f"reference host loop (notebook, numpy {np.__version__}), host CPU  {t_ref * 1e3:9.1f} ms per sample "
          f"({args.samples} sample(s) per call)")


def gpu(args):
    import torch

    import bench
    import sr3d_amd
    ops = sr3d_amd.ops

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / iters

    dev = torch.device("cuda:0")
    cfg = bench.make_config("l1")
    torch.manual_seed(0)
    model = sr3d_amd.make_model(cfg).to(dev).eval()
    x, bm, _ = bench.synthetic_batch(1, (32, 320, 320), 4, 5, dev)
    g = torch.Generator().manual_seed(2)
    truth = (295 + 5 * torch.randn(1, 4, 40, Y, X, generator=g)).to(dev)
    p = torch.rand(1, 4, 32, Y, X, generator=g).to(dev)
    tz = torch.from_numpy(np.ascontiguousarray(building().T)).to(dev)
    s0, m0 = cfg["data"]["stds"][0], MEAN_T
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    cols = Y * X
    t_map = timed(lambda: ops.surface_temperature(truth, tz), args.iters)
    t_fused = timed(lambda: ops.surface_temperature_errors(p, truth, tz, pred_scale=s0, pred_mean=m0, acc=acc),
                    args.iters)
    with torch.no_grad():
        t_fwd = timed(lambda: model(x, bm), max(3, args.iters // 5))

        def sample():
            pred = model(x, bm)
            ops.surface_temperature_errors(pred, truth, tz, pred_scale=s0, pred_mean=m0, acc=acc)
        t_sample = timed(sample, max(3, args.iters // 5))
    for name, ms, nbytes in (("map only (truth, 1 launch)", t_map, 20 * cols),
                             ("fused: 2 maps + error sums (1 launch)", t_fused, 32 * cols)):
        print(f"{name:40s} {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:7.0f} GB/s algorithmic "
              f"({nbytes / ms / 1e6 / PEAK * 1e9:5.1%})")
    print(f"{'model forward (1,4,8,80,80) -> 32x320x320':40s} {t_fwd:9.2f} ms")
    print(f"{'forward + fused 2 m call':40s} {t_sample:9.2f} ms per sample")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host", action="store_true", help="time the host CPU versions instead (no GPU needed)")
    ap.add_argument("--reference", default=os.environ.get("SR3D_REFERENCE", "/root/reference/pytorch"))
    ap.add_argument("--samples", type=int, default=1)
    args = ap.parse_args()
    host(args) if args.host else gpu(args)


if __name__ == "__main__":
    main()
