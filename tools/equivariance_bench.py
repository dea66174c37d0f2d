#!/usr/bin/env python3
"""Rotation-equivariance evaluation at the test-set shape: LR (1,4,8,80,80) -> HR (1,4,32,320,320), default.yml widths,
a seeded synthetic mask.  Prints device-event times and achieved GB/s of each rotation kernel and of the fused error,
the time of one calc_equivariance_errors call and of a 12-angle sweep, and the reference's scipy composition on the
host CPU if scipy is importable.

Bytes are ALGORITHMIC: the field read once and written once (the fused error: preds and preds_after_rot read once);
the fp64 spline workspace is reported separately (prefilter: tmp written + read, coefficients written; gather:
coefficients read once).  usage: python tools/equivariance_bench.py [--iters 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import sr3d_amd  # noqa: E402
from sr3d_amd.src import equivariance_error_calculator as eq  # noqa: E402

PEAK = 8.0e12   # MI355X HBM3E peak, B/s
MEANS = [302.0, -6.5, -9.1, -3.5]   # the reference's config/default.yml data.means
ANGLE = 30.0
ANGLES = [float(a) for a in range(15, 360, 30)]   # 12 angles
WINDOW = dict(sx=40, ex=-40, sy=40, ey=-40)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def row(name, ms, algo, ws):
    print(f"{name:34s} {ms * 1e3:9.1f} us  {algo / ms / 1e6:7.0f} GB/s algorithmic ({algo / ms / 1e6 / PEAK * 1e9:5.1%})"
          f"  {(algo + ws) / ms / 1e6:7.0f} GB/s with the fp64 workspace ({(algo + ws) / ms / 1e6 / PEAK * 1e9:5.1%})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = sr3d_amd.ops
    cfg = bench.make_config("l1")
    means, scales = MEANS, cfg["data"]["stds"]
    torch.manual_seed(0)
    model = sr3d_amd.make_model(cfg).to(dev).eval()
    x, b, y = bench.synthetic_batch(1, (32, 320, 320), 4, 5, dev)
    p = torch.rand_like(y)

    print(f"rotation kernels at {ANGLE} degrees (device events, mean of {args.iters})")
    for name, t in (("LR fields (1,4,8,80,80)", x), ("HR prediction (1,4,32,320,320)", p),
                    ("HR building mask (1,1,32,320,320)", b)):
        n = t.numel()
        ws = ops.rotate_workspace(t)
        if t.shape[1] == 4:
            def full():
                return ops.rotate_fields(t, means, scales, ANGLE, workspace=ws)

            def gather():
                return ops.rotate_fields(t, means, scales, ANGLE, workspace=ws, coef_ready=True)
        else:
            def full():
                return ops.rotate_building(t, ANGLE, workspace=ws)

            def gather():
                return ops.rotate_building(t, ANGLE, workspace=ws, coef_ready=True)
        t_full, t_gather = timed(full, args.iters), timed(gather, args.iters)
        t_pre = max(t_full - t_gather, 1e-9)
        print(f"  {name}")
        row("    prefilter (y then x FIR)", t_pre, 4 * n, 24 * n)
        row("    gather + epilogue", t_gather, 4 * n, 8 * n)
        row("    whole call", t_full, 8 * n, 32 * n)
    n = p.numel()
    wp = ops.rotate_workspace(p)
    ops.equivariance_errors(p, y, means, scales, ANGLE, workspace=wp, **WINDOW)
    t_err = timed(lambda: ops.equivariance_errors(p, y, means, scales, ANGLE, workspace=wp, coef_ready=True, **WINDOW),
                  args.iters)
    row("  fused error (window 240x240)", t_err, 8 * n * (240 * 240) / (320 * 320), 8 * n * (240 * 240) / (320 * 320))
    t_err_full = timed(lambda: ops.equivariance_errors(p, y, means, scales, ANGLE, workspace=wp, **WINDOW), args.iters)
    row("  fused error incl. prefilter", t_err_full, 8 * n, 32 * n)

    kw = dict(Xs=x, bs=b, model=model, means=means, scales=scales, device="cuda:0", **WINDOW)
    with torch.no_grad():
        t_fwd = timed(lambda: model(x, b), max(3, args.iters // 4))
    t_call = timed(lambda: eq.calc_equivariance_errors(angle=ANGLE, **kw), max(3, args.iters // 4))
    t_sweep = timed(lambda: eq.calc_equivariance_errors_over_angles(angles=ANGLES, **kw), 2)
    print(f"model forward                       {t_fwd:9.2f} ms")
    print(f"calc_equivariance_errors (1 angle)  {t_call:9.2f} ms per sample")
    print(f"12-angle sweep                      {t_sweep:9.2f} ms per sample ({t_sweep / 12:.2f} ms per angle)")

    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        print("reference composition (scipy, host CPU): not measured (scipy is not importable here)")
        return
    xs, bs, ps = x.cpu().numpy(), b.cpu().numpy(), p.cpu().numpy()
    m = np.array(means)[None, :, None, None, None]
    s = np.array(scales)[None, :, None, None, None]
    t0 = time.perf_counter()
    scipy.ndimage.rotate(xs * s + m, angle=ANGLE, axes=(-2, -1), reshape=False)
    t1 = time.perf_counter()
    scipy.ndimage.rotate(bs, angle=ANGLE, axes=(-2, -1), reshape=False)
    t2 = time.perf_counter()
    scipy.ndimage.rotate(ps * s + m, angle=ANGLE, axes=(-2, -1), reshape=False)
    t3 = time.perf_counter()
    print(f"reference composition (scipy {scipy.__version__}, one host thread as the reference calls it): LR fields "
          f"{(t1 - t0) * 1e3:.0f} ms, HR mask {(t2 - t1) * 1e3:.0f} ms, HR prediction {(t3 - t2) * 1e3:.0f} ms, "
          f"total {(t3 - t0) * 1e3:.0f} ms per angle")


if __name__ == "__main__":
    main()
