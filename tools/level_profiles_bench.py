#!/usr/bin/env python3
"""Height-resolved evaluation at the evaluation size (1, 4, 32, 320, 320), a tower mask:
  * one ops.eval_level_profiles call (all 16 profiles at all 32 levels: two launches);
  * one ops.eval_metrics call (the whole-volume pass, cache defeated: the kernel of sr3d_eval.hip);
  * Z ops.eval_metrics calls with lev = 0 .. Z-1, the only route to a two-metric profile without the profile kernel;
  * the bandwidth bound of one pass: 36 B per voxel at the 6.29 TB/s measured copy rate.
Device-event times around `--iters` back-to-back calls, median and best of 5 repeats.  The 118 MB of inputs stay in
the 256 MB Infinity Cache between calls, for all three alike: the ratios are the figures to read, not the GB/s.
usage: python tools/level_profiles_bench.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

COPY_BW = 6.29e12   # MI355X measured float4 copy rate, B/s
SHAPE = (1, 4, 32, 320, 320)
STDS = [8.4, 14.4, 21.6, 7.0]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e) / iters * 1e3)
    return sorted(times)[len(times) // 2], min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import sr3d_amd
    from helpers import synthetic_inputs
    ops, L = sr3d_amd.ops, sr3d_amd._lib
    dev = "cuda:0"
    B, _, Z, Y, X = SHAPE
    _, b, y = synthetic_inputs(B, (Z, Y, X), 4, 17, "tower")
    p = y + 0.2 * (torch.rand(y.shape, generator=torch.Generator().manual_seed(18)) - 0.5)
    p, y, b = p.to(dev), y.to(dev), b.to(dev)
    vox = B * Z * Y * X
    bound = 36.0 * vox / COPY_BW * 1e6

    def profiles():
        return ops.eval_level_profiles(p, y, b, STDS)

    def metrics(lev=0):
        ops.invalidate_eval_cache()     # time the kernel, not the per-batch cache
        return ops.eval_metrics(p, y, b, STDS, 5.0, lev)

    def metrics_every_level():
        for k in range(Z):
            metrics(k)

    with torch.no_grad():
        values, _ = profiles()
        per_lev = torch.stack([metrics(k) for k in range(Z)])
        i, j = L.PROFILE_INDEX["AbsDiffTemperature"], L.EVAL_INDEX["AbsDiffTemperatureLev"]
        worst = float(((values[i] - per_lev[:, j]).abs() / per_lev[:, j].abs()).max())
        print(f"HR {SHAPE}, tower mask, {float(1 - b.mean()):.1%} built; AbsDiffTemperature profile vs {Z} lev=k passes: "
              f"worst relative difference {worst:.1e}")
        print(f"bandwidth bound of one pass: {36.0 * vox / 1e6:.1f} MB -> {bound:.1f} us at {COPY_BW / 1e12:.2f} TB/s")
        m_med, m_best = timed(metrics, args.iters)
        print(f"eval_metrics, one call (whole volume, one lev):        median {m_med:9.1f} us, best {m_best:9.1f} us "
              f"= {36.0 * vox / m_best / 1e3:.0f} GB/s of 36 B/voxel")
        p_med, p_best = timed(profiles, args.iters)
        print(f"eval_level_profiles, one call ({L.PROFILE_COUNT} profiles x {Z} levels):  median {p_med:9.1f} us, best "
              f"{p_best:9.1f} us = {36.0 * vox / p_best / 1e3:.0f} GB/s of 36 B/voxel, {bound / p_best:.0%} of the bound")
        z_med, z_best = timed(metrics_every_level, max(1, args.iters // 4))
        print(f"eval_metrics x {Z} (lev = 0 .. {Z - 1}; two profiles only):    median {z_med:9.1f} us, best {z_best:9.1f} us")
        print(f"profile call / single eval_metrics launch: {p_med / m_med:.2f}x (the per-plane reduction: 22 more "
              f"cross-lane shuffles per plane and row on top of the stencil's 14)")
        print(f"{Z} eval_metrics passes / profile call: {z_med / p_med:.1f}x")


if __name__ == "__main__":
    main()
