#!/usr/bin/env python3
"""Wall-distance-resolved evaluation at the evaluation size (1, 4, 32, 320, 320), a tower mask, D = 8; in one run:
  * ops.wall_distance at cap 8 (three launches), against 8 launches of sr3d_near_wall (the iteration it replaces) and
    against its bandwidth bound: 5 B per voxel (fp32 mask in, byte out) at the 6.29 TB/s measured copy rate;
  * one ops.eval_wall_distance_profiles call with the distance given (16 rows x 10 bins: three launches), against 10
    ops.eval_metrics calls (cache defeated): one masked whole-volume pass per bin is the route without the kernel;
  * ops.eval_level_profiles and one ops.eval_metrics call, the two passes the stencil is shared with.
Device-event times around `--iters` back-to-back calls, median and best of 5 repeats.  The 118 MB of inputs stay in
the 256 MB Infinity Cache between calls, for all alike: the ratios are the figures to read, not the GB/s.
usage: python tools/wall_distance_bench.py [--iters 20]"""
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
D = 8


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
    dist = ops.wall_distance(b, D)
    near_out = torch.empty_like(b)

    def distance():
        return ops.wall_distance(b, D)

    def near_wall_x(n=D):          # n launches of the 27-tap kernel (raw C ABI: no allocation in the loop)
        for _ in range(n):
            L.check(L.lib.sr3d_near_wall(L.dev_ptr(b), L.dev_ptr(near_out), B, Z, Y, X, L.stream_ptr()), "sr3d_near_wall")

    def profiles():
        return ops.eval_wall_distance_profiles(p, y, b, STDS, max_distance=D, dist=dist)

    def metrics():
        ops.invalidate_eval_cache()     # time the kernel, not the per-batch cache
        return ops.eval_metrics(p, y, b, STDS, 5.0, 0)

    def metrics_per_bin():
        for _ in range(D + 2):
            metrics()

    def level_profiles():
        return ops.eval_level_profiles(p, y, b, STDS)

    with torch.no_grad():
        values, sums = profiles()
        whole = metrics()
        cells = sums[L.WALLDIST_SUM_INDEX["cells"]]
        i, j = L.WALLDIST_INDEX["MaskedL1NearWall"], L.EVAL_INDEX["MaskedL1NearWall"]
        print(f"HR {SHAPE}, tower mask, {float(1 - b.mean()):.1%} built, D = {D}; cells per bin "
              f"{[int(c) for c in cells.tolist()]}; MaskedL1NearWall at bin 1 vs eval_metrics: relative difference "
              f"{abs(float(values[i, 1]) - float(whole[j])) / float(whole[j]):.1e}")
        d_bound, p_bound = 5.0 * vox / COPY_BW * 1e6, 37.0 * vox / COPY_BW * 1e6
        d_med, d_best = timed(distance, args.iters)
        print(f"wall_distance, cap {D} (3 launches):                    median {d_med:9.1f} us, best {d_best:9.1f} us; bound "
              f"{d_bound:.1f} us (5 B/voxel at {COPY_BW / 1e12:.2f} TB/s): {d_bound / d_best:.0%} of it")
        n1_med, n1_best = timed(lambda: near_wall_x(1), args.iters)
        print(f"sr3d_near_wall, one launch:                            median {n1_med:9.1f} us, best {n1_best:9.1f} us")
        n_med, n_best = timed(near_wall_x, args.iters)
        print(f"sr3d_near_wall x {D} (the iteration replaced):            median {n_med:9.1f} us, best {n_best:9.1f} us")
        m_med, m_best = timed(metrics, args.iters)
        print(f"eval_metrics, one call:                                median {m_med:9.1f} us, best {m_best:9.1f} us")
        l_med, l_best = timed(level_profiles, args.iters)
        print(f"eval_level_profiles, one call:                         median {l_med:9.1f} us, best {l_best:9.1f} us")
        p_med, p_best = timed(profiles, args.iters)
        print(f"eval_wall_distance_profiles, one call (dist given):    median {p_med:9.1f} us, best {p_best:9.1f} us; bound "
              f"{p_bound:.1f} us (37 B/voxel): {p_bound / p_best:.0%} of it")
        b_med, b_best = timed(metrics_per_bin, max(1, args.iters // 4))
        print(f"eval_metrics x {D + 2} (one masked pass per bin):           median {b_med:9.1f} us, best {b_best:9.1f} us")
        print(f"distance call / {D} near-wall launches: {d_med / n_med:.2f}x "
              f"({'cheaper' if d_med < n_med else 'NOT cheaper'})")
        print(f"profile call / {D + 2} eval_metrics calls: {p_med / b_med:.2f}x "
              f"({'cheaper' if p_med < b_med else 'NOT cheaper'}); profile call / one eval_metrics call: "
              f"{p_med / m_med:.2f}x; / eval_level_profiles: {p_med / l_med:.2f}x")


if __name__ == "__main__":
    main()
