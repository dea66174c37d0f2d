#!/usr/bin/env python3
"""Error-distribution evaluation at the evaluation size (1, 4, 32, 320, 320), the tower mask of
tools/wall_distance_bench.py, near_width = 1; in one run, the lines alternated round by round:
  * one ops.eval_distributions call with the distance given (two launches), and one that also makes the distance
    (ops.wall_distance: three more launches), against the bandwidth bound: 37 B per voxel (p, t, b, dist) at the
    6.29 TB/s measured copy rate;
  * the same call on identical fields (p == t): every lane of every wave adds to one counter, the worst case for the LDS adds;
  * the torch route it replaces: the 13 series, then one torch.histc per series and class on boolean-selected values
    (26 masked passes; histc has no under- / overflow / NaN slots and no exact min / max, so this is a lower bound);
  * one ops.eval_metrics call (cache defeated), the fused pass over the same inputs that gives the means.
Device-event times around `--iters` back-to-back calls per round, median and best of `--rounds` rounds.  The 118 MB of
inputs stay in the 256 MB Infinity Cache between calls, for all alike: the ratios are the figures to read, not the GB/s.
usage: python tools/error_distributions_bench.py [--iters 20] [--rounds 5]"""
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
NEAR = 1


def once(fn, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import sr3d_amd
    from helpers import synthetic_inputs
    ops, L = sr3d_amd.ops, sr3d_amd._lib
    dev = "cuda:0"
    B, _, Z, Y, X = SHAPE
    _, b, y = synthetic_inputs(B, (Z, Y, X), 4, 17, "tower")
    p = y + 0.03 * torch.randn(y.shape, generator=torch.Generator().manual_seed(18))
    p, y, b = p.to(dev), y.to(dev), b.to(dev)
    vox = B * Z * Y * X
    dist = ops.wall_distance(b, NEAR)
    fluid = b[:, 0] > 0
    masks = [fluid & (dist[:, 0] <= NEAR), fluid & (dist[:, 0] > NEAR)]
    lo, hi = ops.distribution_ranges()
    sc = torch.tensor(STDS[1:], device=dev)[None, :, None, None, None]

    def given():
        return ops.eval_distributions(p, y, b, STDS, near_width=NEAR, dist=dist)

    def with_distance():
        return ops.eval_distributions(p, y, b, STDS, near_width=NEAR)

    def identical():
        return ops.eval_distributions(y, y, b, STDS, near_width=NEAR, dist=dist)

    def torch_route():
        d = p - y
        series = [d[:, 0], d[:, 1], d[:, 2], d[:, 3], torch.linalg.norm(d[:, 1:] * sc, dim=1),
                  *(p[:, c] for c in range(4)), *(y[:, c] for c in range(4))]
        return [torch.histc(v[m], bins=L.DIST_BINS, min=lo[s], max=hi[s]) for s, v in enumerate(series) for m in masks]

    def metrics():
        ops.invalidate_eval_cache()     # time the kernel, not the per-batch cache
        return ops.eval_metrics(p, y, b, STDS, 5.0, 0)

    lines = [("eval_distributions, dist given (2 launches)", given, args.iters),
             ("eval_distributions + wall_distance (5 launches)", with_distance, args.iters),
             ("eval_distributions, p == t, dist given", identical, args.iters),
             ("torch: 13 series + 26 masked torch.histc", torch_route, max(1, args.iters // 4)),
             ("eval_metrics, one call", metrics, args.iters)]
    with torch.no_grad():
        counts, minmax, cells = given()
        ref = torch_route()
        out = counts[:, :, [0, L.DIST_SLOTS - 2, L.DIST_SLOTS - 1]].sum()
        # histc closes the last bin on the right and rounds in its own way: compare totals, not bins
        agree = all(int(ref[2 * s + k].sum()) == int(counts[s, k, 1:257].sum()) for s in range(L.DIST_SERIES) for k in range(2))
        print(f"HR {SHAPE}, tower mask, {float(1 - b.mean()):.1%} built, near_width = {NEAR}; cells built / near / far "
              f"{cells.tolist()}; values outside the ranges or NaN: {int(out)}; binned totals equal torch.histc's: {agree}; "
              f"largest bin {int(counts[:, :, 1:257].max())} of {int(cells[1:].sum())} fluid cells")
        for _, fn, _ in lines:          # warm every line before the first timed round
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in lines}
        for _ in range(args.rounds):    # alternate the lines round by round: drift hits all alike
            for name, fn, iters in lines:
                times[name].append(once(fn, iters))
        bound = 37.0 * vox / COPY_BW * 1e6
        med = {}
        for name, _, _ in lines:
            ts = sorted(times[name])
            med[name] = ts[len(ts) // 2]
            print(f"{name + ':':52s} median {med[name]:9.1f} us, best {ts[0]:9.1f} us")
        g, w, i, t, m = (med[name] for name, _, _ in lines)
        print(f"bandwidth bound: {bound:.1f} us (37 B/voxel at {COPY_BW / 1e12:.2f} TB/s): the call with dist given runs at "
              f"{bound / g:.0%} of it")
        print(f"call / torch route: {g / t:.3f}x ({'cheaper' if g < t else 'NOT cheaper'}; with the distance {w / t:.3f}x); "
              f"call / one eval_metrics call: {g / m:.2f}x; p == t / noisy p: {i / g:.2f}x")


if __name__ == "__main__":
    main()
