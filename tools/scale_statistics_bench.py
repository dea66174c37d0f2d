#!/usr/bin/env python3
"""Scale-resolved evaluation at the evaluation size (1, 4, 32, 320, 320), the tower mask of
tools/wall_distance_bench.py; in one run, the lines alternated round by round:
  * one ops.eval_scale_statistics call at max_lag R = 8 and R = 32, under both pair rules (both ends fluid: one launch;
    unobstructed: three run-length launches more);
  * the torch route it replaces, on the same GPU and the same inputs: the 12 series in fp64, then per direction and lag
    two slices, the validity mask (unobstructed: from a cumulative sum of the built cells) and 8 masked sums per level.
The kernel does 176 fp64 operations per valid pair (a fused multiply-add counted as two); the line "fp64 rate" divides
that by the time.
Device-event times around `--iters` back-to-back calls per round (the torch route: one call), median and best of
`--rounds` rounds.  Before timing, pair counts are compared for equality and the sums by their largest relative
difference.
usage: python tools/scale_statistics_bench.py [--iters 10] [--rounds 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

SHAPE = (1, 4, 32, 320, 320)
LAGS = (8, 32)
OPS_PER_PAIR = 4 * (3 * 14 + 2)  # channels x (series x (5 products, 8 adds, 1 difference) + the error at both ends)


def once(fn, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3


def torch_route(p, t, b, R, unobstructed):
    """(sums (Z, 3, R, 12, 8), pairs (Z, 3, R)) of the whole batch, sliced per direction and lag"""
    f = torch.cat([p.double(), t.double(), p.double() - t.double()], dim=1)          # (B, 12, Z, Y, X)
    fluid = b[:, 0] > 0
    B, _, Z, Y, X = f.shape
    sums = torch.zeros(Z, 3, R, 12, 8, dtype=torch.float64, device=f.device)
    pairs = torch.zeros(Z, 3, R, dtype=torch.int64, device=f.device)
    for d, ax in enumerate((3, 2, 1)):
        n = fluid.shape[ax]
        built = torch.cumsum((~fluid).to(torch.int32), dim=ax) if unobstructed else None
        for r in range(1, min(R, n - 1) + 1):
            valid = fluid.narrow(ax, 0, n - r) & fluid.narrow(ax, r, n - r)
            if unobstructed:        # no built cell in (x, x + r]
                valid = valid & (built.narrow(ax, r, n - r) == built.narrow(ax, 0, n - r))
            zs = valid.shape[1]
            pairs[:zs, d, r - 1] = valid.sum(dim=(0, 2, 3))
            f0, f1 = f.narrow(ax + 1, 0, n - r), f.narrow(ax + 1, r, n - r)
            delta = f1 - f0
            d2 = delta * delta
            v = valid[:, None]
            for m, term in enumerate((delta, d2, d2 * delta, d2 * d2, f0, f1, f0 * f0, f1 * f1)):
                sums[:zs, d, r - 1, :, m] = torch.where(v, term, 0.0).sum(dim=(0, 3, 4)).transpose(0, 1)
    return sums, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import sr3d_amd
    from helpers import synthetic_inputs
    ops = sr3d_amd.ops
    dev = "cuda:0"
    B, _, Z, Y, X = SHAPE
    _, b, y = synthetic_inputs(B, (Z, Y, X), 4, 17, "tower")
    p = y + 0.03 * torch.randn(y.shape, generator=torch.Generator().manual_seed(18))
    p, y, b = p.to(dev), y.to(dev), b.to(dev)
    vox = B * Z * Y * X
    print(f"HR {SHAPE}, tower mask, {float(1 - b.mean()):.1%} built")
    lines = []
    with torch.no_grad():
        for R in LAGS:
            for unob in (False, True):
                rule = "unobstructed" if unob else "both ends fluid"
                sums, pairs = ops.eval_scale_statistics(p, y, b, max_lag=R, unobstructed=unob)
                rs, rn = torch_route(p, y, b, R, unob)
                rel = float(((sums - rs).abs() / rs.abs().clamp_min(1e-300)).max())
                print(f"R = {R:2d}, {rule}: {int(pairs.sum())} pairs, equal to the torch route's: {bool(torch.equal(pairs, rn))}; "
                      f"largest relative difference of a sum: {rel:.2e}")
                del rs, rn
                lines.append((f"eval_scale_statistics, R = {R}, {rule}", R, int(pairs.sum()),
                              lambda R=R, unob=unob: ops.eval_scale_statistics(p, y, b, max_lag=R, unobstructed=unob),
                              args.iters))
                lines.append((f"torch route, R = {R}, {rule}", R, 0,
                              lambda R=R, unob=unob: torch_route(p, y, b, R, unob), 1))
        for _, _, _, fn, iters in lines:
            if iters > 1:
                for _ in range(2):
                    fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in lines}
        for _ in range(args.rounds):        # alternate the lines round by round: drift hits all alike
            for name, _, _, fn, iters in lines:
                times[name].append(once(fn, iters))
        med = {}
        for name, R, npairs, _, _ in lines:
            ts = sorted(times[name])
            med[name] = ts[len(ts) // 2]
            extra = f", fp64 rate {npairs * OPS_PER_PAIR / med[name] / 1e6:6.2f} Tops/s" if npairs else ""
            print(f"{name + ':':58s} median {med[name]:11.1f} us, best {ts[0]:11.1f} us{extra}")
        for R in LAGS:
            for rule in ("both ends fluid", "unobstructed"):
                k, tr = med[f"eval_scale_statistics, R = {R}, {rule}"], med[f"torch route, R = {R}, {rule}"]
                print(f"R = {R:2d}, {rule}: call / torch route = {k / tr:.4f}x ({'cheaper' if k < tr else 'NOT cheaper'}); "
                      f"{k / (3 * R) :.1f} us per direction and lag, {k * 1e3 / (vox * 3 * R):.3f} ns per voxel, direction and lag")


if __name__ == "__main__":
    main()
