#!/usr/bin/env python3
"""LR training data per time step at the script's size: raw (4, 40, 400, 400) fp32, margin 40, buildings of odd widths.

GPU (default): device-event time of one ops.coarse_grain_outside_buildings call (all four channels), its MINIMAL
traffic (raw read once, the HR mask once, the HR window and the LR blocks written once: 175 MB) and the share of the
6.29 TB/s measured copy rate that traffic would take (the bandwidth bound over the measured time).
--host: the block form of the numpy restatement (tests/lr_data_ref.py) on the host CPU per time step -- the
restatement, not the reference (whose xarray / dask / OpenCV path is not available here).
usage: python tools/lr_data_bench.py [--iters 50] [--host]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

COPY_BW = 6.29e12   # MI355X measured float4 copy rate, B/s (MI355X_MICROARCH: HBM)
C, Z, Y, X, M = 4, 40, 400, 400, 40


def case():
    import lr_data_ref as R
    rng = np.random.default_rng(7)
    levs = 17.5 + 5.0 * np.arange(Z)
    raw = np.empty((C, Z, Y, X), np.float32)
    raw[0] = 300 + 3 * rng.standard_normal((Z, Y, X), dtype=np.float32)
    raw[1:] = 4 * rng.standard_normal((C - 1, Z, Y, X), dtype=np.float32)
    hr_tz = np.full((Y, X), 10.0)
    for _ in range(120):
        y0, x0 = rng.integers(0, Y - 20, 2)
        h, w = rng.integers(1, 19, 2)
        hr_tz[y0:y0 + h, x0:x0 + w] = rng.choice([rng.uniform(20, 120), rng.uniform(150, 300)])
    hm = R.calc_is_in_building(hr_tz, np.full((Y, X), 15.0), levs) > 0
    raw[0][:, hr_tz > levs[-1]] = np.nan
    hm |= np.isnan(raw[0])
    lr_tz = hr_tz.reshape(Y // 4, 4, X // 4, 4).max(axis=(1, 3))
    return raw, hm, lr_tz, np.full(lr_tz.shape, 15.0), levs


def min_bytes():
    Yc, Xc = Y - 2 * M, X - 2 * M
    return C * Z * Y * X * 4 + Z * Y * X + C * Z * Yc * Xc * 4 + C * (Z // 4) * (Yc // 4) * (Xc // 4) * 4


def host(args):
    import lr_data_ref as R
    raw, hm, tz, ez, levs = case()
    t0 = time.perf_counter()
    for _ in range(args.samples):
        R.lr_data_ref(raw, hm, tz, ez, levs, margin=M)
    dt = (time.perf_counter() - t0) / args.samples
    print(f"numpy restatement, block form (tests/lr_data_ref.py), host CPU: {dt * 1e3:9.1f} ms per time step "
          f"(the restatement, not the reference)")


def gpu(args):
    import torch

    import sr3d_amd
    from sr3d_amd.src.training_data_maker import lr_building_tops
    ops = sr3d_amd.ops
    dev = torch.device("cuda:0")
    raw, hm, tz, ez, levs = case()
    rt = torch.from_numpy(raw).to(dev)
    ht = torch.from_numpy(hm).to(dev)
    tops = torch.from_numpy(lr_building_tops(tz, ez, levs)).to(dev)

    def call():
        return ops.coarse_grain_outside_buildings(rt, ht, tops, hr_margin=M, lev=levs)

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e) / args.iters * 1e3)
    nb = min_bytes()
    best, med = min(times), sorted(times)[len(times) // 2]
    bound = nb / COPY_BW * 1e6
    print(f"shape (4, {Z}, {Y}, {X}), margin {M}: minimal traffic {nb / 1e6:.1f} MB -> {bound:.1f} us at "
          f"{COPY_BW / 1e12:.2f} TB/s")
    print(f"coarse_grain_outside_buildings (3 launches, events around {args.iters} calls x 5): "
          f"median {med:.1f} us, best {best:.1f} us per time step = {nb / best / 1e3:.0f} GB/s, "
          f"{bound / best:.0%} of the bandwidth bound")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--samples", type=int, default=1)
    args = ap.parse_args()
    host(args) if args.host else gpu(args)


if __name__ == "__main__":
    main()
