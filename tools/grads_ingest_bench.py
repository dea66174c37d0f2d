#!/usr/bin/env python3
"""GrADS ingest per time step at the reference's shape: four big-endian variables (tm, vl, vp, vr), a 40-level window
(from level 4) of 44-level files, 400 x 400 -- written as synthetic GrADS files into a temporary directory first.

GPU (default):
  * device-event time of one ops.grads_decode call against its bandwidth bound: the bytes it must read (4 x 40 x 400
    x 400 x 4) plus the bytes it must write (the same), at the 6.29 TB/s measured copy rate tools/lr_data_bench.py
    uses.  The `options sequential` layout (record markers: the 4-byte path) is timed next to it.
  * the whole per-step pipeline -- stage (memmap -> pinned buffer), copy to the device, decode, coarse-grain, results
    back to the host -- with and without the one-step-ahead overlap (AtmosData.steps), and its parts one by one.  The
    files were just written, so they come from the page cache: the stage figure is a host memory copy, a floor for
    what a real file system costs.
--host: the numpy restatement of the decode (tests/grads_ref.py) on one host core per time step.
usage: python tools/grads_ingest_bench.py [--iters 50] [--steps 8] [--host]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

COPY_BW = 6.29e12   # MI355X measured float4 copy rate, B/s (tools/lr_data_bench.py)
ZF, Z0, Z, Y, X, M, T = 44, 4, 40, 400, 400, 40, 3
UNDEF = -9.99e33
NAMES = ("tm", "vl", "vp", "vr")


def write_case(d, sequential=False):
    """T time steps of the four variables, undef inside a few buildings"""
    import grads_ref as G
    rng = np.random.default_rng(7)
    tz = np.full((Y, X), 10.0)
    for _ in range(120):
        y0, x0 = rng.integers(0, Y - 20, 2)
        h, w = rng.integers(1, 19, 2)
        tz[y0:y0 + h, x0:x0 + w] = rng.uniform(20, 200)
    lev = -2.5 + 5.0 * np.arange(ZF)
    inside = lev[:, None, None] < tz[None]
    for k, n in enumerate(NAMES):
        a = (300.0 if k == 0 else 0.0) + 3 * rng.standard_normal((T, ZF, Y, X), dtype=np.float32)
        a[:, inside] = np.float32(UNDEF)
        G.write_grads(os.path.join(d, f"atmos_0n_{n}.ctl"), {n: a}, undef=UNDEF, lev=lev, big_endian=True,
                      sequential=sequential)
    return tz, lev[Z0:Z0 + Z]


def load(d):
    from sr3d_amd.src.training_data_maker import _load_atmos_data
    return _load_atmos_data(d, min_index_height=Z0, max_index_height=Z0 + Z, margin=0, discarded_initial_period=0)


def host(args):
    import grads_ref as G
    with tempfile.TemporaryDirectory() as d:
        write_case(d)
        data = load(d)
        bufs = [bytes(v.step_bytes(0)) for v in (data.tm, data.vl, data.vp, data.vr)]
        slab = Y * X * 4
        t0 = time.perf_counter()
        for _ in range(args.samples):
            G.decode_buffers(bufs, (Z, Y, X), 0, slab, UNDEF, True)
        dt = (time.perf_counter() - t0) / args.samples
    print(f"numpy restatement of the decode (tests/grads_ref.py), one host core: {dt * 1e3:9.1f} ms per time step")


def event_time(fn, iters, rounds=5):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e) / iters * 1e3)
    return min(times), sorted(times)[len(times) // 2]


def gpu(args):
    import torch

    import sr3d_amd
    from sr3d_amd.src.training_data_maker import lr_building_tops
    ops = sr3d_amd.ops
    dev = torch.device("cuda:0")
    nb = 2 * 4 * Z * Y * X * 4
    bound = nb / COPY_BW * 1e6
    print(f"shape 4 x ({Z} of {ZF}, {Y}, {X}) big endian: {nb / 2e6:.1f} MB read + {nb / 2e6:.1f} MB written -> "
          f"{bound:.1f} us at {COPY_BW / 1e12:.2f} TB/s")
    for sequential in (False, True):
        with tempfile.TemporaryDirectory() as d:
            tz, levs = write_case(d, sequential)
            data = load(d)
            pin = torch.empty(data.staging_bytes, dtype=torch.uint8).pin_memory()
            staged = data.stage(0, pin).to(dev)
            best, med = event_time(lambda: data.decode(staged), args.iters)
            kind = "sequential records, 4-byte loads and stores" if sequential else "direct, 16-byte loads and stores"
            print(f"grads_decode ({kind}; events around {args.iters} calls x 5): median {med:.1f} us, best "
                  f"{best:.1f} us per time step = {nb / best / 1e3:.0f} GB/s, {bound / best:.0%} of the bandwidth "
                  f"bound")
            if sequential:
                continue
            # ---- the parts of one step, one by one
            t0 = time.perf_counter()
            for k in range(args.steps):
                data.stage(k % T, pin)
            t_stage = (time.perf_counter() - t0) / args.steps * 1e6
            buf = torch.empty_like(staged)
            h2d, _ = event_time(lambda: buf.copy_(pin, non_blocking=True), 5)
            hm = torch.from_numpy(np.broadcast_to(levs[:, None, None] < tz[None], (Z, Y, X)).copy()).to(dev)
            lr_tz = tz.reshape(Y // 4, 4, X // 4, 4).max(axis=(1, 3))
            tops = torch.from_numpy(lr_building_tops(lr_tz, np.full(lr_tz.shape, 15.0), levs)).to(dev)
            raw = data.decode(staged)
            cg, _ = event_time(lambda: ops.coarse_grain_outside_buildings(raw, hm, tops, hr_margin=M, lev=levs),
                               args.iters)
            hr, lr = ops.coarse_grain_outside_buildings(raw, hm, tops, hr_margin=M, lev=levs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                hr.cpu(), lr.cpu()
            t_d2h = (time.perf_counter() - t0) / 3 * 1e6
            print(f"one step's parts: stage (page cache -> pinned, {data.staging_bytes / 1e6:.1f} MB) {t_stage:.0f} us"
                  f" = {data.staging_bytes / t_stage / 1e3:.1f} GB/s; copy to the device {h2d:.0f} us = "
                  f"{data.staging_bytes / h2d / 1e3:.1f} GB/s; decode {best:.0f} us; coarse-grain {cg:.0f} us; "
                  f"results to pageable host memory {t_d2h:.0f} us")

            # ---- the pipeline as the script runs it, without writing files
            def pipeline(overlap):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _, r in data.steps([k % T for k in range(args.steps)], dev, overlap=overlap):
                    h, l_ = ops.coarse_grain_outside_buildings(r, hm, tops, hr_margin=M, lev=levs)
                    h.cpu(), l_.cpu()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.steps * 1e3
            pipeline(True)
            for overlap in (False, True):
                ms = min(pipeline(overlap) for _ in range(3))
                print(f"pipeline (stage, copy, decode, coarse-grain, results to the host; {args.steps} steps, best "
                      f"of 3), {'one step ahead on a side stream' if overlap else 'no overlap'}: {ms:.2f} ms per "
                      f"time step -- the decode kernel is {best / 1e3 / ms:.1%} of it")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--samples", type=int, default=1)
    args = ap.parse_args()
    host(args) if args.host else gpu(args)


if __name__ == "__main__":
    main()
