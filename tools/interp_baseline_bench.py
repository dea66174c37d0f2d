#!/usr/bin/env python3
"""The interpolation baseline at the evaluation size: LR (1, 4, 8, 80, 80) -> HR (1, 4, 32, 320, 320), a tower mask
with about 20 % of the columns built (some through the whole depth, so the y pass has work).

GPU (default):
  * device-event time of one ops.interp_baseline call (five launches) and of the call plus the fused metrics pass
    (ops.eval_metrics), i.e. what optim_helper.evaluate spends per sample on the device for this "model";
  * the bandwidth bound: output bytes + LR bytes at the 6.29 TB/s measured copy rate, and its share of the call;
  * each kernel's time, from a child process under `rocprofv3 --kernel-trace --stats` (--no-trace skips it).
--host: the numpy restatement (tests/interp_baseline_ref.py) on one host core -- the restatement, not the reference
(whose xarray path is not available here).
usage: python tools/interp_baseline_bench.py [--iters 50] [--host] [--no-trace]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

COPY_BW = 6.29e12   # MI355X measured float4 copy rate, B/s (MI355X_MICROARCH: HBM)
SHAPE, SCALE = (1, 4, 8, 80, 80), 4
STDS = [8.4, 14.4, 21.6, 7.0]


def case():
    import interp_baseline_ref as R
    return R.tower_case(seed=5, shape=SHAPE)


def min_bytes():
    n = int(np.prod(SHAPE))
    return n * 4 * SCALE ** 3 + n * 4


def host(args):
    import interp_baseline_ref as R
    lr, mask = case()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    r = R.interp_baseline_ref(lr, mask, SCALE)
    dt = time.perf_counter() - t0
    print(f"numpy restatement (tests/interp_baseline_ref.py), one host core: {dt * 1e3:9.1f} ms per sample, NaN cells "
          f"after mask / z / y / x: {r['n_nan']} (the restatement, not the reference)")


def tensors():
    import torch
    dev = torch.device("cuda:0")
    lr, mask = case()
    g = torch.Generator().manual_seed(1)
    hr_shape = SHAPE[:2] + tuple(SCALE * n for n in SHAPE[2:])
    ys = torch.rand(hr_shape, generator=g).to(dev)
    bs = (torch.rand((1, 1) + hr_shape[2:], generator=g) > 0.2).float().to(dev)
    return torch.from_numpy(lr).to(dev), torch.from_numpy(mask).to(dev), ys, bs


def calls_only(args):
    """the traced child: a few calls, nothing else"""
    import torch

    import sr3d_amd
    lr, mask, _, _ = tensors()
    out = torch.empty(SHAPE[:2] + tuple(SCALE * n for n in SHAPE[2:]), device=lr.device)
    with torch.no_grad():
        for _ in range(args.iters):
            sr3d_amd.ops.interp_baseline(lr, mask, SCALE, out=out)
    torch.cuda.synchronize()


def trace(args):
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("per-kernel times: rocprofv3 not found: not measured")
        return
    d = tempfile.mkdtemp(prefix="interp_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "s", "--",
                            sys.executable, os.path.abspath(__file__), "--calls-only", "--iters", str(args.iters)],
                           capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print(f"per-kernel times: the traced run failed (exit {r.returncode}): not measured\n{r.stderr[-1000:]}")
            return
        print(f"per kernel (rocprofv3 --kernel-trace --stats, {args.iters} calls, tracing on):")
        for row in csv.DictReader(open(found[0])):
            if "interp_" in row["Name"]:
                print(f"  {float(row['TotalDurationNs']) / int(row['Calls']) / 1e3:9.2f} us  x{int(row['Calls']):5d}  "
                      f"{row['Name'][:90]}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def timed(fn, iters):
    import torch
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


def gpu(args):
    import torch

    import sr3d_amd
    ops = sr3d_amd.ops
    lr, mask, ys, bs = tensors()
    out = torch.empty_like(ys)

    def call():
        return ops.interp_baseline(lr, mask, SCALE, out=out)

    def call_and_metrics():
        hr, _ = call()
        ops.invalidate_eval_cache()
        return ops.eval_metrics(hr, ys, bs, STDS, 5.0, 0)

    with torch.no_grad():
        _, n = call()
        nb, bound = min_bytes(), min_bytes() / COPY_BW * 1e6
        print(f"LR {SHAPE} x{SCALE}, {float(mask[0].float().mean()):.0%} of the columns built, "
              f"{int(mask.all(dim=0).sum())} through the whole depth, unfilled cells {int(n)}")
        print(f"output + LR bytes {nb / 1e6:.1f} MB -> {bound:.1f} us at {COPY_BW / 1e12:.2f} TB/s")
        med, best = timed(call, args.iters)
        print(f"interp_baseline (5 launches, events around {args.iters} calls x 5): median {med:.1f} us, best "
              f"{best:.1f} us per sample = {nb / best / 1e3:.0f} GB/s, {bound / best:.0%} of the bandwidth bound")
        med2, best2 = timed(call_and_metrics, args.iters)
        print(f"interp_baseline + fused metrics pass: median {med2:.1f} us, best {best2:.1f} us per sample")
    if not args.no_trace:
        trace(args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--calls-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.calls_only:
        calls_only(args)
    elif args.host:
        host(args)
    else:
        gpu(args)


if __name__ == "__main__":
    main()
