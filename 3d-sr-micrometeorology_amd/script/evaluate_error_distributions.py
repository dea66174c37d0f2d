#!/usr/bin/env python3
"""Error distributions on the test split: how bad the worst cells are, whether the error is biased, and whether the
super-resolved fields reproduce the distribution of the truth.  The trainer's whole-domain test loader and one fused
histogram pass per sample (src/error_distributions.py); one row per (series, class): the signed normalised errors of
the four channels, the velocity-error norm, the predicted and the true fields, over the fluid cells within
``--near_width`` cells of a wall (``near_wall``), the other fluid cells (``far``) and both (``fluid``).  Columns: the
cell, underflow, overflow and NaN counts, the exact min and max, the quantiles ``q0.1 .. q99.9``, ``abs_q50 ..
abs_q99.9`` of |error|, ``w1_to_pred`` (1-Wasserstein distance between the true and the predicted field's histogram)
and everything again in physical units (``*_phys``).

Writes ``error_distribution_scores.csv`` to ``--out_dir``; with ``--baseline`` the interpolation baseline is scored the
same way into ``interpolation_baseline_error_distribution_scores.csv``.  ``--save_histograms`` also writes the pooled
counts, ranges and cell counts as an ``.npz`` next to the table: enough to re-derive any quantile later.  A series with
values outside its range is named in a warning with its exact min and max: widen that range.

    python 3d-sr-micrometeorology_amd/script/evaluate_error_distributions.py --config_path config/default.yml \\
           --weight_path results/weights.pth --data_root data/DL_data --out_dir results --near_width 1
"""
import argparse
import logging
import os
import pathlib
import sys

HERE = str(pathlib.Path(__file__).resolve().parent)
ROOT = str(pathlib.Path(__file__).resolve().parents[2])
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from evaluate_vertical_profiles import load_baseline, load_model  # noqa: E402  (same models, same loader)

logger = logging.getLogger()

MODEL_CSV = "error_distribution_scores.csv"
BASELINE_CSV = "interpolation_baseline_error_distribution_scores.csv"


def write_distributions(*, dataloader, model, config, device, out_dir, file_name, near_width=1, err_range=(-0.5, 0.5),
                        field_range=(-0.5, 1.5), vel_norm_range=(0.0, 8.0), save_histograms=False):
    """score ``model`` over ``dataloader`` and write the table (and the histograms); returns (path, DataFrame)"""
    from sr3d_amd.src.error_distributions import evaluate_error_distributions
    df, hist = evaluate_error_distributions(model, dataloader, config, device=device, near_width=near_width,
                                            err_range=err_range, field_range=field_range,
                                            vel_norm_range=vel_norm_range, return_histograms=True)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, file_name)
    df.to_csv(path, index=False)
    if save_histograms:
        np.savez(os.path.splitext(path)[0] + "_histograms.npz", **hist)
    return path, df


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config_path", type=str, required=True)
    ap.add_argument("--weight_path", type=str, default=None, help="state dict of the trained model")
    ap.add_argument("--data_root", type=str, default=f"{ROOT}/data/DL_data")
    ap.add_argument("--baseline", action="store_true", help="score the interpolation baseline instead of a model")
    ap.add_argument("--lr_build_path", type=str, default=None, help="default: <data root>/10/lr_is_in_build.npy")
    ap.add_argument("--near_width", type=int, default=1, help="near-wall class: fluid cells within N cells of a wall "
                    "(0 .. 254; 0: no near-wall class)")
    ap.add_argument("--err_range", type=float, nargs=2, default=(-0.5, 0.5), metavar=("LO", "HI"),
                    help="range of the signed normalised errors (symmetric ranges also give the |error| quantiles)")
    ap.add_argument("--field_range", type=float, nargs=2, default=(-0.5, 1.5), metavar=("LO", "HI"),
                    help="range of the normalised predicted and true fields")
    ap.add_argument("--vel_norm_range", type=float, nargs=2, default=(0.0, 8.0), metavar=("LO", "HI"),
                    help="range of the velocity-error norm, m/s")
    ap.add_argument("--save_histograms", action="store_true", help="also write the pooled counts, ranges and cells (.npz)")
    ap.add_argument("--out_dir", type=str, default=".")
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format="%(message)s", handlers=[logging.StreamHandler(sys.stdout)])
    if not torch.cuda.is_available():
        raise Exception("No GPU.")

    import sr3d_amd  # noqa: F401
    from sr3d_amd.src.dataloader import make_evaluation_dataloader_without_random_cropping

    with open(args.config_path) as f:
        config = yaml.safe_load(f)
    loader = make_evaluation_dataloader_without_random_cropping(config, pathlib.Path(args.data_root), batch_size=1,
                                                                num_workers=0)
    model = (load_baseline(args, config, loader) if args.baseline else load_model(args, config)).to("cuda:0").eval()
    path, df = write_distributions(dataloader=loader, model=model, config=config, device="cuda:0", out_dir=args.out_dir,
                                   file_name=BASELINE_CSV if args.baseline else MODEL_CSV, near_width=args.near_width,
                                   err_range=tuple(args.err_range), field_range=tuple(args.field_range),
                                   vel_norm_range=tuple(args.vel_norm_range), save_histograms=args.save_histograms)
    logger.info(f"wrote {path}: {len(df)} rows x {len(df.columns)} columns")
    logger.info(df[df["class"] == "fluid"][["series", "cells", "underflow", "overflow", "q1", "q50", "q99"]]
                .to_string(index=False))


if __name__ == "__main__":
    main()
