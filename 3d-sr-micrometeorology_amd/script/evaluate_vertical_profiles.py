#!/usr/bin/env python3
"""Vertical profiles of the evaluation metrics on the test split: how the error of a trained model (or of the
interpolation baseline) depends on height.  The trainer's whole-domain test loader, one fused pass per sample
(src/level_profiles.py), one row per level: ``level``, ``height_m``, a column per metric and the cell counts.

Writes ``vertical_profile_scores.csv`` to ``--out_dir``; with ``--baseline`` the interpolation baseline is scored the
same way into ``interpolation_baseline_vertical_profile_scores.csv`` (LR building mask as in
script/evaluate_interpolation_baseline.py).  ``--pooled`` divides the numerators summed over the test split by the
summed denominators instead of averaging the per-sample ratios.

    python 3d-sr-micrometeorology_amd/script/evaluate_vertical_profiles.py --config_path config/default.yml \\
           --weight_path results/weights.pth --data_root data/DL_data --out_dir results
"""
import argparse
import logging
import os
import pathlib
import sys

ROOT = str(pathlib.Path(__file__).resolve().parents[2])
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

logger = logging.getLogger()

MODEL_CSV = "vertical_profile_scores.csv"
BASELINE_CSV = "interpolation_baseline_vertical_profile_scores.csv"


def write_profiles(*, dataloader, model, stds, device, out_dir, file_name, pooled=False, delta_meter=5.0):
    """score ``model`` over ``dataloader`` and write the table; returns (path, DataFrame)"""
    from sr3d_amd.src.level_profiles import evaluate_level_profiles
    df = evaluate_level_profiles(dataloader=dataloader, model=model, stds=stds, device=device,
                                 delta_meter=delta_meter, pooled=pooled)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, file_name)
    df.to_csv(path, index=False)
    return path, df


def load_baseline(args, config, loader):
    from sr3d_amd.src.interpolation_baseline import InterpolationBaseline
    scale = 2 ** int(config["model"]["num_x2upsample"])
    z_lr = loader.dataset[0][0].shape[1]
    build_path = args.lr_build_path or os.path.join(args.data_root, "10", "lr_is_in_build.npy")
    lr_is_in_build = np.load(build_path)
    if lr_is_in_build.ndim != 4 or lr_is_in_build.shape[1] < z_lr:
        raise ValueError(f"{build_path}: expected (channels, >= {z_lr}, y, x), got {lr_is_in_build.shape}")
    return InterpolationBaseline(lr_is_in_build[0, :z_lr], scale)


def load_model(args, config):
    from sr3d_amd.src.model_maker import make_model
    if not args.weight_path:
        raise ValueError("--weight_path is required unless --baseline is given")
    model = make_model(config)
    model.load_state_dict(torch.load(args.weight_path, map_location="cpu"))
    return model


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config_path", type=str, required=True)
    ap.add_argument("--weight_path", type=str, default=None, help="state dict of the trained model")
    ap.add_argument("--data_root", type=str, default=f"{ROOT}/data/DL_data")
    ap.add_argument("--baseline", action="store_true", help="score the interpolation baseline instead of a model")
    ap.add_argument("--lr_build_path", type=str, default=None, help="default: <data root>/10/lr_is_in_build.npy")
    ap.add_argument("--pooled", action="store_true", help="ratio of sums over the split, not the mean of ratios")
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
    path, df = write_profiles(dataloader=loader, model=model, stds=config["data"]["stds"], device="cuda:0",
                              out_dir=args.out_dir, file_name=BASELINE_CSV if args.baseline else MODEL_CSV,
                              pooled=args.pooled)
    logger.info(f"wrote {path}: {len(df)} levels x {len(df.columns)} columns")
    logger.info(df[["level", "height_m", "AbsDiffTemperature", "DiffVelocityNorm", "FluidCells"]].to_string(index=False))


if __name__ == "__main__":
    main()
