#!/usr/bin/env python3
"""Evaluation metrics on the test split by distance from the nearest building: how the error of a trained model (or of
the interpolation baseline) depends on how close a cell is to a wall.  The trainer's whole-domain test loader, one
distance transform and one fused pass per sample (src/wall_distance_profiles.py), one row per distance class:
``distance_cells``, ``distance_m``, a column per metric and the cell counts.  The last row holds every cell farther
than ``--max_distance`` cells; ``MaskedL1NearWall`` / ``MaskedL2NearWall`` at row k are the reference's modules with
``num_filter_applications=k``.

Writes ``wall_distance_scores.csv`` to ``--out_dir``; with ``--baseline`` the interpolation baseline is scored the same
way into ``interpolation_baseline_wall_distance_scores.csv``.  ``--pooled`` divides the numerators summed over the test
split by the summed denominators instead of averaging the per-sample ratios.

    python 3d-sr-micrometeorology_amd/script/evaluate_wall_distance_profiles.py --config_path config/default.yml \\
           --weight_path results/weights.pth --data_root data/DL_data --out_dir results --max_distance 8
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

import torch  # noqa: E402
import yaml  # noqa: E402

from evaluate_vertical_profiles import load_baseline, load_model  # noqa: E402  (same models, same loader)

logger = logging.getLogger()

MODEL_CSV = "wall_distance_scores.csv"
BASELINE_CSV = "interpolation_baseline_wall_distance_scores.csv"


def write_profiles(*, dataloader, model, stds, device, out_dir, file_name, max_distance=8, pooled=False,
                   delta_meter=5.0):
    """score ``model`` over ``dataloader`` and write the table; returns (path, DataFrame)"""
    from sr3d_amd.src.wall_distance_profiles import evaluate_wall_distance_profiles
    df = evaluate_wall_distance_profiles(dataloader=dataloader, model=model, stds=stds, device=device,
                                         max_distance=max_distance, delta_meter=delta_meter, pooled=pooled)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, file_name)
    df.to_csv(path, index=False)
    return path, df


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config_path", type=str, required=True)
    ap.add_argument("--weight_path", type=str, default=None, help="state dict of the trained model")
    ap.add_argument("--data_root", type=str, default=f"{ROOT}/data/DL_data")
    ap.add_argument("--baseline", action="store_true", help="score the interpolation baseline instead of a model")
    ap.add_argument("--lr_build_path", type=str, default=None, help="default: <data root>/10/lr_is_in_build.npy")
    ap.add_argument("--pooled", action="store_true", help="ratio of sums over the split, not the mean of ratios")
    ap.add_argument("--max_distance", type=int, default=8, help="distance classes 1 .. N cells (1 .. 30), then 'farther'")
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
                              max_distance=args.max_distance, pooled=args.pooled)
    logger.info(f"wrote {path}: {len(df)} distance classes x {len(df.columns)} columns")
    logger.info(df[["distance_cells", "distance_m", "MaskedL1", "AbsDiffTemperature", "DiffVelocityNorm", "Cells"]]
                .to_string(index=False))


if __name__ == "__main__":
    main()
