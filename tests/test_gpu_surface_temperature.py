"""Near-surface (2 m) temperature on the MI355X (csrc/sr3d_surface.hip): the kernel bit for bit against the reference
notebook's outputs (tests/golden/surface_temperature.npz) and its numpy restatement (tests/surface_ref.py) on every
branch, in-place reads, the affine step, odd shapes, the fused error sums and their determinism, the notebook-facing
function and script/make_2m_temperature.py end to end."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import surface_ref as sr
from data_fixture import write_synthetic_tree
from helpers import ROOT, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("surface_temperature.npz")


def engine_src(t_nzxy: np.ndarray) -> torch.Tensor:
    """the notebook's (N, Z, X, Y) -> the engine's (N, 1, Z, Y, X) on the GPU"""
    return torch.from_numpy(np.ascontiguousarray(t_nzxy.transpose(0, 1, 3, 2)))[:, None].to(DEV)


def tz_map(building_xy: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(building_xy.T)).to(DEV)


def to_nxy(m: torch.Tensor) -> np.ndarray:
    return m.transpose(1, 2).cpu().numpy()


def assert_same(a: np.ndarray, b: np.ndarray):
    """bit-equal values, NaN in the same places"""
    a, b = torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"NaN differs at {int((na != nb).sum())} columns"
    assert torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)), \
        f"max |diff| {float((a[~na] - b[~nb]).abs().max())}"


def branch_tz(rng, shape, H):
    """building tops over every branch: below H[0], on a level, between, (H[-2], H[-1]], above H[-1], NaN"""
    n = int(np.prod(shape))
    k = rng.integers(0, 6, n)
    v = np.where(k == 0, rng.uniform(-5.0, H[0], n), 0.0)
    v = np.where(k == 1, H[rng.integers(0, len(H), n)], v)
    v = np.where(k == 2, rng.uniform(H[0], H[-1], n), v)
    step = H[-1] - H[-2] if len(H) > 1 else 5.0
    v = np.where(k == 3, H[-1] - rng.uniform(0.0, step, n), v)
    v = np.where(k == 4, rng.uniform(H[-1] + 1e-6, H[-1] + 50.0, n), v)
    v = np.where(k == 5, np.nan, v)
    return v.reshape(shape)


def test_kernel_matches_notebook_on_every_branch(eng, gold):
    tz = tz_map(gold["tz_m0"])
    for k in ("true", "pred"):
        out = eng.ops.surface_temperature(engine_src(gold[k]), tz)
        torch.cuda.synchronize()
        assert_same(to_nxy(out), gold[f"{k}_2m"])


def test_in_place_strided_read_equals_contiguous_slice(eng, gold):
    B, Z, X, Y = gold["true"].shape
    big = torch.randn(B, 4, 40, Y, X, device=DEV) * 3 + 290
    big[:, 2, :32] = engine_src(gold["true"])[:, 0]
    tz = tz_map(gold["tz_m0"])
    a = eng.ops.surface_temperature(big, tz, channel=2, levels=32)
    b = eng.ops.surface_temperature(big[:, 2:3, :32].contiguous(), tz, channel=0, levels=32)
    torch.cuda.synchronize()
    assert_same(a.cpu().numpy(), b.cpu().numpy())
    assert_same(to_nxy(a), gold["true_2m"])


def test_affine_step_is_torch_dimensionalize(eng, gold):
    g = torch.Generator().manual_seed(5)
    B, Z, X, Y = gold["pred"].shape
    p = torch.rand(B, 4, Z, Y, X, generator=g)
    std, mean = torch.Tensor([8.4, 14.4, 21.6, 7.0]), torch.Tensor([300.0, -6.5, -9.1, -3.5])
    dim = p * std[None, :, None, None, None] + mean[None, :, None, None, None]        # make_inference, fp32
    for c in (0, 3):
        out = eng.ops.surface_temperature(p.to(DEV), tz_map(gold["tz_m0"]), channel=c, scale=float(std[c]),
                                          mean=float(mean[c]))
        ref = sr.t2m_ref(dim[:, c].numpy().transpose(0, 1, 3, 2), gold["tz_m0"])
        assert_same(to_nxy(out), ref)


@pytest.mark.parametrize("shape,levels,channel", [((3, 4, 35, 29, 37), 30, 1), ((1, 2, 7, 1, 5), 7, 0),
                                                  ((2, 1, 40, 17, 321), 32, 0), ((3, 1, 3, 3, 3), 1, 0)])
def test_odd_shapes_and_batches(eng, shape, levels, channel):
    rng = np.random.default_rng(sum(shape))
    B, C, Zs, Y, X = shape
    H = np.arange(levels) * 5.0 + 17.5
    x = (290 + 5 * rng.standard_normal(shape)).astype(np.float32)
    x[rng.random(shape) < 0.03] = np.nan
    b_xy = branch_tz(rng, (X, Y), H)
    out = eng.ops.surface_temperature(torch.from_numpy(x).to(DEV), tz_map(b_xy), channel=channel, levels=levels)
    ref = sr.t2m_ref(x[:, channel, :levels].transpose(0, 1, 3, 2), b_xy, H)
    assert_same(to_nxy(out), ref)


def test_nan_t2_propagates_when_tz_is_on_a_level(eng):
    H = np.arange(32) * 5.0 + 17.5
    x = np.full((1, 1, 32, 1, 3), 300.0, np.float32)
    x[0, 0, 5, 0, :] = np.nan                                     # level above H[4]
    b = np.array([[H[4]], [H[4] + 1.0], [np.nan]])                # (X, Y) = (3, 1)
    out = eng.ops.surface_temperature(torch.from_numpy(x).to(DEV), tz_map(b)).cpu().numpy()
    assert np.isnan(out).all()


def test_fused_errors_match_numpy_and_notebook(eng, gold):
    B, Z, X, Y = gold["true"].shape
    big = torch.full((B, 4, 40, Y, X), 123.0, device=DEV)
    big[:, 0, :32] = engine_src(gold["true"])[:, 0]               # the HR truth layout, read in place
    pred = engine_src(gold["pred"])
    pm, tm, acc = eng.ops.surface_temperature_errors(pred, big, tz_map(gold["tz_m0"]))
    torch.cuda.synchronize()
    assert_same(to_nxy(pm), gold["pred_2m"])
    assert_same(to_nxy(tm), gold["true_2m"])
    ref = sr.errors_ref(gold["pred_2m"], gold["true_2m"])
    got = acc.cpu().tolist()
    assert got[2] == ref[2] > 0
    assert abs(got[0] - ref[0]) <= 1e-12 * ref[0] and abs(got[1] - ref[1]) <= 1e-12 * ref[1]
    from sr3d_amd.src.surface_temperature import calc_2m_temperature_errors
    e = calc_2m_temperature_errors(acc)
    assert abs(e["RMSE"] - float(gold["rmse"])) <= 1e-5 * float(gold["rmse"])
    assert abs(e["MAE"] - float(gold["mae"])) <= 1e-5 * float(gold["mae"])
    # maps=False: the same sums, no maps
    pm2, tm2, acc2 = eng.ops.surface_temperature_errors(pred, big, tz_map(gold["tz_m0"]), maps=False)
    assert pm2 is None and tm2 is None and torch.equal(acc2, acc)


@pytest.mark.parametrize("Y,X", [(320, 320), (61, 83)])
def test_fused_sums_are_deterministic_and_per_sample(eng, Y, X):
    """two calls accumulated = one call on the concatenated batch, bit for bit; a repeat gives the same bits"""
    rng = np.random.default_rng(Y + X)
    H = np.arange(32) * 5.0 + 17.5
    b_xy = branch_tz(rng, (X, Y), H)
    tz = tz_map(b_xy)
    p = torch.from_numpy(rng.random((3, 4, 32, Y, X), dtype=np.float32)).to(DEV)
    t = torch.from_numpy((295 + 8 * rng.standard_normal((3, 4, 40, Y, X))).astype(np.float32)).to(DEV)
    kw = dict(pred_scale=8.4, pred_mean=300.0)
    _, _, one = eng.ops.surface_temperature_errors(p, t, tz, maps=False, **kw)
    _, _, two = eng.ops.surface_temperature_errors(p[:1], t[:1], tz, maps=False, **kw)
    _, _, two = eng.ops.surface_temperature_errors(p[1:], t[1:], tz, acc=two, maps=False, **kw)
    pm, tm, again = eng.ops.surface_temperature_errors(p, t, tz, **kw)
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(one, again)
    ref = sr.errors_ref(to_nxy(pm), to_nxy(tm))
    got = one.cpu().tolist()
    assert got[2] == ref[2] and abs(got[0] - ref[0]) <= 1e-12 * ref[0] and abs(got[1] - ref[1]) <= 1e-12 * ref[1]
    dim = (p[:, 0, :32].cpu() * torch.tensor(8.4, dtype=torch.float32) + torch.tensor(300.0)).numpy()
    assert_same(to_nxy(pm), sr.t2m_ref(dim.transpose(0, 1, 3, 2), b_xy, H))
    assert_same(to_nxy(tm), sr.t2m_ref(t[:, 0, :32].cpu().numpy().transpose(0, 1, 3, 2), b_xy, H))


def test_infer_2m_height_temperature_round_trip(eng, gold):
    from sr3d_amd.src.surface_temperature import infer_2m_height_temperature
    out = infer_2m_height_temperature(gold["true"], gold["tz_m0"])
    assert out.shape == gold["true_2m"].shape and out.flags["C_CONTIGUOUS"]
    assert_same(out, gold["true_2m"])


def write_building_file(path, X, Y, margin, H, rng):
    n_i, n_j = X + 2 * margin, Y + 2 * margin
    tz = branch_tz(rng, (n_i, n_j), H)
    with open(path, "w") as f:
        f.write("    i    j        Ez        Tz       Tzl\n")
        for i in range(n_i):
            for j in range(n_j):
                if np.isnan(tz[i, j]):
                    continue                                    # missing pair -> NaN
                f.write(f"{i:5d}{j:5d} {rng.uniform(0, 10):9.2f} {tz[i, j]:.6f} {0.0:9.2f}\n")


def test_make_2m_temperature_script(eng, tmp_path):
    from sr3d_amd.src.building_height_helper import read_building_height
    from sr3d_amd.src.dataloader import make_evaluation_dataloader_without_random_cropping
    HR, L, margin = (40, 32, 32), 24, 2
    data_root = write_synthetic_tree(tmp_path / "d", HR=HR, days=5)
    cfg = {
        "data": {"data_dir_names": ["10"], "train_valid_test_ratios": [0.6, 0.2, 0.2], "hr_org_size": [32, 32, 32],
                 "hr_crop_size": [32, 32, 32], "means": [302.0, -6.5, -9.1, -3.5], "stds": [8.4, 14.4, 21.6, 7.0],
                 "datasizes": {"train": None, "valid": None, "test": None}, "nan_value": 0.0, "seed": 42,
                 "scale_factor": 4},
        "model": {"model_name": "unet", "in_channels": 4, "out_channels": 4, "num_feat0": 4, "num_feat1": 8,
                  "num_feat2": 8, "num_feat3": 16, "num_feat4": 16, "num_x2upsample": 2, "num_latent_layers": 3,
                  "n_layers_in_block": 2, "bias_feat_extraction": False,
                  "conv_mode_feat_extraction": "g_conv_with_separated_bias",
                  "conv_mode_down_block": "g_conv_with_separated_bias", "conv_mode_up_block": None},
    }
    (tmp_path / "exp").mkdir()
    cfg_path = tmp_path / "exp" / "tiny.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    torch.save(eng.make_model(cfg).state_dict(), tmp_path / "w.pth")
    H = np.arange(L) * 5.0 + 17.5
    bpath = tmp_path / "EleTopoZ.txt"
    write_building_file(bpath, HR[2], HR[1], margin, H, np.random.default_rng(9))

    script = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "make_2m_temperature.py")
    common = [sys.executable, script, "--config_path", str(cfg_path), "--data_root", str(data_root), "--building_path",
              str(bpath), "--margin", str(margin), "--num_levels", str(L)]

    def run(extra):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return {k: float(v) for k, v in re.findall(r"^(RMSE|MAE) = (\S+)$", r.stdout, flags=re.M)}

    e1 = run(["--weight_path", str(tmp_path / "w.pth"), "--out_dir", str(tmp_path / "o1"), "--write_sr",
              str(tmp_path / "sr")])
    e2 = run(["--inference_dir", str(tmp_path / "sr"), "--out_dir", str(tmp_path / "o2")])

    ds = make_evaluation_dataloader_without_random_cropping(cfg, data_root, batch_size=1, num_workers=0).dataset
    assert len(ds.hr_files) >= 2
    building = read_building_height(str(bpath), "Tz", margin=margin)           # (X, Y)
    preds, trues = [], []
    for lr_path, hr_path in zip(ds.lr_files, ds.hr_files):
        s = np.load(tmp_path / "sr" / os.path.basename(lr_path).replace("LR", "SR"))
        assert s.shape == (1, 4, 32, 32, 32) and s.dtype == np.float32
        preds.append(sr.t2m_ref(s[:, 0, :L].transpose(0, 1, 3, 2), building, H))
        trues.append(sr.t2m_ref(np.load(hr_path)[None, 0, :L].transpose(0, 1, 3, 2), building, H))
    pred_2m, true_2m = np.concatenate(preds), np.concatenate(trues)
    assert np.isnan(true_2m).any() and np.isfinite(true_2m).any()
    for out in ("o1", "o2"):
        for label, ref in (("pred", pred_2m), ("true", true_2m)):
            with open(tmp_path / out / f"{label}_2m_t_tiny.pickle", "rb") as f:
                assert_same(pickle.load(f), ref)
    d = pred_2m - true_2m                                                        # the notebook's float32 nanmean
    rmse, mae = float(np.sqrt(np.nanmean(d ** 2))), float(np.nanmean(np.abs(d)))
    for e in (e1, e2):
        assert abs(e["RMSE"] - rmse) <= 1e-5 * rmse and abs(e["MAE"] - mae) <= 1e-5 * mae
    assert e1 == e2
