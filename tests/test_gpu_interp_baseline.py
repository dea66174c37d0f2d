"""The interpolation baseline on the MI355X (csrc/sr3d_interp.hip): the trilinear upsample alone against CPU
F.interpolate, every fill rule against the numpy restatement (tests/interp_baseline_ref.py, pinned to scipy by
tests/golden/interp_baseline.npz), a realistic tower mask twice in a row / on a strided view / on an unaligned output,
the nn.Module through optim_helper.evaluate, fill_na's asserts and script/evaluate_interpolation_baseline.py end to end.

Tolerances.  Trilinear: the kernel's summation order is chosen to match ATen's CPU kernel for contiguous tensors (each
w0 * a + w1 * b as fma(a, w0, fl(w1 * b))), so the upsample is asserted BIT-EQUAL to F.interpolate; the plain sum would
differ in about 30 % of the cells.  The 2 ulp of the largest magnitude in the 8-cell stencil that any fp32 evaluation of
the same exactly-weighted sum meets is asserted first, so a failure says which of the two it is.  Filled cells: the fill
is fp64 rounded once, so with a bit-equal upsample the whole output is asserted bit-equal to the fp32 restatement, and
max|a - b| / max|b| <= 1e-5 against the fp64 restatement, the project's fp32 parity bound (the fp32 restatement sits at
3-7e-7 on these shapes).  No case needs the tolerance."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F
import yaml

import interp_baseline_ref as R
from data_fixture import write_synthetic_tree
from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "evaluate_interpolation_baseline.py")
CASES = [(n, s) for s in sorted(R.RULE_SHAPES) for n in sorted(R.RULE_CASES)]
STDS = [8.4, 14.4, 21.6, 7.0]


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


def run_op(eng, lr, mask, scale, **kw):
    lr_t = lr if isinstance(lr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lr)).to(DEV)
    with torch.no_grad():
        hr, n = eng.ops.interp_baseline(lr_t, torch.from_numpy(np.asarray(mask)).to(DEV), scale, **kw)
    return hr.cpu().numpy(), int(n)


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN differs at {int((na != nb).sum())} cells"
    ok = a[~na].view(np.int32) == b[~nb].view(np.int32)
    assert ok.all(), f"{int((~ok).sum())} cells differ, max |diff| {float(np.abs(a[~na] - b[~nb]).max())}"


def stencil_max(lr, scale):
    """the largest |value| among the 8 LR cells each HR cell is interpolated from"""
    def idx(n):
        src = np.maximum(np.float32(0), np.float32(1 / scale) * (np.arange(n * scale, dtype=np.float32)
                                                                + np.float32(0.5)) - np.float32(0.5))
        i0 = src.astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1)
    a = np.abs(lr)
    zs, ys, xs = (idx(n) for n in lr.shape[-3:])
    m = np.zeros(lr.shape[:-3] + tuple(scale * n for n in lr.shape[-3:]), np.float32)
    for iz in zs:
        for iy in ys:
            for ix in xs:
                m = np.maximum(m, a[..., iz[:, None, None], iy[None, :, None], ix[None, None, :]])
    return m


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("shape", [(1, 4, 3, 5, 7), (2, 3, 4, 6, 5), (1, 4, 2, 4, 17)])
def test_trilinear_alone(eng, shape, scale):
    g = torch.Generator().manual_seed(sum(shape) + scale)
    lr = torch.randn(shape, generator=g) * torch.tensor([300.0, 5.0, 5.0, 1.0])[:shape[1], None, None, None]
    want = F.interpolate(lr, scale_factor=scale, mode="trilinear").numpy()
    got, n = run_op(eng, lr.numpy(), np.zeros(shape[2:], np.uint8), scale)
    assert n == 0 and got.shape == want.shape and not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - want) / np.spacing(stencil_max(lr.numpy(), scale))
    print(f"trilinear {shape} x{scale}: {int((got != want).sum())} of {got.size} cells differ, "
          f"max {err.max():.2f} ulp of the stencil maximum")
    assert err.max() <= 2.0
    same_bits(got, want)                                 # ATen's order of rounding, not only a reordering of it


@pytest.mark.parametrize("name,scale", CASES)
def test_rule_cases(eng, name, scale):
    lr, mask = R.rule_case(name, scale)
    f32 = R.interp_baseline_ref(lr[None], mask, scale)
    f64 = R.interp_baseline_ref(lr[None], mask, scale, dtype=np.float64)
    after_mask, after_z, after_y, after_x = f32["n_nan"]
    done = R.RULE_CASES[name]
    assert after_mask > 0 and (after_z == 0) == (done == "z") and (after_y == 0) == (done in ("z", "y"))
    assert (after_x == 0) == (done != "never")

    got, n = run_op(eng, lr[None], mask, scale)
    plain, n0 = run_op(eng, lr[None], np.zeros_like(mask), scale)
    assert n == after_x and np.array_equal(np.isnan(got), np.isnan(f32["out"]))
    kept = ~np.isnan(f32["masked"])                      # valid after step 2: the kernel's own upsample, untouched
    assert np.array_equal(got[kept].view(np.int32), plain[kept].view(np.int32))
    assert n0 == 0 and not np.isnan(plain).any()         # (lr_nan: its NaN cells are filled along z as well)
    # the fill bit for bit: the restatement's three passes on the kernel's own masked upsample
    same_bits(got, R.fill(np.where(np.isnan(f32["masked"]), np.float32(np.nan), plain))[0])
    # ... and everything against the fp64 restatement, then bit for bit against the fp32 one
    fin = ~np.isnan(f64["out"])
    if fin.any():
        err = np.abs(got[fin] - f64["out"][fin]).max() / np.abs(f64["out"][fin]).max()
        print(f"{name} x{scale}: {err:.2e} of the fp64 restatement, {int((got[fin] != f32['out'][fin]).sum())} cells "
              "differ from the fp32 one")
        assert err <= TOL
    same_bits(got, f32["out"])


def test_tower_mask_repeat_strided_and_unaligned(eng):
    lr, mask = R.tower_case()
    f32 = R.interp_baseline_ref(lr, mask, 4)
    f64 = R.interp_baseline_ref(lr, mask, 4, dtype=np.float64)
    assert f32["n_nan"][1] > 0 and f32["n_nan"][3] == 0
    lr_t, m_t = torch.from_numpy(lr).to(DEV), torch.from_numpy(mask).to(DEV)
    out = torch.empty(1, 4, 32, 80, 96, device=DEV)
    with torch.no_grad():
        a, na = eng.ops.interp_baseline(lr_t, m_t, 4, out=out)
        first = a.clone()
        b, nb = eng.ops.interp_baseline(lr_t, m_t, 4, out=out)             # twice on the same buffers
        assert b.data_ptr() == out.data_ptr() and int(na) == int(nb) == 0
        assert torch.equal(first.view(torch.int32), b.view(torch.int32))
        big = torch.full((1, 9, 8, 20, 24), float("inf"), device=DEV)
        view = big[:, 1::2]                                                # offset, channel stride of two volumes
        view.copy_(lr_t)
        assert not view.is_contiguous()
        c, _ = eng.ops.interp_baseline(view, m_t.bool(), 4)
        assert torch.equal(first.view(torch.int32), c.view(torch.int32))
        flat = torch.empty(first.numel() + 1, device=DEV)
        off = flat[1:].view(first.shape)                                   # base 4 bytes past a 16-byte boundary
        assert off.data_ptr() % 16 == 4
        d, _ = eng.ops.interp_baseline(lr_t, m_t.double(), 4, out=off)
        assert torch.equal(first.view(torch.int32), d.view(torch.int32))
    got = first.cpu().numpy()
    plain, _ = run_op(eng, lr, np.zeros_like(mask), 4)
    same_bits(got, R.fill(np.where(np.isnan(f32["masked"]), np.float32(np.nan), plain))[0])
    err = np.abs(got - f64["out"]).max() / np.abs(f64["out"]).max()
    print(f"tower: {err:.2e} of the fp64 restatement")
    assert err <= TOL
    same_bits(got, f32["out"])


def test_python_argument_errors(eng):
    ops = eng.ops
    lr = torch.rand(1, 4, 3, 5, 7, device=DEV)
    m = torch.zeros(3, 5, 7, dtype=torch.uint8, device=DEV)
    for args, exc in (((lr, m, 3), ValueError), ((lr, m[:2], 4), ValueError), ((lr[0], m, 4), ValueError),
                      ((lr.double(), m, 4), TypeError), ((lr.cpu(), m, 4), RuntimeError), ((lr, m.cpu(), 4), ValueError),
                      ((lr[..., ::2], m[..., ::2], 4), ValueError)):
        with pytest.raises(exc):
            ops.interp_baseline(*args)
    with pytest.raises(ValueError):
        ops.interp_baseline(lr, m, 4, out=torch.empty(1, 4, 12, 20, 27, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.interp_baseline(lr.clone().requires_grad_(True), m, 4)
    # the C ABI on the device: a good call, then a short workspace
    L = eng._lib
    import ctypes as C
    out, n = torch.empty(1, 4, 12, 20, 28, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.lib.sr3d_interp_baseline_workspace_bytes(1, 4, 3, 5, 7, 4), dtype=torch.uint8, device=DEV)
    call = lambda nbytes: L.lib.sr3d_interp_baseline(  # noqa: E731
        C.c_void_p(lr.data_ptr()), 420, 105, L.DTYPE_F32, 1, 4, 3, 5, 7, C.c_void_p(m.data_ptr()), 3, 5, 7, 4,
        C.c_void_p(out.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, L.stream_ptr())
    assert call(ws.numel()) == 0 and call(ws.numel() - 4) == -3
    ws = torch.empty(ws.numel() + 4, dtype=torch.uint8, device=DEV)[2:]    # a workspace that is not 4-byte aligned
    assert ws.data_ptr() % 4 == 2 and call(ws.numel()) == -1 and "4-byte aligned" in L.lib.sr3d_last_error().decode()
    torch.cuda.synchronize()
    assert int(n) == 0 and not torch.isnan(out).any()


def metric_modules(lm):
    return {"L1": lm.MyL1Loss(), "MaskedL1": lm.MaskedL1Loss(), "MaskedL1NearWall": lm.MaskedL1LossNearWall(),
            "ResidualContinuityEq": lm.ResidualContinuity(STDS[1:]), "AbsDiffTemperature": lm.AbsDiffTemperature(STDS[0]),
            "DiffVelocityNorm": lm.DiffVelocityVectorNorm(STDS[1:]),
            "AbsDiffTemperatureLevZero": lm.AbsDiffTemperature(STDS[0], lev=0),
            "DiffVelocityNormLevZero": lm.DiffVelocityVectorNorm(STDS[1:], lev=0),
            "AbsDiffDivergence": lm.AbsDiffDivergence(STDS[1:]), "DiffOmegaVectorNorm": lm.DiffOmegaVectorNorm(STDS[1:])}


def test_module_through_evaluate(eng):
    from sr3d_amd.src.interpolation_baseline import InterpolationBaseline
    from sr3d_amd.src.optim_helper import evaluate
    L, lm = eng._lib, eng.src.loss_maker
    g = torch.Generator().manual_seed(12)
    mask = (torch.arange(2)[:, None, None] < torch.randint(0, 3, (4, 6), generator=g)[None]).to(torch.uint8)
    samples = [(torch.rand(1, 4, 2, 4, 6, generator=g), (torch.rand(1, 8, 16, 24, generator=g) > 0.2).float(),
                torch.rand(1, 4, 8, 16, 24, generator=g)) for _ in range(2)]
    model = InterpolationBaseline(mask.numpy().astype(np.float64), 4).to(DEV)
    assert list(model.parameters()) == [] and model.lr_is_in_build.device.type == "cuda"
    res = evaluate(dataloader=samples, model=model, loss_fns=metric_modules(lm), device=DEV)
    assert int(model.n_unfilled) == 0
    direct = []
    with torch.no_grad():
        for Xs, bs, ys in samples:
            hr, _ = eng.ops.interp_baseline(Xs.to(DEV), mask.to(DEV), 4)
            assert torch.equal(model(Xs.to(DEV), None), hr) and tuple(hr.shape) == (1, 4, 8, 16, 24)
            direct.append(eng.ops.eval_metrics(hr, ys.to(DEV), bs.unsqueeze(1).to(DEV), STDS, 5.0, 0).cpu().clone())
    # the meter adds Python floats (the fp32 values, exactly) and divides by the count: the same in fp64 here
    mean = (direct[0].double() + direct[1].double()) / 2
    index = {"L1": "L1", "MaskedL1": "MaskedL1", "MaskedL1NearWall": "MaskedL1NearWall",
             "ResidualContinuityEq": "ResidualContinuity", "AbsDiffTemperature": "AbsDiffTemperature",
             "DiffVelocityNorm": "DiffVelocityNorm", "AbsDiffTemperatureLevZero": "AbsDiffTemperatureLev",
             "DiffVelocityNormLevZero": "DiffVelocityNormLev", "AbsDiffDivergence": "AbsDiffDivergence",
             "DiffOmegaVectorNorm": "DiffOmegaNorm"}
    for name, meter in res.items():
        want = float(mean[L.EVAL_INDEX[index[name]]])
        assert meter.count == 2 and meter.avg == want, (name, meter.avg, want)


def test_fill_na_asserts(eng):
    from sr3d_amd.src.interpolation_baseline import fill_na
    lr, mask = R.rule_case("column", 4)
    out = fill_na(torch.from_numpy(lr), mask.astype(np.float64))
    assert tuple(out.shape) == (4, 12, 20, 28) and out.is_cuda and not torch.isnan(out).any()
    same_bits(out.cpu().numpy(), run_op(eng, lr[None], mask, 4)[0][0])
    with pytest.raises(AssertionError, match="No Nan values"):
        fill_na(torch.from_numpy(lr), np.zeros_like(mask))
    with pytest.raises(AssertionError):
        fill_na(torch.from_numpy(lr), np.ones_like(mask))


def test_script_end_to_end(eng, tmp_path):
    from sr3d_amd.src.dataloader import make_evaluation_dataloader_without_random_cropping
    from sr3d_amd.src.interpolation_baseline import InterpolationBaseline
    from sr3d_amd.src.optim_helper import evaluate
    HR = (32, 16, 24)
    data_root = write_synthetic_tree(tmp_path / "d", HR=HR, days=5)
    hr_build = np.load(data_root / "10" / "hr_is_in_build.npy")[0]
    lr_build = hr_build.reshape(8, 4, 4, 4, 6, 4).mean(axis=(1, 3, 5)) > 0.5
    lr_build[:, 1, 2] = True                         # a whole column: the y pass has work
    lr_file = np.zeros((4, 10, 4, 6))                # more levels than the loader's LR, as the LR-data script writes
    lr_file[:, :8] = lr_build
    np.save(data_root / "10" / "lr_is_in_build.npy", lr_file)
    cfg = {"data": {"data_dir_names": ["10"], "train_valid_test_ratios": [0.6, 0.2, 0.2], "hr_org_size": list(HR),
                    "hr_crop_size": list(HR), "means": [302.0, -6.5, -9.1, -3.5], "stds": STDS,
                    "datasizes": {"train": None, "valid": None, "test": None}, "nan_value": 0.0, "seed": 42,
                    "scale_factor": 4},
           "model": {"model_name": "unet", "num_x2upsample": 2}}
    cfg_path = tmp_path / "tiny.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, SCRIPT, "--config_path", str(cfg_path), "--data_root", str(data_root),
                        "--out_dir", str(tmp_path / "o")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    scores = pd.read_csv(tmp_path / "o" / "interpolation_baseline_scores.csv")
    names = list(metric_modules(eng.src.loss_maker))
    assert list(scores.columns) == names and len(scores) == 1

    loader = make_evaluation_dataloader_without_random_cropping(cfg, data_root, batch_size=1, num_workers=0)
    assert len(loader.dataset) >= 2
    model = InterpolationBaseline(lr_build, 4).to(DEV)
    res = evaluate(dataloader=loader, model=model, loss_fns=metric_modules(eng.src.loss_maker), device=DEV)
    for k in names:
        assert np.isfinite(res[k].avg) and abs(float(scores[k][0]) - res[k].avg) <= 1e-9 * abs(res[k].avg), k
        assert f"{k}: {res[k].avg:.8f}" in r.stdout
