"""Rotation about z and the fused equivariance error on the MI355X (csrc/sr3d_rotate.hip) against the reference's
scipy outputs (tests/golden/equivariance*.npz) and the fp64 restatement tests/rotate_ref.py."""
import numpy as np
import pytest
import torch

import rotate_ref as rr
from helpers import cfg_of, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EDGE = 1e-9


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def eq(eng):
    from sr3d_amd.src import equivariance_error_calculator
    return equivariance_error_calculator


@pytest.fixture(scope="module")
def gold():
    return load_golden("equivariance.npz")


@pytest.fixture(scope="module")
def gm():
    return load_golden("equivariance_model.npz")


def key(a):
    return f"{a:+.1f}"


def edge_band(angle, Y, X):
    """(Y, X) bool: source coordinate within EDGE of a plane edge -- the inside / outside call there rests on the last
    bit of the fp64 coordinate, so those voxels are excluded (and asserted to be few)"""
    cy, cx = rr.source_coords(angle, Y, X)
    def near(c, n):   # an exact hit (multiples of 90 degrees: integer coordinates) is unambiguous
        return ((c.abs() < EDGE) & (c != 0)) | (((c - (n - 1)).abs() < EDGE) & (c != n - 1))

    band = (near(cy, Y) & (cx >= -EDGE) & (cx <= X - 1 + EDGE)) | (near(cx, X) & (cy >= -EDGE) & (cy <= Y - 1 + EDGE))
    assert int(band.sum()) <= max(4, (Y + X) // 4), (angle, int(band.sum()))
    return band.numpy()


def lr_fields(g):
    return torch.rand(1, 4, 8, 80, 80, generator=torch.Generator().manual_seed(int(g["fb/seed"])))


def test_fields_and_mask_against_scipy(eng, gold):
    m, s = gold["means"], gold["scales"]
    xa = torch.from_numpy(gold["fa/x"]).to(DEV)
    xb = lr_fields(gold).to(DEV)
    bm = torch.from_numpy(gold["mk/b"]).to(DEV)
    for a in gold["angles"]:
        for x, pk in ((xa, "fa"), (xb, "fb")):
            y = eng.ops.rotate_fields(x, m, s, a).cpu().numpy()
            keep = ~edge_band(a, x.shape[-2], x.shape[-1])
            for i, (b, c, z) in enumerate(gold[f"{pk}/planes"]):
                err = np.abs(y[b, c, z] - gold[f"{pk}/{key(a)}"][i])[keep]
                assert err.max() <= 1e-6, (pk, a, b, c, z, err.max())
        ref = gold[f"mk/{key(a)}"]
        th = np.float32(0.1)
        got = eng.ops.rotate_building(bm, a, 0.1).cpu().numpy()
        exp = (ref > th).astype(np.float32)
        tie = np.abs(ref - th) <= 1e-6
        assert np.array_equal(got[~tie], exp[~tie]), a
        assert set(np.unique(got)) <= {0.0, 1.0}


def test_multiples_of_90_are_exact_rot90(eng, gold):
    m, s = gold["means"], gold["scales"]
    x = lr_fields(gold)
    mt = torch.tensor(m).view(1, 4, 1, 1, 1)
    st = torch.tensor(s).view(1, 4, 1, 1, 1)
    phys = x.double() * st + mt
    for a, k in ((90.0, 1), (180.0, 2), (-90.0, -1), (450.0, 1)):
        exp = ((rr.mix_velocity(torch.rot90(phys, k, dims=(-2, -1)), a) - mt) / st).clamp(0, 1)
        got = eng.ops.rotate_fields(x.to(DEV), m, s, a).cpu().double()
        assert (got - exp).abs().max() <= 1.2e-7, a      # one fp32 rounding of the output
        b = (torch.rand(1, 2, 3, 80, 80, generator=torch.Generator().manual_seed(3)) > 0.5).float()
        gb = eng.ops.rotate_building(b.to(DEV), a).cpu()
        assert torch.equal(gb, torch.rot90(b, k, dims=(-2, -1))), a


@pytest.mark.parametrize("shape", [(2, 4, 3, 37, 53), (1, 4, 2, 1, 7), (3, 4, 1, 5, 1), (1, 4, 5, 2, 3), (1, 4, 1, 1, 1),
                                   (1, 4, 6, 67, 45)])
def test_odd_shapes_against_restatement(eng, gold, shape):
    m, s = gold["means"], gold["scales"]
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    for a in (30.0, -63.0, 17.5, 90.0, 200.0):
        exp = rr.rotate_fields(x, m, s, a).numpy()
        got = eng.ops.rotate_fields(x.to(DEV), m, s, a).cpu().numpy()
        keep = ~edge_band(a, shape[-2], shape[-1])
        assert np.abs(got - exp)[..., keep].max() <= 1e-6, (shape, a)
        phys = eng.ops.rotate_fields(x.to(DEV), m, s, a, rescaled=False).cpu().numpy()
        exp_p = rr.rotate_fields(x, m, s, a, rescaled=False).numpy()
        assert (np.abs(phys - exp_p)[..., keep] <= 1e-6 * np.maximum(1.0, np.abs(exp_p)[..., keep])).all(), (shape, a)
        b = x[:, :2]
        gb = eng.ops.rotate_building(b.to(DEV), a, 0.4).cpu().numpy()
        v = rr.rotate(b, a).float().numpy()
        sure = (np.abs(v - np.float32(0.4)) > 1e-6) & keep
        assert np.array_equal(gb[sure], (v > np.float32(0.4)).astype(np.float32)[sure]), (shape, a)


def test_fused_error_on_reference_predictions(eng, gm):
    sx, ex, sy, ey = (int(v) for v in gm["window"])
    preds = torch.from_numpy(gm["preds"]).to(DEV)
    par = torch.from_numpy(gm["preds_after_rot"]).to(DEV)
    out = eng.ops.equivariance_errors(preds, par, gm["means"], gm["scales"], float(gm["angle"]), sx, ex, sy, ey)
    out = out.cpu().numpy()
    for i, k in enumerate(("tm", "vr", "vl_vp")):
        ref = float(gm[f"err/{k}"])
        assert abs(out[i] - ref) <= 1e-5 * abs(ref), (k, out[i], ref)


def _tiny_model(eng):
    tiny = load_golden("model_tiny_a.npz")
    model = eng.make_model(cfg_of(tiny))
    model.load_state_dict(sub(tiny, "sd"))
    return model.to(DEV)


def test_end_to_end_against_reference_dict(eng, eq, gm):
    model = _tiny_model(eng)
    sx, ex, sy, ey = (int(v) for v in gm["window"])
    kw = dict(model=model, means=list(gm["means"]), scales=list(gm["scales"]), angle=float(gm["angle"]), sx=sx, ex=ex,
              sy=sy, ey=ey, device="cuda:0")
    x, b = torch.from_numpy(gm["x"]), torch.from_numpy(gm["b"])
    d_cpu = eq.calc_equivariance_errors(Xs=x, bs=b, **kw)
    d_np = eq.calc_equivariance_errors(Xs=gm["x"], bs=gm["b"], **kw)
    d_dev = eq.calc_equivariance_errors(Xs=x.to(DEV), bs=b.to(DEV), **kw)
    assert set(d_cpu) == {"tm", "vr", "vl_vp"}
    for k in d_cpu:
        ref = float(gm[f"err/{k}"])
        assert isinstance(d_cpu[k], np.float64)
        assert abs(d_cpu[k] - ref) <= 1e-4 * abs(ref), (k, d_cpu[k], ref)
        assert d_cpu[k] == d_np[k] == d_dev[k], k
    # the reference's other public functions, in its types
    rp, pa = eq.calc_preds_for_equivariance_errors(Xs=x, bs=b, model=model, means=kw["means"], scales=kw["scales"],
                                                   angle=kw["angle"], device="cuda:0")
    assert isinstance(rp, np.ndarray) and rp.dtype == np.float64 and rp.shape == (1, 4, 16, 32, 48)
    d = rp - pa
    assert abs(eq.calc_error_ratio(d[:, 0], sx, ex, sy, ey) - d_cpu["tm"]) <= 1e-6 * d_cpu["tm"]
    rb = eq.rotate_building_height(b, 30.0)
    assert isinstance(rb, np.ndarray) and rb.dtype == np.float32
    rx = eq.rotate_temperature_velocity(gm["x"], kw["means"], kw["scales"], 30.0)
    assert isinstance(rx, np.ndarray) and rx.dtype == np.float64 and rx.shape == gm["x"].shape


def test_bf16_storage_model_runs(eng, eq, gm):
    tiny = load_golden("model_tiny_a.npz")
    cfg = cfg_of(tiny)
    cfg["model"]["storage_dtype"] = "bf16"
    model = eng.make_model(cfg)
    model.load_state_dict(sub(tiny, "sd"))
    model.to(DEV)
    sx, ex, sy, ey = (int(v) for v in gm["window"])
    d = eq.calc_equivariance_errors(Xs=gm["x"], bs=gm["b"], model=model, means=list(gm["means"]),
                                    scales=list(gm["scales"]), angle=30.0, sx=sx, ex=ex, sy=sy, ey=ey, device="cuda:0")
    for k in d:   # bf16 activations: the same errors to within bf16 noise of the two predictions
        ref = float(gm[f"err/{k}"])
        assert np.isfinite(d[k]) and 0.5 * ref <= d[k] <= 2.0 * ref, (k, d[k], ref)


def test_full_size_at_30_degrees(eng, gold):
    m, s = gold["means"], gold["scales"]
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 4, 32, 320, 320, generator=g)
    b = (torch.rand(1, 1, 32, 320, 320, generator=g) > 0.3).float()
    a = 30.0
    keep = ~edge_band(a, 320, 320)
    y = eng.ops.rotate_fields(x.to(DEV), m, s, a).cpu().numpy()
    yb = eng.ops.rotate_building(b.to(DEV), a).cpu().numpy()
    for c, z in ((0, 0), (1, 5), (2, 5), (3, 31), (1, 17), (2, 30), (0, 12), (3, 8)):
        exp = rr.rotate_fields(x[:, :, z:z + 1], m, s, a).numpy()[0, c, 0]
        assert np.abs(y[0, c, z] - exp)[keep].max() <= 1e-6, (c, z)
        v = rr.rotate(b[:, :, z:z + 1], a).float().numpy()[0, 0, 0]
        sure = (np.abs(v - np.float32(0.1)) > 1e-6) & keep
        assert np.array_equal(yb[0, 0, z][sure], (v > np.float32(0.1)).astype(np.float32)[sure]), z
    # fused error against a host fp64 evaluation (preds_after_rot: a perturbed rotation, as a model would give)
    par = (torch.from_numpy(y) + 0.01 * torch.rand(1, 4, 32, 320, 320, generator=g)).float()
    win = (40, -40, 25, 300)
    got = eng.ops.equivariance_errors(x.to(DEV), par.to(DEV), m, s, a, *win).cpu().numpy()
    exp = rr.equivariance_errors(x, par, m, s, a, *win)
    for i in range(3):
        assert abs(got[i] - exp[i]) <= 1e-6 * abs(exp[i]), (i, got[i], exp[i])


def test_angle_sweep_equals_single_calls(eng, eq, gm):
    model = _tiny_model(eng)
    kw = dict(Xs=gm["x"], bs=gm["b"], model=model, means=list(gm["means"]), scales=list(gm["scales"]), sx=2, ex=-3,
              sy=-20, ey=30, device="cuda:0")
    angles = [30.0, 90.0, -63.0, 17.5]
    sweep = eq.calc_equivariance_errors_over_angles(angles=angles, **kw)
    assert len(sweep) == len(angles)
    for a, d in zip(angles, sweep):
        single = eq.calc_equivariance_errors(angle=a, **kw)
        assert d == single, (a, d, single)
