"""CPU-side checks of the rotation / equivariance-error feature: the fp64 restatement (tests/rotate_ref.py) against
the reference's scipy outputs, argument validation of the C ABI, the workspace size, and no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import rotate_ref as rr
from helpers import load_golden


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("equivariance.npz")


def key(a):
    return f"{a:+.1f}"


def lr_fields(g):
    x = torch.rand(1, 4, 8, 80, 80, generator=torch.Generator().manual_seed(int(g["fb/seed"])))
    assert abs(float(x.double().sum()) - float(g["fb/sum"])) < 1e-6
    return x


def test_restatement_matches_scipy_fields(gold):
    m, s = gold["means"], gold["scales"]
    xb = lr_fields(gold)
    for a in gold["angles"]:
        ya = rr.rotate_fields(torch.from_numpy(gold["fa/x"]), m, s, a).numpy()
        got = np.stack([ya[b, c, z] for b, c, z in gold["fa/planes"]])
        assert np.abs(got - gold[f"fa/{key(a)}"]).max() <= 1e-12, a
        pb = gold["fb/planes"]
        for i, (b, c, z) in enumerate(pb):
            # one (b, z) slab of all 4 channels is enough: the channel mix only couples channels of one plane
            yb = rr.rotate_fields(xb[b:b + 1, :, z:z + 1], m, s, a).numpy()[0, c, 0]
            assert np.abs(yb - gold[f"fb/{key(a)}"][i]).max() <= 1e-12, a


def test_restatement_matches_scipy_mask(gold):
    b = torch.from_numpy(gold["mk/b"])
    for a in gold["angles"]:
        got = rr.rotate(b, a).numpy()
        # scipy rounded its fp64 result to fp32: within one fp32 ulp of values <= 1
        assert np.abs(got - gold[f"mk/{key(a)}"]).max() <= 1.2e-7, a


def test_restatement_small_planes():
    """folded mirror extension (n < 28), n = 1 and n = 2 against closed forms: a constant plane is reproduced inside"""
    for Y, X in ((1, 1), (1, 7), (2, 3), (5, 1), (13, 29)):
        a = torch.full((1, 1, Y, X), 0.75, dtype=torch.float64)
        assert torch.allclose(rr.spline_coefficients(a), a, rtol=0, atol=1e-14)
        r = rr.rotate(a, 0.0)
        assert torch.allclose(r, a, rtol=0, atol=1e-14)


def test_workspace_bytes(eng):
    f = eng._lib.lib.sr3d_rotate_workspace_bytes
    n = 1 * 4 * 32 * 320 * 320
    blocks = 20 * 20 * 8 * 1     # 16 x 16 tiles of the full plane, 4 z planes per workgroup
    assert f(1, 4, 32, 320, 320) == 2 * 8 * n + 3 * 8 * blocks
    assert f(2, 1, 3, 37, 53) == 2 * 8 * (2 * 3 * 37 * 53) + 3 * 8 * (3 * 4 * 1 * 2)
    assert f(0, 4, 8, 8, 8) == 0 and f(1, 4, 8, -1, 8) == 0


def test_argument_errors_are_reported_not_crashes(eng):
    L = eng._lib
    lib = L.lib
    m = (C.c_double * 4)(302.0, -6.5, -9.1, -3.5)
    s = (C.c_double * 4)(8.4, 14.4, 21.6, 7.0)
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below fails validation on the host
    ws_n = lib.sr3d_rotate_workspace_bytes(1, 4, 4, 16, 16)
    # C != 4 for the field call
    assert lib.sr3d_rotate_fields(fake, fake, 1, 3, 4, 16, 16, m, s, 30.0, 0, fake, ws_n, None) == -1
    assert b"4 channels" in lib.sr3d_last_error()
    # null workspace, too small a workspace
    assert lib.sr3d_rotate_fields(fake, fake, 1, 4, 4, 16, 16, m, s, 30.0, 0, None, ws_n, None) == -1
    assert b"workspace" in lib.sr3d_last_error()
    assert lib.sr3d_rotate_fields(fake, fake, 1, 4, 4, 16, 16, m, s, 30.0, 0, fake, ws_n - 8, None) == -3
    assert lib.sr3d_rotate_building(fake, fake, 1, 1, 4, 16, 16, 30.0, 0.1, 0, None, ws_n, None) == -1
    # zero scale, unknown flag, non-finite angle
    z = (C.c_double * 4)(8.4, 0.0, 21.6, 7.0)
    assert lib.sr3d_rotate_fields(fake, fake, 1, 4, 4, 16, 16, m, z, 30.0, 0, fake, ws_n, None) == -1
    assert lib.sr3d_rotate_fields(fake, fake, 1, 4, 4, 16, 16, m, s, 30.0, 8, fake, ws_n, None) == -1
    assert lib.sr3d_rotate_fields(fake, fake, 1, 4, 4, 16, 16, m, s, float("nan"), 0, fake, ws_n, None) == -1
    # windows out of range / empty (Python-slice bounds: negative counts from the end)
    out = C.c_void_p(0x2000)
    for sy, ey, sx, ex in ((0, 17, 0, 16), (-17, 16, 0, 16), (5, 5, 0, 16), (0, 16, 10, 3), (0, 16, 0, -16)):
        rc = lib.sr3d_equivariance_errors(fake, fake, 1, 4, 16, 16, m, s, 30.0, sy, ey, sx, ex, 0, out, fake, ws_n, None)
        assert rc == -1, (sy, ey, sx, ex)
        assert b"window" in lib.sr3d_last_error()
    assert lib.sr3d_equivariance_errors(fake, fake, 1, 4, 16, 16, m, s, 30.0, 0, 16, 0, 16, 0, out, None, ws_n,
                                        None) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_no_cpu_path(eng):
    from sr3d_amd.src import equivariance_error_calculator as eq
    x = torch.rand(1, 4, 2, 8, 8)
    b = torch.ones(1, 1, 2, 8, 8)
    ms = ([302.0, -6.5, -9.1, -3.5], [8.4, 14.4, 21.6, 7.0])
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.rotate_fields(x, *ms, 30.0)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.rotate_building(b, 30.0)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.equivariance_errors(x, x, *ms, 30.0, 0, 8, 0, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.rotate_workspace(x)
    with pytest.raises(RuntimeError, match="GPU"):
        eq.rotate_temperature_velocity(x.numpy(), *ms, 30.0)
    with pytest.raises(RuntimeError, match="GPU"):
        eq.rotate_building_height(b, 30.0)
    kw = dict(Xs=x, bs=b, model=torch.nn.Identity(), means=ms[0], scales=ms[1], device="cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        eq.calc_preds_for_equivariance_errors(angle=30.0, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        eq.calc_equivariance_errors(angle=30.0, sx=0, ex=8, sy=0, ey=8, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        eq.calc_equivariance_errors_over_angles(angles=[30.0], sx=0, ex=8, sy=0, ey=8, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        eq.calc_equivariance_errors(angle=30.0, sx=0, ex=8, sy=0, ey=8, **dict(kw, device="cpu"))


def test_module_imports_neither_scipy_nor_pandas():
    import subprocess
    import sys
    code = ("import sys; sys.modules['scipy'] = None; sys.modules['pandas'] = None; import sr3d_amd; "
            "from sr3d_amd.src import equivariance_error_calculator as eq; print(eq.calc_equivariance_errors.__name__)")
    from helpers import ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "calc_equivariance_errors" in r.stdout, r.stderr
