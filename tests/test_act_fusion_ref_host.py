"""The reference that tests/test_gpu_act_fusion.py holds the fused activation-backward epilogue against
(tests/act_fusion_ref.py), pinned on the CPU: its closed form equals fp64 autograd through the layers it stands for."""
import torch
import torch.nn.functional as F

import act_fusion_ref as A
from oracle import ref_cpu as R


def _chain(unshuffle, n_dy):
    g = torch.Generator().manual_seed(4 + n_dy + 10 * unshuffle)
    c, coarse = 3, (2, 3, 4)
    fine = tuple(2 * n for n in coarse) if unshuffle else coarse
    x0 = torch.rand(2, 5, *coarse, generator=g, dtype=torch.float64) - 0.5
    wp = torch.randn(8 * c if unshuffle else c, 5, 3, 3, 3, generator=g, dtype=torch.float64) * 0.2
    skip = torch.rand(2, 4, *fine, generator=g, dtype=torch.float64) - 0.5
    ws = [torch.randn(6, 4 + c, 3, 3, 3, generator=g, dtype=torch.float64) * 0.2 for _ in range(n_dy)]
    dys = [torch.rand(2, 6, *fine, generator=g, dtype=torch.float64) - 0.5 for _ in range(n_dy)]
    pre = F.conv3d(x0, wp, None, padding=1).requires_grad_(True)
    y = F.leaky_relu(pre, A.SLOPE)
    y = R.unshuffle_voxels(y, 2) if unshuffle else y
    skip.requires_grad_(True)
    x = torch.cat([skip, y], 1)
    sum((F.conv3d(x, w, None, padding=1) * d).sum() for w, d in zip(ws, dys)).backward()
    return dys, ws, y.detach(), pre.grad, skip.grad


def test_closed_form_equals_fp64_autograd_through_the_two_layers():
    for unshuffle in (False, True):
        for n_dy in (1, 2):
            dys, ws, y, dpre, dskip = _chain(unshuffle, n_dy)
            got = A.fused_reference(A.input_gradient(dys, ws, 4, 7), y, unshuffle)
            assert got.shape == dpre.shape
            assert float((got - dpre).abs().max()) < 1e-13 * float(dpre.abs().max())
            plain = A.input_gradient(dys, ws, 0, 4)
            assert float((plain - dskip).abs().max()) < 1e-13 * float(dskip.abs().max())


def test_slab_form_of_the_input_gradient_equals_conv_transpose():
    g = torch.Generator().manual_seed(1)
    dys = [torch.rand(1, 5, 5, 4, 6, generator=g) - 0.5 for _ in range(2)]
    ws = [torch.randn(5, 9, 3, 3, 3, generator=g) for _ in range(2)]
    a, b = A.input_gradient(dys, ws, 2, 9), A.input_gradient_slabs(dys, ws, 2, 9, slab=2)
    assert a.shape == b.shape and float((a - b).abs().max()) < 1e-13 * float(a.abs().max())


def test_zeros_of_either_sign_take_the_slope():
    y = torch.tensor([0.0, -0.0, 1e-30, -1e-30]).view(1, 1, 1, 1, 4)
    got = A.fused_reference(torch.ones(1, 1, 1, 1, 4, dtype=torch.float64), y, False).flatten().tolist()
    assert got == [A.SLOPE, A.SLOPE, 1.0, A.SLOPE]


def test_shuffle_inverts_unshuffle():
    g = torch.Generator().manual_seed(2)
    t = torch.rand(2, 24, 3, 2, 5, generator=g)
    assert torch.equal(R.shuffle_voxels(R.unshuffle_voxels(t, 2), 2), t)
    u = torch.rand(2, 3, 6, 4, 10, generator=g)
    assert torch.equal(R.unshuffle_voxels(R.shuffle_voxels(u, 2), 2), u)


def test_inputs_carry_signed_zeros_and_are_bf16_representable_on_request():
    dys, ws, y = A.make_inputs(7, 9, 5, 2, (3, 4, 50), 2, seed=3, bf16=True)
    assert len(dys) == 2 and len(ws) == 2 and y.shape == (2, 7, 3, 4, 50)
    for t in dys + ws + [y]:
        assert torch.equal(A.rep(t), t)
    zeros = y == 0
    neg = torch.signbit(y) & zeros
    n = y.numel()
    assert 0.005 * n < int(neg.sum()) < 0.02 * n and 0.005 * n < int((zeros & ~neg).sum()) < 0.02 * n
    assert float(y.abs().max()) <= 0.5
