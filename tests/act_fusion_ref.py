"""fp64 reference of the input gradient with a fused LeakyReLU backward (sr3d_conv3d_bwd_data_act), plain
PyTorch on the CPU; tests/test_gpu_act_fusion.py holds the kernels against it, tests/test_act_fusion_ref_host.py pins it
against fp64 autograd without a GPU.

A case is written as its destination slices: "33*" is the fused slice of 33 channels, "1x" a slice that needs no gradient
(NULL pointer: its channels still count towards Cin), "64" an ordinary slice."""
import torch
import torch.nn.functional as F

from helpers import q, rep  # noqa: F401  (q: for the tests that compare bf16 results)
from oracle import ref_cpu as R

SLOPE = 0.01


def parse(spec):
    """["16", "1x", "9*"] -> ([16, 1, 9], needs [True, False, True], index of the fused slice)"""
    cs = [int(s.rstrip("*x")) for s in spec]
    needs = ["x" not in s for s in spec]
    fused = [i for i, s in enumerate(spec) if "*" in s]
    assert len(fused) == 1, spec
    return cs, needs, fused[0]


def make_act_y(shape, seed, bf16=False):
    """the producer's output y as GIVEN data (no producer, so the branch of every element is unambiguous): uniform in
    (-0.5, 0.5) with about 1 % of the elements exactly +0.0 and 1 % exactly -0.0"""
    g = torch.Generator().manual_seed(seed)
    act_y = torch.rand(*shape, generator=g) - 0.5
    u = torch.rand(act_y.shape, generator=g)
    act_y[u < 0.01] = 0.0
    act_y[u > 0.99] = -0.0
    return rep(act_y) if bf16 else act_y


def make_inputs(c_fused, cin, cout, n_dy, grid, batch, seed, bf16=False, dy_scale=1.0, w_scale=1.0, out_grid=None):
    """seeded dY slices (on `out_grid`, the layer's output grid: `grid` at stride 1), weights and `act_y`"""
    g = torch.Generator().manual_seed(seed)
    dys = [(torch.rand(batch, cout, *(out_grid or grid), generator=g) - 0.5) * dy_scale for _ in range(n_dy)]
    ws = [torch.randn(cout, cin, 3, 3, 3, generator=g) * (0.05 * w_scale) for _ in range(n_dy)]
    if bf16:
        dys, ws = [rep(d) for d in dys], [rep(w) for w in ws]
    return dys, ws, make_act_y((batch, c_fused, *grid), seed + 1, bf16)


def input_gradient(dys, ws, c0, c1):
    """channels c0 .. c1 of dL/dx of y = conv3d(x, W), summed over the dY slices (gated layers have two), in fp64"""
    dy = torch.cat([d.double() for d in dys], 1)
    w = torch.cat([w[:, c0:c1].double() for w in ws], 0)
    return F.conv_transpose3d(dy, w, None, stride=1, padding=1)


def input_gradient_slabs(dys, ws, c0, c1, slab=2):
    """the same sum written as a correlation with the mirrored kernel, a few z planes at a time: for the large grids, where
    conv_transpose3d's column buffer (27 values per voxel and OUTPUT channel) would not fit"""
    dy = F.pad(torch.cat([d.double() for d in dys], 1), (0, 0, 0, 0, 1, 1))
    w = torch.cat([w[:, c0:c1].double() for w in ws], 0).flip(2, 3, 4).transpose(0, 1).contiguous()
    B, _, Zp, Y, X = dy.shape
    out = torch.empty(B, c1 - c0, Zp - 2, Y, X, dtype=torch.float64)
    for z0 in range(0, Zp - 2, slab):
        z1 = min(z0 + slab, Zp - 2)
        out[:, :, z0:z1] = F.conv3d(dy[:, :, z0:z1 + 2], w, None, padding=(0, 1, 1))
    return out


def fused_reference(dx, act_y, unshuffle):
    """what the fused slice receives: dL/dy * lrelu'(y), the producer's dL/dpre -- for an unshuffle producer in ITS layout,
    (B, 8 C, Z/2, Y/2, X/2)"""
    act_y = act_y.double()
    dpre = dx * torch.where(act_y > 0, torch.ones_like(act_y), torch.full_like(act_y, SLOPE))
    return R.shuffle_voxels(dpre, 2) if unshuffle else dpre
