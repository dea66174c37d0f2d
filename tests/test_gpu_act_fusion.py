"""The fused activation-backward epilogue of the input gradient (sr3d_conv3d_bwd_data_act) as an OP, at ragged
shapes (pytest -m gpu, on the MI355X box): hconv_kernel's 16-byte and scalar epilogues in their plain and unshuffle store
form, fp32 and bf16; the VALU remainder kernel smalln_fwd_kernel<1|2|4>; the predicate sr3d_conv3d_bwd_data_fuses_act; the
row compaction of bwd_data_impl; the _ActBox hand-over of ops.py through autograd; `dual=True` of the gated layer.

References: tests/act_fusion_ref.py (fp64, pinned on the CPU by tests/test_act_fusion_ref_host.py).  Tolerances are the
project's own and nothing else: TOL = 1e-5 normwise for fp32, `within_one_ulp` against the fp64 result rounded ONCE to bf16
(the fused kernel rounds once; the two-pass form rounds twice, so bf16 is not compared with it), and bit equality where
include/sr3d.h promises it (fp32: the fused store against sr3d_conv3d_bwd_data + sr3d_lrelu_bwd, the exported maximum
against the stored values).

Every destination lives inside a larger allocation, pre-filled with NaN between two sentinel bands: an unwritten tail
leaves a NaN, a wide store past a ragged edge lands in a band -- inside the allocation either way."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import act_fusion_ref as A
from helpers import relerr, within_one_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
F32, BF = torch.float32, torch.bfloat16
BAND, SENTINEL = 256, 7.0       # elements before and after a destination (1024 / 512 bytes: the start stays 16-byte aligned)
BIG = (16, 128, 256)            # 524 288 voxels: bwd_rem_rows hands 1..4 rows to the VALU kernel from 500 000 voxels up


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def L(eng):
    return eng._lib


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("SR3D_SPLIT_F16", "2")
    monkeypatch.delenv("SR3D_HCONV_SCALAR_EPILOGUE", raising=False)


# ------------------------------------------------------------------------------------------------ the op through the C ABI
class Framed:
    """a destination of `shape` inside a larger allocation: NaN between two sentinel bands"""

    def __init__(self, shape, dt):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=dt, device=DEV)
        self.buf[BAND:BAND + n] = float("nan")
        self.t = self.buf[BAND:BAND + n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def bands_intact(self):
        return bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[-BAND:] == SENTINEL).all())

    def untouched(self):
        return self.bands_intact() and bool(torch.isnan(self.t).all())


def setup(L, spec, cout, n_dy, grid, dt, batch=2, unshuffle=False, stride=1, dy_scale=1.0, w_scale=1.0, act=None, shared=None):
    """one layer's input gradient: descriptor, inputs on the CPU (for the reference) and on the GPU"""
    cs, needs, fuse = A.parse(spec)
    cin = sum(cs)
    og = tuple((n - 1) // stride + 1 for n in grid)
    seed = 1000 * cin + 10 * cout + n_dy + sum(grid)
    if shared is None:
        dys, ws, act_y = A.make_inputs(cs[fuse], cin, cout, n_dy, grid, batch, seed, dt == BF, dy_scale, w_scale, out_grid=og)
    else:       # (the large cases share dY and one weight tensor: channel c of the gradient does not depend on Cin)
        dys, ws = shared.dys, [w[:, :cin].contiguous() for w in shared.ws]
        act_y = A.make_act_y((batch, cs[fuse], *grid), seed, dt == BF)
    s = SimpleNamespace(cs=cs, needs=needs, fuse=fuse, cin=cin, cout=cout, n_dy=n_dy, grid=grid, dt=dt, B=batch,
                        unshuffle=unshuffle, dys_cpu=dys, ws_cpu=ws, act_y_cpu=act_y)
    s.desc = L.conv_desc(batch, cin, cout, *grid, stride, dt)
    s.act = (L.ACT_LRELU if act is None else act) | (L.ACT_UNSHUFFLE if unshuffle else 0)
    s.dys = [d.to(DEV).to(dt) for d in dys]
    s.ws = [w.to(DEV) for w in ws] + [None] * (2 - n_dy)      # (weights stay fp32 in both storage modes)
    s.act_y = act_y.to(DEV).to(dt)
    s.nbytes = L.lib.sr3d_conv3d_bwd_data_workspace_bytes(C.byref(s.desc), n_dy)
    s.ws_buf = torch.empty(max(1, s.nbytes // 4), dtype=F32, device=DEV)
    return s


def destinations(s):
    return [Framed((s.B, c, *s.grid), s.dt) if need else None for c, need in zip(s.cs, s.needs)]


def dst_array(L, s, dsts):
    return L.slices([d.t if d is not None else (c, None) for d, c in zip(dsts, s.cs)], "dx_dsts", s.dt)


def predicate(L, s, dsts):
    return L.lib.sr3d_conv3d_bwd_data_fuses_act(C.byref(s.desc), s.n_dy, dst_array(L, s, dsts), len(dsts), s.fuse, s.act)


def call_fused(L, s, dsts, amax):
    dy_arr, dst_arr = L.slices(s.dys, "dy_srcs", s.dt), dst_array(L, s, dsts)
    return L.lib.sr3d_conv3d_bwd_data_act(C.byref(s.desc), dy_arr, s.n_dy, L.dev_ptr(s.ws[0]), L.dev_ptr(s.ws[1]), dst_arr, len(dsts),
                                          s.fuse, L.dev_ptr(s.act_y, "act_y", s.dt), s.act,
                                          C.c_void_p(amax.data_ptr() if amax is not None else 0), L.dev_ptr(s.ws_buf), s.nbytes,
                                          L.stream_ptr())


def call_two_pass(L, s):
    """sr3d_conv3d_bwd_data, then the producer's own activation backward on the fused slice: (destinations, dpre)"""
    dsts = destinations(s)
    dy_arr, dst_arr = L.slices(s.dys, "dy_srcs", s.dt), dst_array(L, s, dsts)
    L.check(L.lib.sr3d_conv3d_bwd_data(C.byref(s.desc), dy_arr, s.n_dy, L.dev_ptr(s.ws[0]), L.dev_ptr(s.ws[1]), dst_arr, len(dsts),
                                       L.dev_ptr(s.ws_buf), s.nbytes, L.stream_ptr()), "bwd_data")
    dx, c, (Z, Y, X) = dsts[s.fuse].t, s.cs[s.fuse], s.grid
    dpre = Framed(dx.shape, s.dt)
    if s.unshuffle:
        L.check(L.lib.sr3d_unshuffle_lrelu_bwd(L.dev_ptr(dx, "dy", s.dt), L.dev_ptr(s.act_y, "y", s.dt), L.dev_ptr(dpre.t, "dpre", s.dt),
                                               s.B, c, Z // 2, Y // 2, X // 2, s.desc.dtype, None, L.stream_ptr()), "unshuffle_lrelu_bwd")
    else:
        L.check(L.lib.sr3d_lrelu_bwd(L.dev_ptr(dx, "dy", s.dt), L.dev_ptr(s.act_y, "y", s.dt), L.dev_ptr(dpre.t, "dpre", s.dt),
                                     dx.numel(), s.desc.dtype, None, L.stream_ptr()), "lrelu_bwd")
    assert dpre.bands_intact()
    return dsts, dpre


def check_values(L, s, reference=None):
    """checks (a) - (d) of one case; `reference(c0, c1)` gives channels c0 .. c1 of the fp64 input gradient"""
    if reference is None:
        reference = lambda c0, c1: A.input_gradient(s.dys_cpu, s.ws_cpu, c0, c1)   # noqa: E731
    what = f"{s.cs} fused {s.fuse} Cout {s.cout} x{s.n_dy} {s.grid} {s.dt}"
    dsts = destinations(s)
    assert predicate(L, s, dsts) == 1, what
    amax = torch.zeros(64, dtype=torch.int32, device=DEV) if s.dt == F32 else None      # (bf16 exports no maximum: NULL)
    rc = call_fused(L, s, dsts, amax)
    assert rc == 0, (what, L.lib.sr3d_last_error().decode())
    torch.cuda.synchronize()
    Z, Y, X = s.grid
    c0 = 0
    for i, (c, d) in enumerate(zip(s.cs, dsts)):
        if d is not None:       # (a slice without a pointer has nothing to be written to; its channels count: c0 moves on)
            assert d.bands_intact(), (what, i)
            assert not bool(torch.isnan(d.t).any()), (what, i)
            ref, got = reference(c0, c0 + c), d.t
            if i == s.fuse:
                ref = A.fused_reference(ref, s.act_y_cpu, s.unshuffle)
                if s.unshuffle:
                    got = got.view(s.B, 8 * c, Z // 2, Y // 2, X // 2)
            if s.dt == F32:
                e = relerr(got, ref)
                print(f"{what}: slice {i} relerr {e:.2e}")
                assert e < TOL, (what, i, e)
            else:
                within_one_ulp(got, A.q(ref), f"{what}: slice {i}")
        c0 += c
    if s.dt != F32:
        return dsts
    # (b) bit equality with the two-pass form
    two, dpre = call_two_pass(L, s)
    for i, d in enumerate(dsts):
        if d is not None:
            assert torch.equal(d.t, dpre.t if i == s.fuse else two[i].t), (what, i)
    # (c) the exported maximum is the maximum of what was stored; without the export the same bits are stored
    stored = dsts[s.fuse].t
    assert float(amax.view(F32).max()) == float(stored.abs().max()), (what, float(amax.view(F32).max()), float(stored.abs().max()))
    again = destinations(s)
    assert call_fused(L, s, again, None) == 0
    for a, d in zip(again, dsts):
        if d is not None:
            assert a.bands_intact() and torch.equal(a.t, d.t), what
    return dsts


def _id(v):
    if isinstance(v, list):
        return "+".join(v)
    if isinstance(v, tuple):
        return "x".join(f"{n:g}" for n in v)
    return str(v).replace("torch.", "")


# spec, Cout, n_dy, grid, (dy_scale, w_scale): what each row reaches
PLAIN = [
    (["33*"], 72, 1, (5, 7, 33), (1, 1)),                # scalar epilogue, ragged in all three dimensions
    (["64", "1x", "65*"], 48, 1, (6, 10, 40), (1, 1)),   # third slice behind a NULL slice, straddles row blocks, 8-voxel last x tile
    (["40*", "24"], 130, 1, (3, 9, 70), (1, 1)),         # scalar epilogue, fused slice first, K with a tail chunk
    (["36*", "1x"], 40, 2, (5, 6, 36), (1, 1)),          # gated consumer: w_gate and two dY slices
    (["64*"], 64, 1, (4, 8, 32), (1e-4, 1.6e-3)),        # |dx| ~ 0.6 dy_scale w_scale = 1e-7 ...
    (["64*"], 64, 1, (4, 8, 32), (25.0, 20.0)),          # ... and 300: the per-call power-of-two scaling next to the exported maximum
    (["33*"], 8, 1, (5, 6, 35), (1, 1)),                 # K <= 8: one half chunk
]
UNSHUFFLE = [
    (["16", "1x", "9*"], 40, 1, (6, 10, 40)),            # UpBlock's slice order, partial x tile
    (["16*"], 64, 1, (4, 8, 36)),                        # a single slice, X = 36
    (["20", "1x", "12*"], 24, 2, (6, 8, 40)),            # gated consumer
]
# the two small launches that fp32 refuses (see REFUSED) have the epilogue in bf16: values there
BF16_ONLY = [
    (["8*"], 64, 1, (4, 6, 36)),                         # fewer than 16 rows
    (["33*"], 16, 1, (5, 7, 33)),                        # K in 9 .. 31
]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("spec,cout,n_dy,grid,scales", PLAIN, ids=_id)
def test_plain_store_vs_fp64_and_the_two_pass_form(L, spec, cout, n_dy, grid, scales, dt):
    check_values(L, setup(L, spec, cout, n_dy, grid, dt, dy_scale=scales[0], w_scale=scales[1]))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("spec,cout,n_dy,grid", UNSHUFFLE, ids=_id)
def test_unshuffle_store_vs_fp64_and_the_two_pass_form(L, spec, cout, n_dy, grid, dt):
    check_values(L, setup(L, spec, cout, n_dy, grid, dt, unshuffle=True))


@pytest.mark.parametrize("spec,cout,n_dy,grid", BF16_ONLY, ids=_id)
def test_bf16_has_the_epilogue_where_fp32_leaves_for_another_kernel(L, spec, cout, n_dy, grid):
    check_values(L, setup(L, spec, cout, n_dy, grid, BF))


def test_scalar_and_16_byte_epilogue_store_the_same_bits(L, monkeypatch):
    s = setup(L, ["64*"], 64, 1, (4, 8, 32), F32)
    out = {}
    for env in (None, "1"):
        if env is not None:
            monkeypatch.setenv("SR3D_HCONV_SCALAR_EPILOGUE", env)
        out[env] = check_values(L, s)[0].t
    assert torch.equal(out[None], out["1"])


# ---- the large cases: the VALU remainder kernel next to the MFMA kernel (fp32, B = 1)
class SharedReference:
    """fp64 input gradient of the large cases, channel by channel, computed once per channel for all of them"""

    def __init__(self, bf16):
        g = torch.Generator().manual_seed(2024)
        self.dys = [torch.rand(1, 8, *BIG, generator=g) - 0.5]
        self.ws = [torch.randn(8, 130, 3, 3, 3, generator=g) * 0.05]
        if bf16:
            self.dys, self.ws = [A.rep(self.dys[0])], [A.rep(self.ws[0])]
        self.done = {}

    def __call__(self, c0, c1):
        miss = [c for c in range(c0, c1) if c not in self.done]
        if miss:
            r = A.input_gradient_slabs(self.dys, self.ws, miss[0], miss[-1] + 1)
            for k, c in enumerate(range(miss[0], miss[-1] + 1)):
                self.done.setdefault(c, r[:, k])
        return torch.stack([self.done[c] for c in range(c0, c1)], 1)


@pytest.fixture(scope="module")
def big():
    refs = {F32: SharedReference(False), BF: SharedReference(True)}
    yield refs
    for r in refs.values():
        r.done.clear()


REMAINDER = [
    (["65*"], F32, False),               # one remainder row of the fused slice in smalln_fwd_kernel<1>, 64 rows in the MFMA kernel
    (["64", "2*"], F32, False),          # <2>: every fused row is a remainder row
    (["64", "4*"], F32, False),          # <4>
    (["2*", "64"], F32, False),          # the remainder rows are the OTHER slice's: plain epilogue next to a fused MFMA slice
    (["65*"], BF, False),                # (bf16 has no remainder kernel: all 65 rows in the MFMA kernel)
    (["64", "1x", "65*"], F32, True),    # up1's row arithmetic: 129 rows, the remainder row in the VALU kernel's shuffled store
]


@pytest.mark.parametrize("spec,dt,unshuffle", REMAINDER, ids=_id)
def test_remainder_rows_vs_fp64_and_the_two_pass_form(L, big, spec, dt, unshuffle):
    ref = big[dt]
    check_values(L, setup(L, spec, 8, 1, BIG, dt, batch=1, unshuffle=unshuffle, shared=ref), ref)


# ---- launches without the epilogue: the predicate answers 0, the call is an error before any launch
REFUSED = {
    "stride 2, fp32": dict(spec=["33*"], cout=72, grid=(6, 10, 40), dt=F32, stride=2),
    "stride 2, bf16": dict(spec=["33*"], cout=72, grid=(6, 10, 40), dt=BF, stride=2),
    "fewer than 16 rows": dict(spec=["8*"], cout=64, grid=(4, 6, 36), dt=F32),
    "K in 9..31": dict(spec=["33*"], cout=16, grid=(5, 7, 33), dt=F32),
    "split kernels off": dict(spec=["33*"], cout=72, grid=(5, 7, 33), dt=F32, env={"SR3D_SPLIT_F16": "0"}),
    "fused slice without a pointer": dict(spec=["40", "24x*"], cout=48, grid=(4, 6, 36), dt=F32),
    "fused slice without a pointer, bf16": dict(spec=["40", "24x*"], cout=48, grid=(4, 6, 36), dt=BF),
    "relu": dict(spec=["33*"], cout=72, grid=(5, 7, 33), dt=F32, act=1),
    "unshuffle, odd Z": dict(spec=["16*"], cout=64, grid=(5, 8, 40), dt=F32, unshuffle=True),
    "unshuffle, odd Y": dict(spec=["16*"], cout=64, grid=(6, 9, 40), dt=F32, unshuffle=True),
    "unshuffle, X % 4 = 2": dict(spec=["16*"], cout=64, grid=(6, 10, 38), dt=F32, unshuffle=True),
    "unshuffle, odd Z, bf16": dict(spec=["16*"], cout=64, grid=(5, 8, 40), dt=BF, unshuffle=True),
    "unshuffle, odd Y, bf16": dict(spec=["16*"], cout=64, grid=(6, 9, 40), dt=BF, unshuffle=True),
    "unshuffle, X % 4 = 2, bf16": dict(spec=["16*"], cout=64, grid=(6, 10, 38), dt=BF, unshuffle=True),
    "unshuffle, scalar epilogue asked for": dict(spec=["16*"], cout=64, grid=(4, 8, 36), dt=F32, unshuffle=True,
                                                 env={"SR3D_HCONV_SCALAR_EPILOGUE": "1"}),
    # 520 192 voxels, X % 4 = 2: the fused slice's remainder row would need the VALU kernel's 16-byte form
    "remainder row, X % 4 = 2": dict(spec=["65*"], cout=8, grid=(16, 128, 254), dt=F32, batch=1),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_predicate_answers_0_and_the_call_is_refused_before_any_launch(L, monkeypatch, name):
    kw = dict(REFUSED[name])
    for k, v in kw.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    s = setup(L, kw.pop("spec"), kw.pop("cout"), 1, kw.pop("grid"), kw.pop("dt"), **kw)
    dsts = destinations(s)
    assert predicate(L, s, dsts) == 0, name
    amax = torch.zeros(64, dtype=torch.int32, device=DEV) if s.dt == F32 else None
    rc = call_fused(L, s, dsts, amax)
    torch.cuda.synchronize()
    assert rc != 0, name
    assert len(L.lib.sr3d_last_error()) > 0
    assert all(d.untouched() for d in dsts if d is not None), name
    assert amax is None or int(amax.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ the hand-over in ops.py
def _leaf(shape, g, scale=1.0, shift=0.5):
    return ((torch.rand(*shape, generator=g) - shift) * scale)


def _mask(shape, g):
    return (torch.rand(*shape, generator=g) > 0.2).float()


def _w(cout, cin, g):
    return torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05


def chain_plain(eng, grid, coarse):
    g = torch.Generator().manual_seed(31)
    P = {"x": _leaf((2, 20, *grid), g), "w1": _w(33, 20, g), "b1": _leaf((33,), g, 0.2), "w2": _w(40, 33, g), "b2": _leaf((40,), g, 0.2)}

    def fwd(p):
        y1 = eng.ops.conv3d_act([p["x"]], p["w1"], p["b1"], act="lrelu", defer_act_bwd=True)
        return eng.ops.conv3d_act([y1], p["w2"], p["b2"], act="lrelu"), y1
    return P, {}, fwd, 1, (2, 0)


def chain_gated(eng, grid, coarse):
    g = torch.Generator().manual_seed(32)
    P = {"x": _leaf((2, 20, *grid), g), "w1": _w(33, 20, g), "b1": _leaf((33,), g, 0.2), "wf": _w(24, 34, g), "wg": _w(24, 34, g),
         "bg": _leaf((24,), g, 0.2)}
    K = {"m": _mask((2, 1, *grid), g)}

    def fwd(p):
        y1 = eng.ops.conv3d_act([p["x"]], p["w1"], p["b1"], act="lrelu", defer_act_bwd=True)
        return eng.ops.gated_conv3d_act([y1, p["m"]], p["wf"], p["wg"], None, p["bg"], act="relu"), y1
    return P, K, fwd, 1, (1, 0)


def chain_unshuffle(eng, grid, coarse):
    g = torch.Generator().manual_seed(33)
    P = {"x": _leaf((2, 12, *coarse), g), "w1": _w(72, 12, g), "b1": _leaf((72,), g, 0.2), "skip": _leaf((2, 16, *grid), g),
         "w2": _w(40, 26, g), "b2": _leaf((40,), g, 0.2)}
    K = {"m": _mask((2, 1, *grid), g)}

    def fwd(p):
        y1 = eng.ops.conv3d_act([p["x"]], p["w1"], p["b1"], act="lrelu", unshuffle=True, defer_act_bwd=True)
        return eng.ops.conv3d_act([p["skip"], p["m"], y1], p["w2"], p["b2"], act="lrelu"), y1
    return P, K, fwd, 1, (1, 1)


def chain_upblock(eng, grid, coarse):
    from sr3d_amd.model.unet import UpBlock
    g = torch.Generator().manual_seed(34)
    torch.manual_seed(34)
    block = UpBlock(32, 17, 32, bias=True, conv_mode=None, n_layers_in_block=2)
    P = {"x1": _leaf((2, 31, *coarse), g), "skip": _leaf((2, 16, *grid), g)}
    P.update({k: v.detach().clone() for k, v in block.named_parameters()})
    K = {"mc": _mask((2, 1, *coarse), g), "mf": _mask((2, 1, *grid), g)}

    def fwd(p):      # (with the run's own leaves as parameters: their .grad is what the test reads)
        return torch.func.functional_call(block, {k: p[k] for k, _ in block.named_parameters()},
                                          ([p["x1"], p["mc"]], [p["skip"], p["mf"]]), {"defer_act_bwd": True}), None
    # up -> convs[0] -> convs[1]; the block's own output defers too, but nothing in this chain consumes it
    return P, K, fwd, 2, (2, 1)


def run_chain(eng, monkeypatch, chain, fused):
    """one forward + backward; gradients of every leaf, calls of the two activation-backward passes, what the predicate was
    asked and answered, every _ActBox the forward made"""
    P, K, fwd, _, _ = chain
    lib, ops = eng._lib.lib, eng.ops
    calls, asked, boxes = {"act": 0, "unsh": 0}, [], []
    orig = {n: getattr(lib, n) for n in ("sr3d_lrelu_bwd", "sr3d_unshuffle_lrelu_bwd", "sr3d_conv3d_bwd_data_fuses_act")}

    def counted(*a):
        calls["act"] += 1
        return orig["sr3d_lrelu_bwd"](*a)

    def counted_u(*a):
        calls["unsh"] += 1
        return orig["sr3d_unshuffle_lrelu_bwd"](*a)

    def answered(*a):
        r = orig["sr3d_conv3d_bwd_data_fuses_act"](*a)
        asked.append((bool(a[5] & eng._lib.ACT_UNSHUFFLE), int(r)))
        return r

    class Box(ops._ActBox):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            boxes.append(self)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "FUSE_ACT_BWD", fused)
        mp.setattr(ops, "_ActBox", Box)
        mp.setattr(lib, "sr3d_lrelu_bwd", counted)
        mp.setattr(lib, "sr3d_unshuffle_lrelu_bwd", counted_u)
        mp.setattr(lib, "sr3d_conv3d_bwd_data_fuses_act", answered)
        p = {k: v.to(DEV).requires_grad_(True) for k, v in P.items()}
        p.update({k: v.to(DEV) for k, v in K.items()})
        y, y1 = fwd(p)
        gy = torch.rand(y.shape, generator=torch.Generator().manual_seed(5)) - 0.5
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
    grads = {k: p[k].grad.detach().clone() for k in P}
    return SimpleNamespace(grads=grads, calls=(calls["act"], calls["unsh"]), asked=asked, boxes=boxes, p=p, y=y, y1=y1, gy=gy)


# chain, fine grid, coarse grid, what the issue states about the grid: does the unshuffle hand-over fuse?
CHAINS = [
    (chain_plain, (6, 10, 20), None, None), (chain_plain, (6, 10, 18), None, None), (chain_plain, (5, 7, 33), None, None),
    (chain_gated, (6, 10, 20), None, None), (chain_gated, (6, 10, 18), None, None), (chain_gated, (5, 7, 33), None, None),
    (chain_unshuffle, (6, 10, 20), (3, 5, 10), 1), (chain_unshuffle, (6, 10, 18), (3, 5, 9), 0),
    (chain_upblock, (6, 10, 20), (3, 5, 10), 1), (chain_upblock, (6, 10, 18), (3, 5, 9), 0),
]


@pytest.mark.parametrize("make,grid,coarse,unsh_fuses", CHAINS,
                         ids=[f"{m.__name__[6:]}-{'x'.join(map(str, g))}" for m, g, _, _ in CHAINS])
def test_hand_over_through_autograd_gives_the_bits_of_the_separate_pass(eng, monkeypatch, make, grid, coarse, unsh_fuses):
    chain = make(eng, grid, coarse)
    _, _, _, n_handovers, n_passes = chain
    on, off, on2 = (run_chain(eng, monkeypatch, chain, f) for f in (True, False, True))
    # without the fusion: every LeakyReLU layer runs its own pass, the predicate is never asked
    assert off.calls == n_passes and off.asked == []
    # with it: every deferring layer that has a consumer asks once; the passes that disappear are those it answered 1 for
    assert len(on.asked) == n_handovers, on.asked
    fused_plain = sum(a for unsh, a in on.asked if not unsh)
    fused_unsh = sum(a for unsh, a in on.asked if unsh)
    assert on.calls == (off.calls[0] - fused_plain, off.calls[1] - fused_unsh), (on.calls, off.calls, on.asked)
    # (what the grids were chosen for: plain hand-overs fuse on all of them, by the scalar epilogue where X % 4 != 0; the
    #  unshuffle hand-over needs X % 4 == 0 on the consumer's grid)
    assert all(a == (unsh_fuses if unsh else 1) for unsh, a in on.asked), on.asked
    for k, gr in on.grads.items():
        assert torch.equal(gr, off.grads[k]), k
        assert torch.equal(gr, on2.grads[k]), k        # a second backward over a fresh forward: the same bits
    for r in (on, off, on2):
        assert len(r.boxes) >= n_handovers
        assert all(b.done is False and b.amax is None for b in r.boxes)


def test_hand_over_chain_vs_fp64_with_the_engines_branches(eng, monkeypatch):
    """the producer's dL/dpre by hand: conv_transpose(consumer's dL/dpre) * lrelu'(y) with the branch of the y the engine
    stored (the idea of ops.KINK_LOG); its weight, bias and input gradients against that at TOL"""
    r = run_chain(eng, monkeypatch, chain_plain(eng, (5, 7, 33), None), True)
    assert r.asked == [(False, 1)] and r.calls == (1, 0)
    d = lambda t: t.detach().cpu().double()   # noqa: E731
    slope = lambda y: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, A.SLOPE))   # noqa: E731
    y1, y2 = d(r.y1), d(r.y)
    dpre2 = r.gy.double() * slope(y2)
    w2 = d(r.p["w2"]).requires_grad_(True)
    F.conv3d(y1, w2, None, padding=1).backward(dpre2)
    dpre1 = F.conv_transpose3d(dpre2, w2.detach(), None, padding=1) * slope(y1)
    x, w1 = d(r.p["x"]).requires_grad_(True), d(r.p["w1"]).requires_grad_(True)
    F.conv3d(x, w1, None, padding=1).backward(dpre1)
    ref = {"x": x.grad, "w1": w1.grad, "b1": dpre1.sum(dim=(0, 2, 3, 4)), "w2": w2.grad, "b2": dpre2.sum(dim=(0, 2, 3, 4))}
    for k, v in ref.items():
        e = relerr(r.grads[k], v)
        print(f"hand-over chain vs fp64: {k} relerr {e:.2e}")
        assert e < TOL, (k, e)


# ------------------------------------------------------------------------------------------------ dual=True of the gated layer
class _NoGradient(torch.autograd.Function):
    """identity whose backward hands nothing on: the gated layer's backward then runs with no incoming gradient at all"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("stride", [1, 2])
def test_gated_layer_with_two_output_handles_vs_fp64(eng, stride):
    g = torch.Generator().manual_seed(40 + stride)
    grid, cout = (5, 6, 35), 24
    x = (torch.rand(2, 20, *grid, generator=g) - 0.3).double()
    m = (torch.rand(2, 1, *grid, generator=g) > 0.2).double()
    wf, wg = ((torch.randn(cout, 21, 3, 3, 3, generator=g) * 0.05).double() for _ in range(2))
    bg = (torch.randn(cout, generator=g) * 0.1).double()
    xc = torch.cat([x, m], 1)
    with torch.no_grad():
        pre_f = F.conv3d(xc, wf, None, stride=stride, padding=1)
    # keep the comparison on the smooth part: no gradient through pre-activations within 1e-4 of the ReLU kink
    g1, g2 = ((torch.rand(pre_f.shape, generator=g) - 0.5).double() * (pre_f.abs() > 1e-4) for _ in range(2))

    def reference(gs):
        lv = [t.clone().requires_grad_(True) for t in (x, wf, wg, bg)]
        xr = torch.cat([lv[0], m], 1)
        y = torch.sigmoid(F.conv3d(xr, lv[2], lv[3], stride=stride, padding=1)) * torch.relu(F.conv3d(xr, lv[1], None, stride=stride, padding=1))
        sum((y * t).sum() for t in gs).backward()          # (y is used once per handle)
        return y.detach(), [t.grad for t in lv]

    def engine():
        lv = [t.float().to(DEV).requires_grad_(True) for t in (x, wf, wg, bg)]
        ya, yb = eng.ops.gated_conv3d_act([lv[0], m.float().to(DEV)], lv[1], lv[2], None, lv[3], act="relu", stride=stride, dual=True)
        assert ya.data_ptr() == yb.data_ptr()
        return ya, yb, lv

    dev = lambda t: t.float().to(DEV)   # noqa: E731
    # both handles receive a gradient
    y_ref, ref = reference([g1, g2])
    ya, yb, lv = engine()
    assert relerr(ya, y_ref) < TOL
    torch.autograd.backward([ya, yb], [dev(g1), dev(g2)])
    for name, a, b in zip(("x", "wf", "wg", "bg"), lv, ref):
        assert relerr(a.grad, b) < TOL, ("both", name, relerr(a.grad, b))
    # only the second does
    _, ref = reference([g2])
    ya, yb, lv = engine()
    yb.backward(dev(g2))
    for name, a, b in zip(("x", "wf", "wg", "bg"), lv, ref):
        assert relerr(a.grad, b) < TOL, ("second", name, relerr(a.grad, b))
    # neither does: the sources receive none either
    ya, yb, lv = engine()
    other = torch.ones(3, device=DEV, requires_grad=True)
    (_NoGradient.apply(ya).sum() + _NoGradient.apply(yb).sum() + (other * other).sum()).backward()
    assert all(t.grad is None for t in lv) and torch.equal(other.grad, torch.full((3,), 2.0, device=DEV))
