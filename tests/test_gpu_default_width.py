"""Parity at default.yml channel widths (64/128/128/256/256, 65.47 M parameters) -- the widths the benchmark runs.

Three layers of evidence (pytest -m gpu, on the MI355X box):
 * the whole model (forward, loss, dL/dpred, all 48 parameter gradients) against golden vectors written by the
   imported reference (oracle/make_golden.py:default_width_fixture) AND against the CPU oracle run live -- the
   launch shapes the benchmark spends its time in: gradient GEMMs with 1032 / 2056 rows, K = 514 / 386 / 258,
   per-tile workgroups on the small grids of levels 3-4, 193- / 257-row tails, the few-channel weight gradient;
 * single layers at full width: forward + input gradient + weight gradient;
 * the same tests again with the direct (non-Winograd) kernels selected.

Tolerance: 1e-5 normwise for everything (north_star); a parameter gradient may alternatively be within 1e-5 of the
reference's fp64 run (the fp32 reference itself is up to 5e-6 away from it)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import cfg_of, load_golden, relerr, sampled, synthetic_inputs
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sr3d_amd
    return sr3d_amd


@pytest.mark.parametrize("fname", ["model_default_a.npz", "model_default_b.npz"])
def test_whole_model_default_widths(eng, fname):
    d = load_golden(fname)
    cfg, meta = cfg_of(d), json.loads(str(d["meta"]))
    torch.manual_seed(meta["seed"])
    model = eng.make_model(cfg)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert len(sd) == 48
    for k, v in sd.items():      # same initial weights as the reference had when it wrote the fixture
        assert int(v.view(torch.int32).to(torch.int64).sum()) == int(d["sdsum/" + k]), k
    x, b, y = synthetic_inputs(1, tuple(meta["hr"]), meta["s"], meta["seed"] + 1, meta["mask_kind"])
    model.to(DEV)
    xd, bd, yd = x.to(DEV), b.to(DEV), y.to(DEV)

    eng.ops.KINK_LOG = []                      # record which branch every fused activation took (test hook)
    try:
        pred = model(xd, bd)
    finally:
        kinks, eng.ops.KINK_LOG = eng.ops.KINK_LOG, None
    assert len(kinks) == 23
    assert relerr(pred, d["pred"]) < TOL
    assert relerr(pred.flatten()[::4], d["f64/pred_s4"]) < TOL

    # both losses on the engine's own prediction, against the reference's values on ITS prediction
    mixed_cfg = {"data": cfg["data"], "train": {"loss": {"name": "MixedDivergenceGradientL2Loss",
                                                        "weight_gradient_loss": 1.0, "weight_divergence_loss": 10.0}}}
    lf = eng.make_loss(mixed_cfg)
    p2 = pred.detach().clone().requires_grad_(True)
    terms = lf.calc_loss_terms(predicts=p2, targets=yd, masks=bd)
    for a, r in zip(terms, d["loss/mixed/terms"]):
        assert abs(float(a.detach()) - float(r)) <= TOL * abs(float(r)), (float(a.detach()), float(r))
    tot = lf(p2, yd, bd)
    assert abs(float(tot.detach()) - float(d["loss/mixed/total"])) <= TOL * float(d["loss/mixed/total"])
    if "loss/mixed/dpred" in d:
        tot.backward()
        assert relerr(p2.grad, d["loss/mixed/dpred"]) < TOL
    l1 = eng.make_loss({"train": {"loss": {"name": "L1"}}})(pred.detach(), yd, bd)
    assert abs(float(l1) - float(d["loss/l1/total"])) <= TOL * float(d["loss/l1/total"])

    loss = eng.make_loss(cfg)(pred, yd, bd)
    assert abs(float(loss.detach()) - float(d["train_loss"])) <= TOL * float(d["train_loss"])
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}

    # (1) TIGHT: the oracle evaluated with the HIP path's own branch decisions (activations; sign(p - t) of the L1
    # loss).  Both sides are then the same smooth function and every parameter gradient must agree to 1e-5.
    l1_sign = torch.sign(pred.detach().cpu() - y)
    fp, fl, _, fg = R.loss_and_grads(sd, cfg, x, b, y, kinks=kinks, l1_sign=l1_sign)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, _, _, fg64 = R.loss_and_grads(sd64, cfg, x.double(), b.double(), y.double(), kinks=kinks, l1_sign=l1_sign)
    assert relerr(pred, fp) < TOL
    assert abs(float(loss.detach()) - float(fl)) <= TOL * float(fl)
    forced = {k: min(relerr(g, fg[k]), relerr(g, fg64[k])) for k, g in grads.items()}
    worst = max(forced, key=forced.get)
    print(f"{fname}: worst parameter gradient with forced decisions: {worst} {forced[worst]:.2e}")
    assert forced[worst] < TOL, (worst, forced[worst])

    # (2) AUDIT of the decisions.  (1) takes the HIP path's branch decisions as given; here every one of them is held
    # against the oracle's OWN decisions (KinkRecorder) on the same inputs.  ReLU / LeakyReLU are continuous, so a
    # decision that falls differently changes no forward value beyond rounding -- it can only differ where the
    # oracle's pre-activation is within rounding distance of 0.  Asserted: (a) every differing element has
    # |pre-activation| <= KINK_C * eps * (sum_k |w_k| |x_k| + |bias|) of its own dot product (eps = 2^-24; the factor
    # covers the rounding that the inputs accumulated over up to 23 layers), (b) the number of differing decisions is
    # a handful (<= 4 + FLIP_RATE of the elements of any activation), not a systematic set.
    rec = R.KinkRecorder(audit=True)
    R.unet_forward(sd, cfg["model"], x, b, kinks=rec)
    assert len(rec) == len(kinks) == len(rec.pre) == len(rec.scale) == len(ACT_LAYERS)
    flips, worst_ratio = [], 0.0
    for name, mine, theirs, pre, sc in zip(ACT_LAYERS, kinks, rec, rec.pre, rec.scale):
        assert mine.shape == theirs.shape == pre.shape == sc.shape, name
        diff = mine != theirs
        n = int(diff.sum())
        flips.append(n)
        if n:
            ratio = float((pre[diff].abs() / (EPS32 * sc[diff])).max())
            worst_ratio = max(worst_ratio, ratio)
            assert ratio <= KINK_C, (name, n, ratio)
        assert n <= 4 + FLIP_RATE * mine.numel(), (name, n, mine.numel())
    total_el = sum(m.numel() for m in kinks)
    print(f"{fname}: {sum(flips)} of {total_el} activation decisions differ from the oracle's ({flips}); worst "
          f"|pre| / (eps * sum|w||x|) among them: {worst_ratio:.2f} (bound {KINK_C})")

    # (3) FREE-RUNNING agreement with the reference (golden vectors) and the oracle, at 1e-5, for every parameter
    # whose gradient no differing decision can reach: a decision of activation i enters the gradients of layer i and
    # of every layer BEFORE it, so the parameters of the layers after the last differing activation -- `last` always
    # -- are the same smooth function on both sides.  For the others the tight statement is (1); they are reported.
    rp, rl, rdp, rg = R.loss_and_grads(sd, cfg, x, b, y)
    assert relerr(pred, rp) < TOL
    assert abs(float(loss.detach()) - float(rl)) <= TOL * float(rl)
    _, _, _, rg64 = R.loss_and_grads(sd64, cfg, x.double(), b.double(), y.double())
    last_flip = max([i for i, n in enumerate(flips) if n], default=-1)
    rows, bad = [], []
    for k, g in grads.items():
        gs = sampled(g)
        g32, g64 = T_(d["grad/" + k]), T_(d["f64/grad/" + k])
        layer = k.rsplit(".", 1)[0]
        for suffix in (".conv.conv3d", ".conv.mask_conv3d", ".conv"):
            if layer.endswith(suffix):
                layer = layer[:-len(suffix)]
        idx = ACT_LAYERS.index(layer) if layer in ACT_LAYERS else (-1 if layer == "conv0" else len(ACT_LAYERS))
        clean = last_flip < 0 or idx > last_flip
        row = {"param": k, "forced": forced[k], "clean": clean,
               "gold32": relerr(gs, g32), "gold64": relerr(gs, g64), "gold_floor": relerr(g32, g64),
               "orc32": relerr(g, rg[k]), "orc64": relerr(g, rg64[k]), "orc_floor": relerr(rg[k], rg64[k])}
        rows.append(row)
        if clean and not (min(row["orc32"], row["orc64"]) < TOL and min(row["gold32"], row["gold64"]) < TOL):
            bad.append(row)
        # ... and a gross-error net under the others: a differing decision moves a gradient by ~ 1 / sqrt(elements of its
        # activation) (5.6e-3 for one of the 32 k outputs of a level-4 layer), the reference's own fp32-vs-fp64 floor is
        # the same lottery; a wrong tile or tap that only shows with free decisions would be O(0.1 .. 1)
        if not clean and min(row["orc32"], row["orc64"]) > max(FREE_LOOSE, 10.0 * row["orc_floor"]):
            bad.append(row)
    out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpurun_out")
    os.makedirs(out_dir, exist_ok=True)
    tag = os.environ.get("SR3D_WINOGRAD", "1") + os.environ.get("SR3D_WINOGRAD_WGRAD", "1") + \
        ("_split" if os.environ.get("SR3D_SPLIT_F16") == "2" else "")
    with open(os.path.join(out_dir, f"default_width_grad_errors_{fname[:-4]}_{tag}.json"), "w") as f:
        json.dump({"flips": dict(zip(ACT_LAYERS, flips)), "worst_kink_ratio": worst_ratio, "rows": rows}, f, indent=1)
    nclean = sum(r["clean"] for r in rows)
    print(f"{fname}: free decisions: {nclean} of {len(rows)} parameters behind the last differing decision, worst of them vs "
          f"oracle {max([min(r['orc32'], r['orc64']) for r in rows if r['clean']], default=0):.2e}; all parameters: worst vs "
          f"fp32 oracle {max(r['orc32'] for r in rows):.2e}, oracle fp32-vs-fp64 floor {max(r['orc_floor'] for r in rows):.2e}")
    assert nclean >= 2          # `last.weight`, `last.bias` at the very least
    assert not bad, bad


EPS32 = 2.0 ** -24
FREE_LOOSE = 2e-2    # free-running bound for parameters a differing decision can reach (see (3) above)
KINK_C = 8.0         # differing decisions must have |pre| <= KINK_C * eps * sum|w||x| (worst observed: 2.05; a typical
                     # pre-activation sits at ~3e5 on this scale, so a systematically wrong branch cannot hide here)
FLIP_RATE = 2e-6     # share of an activation's elements that may differ (observed: 3-13 of 3e7 decisions in the whole
                     # model, at most 4 in one layer: profiles/r03a_default_width_decision_audit_*.json)
# the 23 activations in forward order (= order of ops.KINK_LOG and of the oracle's KinkRecorder)
ACT_LAYERS = (["down%d.convs.%d" % (i, j) for i in (1, 2, 3, 4) for j in (0, 1)] +
              ["latent_layers.0", "latent_layers.2", "latent_layers.4"] +
              [n for i in (4, 3, 2, 1) for n in ("up%d.up.0" % i, "up%d.convs.0" % i, "up%d.convs.1" % i)])


def T_(a):
    return torch.from_numpy(a)


# (name, Cin, Cout, stride, grid, gated, act, unshuffle, split): split = channel counts of the virtual concat and
# whether each slice wants a gradient (mask slices do not: their rows are left out of the backward GEMM)
LAYERS = [
    ("up1.up.0", 129, 1032, 1, (3, 8, 16), False, "lrelu", True, [(128, True), (1, False)]),
    ("up3.up.0", 257, 2056, 1, (2, 4, 8), False, "lrelu", True, [(256, True), (1, False)]),
    ("up4.convs.0", 514, 256, 1, (2, 4, 8), False, "lrelu", False, [(256, True), (1, False), (257, True)]),
    ("up3.convs.0", 386, 128, 1, (4, 8, 16), False, "lrelu", False, [(128, True), (1, False), (257, True)]),
    ("up2.convs.0", 258, 128, 1, (4, 16, 32), False, "lrelu", False, [(128, True), (1, False), (129, True)]),
    ("up1.convs.0", 194, 64, 1, (6, 16, 40), False, "lrelu", False, [(64, True), (1, False), (129, True)]),
    ("down2.convs.0", 129, 128, 2, (8, 16, 32), True, "relu", False, [(128, True), (1, False)]),
    ("down3.convs.1", 256, 256, 1, (2, 8, 8), True, "relu", False, [(256, True)]),
    ("down4.convs.0", 257, 256, 2, (4, 8, 8), True, "relu", False, [(256, True), (1, False)]),
    ("latent.0", 257, 256, 1, (1, 4, 4), False, "lrelu", False, [(256, True), (1, False)]),
    ("last", 69, 4, 1, (8, 16, 32), False, None, False, [(64, True), (5, False)]),
]


def _bounded_away(pre, eps=1e-4):
    """activations are compared where no pre-activation sits within rounding distance of the kink"""
    return float(pre.abs().min()) > eps


@pytest.mark.parametrize("name,cin,cout,stride,grid,gated,act,unshuffle,split", LAYERS, ids=[c[0] for c in LAYERS])
def test_fullwidth_layer_fwd_dgrad_wgrad(eng, name, cin, cout, stride, grid, gated, act, unshuffle, split):
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.rand(2, cin, *grid, generator=g) - 0.5
    std = (2.0 / (27 * cin)) ** 0.5
    wf = torch.randn(cout, cin, 3, 3, 3, generator=g) * std
    wg = torch.randn(cout, cin, 3, 3, 3, generator=g) * std
    bias = torch.randn(cout, generator=g) * 0.1

    def actf(t):
        return {"relu": F.relu, "lrelu": lambda u: F.leaky_relu(u, 0.01), None: lambda u: u}[act](t)

    xr, wfr, wgr, br = (t.clone().requires_grad_(True) for t in (x, wf, wg, bias))
    if gated:
        ref = torch.sigmoid(F.conv3d(xr, wgr, br, stride=stride, padding=1)) * actf(F.conv3d(xr, wfr, None, stride=stride, padding=1))
    else:
        ref = actf(F.conv3d(xr, wfr, br, stride=stride, padding=1))
        if unshuffle:
            ref = R.unshuffle_voxels(ref, 2)
    # no gradient through elements whose pre-activation sits within rounding distance of the kink: there two correct
    # fp32 algorithms may pick different slopes, and one flipped slope is a 1e-3 change of the input gradient
    with torch.no_grad():
        pre = F.conv3d(x, wf, None if gated else bias, stride=stride, padding=1)
        safe = (pre.abs() > 1e-5).float()
        if unshuffle:
            safe = R.unshuffle_voxels(safe, 2)
    gy = (torch.rand(ref.shape, generator=g) - 0.5) * safe
    ref.backward(gy)

    parts, c0 = [], 0
    for c, need in split:
        parts.append(x[:, c0:c0 + c].contiguous().to(DEV).requires_grad_(need))
        c0 += c
    assert c0 == cin
    wfd, wgd, bd = (t.to(DEV).requires_grad_(True) for t in (wf, wg, bias))
    if gated:
        y = eng.ops.gated_conv3d_act(parts, wfd, wgd, None, bd, act=act, stride=stride)
    else:
        y = eng.ops.conv3d_act(parts, wfd, bd, act=act, stride=stride, unshuffle=unshuffle)
    assert relerr(y, ref) < TOL
    y.backward(gy.to(DEV))
    c0 = 0
    for (c, need), p in zip(split, parts):
        if need:
            assert relerr(p.grad, xr.grad[:, c0:c0 + c]) < TOL, f"input gradient of slice at channel {c0}"
        else:
            assert p.grad is None
        c0 += c
    assert relerr(wfd.grad, wfr.grad) < TOL
    if gated:
        assert relerr(wgd.grad, wgr.grad) < TOL
    assert relerr(bd.grad, br.grad) < TOL


def test_193_gradient_rows_on_a_large_grid(eng):
    """up1.convs.0's input gradient: 64 + 129 = 193 rows (the mask slice in the middle needs none) on a grid with
    more than 500k voxels, where the 193rd row leaves the MFMA tiles for the small-N kernel.  The oracle runs in fp64: an
    fp32 CPU weight gradient over 500k voxels is itself ~1e-5 off, by how many threads split its reduction"""
    g = torch.Generator().manual_seed(193)
    grid = (16, 128, 256)
    cin, cout = 194, 64
    x = torch.rand(1, cin, *grid, generator=g) - 0.5
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
    gy = torch.rand(1, cout, *grid, generator=g) - 0.5
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv3d(xr, wr, None, padding=1).backward(gy.double())
    parts = [x[:, :64].contiguous().to(DEV).requires_grad_(True), x[:, 64:65].contiguous().to(DEV),
             x[:, 65:].contiguous().to(DEV).requires_grad_(True)]
    wd = w.to(DEV).requires_grad_(True)
    y = eng.ops.conv3d_act(parts, wd, None, act=None)
    y.backward(gy.to(DEV))
    assert relerr(parts[0].grad, xr.grad[:, :64]) < TOL
    assert relerr(parts[2].grad, xr.grad[:, 65:]) < TOL
    assert relerr(parts[2].grad[:, -1], xr.grad[:, -1]) < TOL      # the row the VALU kernel computed
    assert relerr(wd.grad, wr.grad) < TOL


@pytest.mark.parametrize("shape,cin,cout,gated,act", [
    ((7, 10, 36), 40, 72, False, "lrelu"), ((3, 5, 18), 17, 8, True, "relu"), ((9, 6, 50), 33, 12, True, None),
    ((5, 40, 40), 40, 72, True, "relu"), ((4, 9, 20), 33, 40, False, "lrelu"), ((7, 24, 48), 64, 64, True, "relu")])
def test_winograd_ragged_tiles_with_activation(eng, shape, cin, cout, gated, act):
    """Winograd epilogue branches (activation, gate) at ragged tile edges.  The bias pushes every pre-activation away
    from the kink (checked on the oracle side), so that no legitimate rounding difference can flip a slope."""
    g = torch.Generator().manual_seed(sum(shape) + cin + cout)
    x = torch.rand(2, cin, *shape, generator=g) - 0.5
    wf = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.005
    wg = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.2
    sign = torch.where(torch.arange(cout) % 2 == 0, 1.0, -1.0)
    bf = sign * 0.6          # |conv(x; wf)| has a standard deviation below 0.07: half of the channels positive, half negative
    bg = torch.randn(cout, generator=g) * 0.1
    xr, wfr, wgr, bfr, bgr = (t.clone().requires_grad_(True) for t in (x, wf, wg, bf, bg))
    pre = F.conv3d(xr, wfr, bfr, padding=1)
    assert _bounded_away(pre.detach())
    a = {"relu": F.relu, "lrelu": lambda u: F.leaky_relu(u, 0.01), None: lambda u: u}[act](pre)
    ref = torch.sigmoid(F.conv3d(xr, wgr, bgr, padding=1)) * a if gated else a
    gy = torch.rand(ref.shape, generator=g) - 0.5
    ref.backward(gy)
    xd, wfd, wgd, bfd, bgd = (t.to(DEV).requires_grad_(True) for t in (x, wf, wg, bf, bg))
    if gated:
        y = eng.ops.gated_conv3d_act([xd], wfd, wgd, bfd, bgd, act=act)
    else:
        y = eng.ops.conv3d_act([xd], wfd, bfd, act=act)
    assert relerr(y, ref) < TOL
    y.backward(gy.to(DEV))
    assert relerr(xd.grad, xr.grad) < TOL
    assert relerr(wfd.grad, wfr.grad) < TOL
    assert relerr(bfd.grad, bfr.grad) < TOL
    if gated:
        assert relerr(wgd.grad, wgr.grad) < TOL
        assert relerr(bgd.grad, bgr.grad) < TOL


@pytest.mark.parametrize("env", [{"SR3D_WINOGRAD": "0"}, {"SR3D_WINOGRAD_WGRAD": "0"}, {"SR3D_SPLIT_F16": "2"}])
def test_default_widths_on_the_direct_kernels(env):
    """kernel families are selected from the environment: run this file again under each setting (SR3D_SPLIT_F16=2: the
    split-f16 kernel for every eligible stride-1 layer, also at this small grid)"""
    if os.environ.get("SR3D_WINOGRAD") == "0" or os.environ.get("SR3D_WINOGRAD_WGRAD") == "0" or \
            os.environ.get("SR3D_SPLIT_F16") == "2":
        pytest.skip("already inside the re-run")
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "whole_model or fullwidth_layer or 193"], env=e, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_split_f16_kernels_on_a_trained_models_statistics(eng):
    """Every other whole-model check runs on INITIALISATION-time weights.  The block scaling of the split-f16 kernels takes its
    power of two from the largest magnitude of a workgroup's halo tile, so what matters is the dynamic range of real activations:
    here the default.yml model is trained for 150 Adam steps (lr 1e-3, mixed loss, 6 synthetic batches -- no real data is
    available, but the weights leave their initial distribution: sparse ReLU maps, grown gates, biased features), and the
    forward pass and the loss of the TRAINED model are held to the oracle at 1e-5 and all 48 parameter gradients to the fp64
    oracle, with the engine's own activation decisions forced into it (as in test_whole_model_default_widths (1)), twice:
    SR3D_SPLIT_F16=2 (split-f16 kernels on every eligible layer, whatever the grid) and =0 (fp32 MFMA kernels only)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_config, synthetic_batch
    cfg = make_config("mixed")
    hr, scale = (16, 32, 32), 4
    torch.manual_seed(7)
    model = eng.make_model(cfg).to(DEV)
    loss_fn = eng.make_loss(cfg)
    opt = eng.FlatAdam(model.parameters(), lr=1e-3)
    batches = [synthetic_batch(2, hr, scale, 900 + i, DEV) for i in range(6)]
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    first = last = None
    for it in range(150):
        xb, bb, yb = batches[it % len(batches)]
        loss = loss_fn(model(xb, bb), yb, bb)
        opt.zero_grad()
        loss.backward()
        opt.step()
        first = float(loss.detach()) if it == 0 else first
        last = float(loss.detach())
    assert last < 0.5 * first, (first, last)                       # it did train
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    moved = max(float((sd[k] - sd0[k].cpu()).norm() / sd0[k].cpu().norm().clamp_min(1e-12)) for k in sd if k.endswith("weight"))
    assert moved > 0.05, moved                                     # ... away from the initial weights
    x, b, y = (t[:1].cpu() for t in synthetic_batch(2, hr, scale, 4242, "cpu"))
    xd, bd, yd = x.to(DEV), b.to(DEV), y.to(DEV)
    sd64 = {k: v.double() for k, v in sd.items()}
    report = {}
    for mode in ("2", "0"):                # split-f16 on every eligible layer / fp32 MFMA everywhere
        os.environ["SR3D_SPLIT_F16"] = mode
        try:
            eng.ops.KINK_LOG = []
            try:
                pred = model(xd, bd)
            finally:
                kinks, eng.ops.KINK_LOG = eng.ops.KINK_LOG, None
            loss = loss_fn(pred, yd, bd)
            opt.zero_grad()
            loss.backward()
        finally:
            os.environ.pop("SR3D_SPLIT_F16", None)
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
        fp, fl, _, fg = R.loss_and_grads(sd, cfg, x, b, y, kinks=kinks)
        _, _, _, fg64 = R.loss_and_grads(sd64, cfg, x.double(), b.double(), y.double(), kinks=kinks)
        assert relerr(pred, fp) < TOL, (mode, relerr(pred, fp))
        assert abs(float(loss.detach()) - float(fl)) <= TOL * float(fl), mode
        # the yardstick per parameter: the error the fp32 ORACLE itself makes against fp64 on this gradient (a bias gradient
        # of a trained gate is a sum of signed terms that nearly cancel: relative error means little below that floor)
        floor = {k: relerr(fg[k], fg64[k]) for k in grads}
        err = {k: relerr(g, fg64[k]) for k, g in grads.items()}
        report[mode] = (err, floor)
        top = sorted(err, key=err.get, reverse=True)[:6]
        print(f"SR3D_SPLIT_F16={mode}: " + "; ".join(f"{k} {err[k]:.1e} (fp32 oracle {floor[k]:.1e})" for k in top))
    print(f"trained model: loss {first:.3f} -> {last:.3f} in 150 steps, weights moved up to {moved:.2f}")
    split, fp32path = report["2"][0], report["0"][0]
    floor = report["2"][1]
    over = sorted(k for k in split if split[k] >= TOL)
    print(f"parameters over {TOL:g} against fp64 -- split-f16: {len(over)} {over}; fp32 MFMA kernels: "
          f"{sum(v >= TOL for v in fp32path.values())}")
    for k in split:
        # (1) the split-f16 kernels lose nothing against the fp32-MFMA kernels of the same engine on trained statistics
        assert split[k] < max(TOL, 1.5 * fp32path[k]), (k, split[k], fp32path[k])
        # (2) 1e-5 holds wherever the gradient is well conditioned (fp32 oracle within 1e-6 of fp64); where it is not -- the
        # saturated gates of the trained down3 / down4 blocks: d_gate = dy*y*(1-sigma) turns an ABSOLUTE error of the gate's
        # pre-activation into a RELATIVE one of 1-sigma, the fp32 oracle itself is 10-20x its usual error there -- a loose bound
        assert split[k] < (TOL if floor[k] < 1e-6 else 5e-5), (k, split[k], floor[k])
    assert len(over) <= 6, over
