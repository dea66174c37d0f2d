"""The error-distribution evaluation without a GPU: the restatement (tests/error_distributions_ref.py) on constructed
inputs, the functions of src/error_distributions.py that turn counts into quantiles and distances, the meter, the C ABI
(symbols, signatures, index maps, workspace size, argument errors: every one is returned before anything is launched)
and the table script/evaluate_error_distributions.py writes, on a stubbed ``ops.eval_distributions``."""
import ctypes as C
import importlib.util
import logging
import os
import re

import numpy as np
import pytest
import torch

import error_distributions_ref as ER
from helpers import ROOT

SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "evaluate_error_distributions.py")
STDS = [8.4, 14.4, 21.6, 7.0]
MEANS = [300.0, 0.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def ED(eng):
    from sr3d_amd.src import error_distributions
    return error_distributions


def noisy_fields(shape, seed, sigma=0.03):
    """t ~ U[0, 1), p = t + N(0, sigma): the default ranges hold every series"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    return t + sigma * torch.randn(shape, generator=g), t


# ---- the restatement -----------------------------------------------------------------------------------------------
def test_rule_on_edges_infinities_and_nan():
    lo, hi = -0.5, 0.5
    w = 1.0 / 256
    edges = np.float32(lo) + np.arange(257, dtype=np.float32) * np.float32(w)      # exact: multiples of 2^-8
    s = ER.slots(edges, lo, hi)
    assert list(s[:256]) == list(range(1, 257))            # an edge belongs to the bin it opens: left-closed
    assert s[256] == ER.OVER                               # hi itself is overflow
    assert list(ER.slots(edges[:256] + np.float32(w / 2), lo, hi)) == list(range(1, 257))
    # the rule acts on the ROUNDED difference: the fp32 number just below an edge may round onto it (and np.histogram
    # in float64 would put it one bin lower); just below lo there is nothing to round to but a negative number
    below = np.nextafter(edges, np.float32(-np.inf), dtype=np.float32)
    s_below = ER.slots(below, lo, hi)
    assert s_below[0] == ER.UNDER and bool(((s_below[1:] == np.arange(1, 257)) | (s_below[1:] == s[1:])).all())
    assert bool((s_below[1:] == s[1:]).any()) and bool((s_below[1:] != s[1:]).any())
    special = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 0.0, -0.0], dtype=np.float32)
    assert list(ER.slots(special, lo, hi)) == [ER.OVER, ER.UNDER, ER.NAN, ER.OVER, ER.UNDER, 129, 129]


@pytest.mark.parametrize("lo,hi", [(-0.5, 0.5), (-0.5, 1.5), (0.0, 8.0)])
def test_rule_brackets_the_rounded_difference(lo, hi):
    """with 256 / (hi - lo) a power of two the product is exact: k w <= fl(v - lo) < (k + 1) w for every binned value"""
    g = np.random.default_rng(5)
    v = np.concatenate([g.uniform(lo - 0.1, hi + 0.1, 20000), g.normal(lo, 1e-6, 2000), g.normal(hi, 1e-6, 2000),
                        lo + (hi - lo) / 256 * g.integers(0, 257, 2000) + g.normal(0, 1e-7, 2000)]).astype(np.float32)
    s = ER.slots(v, lo, hi)
    w = (hi - lo) / 256
    d = (v - np.float32(lo)).astype(np.float64)            # the fp32-rounded difference, held exactly
    k = s - 1
    mid = (s >= 1) & (s <= 256)
    assert mid.sum() > 15000 and (s == ER.UNDER).sum() > 1000 and (s == ER.OVER).sum() > 1000
    assert bool((k[mid] * w <= d[mid]).all()) and bool((d[mid] < (k[mid] + 1) * w).all())
    assert bool((d[s == ER.UNDER] < 0).all()) and bool((d[s == ER.OVER] >= hi - lo).all())


def test_restatement_counts_classes_and_minmax():
    B, Z, Y, X = 2, 5, 6, 7
    p, t = noisy_fields((B, 4, Z, Y, X), 11)
    b = torch.ones(B, 1, Z, Y, X)
    b[0, 0, :2, 2:4, 3:5] = 0
    b[1, 0, 0, 0, 0] = 0.5          # fractional: fluid (b > 0) and near a wall (1 - b > 0 at distance 0)
    p[0, 0, 4, 5, 6], p[0, 1, 4, 5, 5], t[1, 2, 3, 3, 3] = float("nan"), float("inf"), float("-inf")
    p[0, 3, 0, 2, 3] = float("nan")                          # in a built cell: never counted
    for nw in (0, 1, 2):
        counts, minmax, cells = ER.distributions_ref(p, t, b, STDS, near_width=nw)
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (13, 2, 259) and tuple(minmax.shape) == (13, 2, 2)
        assert int(cells.sum()) == B * Z * Y * X and int(cells[0]) == 8
        for s in range(13):                                  # every series' counts sum to the class's cells
            assert counts[s].sum(dim=1).tolist() == cells[1:].tolist(), (nw, s)
        if nw == 0:
            assert int(cells[1]) == 0 and bool(torch.isinf(minmax[:, 0]).all())
        else:
            near = ER.classes(b, nw) == 0
            assert int(cells[1]) == int(near.sum()) > 0 and bool(near[1, 0, 0, 0])
        both = counts.sum(dim=1)
        I = {n: i for i, n in enumerate(ER.SERIES)}
        assert int(both[I["PRED_T"], ER.NAN]) == 1 and int(both[I["ERR_T"], ER.NAN]) == 1
        assert int(both[I["PRED_W"], ER.NAN]) == 0
        assert int(both[I["PRED_U"], ER.OVER]) == 1 and int(both[I["ERR_U"], ER.OVER]) == 1
        assert int(both[I["TRUTH_V"], ER.UNDER]) == 1 and int(both[I["ERR_V"], ER.OVER]) == 1      # p - (-inf) = +inf
        assert int(both[I["ERR_VEL_NORM"], ER.OVER]) == 2 and int(both[I["ERR_VEL_NORM"], ER.NAN]) == 0
        assert float(minmax[I["PRED_U"]].max()) == float("inf") and float(minmax[I["TRUTH_V"]].min()) == float("-inf")
        assert not bool(torch.isnan(minmax).any())
    per = ER.distributions_ref(p, t, b, STDS, near_width=1, per_sample=True)
    whole = ER.distributions_ref(p, t, b, STDS, near_width=1)
    assert torch.equal(per[0].sum(dim=0), whole[0]) and torch.equal(per[2].sum(dim=0), whole[2])
    assert torch.equal(per[1][..., 0].min(dim=0).values, whole[1][..., 0])


# ---- counts -> quantiles, folded quantiles, distances ----------------------------------------------------------------
def test_bin_edges(ED):
    e = ED.bin_edges(-0.5, 1.5)
    assert e.shape == (257,) and e[0] == -0.5 and e[-1] == 1.5 and e[64] == 0.0 and np.all(np.diff(e) == 2.0 / 256)


def test_quantiles_within_one_bin_of_numpy(ED):
    """noise sigma = 0.03 on t ~ U[0, 1): the default ranges hold everything, so every quantile read off the counts is
    within one bin width of np.quantile of the raw values (a value is displaced by less than a bin)"""
    p, t = noisy_fields((2, 4, 19, 23, 67), 3)
    b = torch.ones(2, 1, 19, 23, 67)
    counts, minmax, cells = ER.distributions_ref(p, t, b, STDS, near_width=0)
    lo, hi = ER.ranges()
    assert int(counts[:, :, [ER.UNDER, ER.OVER, ER.NAN]].sum()) == 0
    assert int(counts[:, 1, 1:257].max()) <= 0.06 * int(cells[2])
    vals = ER.series_values(p, t, STDS)
    qs = np.array(ED.QUANTILES) / 100.0
    for s, name in enumerate(ER.SERIES):
        w = (float(hi[s]) - float(lo[s])) / 256
        got, flag = ED.quantiles_from_counts(counts[s, 1].numpy(), lo[s], hi[s], qs)
        ref = np.quantile(vals[s].astype(np.float64).ravel(), qs)
        print(name, "worst |difference| / bin width", float(np.abs(got - ref).max() / w))
        assert not flag.any() and bool((np.abs(got - ref) <= w).all()), (name, got, ref)
        if name in ("ERR_T", "ERR_U", "ERR_V", "ERR_W"):
            aq = np.array(ED.ABS_QUANTILES) / 100.0
            got, flag = ED.abs_quantiles_from_counts(counts[s, 1].numpy(), lo[s], hi[s], aq)
            ref = np.quantile(np.abs(vals[s].astype(np.float64)).ravel(), aq)
            assert not flag.any() and bool((np.abs(got - ref) <= w).all()), (name, got, ref)
    # leading dimensions are kept
    got, flag = ED.quantiles_from_counts(counts[:4].numpy(), lo[0], hi[0], [0.5])
    assert got.shape == (4, 2, 1) and np.isnan(got[:, 0]).all() and not np.isnan(got[:, 1]).any()


def test_quantiles_on_hand_made_counts(ED):
    c = np.zeros(259, dtype=np.int64)
    got, flag = ED.quantiles_from_counts(c, 0.0, 256.0, [0.0, 0.5, 1.0])
    assert np.isnan(got).all() and not flag.any()              # an empty class
    c[11] = 4                                                   # four values in bin 10 = [10, 11)
    got, flag = ED.quantiles_from_counts(c, 0.0, 256.0, [0.0, 0.5, 1.0])
    assert np.array_equal(got, [10.125, 10.5, 10.875]) and not flag.any()     # linear inside the bin
    c[0], c[257] = 1, 3                                         # one below, three above the range
    got, flag = ED.quantiles_from_counts(c, 0.0, 256.0, [0.0, 0.5, 0.9, 1.0])
    assert got[0] == 0.0 and got[-1] == 256.0 and list(flag) == [True, False, True, True]
    assert 10.0 <= got[1] < 11.0
    c[258] = 100                                                # NaN values never move a quantile
    again, _ = ED.quantiles_from_counts(c, 0.0, 256.0, [0.0, 0.5, 0.9, 1.0])
    assert np.array_equal(again, got)
    with pytest.raises(ValueError):
        ED.quantiles_from_counts(c[:-1], 0.0, 1.0, [0.5])
    with pytest.raises(ValueError):
        ED.quantiles_from_counts(c, 0.0, 1.0, [1.5])


def test_folding_and_wasserstein_are_exact_on_hand_made_counts(ED):
    c = np.zeros(259, dtype=np.int64)
    c[1 + 128], c[1 + 127], c[1 + 130], c[1 + 125], c[1 + 0], c[1 + 255], c[0], c[257] = 5, 7, 2, 3, 1, 1, 4, 6
    under, bins, over = ED.fold_counts(c, -1.0, 1.0)
    assert under == 0 and over == 10 and bins.shape == (128,)
    assert bins[0] == 12 and bins[2] == 5 and bins[127] == 2 and int(bins.sum()) == 19
    with pytest.raises(ValueError):
        ED.fold_counts(c, -0.5, 1.5)
    got, flag = ED.abs_quantiles_from_counts(c, -1.0, 1.0, [0.0, 1.0])
    assert got[0] == 1.0 / 128 * (0.5 / 12) and got[1] == 1.0 and list(flag) == [False, True]
    # two identical histograms: 0; all mass moved by 3 bins: 3 bin widths; half of it: 1.5
    a, b = np.zeros(259, dtype=np.int64), np.zeros(259, dtype=np.int64)
    a[50], b[53] = 8, 8
    w = 2.0 / 256
    assert ED.wasserstein1(a, a, -1.0, 1.0) == 0.0 and ED.wasserstein1(c, c, -1.0, 1.0) == 0.0
    assert ED.wasserstein1(a, b, -1.0, 1.0) == 3 * w == ED.wasserstein1(b, a, -1.0, 1.0)
    b[50], b[53] = 4, 4
    assert ED.wasserstein1(a, b, -1.0, 1.0) == 1.5 * w
    a[258] = 1000                                               # NaN slot: left out
    assert ED.wasserstein1(a, b, -1.0, 1.0) == 1.5 * w
    assert np.isnan(ED.wasserstein1(np.zeros(259, dtype=np.int64), b, -1.0, 1.0))


def test_meter_over_batches_is_the_histogram_of_the_pooled_set(ED):
    """integer adds are exact: three batches through the meter equal one call on their concatenation, bit for bit"""
    Z, Y, X = 5, 6, 9
    batches = []
    for i, n in enumerate((1, 2, 3)):
        p, t = noisy_fields((n, 4, Z, Y, X), 20 + i, sigma=0.3)      # wide noise: under- and overflow are populated
        b = torch.ones(n, 1, Z, Y, X)
        b[:, 0, :2, i:i + 2, 3:5] = 0
        batches.append((p, t, b))
    meter = ED.DistributionMeter()
    with pytest.raises(RuntimeError):
        meter.result()
    for p, t, b in batches:
        meter.update(*ER.distributions_ref(p, t, b, STDS, near_width=1))
    counts, minmax, cells = meter.result()
    ref = ER.distributions_ref(*(torch.cat(x) for x in zip(*batches)), STDS, near_width=1)
    assert counts.dtype == np.int64 and minmax.dtype == np.float32 and cells.dtype == np.int64
    assert np.array_equal(counts, ref[0].numpy()) and np.array_equal(cells, ref[2].numpy())
    assert np.array_equal(minmax.view(np.int32), ref[1].numpy().view(np.int32))
    assert int(counts[:, :, [ER.UNDER, ER.OVER]].sum()) > 0
    with pytest.raises(ValueError):
        meter.update(*ER.distributions_ref(*batches[1], STDS, per_sample=True))


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_cabi_symbols_signatures_and_index_maps(eng):
    L = eng._lib
    P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    FP = C.POINTER(F)
    want = {"sr3d_eval_distributions_workspace_bytes": (SZ, [I] * 4),
            "sr3d_eval_distributions": (I, [P, P, P, P, I, I, I, I, FP, FP, FP, I, I, P, P, P, P, P])}
    for name, (res, args) in want.items():
        assert hasattr(L.lib, name), name
        assert L.SYMBOLS[name][0] is res and L.SYMBOLS[name][1] == args, name
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr3d.h")).read(), flags=re.S)
    decl = re.search(r"\bint sr3d_eval_distributions\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")] == [
        "p", "t", "b", "dist", "B", "Z", "Y", "X", "stds", "lo", "hi", "near_width", "per_sample", "counts_out",
        "minmax_out", "cells_out", "workspace", "stream"]
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSR3D_DIST_([A-Z_]+) = (\d+)", text)}
    assert enum == L.DIST_SERIES_INDEX and [n for n, _ in sorted(enum.items(), key=lambda kv: kv[1])] == list(ER.SERIES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SR3D_DIST_([A-Z]+) (\d+)", text)}
    assert defs == {"SERIES": L.DIST_SERIES, "CLASSES": L.DIST_CLASSES, "BINS": L.DIST_BINS, "SLOTS": L.DIST_SLOTS}
    assert (L.DIST_SERIES, L.DIST_CLASSES, L.DIST_BINS, L.DIST_SLOTS) == (13, 2, 256, 259) == (
        ER.NSERIES, ER.NCLASSES, ER.NBINS, ER.NSLOTS)
    lo, hi = eng.ops.distribution_ranges()
    rlo, rhi = ER.ranges()
    assert lo == rlo.tolist() and hi == rhi.tolist()
    lo, hi = eng.ops.distribution_ranges(err_range=[(-1, 1), (-2, 2), (-3, 3), (-4, 4)], field_range=(0, 1))
    assert lo == [-1, -2, -3, -4, 0, 0, 0, 0, 0, 0, 0, 0, 0] and hi == [1, 2, 3, 4, 8, 1, 1, 1, 1, 1, 1, 1, 1]


def test_cabi_workspace_and_argument_errors(eng):
    L = eng._lib
    ws = L.lib.sr3d_eval_distributions_workspace_bytes
    rec = (13 * 2 * 259 + 3 + 13 * 2 * 2) * 4       # a workgroup's record: the counters, the cell counts, min / max
    # one workgroup per 4096 voxels of a sample, at most 256 per sample
    assert ws(1, 32, 320, 320) == 256 * rec and ws(2, 19, 23, 67) == 2 * 8 * rec and ws(3, 1, 1, 1) == 3 * rec
    assert ws(1, 1, 1, 4096) == rec and ws(1, 1, 1, 4097) == 2 * rec
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0)):
        assert ws(*bad) == 0
    p = C.c_void_p(0x1000)      # never dereferenced: every call below fails its checks before a launch
    sc = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    rlo, rhi = ER.ranges()

    def bounds(lo=None, hi=None, at=0):
        a, b = rlo.copy(), rhi.copy()
        if lo is not None:
            a[at] = lo
        if hi is not None:
            b[at] = hi
        return dict(lo=(C.c_float * 13)(*a.tolist()), hi=(C.c_float * 13)(*b.tolist()))

    def call(**over):
        a = dict(p=p, t=p, b=p, dist=p, B=1, Z=4, Y=6, X=8, stds=sc, nw=1, per=0, counts=p, minmax=p, cells=p, ws=p,
                 **bounds())
        a.update(over)
        return L.lib.sr3d_eval_distributions(a["p"], a["t"], a["b"], a["dist"], a["B"], a["Z"], a["Y"], a["X"], a["stds"],
                                             a["lo"], a["hi"], a["nw"], a["per"], a["counts"], a["minmax"], a["cells"],
                                             a["ws"], None)

    nan, inf = float("nan"), float("inf")
    for over in (dict(p=None), dict(t=None), dict(b=None), dict(stds=None), dict(lo=None), dict(hi=None),
                 dict(counts=None), dict(minmax=None), dict(cells=None), dict(ws=None), dict(B=0), dict(Z=0),
                 dict(Y=-3), dict(X=0), dict(Z=2048, Y=1024, X=1024), dict(B=65536), dict(nw=-1), dict(nw=255),
                 bounds(hi=-0.5), bounds(hi=-0.6), bounds(lo=nan), bounds(hi=nan, at=7), bounds(hi=inf, at=12),
                 bounds(lo=-inf, at=4),
                 bounds(lo=0.0, hi=1e-44, at=3),         # finite, lo < hi, but 256 / (hi - lo) is not an fp32 number
                 dict(p=C.c_void_p(0x1002)), dict(counts=C.c_void_p(0x1004))):
        assert call(**over) == -1, over
        assert L.lib.sr3d_last_error().decode().startswith("eval_distributions: "), over
    assert call(nw=255) == -1 and b"0 .. 254" in L.lib.sr3d_last_error()
    assert call(**bounds(lo=0.5, hi=0.5, at=2)) == -1 and b"series 2" in L.lib.sr3d_last_error()
    with pytest.raises(RuntimeError, match="lo < hi"):
        L.check(call(**bounds(hi=nan)), "sr3d_eval_distributions")


def test_python_surface_refuses_before_any_launch(eng):
    ops = eng.ops
    b = torch.ones(1, 1, 4, 6, 8)
    p = torch.rand(1, 4, 4, 6, 8)
    with pytest.raises(ValueError, match="B,4,Z,Y,X"):
        ops.eval_distributions(p, p, b[:, 0], STDS)
    with pytest.raises(ValueError, match="B,4,Z,Y,X"):
        ops.eval_distributions(p[:, :3], p[:, :3], b, STDS)
    with pytest.raises(ValueError, match="stds"):
        ops.eval_distributions(p, p, b, STDS[:3])
    for kw in (dict(err_range=(0.5, -0.5)), dict(field_range=(0.0, float("nan"))), dict(vel_norm_range=(0.0, float("inf"))),
               dict(err_range=[(-1, 1)] * 3), dict(vel_norm_range=(0.0, 1.0, 2.0))):
        with pytest.raises(ValueError, match="eval_distributions"):
            ops.eval_distributions(p, p, b, STDS, **kw)
    for nw in (-1, 255):
        with pytest.raises(ValueError, match="near_width"):
            ops.eval_distributions(p, p, b, STDS, near_width=nw)
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_distributions(p, p, b, STDS, dist=torch.zeros(b.shape))
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_distributions(p, p, b, STDS, dist=torch.zeros(1, 1, 4, 6, 9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_distributions(p, p, b, STDS, near_width=0)


# ---- the script ------------------------------------------------------------------------------------------------------
def _stub_eval_distributions(p, t, b, stds, *, err_range=(-0.5, 0.5), field_range=(-0.5, 1.5), vel_norm_range=(0.0, 8.0),
                             near_width=1, dist=None, per_sample=False):
    """ops.eval_distributions on the CPU, from the restatement"""
    return ER.distributions_ref(p, t, b, stds, near_width=near_width, per_sample=per_sample, err_range=err_range,
                                field_range=field_range, vel_norm_range=vel_norm_range)


def test_script_table_layout_on_a_stubbed_ops_call(eng, ED, monkeypatch, tmp_path, caplog):
    import pandas as pd
    monkeypatch.setattr(eng.ops, "eval_distributions", _stub_eval_distributions)
    spec = importlib.util.spec_from_file_location("evaluate_error_distributions", SCRIPT)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    assert script.MODEL_CSV == "error_distribution_scores.csv"
    assert script.BASELINE_CSV == "interpolation_baseline_error_distribution_scores.csv"

    Z, Y, X = 7, 9, 12
    loader = []
    for i, n in enumerate((1, 2)):
        pred, y = noisy_fields((n, 4, Z, Y, X), 40 + i)
        b = torch.ones(n, Z, Y, X)
        b[:, :2, 2:4, 3:5] = 0
        loader.append((pred, b, y))
    # one u error above its range, far from the walls; the fields and the velocity norm (0.52 x 14.4 m/s) stay inside
    loader[1][2][1, 1, 6, 8, 11], loader[1][0][1, 1, 6, 8, 11] = 0.25, 0.77

    class Identity(torch.nn.Module):
        def forward(self, X, bb):
            return X

    config = {"data": {"stds": STDS, "means": MEANS}}
    with caplog.at_level(logging.WARNING):
        path, df = script.write_distributions(dataloader=loader, model=Identity(), config=config, device="cpu",
                                              out_dir=str(tmp_path / "out"), file_name=script.MODEL_CSV, near_width=1,
                                              save_histograms=True)
    assert path == str(tmp_path / "out" / "error_distribution_scores.csv")
    back = pd.read_csv(path)
    qcols = [f"q{q:g}" for q in ED.QUANTILES]
    acols = [f"abs_q{q:g}" for q in ED.ABS_QUANTILES]
    assert qcols == ["q0.1", "q1", "q5", "q25", "q50", "q75", "q95", "q99", "q99.9"]
    assert acols == ["abs_q50", "abs_q90", "abs_q99", "abs_q99.9"]
    head = ["series", "class", "cells", "underflow", "overflow", "nan", "min", "max", *qcols, *acols, "w1_to_pred", "clamped"]
    assert list(back.columns[:len(head)]) == head
    assert set(back.columns[len(head):]) == {c + "_phys" for c in ["min", "max", *qcols, *acols, "w1_to_pred"]}
    assert len(back) == 13 * 3 and list(back["series"][::3]) == list(ER.SERIES)
    assert list(back["class"][:3]) == ["near_wall", "far", "fluid"]
    fluid_cells = 3 * (Z * Y * X - 2 * 2 * 2)
    for name in ER.SERIES:
        rows = back[back["series"] == name].set_index("class")
        assert rows["cells"]["near_wall"] + rows["cells"]["far"] == rows["cells"]["fluid"] == fluid_cells
        assert rows["min"]["fluid"] == min(rows["min"]["near_wall"], rows["min"]["far"])
        q = rows.loc["fluid", qcols].to_numpy(dtype=np.float64)
        assert bool((np.diff(q) >= 0).all()) and rows["min"]["fluid"] <= q[0] + 1 / 128 and q[-1] - 1 / 128 <= rows["max"]["fluid"]
        is_err = name in ("ERR_T", "ERR_U", "ERR_V", "ERR_W")
        assert rows[acols].notna().all().all() == is_err and (is_err or rows[acols].isna().all().all())
        assert rows["w1_to_pred"].notna().all() == name.startswith("TRUTH_")
    # the planted error: one overflow in ERR_U (far), the warning names the series and gives its exact maximum
    u = back[back["series"] == "ERR_U"].set_index("class")
    assert (u["overflow"]["near_wall"], u["overflow"]["far"], u["overflow"]["fluid"]) == (0, 1, 1)
    assert int(back["overflow"].sum()) == 2 and int(back["underflow"].sum()) == 0 and int(back["nan"].sum()) == 0
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and warned[0].startswith("ERR_U: 0 values below and 1 above the range -0.5 .. 0.5")
    assert f"max {float(np.float32(u['max']['fluid'])):g}" in warned[0] and 0.51 < u["max"]["fluid"] < 0.53
    # physical units: errors x std, fields x std + mean, the velocity norm as it is
    t_row = back[(back["series"] == "TRUTH_T") & (back["class"] == "fluid")].iloc[0]
    assert np.isclose(t_row["q50_phys"], t_row["q50"] * STDS[0] + MEANS[0], rtol=1e-12)
    assert np.isclose(t_row["w1_to_pred_phys"], t_row["w1_to_pred"] * STDS[0], rtol=1e-12) and t_row["w1_to_pred"] > 0
    e_row = back[(back["series"] == "ERR_V") & (back["class"] == "far")].iloc[0]
    assert np.isclose(e_row["abs_q99_phys"], e_row["abs_q99"] * STDS[2], rtol=1e-12)
    assert np.isclose(e_row["min_phys"], e_row["min"] * STDS[2], rtol=1e-12)
    n_row = back[(back["series"] == "ERR_VEL_NORM") & (back["class"] == "fluid")].iloc[0]
    assert n_row["q50_phys"] == n_row["q50"] and n_row["min"] >= 0
    # the median error of unbiased noise is within a bin of 0, its spread is the noise's
    assert abs(e_row["q50"]) <= 1 / 256 and 0.02 < e_row["abs_q50"] < 0.03 * 0.6745 + 1 / 256
    # the histograms: enough to re-derive every quantile
    z = np.load(str(tmp_path / "out" / "error_distribution_scores_histograms.npz"))
    assert z["counts"].shape == (13, 2, 259) and z["counts"].dtype == np.int64 and list(z["series"]) == list(ER.SERIES)
    assert z["cells"].tolist() == [3 * 8, int(u["cells"]["near_wall"]), int(u["cells"]["far"])] and int(z["near_width"]) == 1
    s = ER.SERIES.index("ERR_V")
    again, _ = ED.quantiles_from_counts(z["counts"][s, 1], z["lo"][s], z["hi"][s], [0.5])
    assert again[0] == e_row["q50"]
