"""The scale-resolved evaluation without a GPU: the restatement (tests/scale_statistics_ref.py) on closed forms, the
functions of src/scale_statistics.py that turn pooled sums into structure functions, correlations and length scales,
the meter, the C ABI (symbols, signatures, index maps, workspace size, argument errors: every one is returned before
anything is launched) and the table script/evaluate_scale_statistics.py writes, on a stubbed
``ops.eval_scale_statistics``."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import scale_statistics_ref as SR
from helpers import ROOT

SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "evaluate_scale_statistics.py")
STDS = [8.4, 14.4, 21.6, 7.0]
M = SR.M


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def SS(eng):
    from sr3d_amd.src import scale_statistics
    return scale_statistics


def quantised_fields(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, shape, generator=g).float() / 256, torch.randint(0, 256, shape, generator=g).float() / 256)


# ---- the restatement -----------------------------------------------------------------------------------------------
def test_restatement_on_a_ramp():
    """f = a x: delta = a r along x and 0 along y and z, so D_k = n (a r)^k, with n = B Z Y (X - r) pairs along x"""
    B, Z, Y, X, R, a = 2, 3, 4, 9, 10, 0.125
    ramp = (a * torch.arange(X).float()).expand(B, 4, Z, Y, X).contiguous()
    sums, pairs, abs_sums = SR.scale_statistics_ref(ramp, torch.zeros_like(ramp), torch.ones(B, 1, Z, Y, X), R)
    assert sums.shape == (Z, 3, R, 12, 8) and pairs.shape == (Z, 3, R) and pairs.dtype == np.int64
    for r in range(1, R + 1):
        n = (B * Z * Y * max(X - r, 0), B * Z * max(Y - r, 0) * X, B * max(Z - r, 0) * Y * X)
        assert pairs[:, :, r - 1].sum(axis=0).tolist() == list(n), r
        for z in range(Z):
            nz = int(pairs[z, 0, r - 1])
            assert nz == B * Y * max(X - r, 0)
            for s in (SR.SERIES.index("PRED_U"), SR.SERIES.index("ERR_W")):      # t = 0: the error is the prediction
                assert sums[z, 0, r - 1, s, :4].tolist() == [nz * (a * r) ** k for k in (1, 2, 3, 4)]
                assert sums[z, 0, r - 1, s, M["F1"]] - sums[z, 0, r - 1, s, M["F0"]] == nz * a * r
            assert not sums[z, 0, r - 1, SR.SERIES.index("TRUTH_T")].any()
            assert not sums[z, 1:, r - 1, :, :4].any()                           # no increment along y and z
            # the level of a z pair is that of its lower cell
            assert int(pairs[z, 2, r - 1]) == (B * Y * X if z + r < Z else 0)
    assert np.array_equal(abs_sums, sums)                                        # every term is non-negative here
    # lags that do not fit are exactly zero
    assert not sums[:, 0, X - 1:].any() and not sums[:, 1, Y - 1:].any() and not sums[:, 2, Z - 1:].any()


def test_restatement_pair_rules_at_a_one_cell_wall():
    """a wall one cell thick at x = w: both rules drop the pairs with an end in the wall; the unobstructed rule also
    drops the pairs that straddle it, x < w < x + r: the first cells max(0, w - r + 1) .. min(w - 1, X - r - 1)"""
    B, Z, Y, X, R, w = 1, 2, 3, 11, 6, 4
    p, t = quantised_fields((B, 4, Z, Y, X), 3)
    b = torch.ones(B, 1, Z, Y, X)
    b[..., w] = 0
    _, open_pairs, _ = SR.scale_statistics_ref(p, t, b, R)
    _, clear_pairs, _ = SR.scale_statistics_ref(p, t, b, R, unobstructed=True)
    for r in range(1, R + 1):
        starts = range(X - r)
        ends_fluid = sum(1 for x in starts if x != w and x + r != w)
        straddle = sum(1 for x in starts if x < w < x + r)
        assert int(open_pairs[0, 0, r - 1]) == Y * ends_fluid, r
        assert int(clear_pairs[0, 0, r - 1]) == Y * (ends_fluid - straddle), r
        assert straddle == min(w - 1, X - r - 1) - max(0, w - r + 1) + 1 and (straddle > 0) == (r > 1), r
    # along y and z every line lies in the wall or outside it: the rules agree
    assert np.array_equal(open_pairs[:, 1:], clear_pairs[:, 1:])
    assert int(open_pairs[0, 1, 0]) == (Y - 1) * (X - 1)
    # a NaN in the wall changes nothing; the same sums to the bit
    pn = p.clone()
    pn[..., w] = float("nan")
    for unob in (False, True):
        a = SR.scale_statistics_ref(p, t, b, R, unobstructed=unob)
        c = SR.scale_statistics_ref(pn, t, b, R, unobstructed=unob)
        assert np.array_equal(a[0].view(np.int64), c[0].view(np.int64)) and np.array_equal(a[1], c[1])


def test_restatement_sums_are_order_independent_on_quantised_fields():
    """multiples of 1 / 256 in [0, 1): every partial sum of every moment is exact in fp64, so per-sample sums add up to
    the whole-batch sums to the bit, and so does a float-sum in another order"""
    p, t = quantised_fields((2, 4, 5, 6, 13), 5)
    b = (torch.rand(2, 1, 5, 6, 13, generator=torch.Generator().manual_seed(6)) > 0.2).float()
    per = SR.scale_statistics_ref(p, t, b, 4, per_sample=True)
    whole = SR.scale_statistics_ref(p, t, b, 4)
    rev = SR.scale_statistics_ref(p.flip(0), t.flip(0), b.flip(0), 4)
    assert np.array_equal(per[0][0] + per[0][1], whole[0]) and np.array_equal(per[1].sum(axis=0), whole[1])
    assert np.array_equal(rev[0], whole[0]) and np.array_equal(rev[1], whole[1])
    # derived sums: sum f f' from the stored moments equals the direct sum
    pn = p.numpy().astype(np.float64)
    fl = b[:, 0].numpy() > 0
    v = fl[..., :-2] & fl[..., 2:]
    direct = np.where(v, pn[:, 1, ..., :-2] * pn[:, 1, ..., 2:], 0.0).sum(axis=(0, 2, 3))
    s = whole[0][:, 0, 1, SR.SERIES.index("PRED_U")]
    assert np.array_equal((s[:, M["FF0"]] + s[:, M["FF1"]] - s[:, M["D2"]]) / 2, direct)


# ---- pooled sums -> statistics ---------------------------------------------------------------------------------------
def synthetic_sums(R, n, s2_p, s2_t, s2_e):
    """(1, 3, R, 12, 8) sums with D2 of pred / truth / err set per lag (arrays of R), same for all channels / directions"""
    sums = np.zeros((1, 3, R, 12, 8))
    pairs = np.full((1, 3, R), n, dtype=np.int64)
    for k, s2 in enumerate((s2_p, s2_t, s2_e)):
        sums[0, :, :, 4 * k:4 * k + 4, M["D2"]] = (n * np.asarray(s2, dtype=np.float64))[None, :, None]
    return sums, pairs


def test_identical_fields_give_correlation_one_error_zero_resolved_lag_one(SS):
    R = 6
    s2 = 0.01 * np.arange(1, R + 1) ** (2.0 / 3.0)
    sums, pairs = synthetic_sums(R, 1000, s2, s2, np.zeros(R))
    assert np.array_equal(SS.increment_correlation(sums, pairs, STDS), np.ones((1, 3, R, 4)))
    assert np.array_equal(SS.relative_error(sums, pairs, STDS), np.zeros((1, 3, R, 4)))
    assert np.array_equal(SS.variance_ratio(sums, pairs, STDS), np.ones((1, 3, R, 4)))
    assert np.array_equal(SS.resolved_lag(sums, pairs, STDS), np.ones((1, 3, 4)))
    S2 = SS.structure_function(sums, pairs, STDS, 2)
    assert S2.shape == (1, 3, R, 12)
    assert np.allclose(S2[0, 1, :, 1], s2 * STDS[1] ** 2, rtol=1e-14) and np.allclose(S2[0, 2, :, 4], s2 * STDS[0] ** 2, rtol=1e-14)
    # from real fields, p == t
    p, _ = quantised_fields((1, 4, 3, 5, 17), 8)
    b = torch.ones(1, 1, 3, 5, 17)
    rs, rn, _ = SR.scale_statistics_ref(p, p, b, 4)
    want = np.broadcast_to(np.where(rn[..., None] > 0, 1.0, np.nan), (3, 3, 4, 4))      # NaN where the lag does not fit
    assert np.array_equal(SS.increment_correlation(rs, rn, STDS), want, equal_nan=True) and np.isnan(want).any()
    res = SS.resolved_lag(*SS.pool_levels(rs, rn), STDS)
    assert res.shape == (3, 4) and np.array_equal(res, np.ones((3, 4)))


def test_resolved_lag_and_relative_error_thresholds(SS):
    rel = np.array([[2.0, 1.2, 0.7, 0.5, 0.3, 0.2], [0.1, 0.9, 0.1, 0.1, np.nan, np.nan], [0.1, 0.2, 0.3, 0.4, 0.45, 0.9],
                    [np.nan] * 6, [0.4, np.nan, 0.3, 0.2, 0.1, 0.0]])
    got = SS.resolved_lag_of(rel, 0.5)
    assert got[0] == 4 and got[1] == 3 and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == 1
    assert SS.resolved_lag_of(rel, 0.25)[0] == 6 and SS.resolved_lag_of(rel, 5.0)[0] == 1


def test_moments_skewness_flatness_and_units(SS):
    """increments +-a with probabilities that give a known skewness: delta = 2 with weight 1 / 5, -1/2 with 4 / 5"""
    n = 500
    sums = np.zeros((3, 2, 12, 8))
    pairs = np.full((3, 2), n, dtype=np.int64)
    vals, wts = np.array([2.0, -0.5]), np.array([0.2, 0.8])
    for k in range(1, 5):
        sums[..., k - 1] = n * float((wts * vals ** k).sum())
    s2, s3, s4 = (float((wts * vals ** k).sum()) for k in (2, 3, 4))
    assert np.allclose(SS.increment_skewness(sums, pairs, STDS), s3 / s2 ** 1.5, rtol=1e-14)
    assert np.allclose(SS.increment_flatness(sums, pairs, STDS), s4 / s2 ** 2, rtol=1e-14)
    for k in (1, 2, 3, 4):
        S = SS.structure_function(sums, pairs, STDS, k)
        want = float((wts * vals ** k).sum()) * np.tile(np.array(STDS), 3) ** k
        assert np.allclose(S, want[None, None], rtol=1e-14), k
    with pytest.raises(ValueError):
        SS.structure_function(sums, pairs, STDS, 5)
    with pytest.raises(ValueError):
        SS.structure_function(sums[..., :7], pairs, STDS, 2)
    with pytest.raises(ValueError):
        SS.structure_function(sums, pairs[:2], STDS, 2)


def rho_sums(rho, n=4096, mean=0.25, var=2.0):
    """(3, R, 12, 8) sums of a stationary series with that autocorrelation: both ends mean and variance as given"""
    rho = np.asarray(rho, dtype=np.float64)
    R = len(rho)
    sums = np.zeros((3, R, 12, 8))
    pairs = np.full((3, R), n, dtype=np.int64)
    sums[..., M["F0"]] = sums[..., M["F1"]] = n * mean
    sums[..., M["FF0"]] = sums[..., M["FF1"]] = n * (var + mean ** 2)
    cross = n * (rho * var + mean ** 2)                    # sum f f'
    sums[..., M["D2"]] = (2 * n * (var + mean ** 2) - 2 * cross)[None, :, None]
    return sums, pairs


def test_autocorrelation_and_integral_scale_of_a_geometric_correlation(SS):
    phi, delta = 0.5, 5.0
    R = 40
    sums, pairs = rho_sums(phi ** np.arange(1, R + 1))
    rho = SS.autocorrelation(sums, pairs, STDS)
    assert rho.shape == (3, R, 12) and np.allclose(rho, (phi ** np.arange(1, R + 1))[None, :, None], rtol=0, atol=1e-12)
    # positive everywhere: the sum runs to R and is flagged; delta (1/2 + phi (1 - phi^R) / (1 - phi))
    scale, trunc = SS.integral_length_scale(sums, pairs, STDS, delta)
    assert scale.shape == (3, 12) and trunc.all()
    assert np.allclose(scale, delta * (0.5 + phi * (1 - phi ** R) / (1 - phi)), rtol=1e-10)
    assert abs(float(scale[0, 0]) - delta * (0.5 + phi / (1 - phi))) < 1e-9            # R = 40: the closed form of the full series
    scale3, trunc3 = SS.integral_length_scale(*rho_sums(phi ** np.arange(1, 4)), STDS, delta)
    assert trunc3.all() and np.allclose(scale3, delta * (0.5 + 0.5 + 0.25 + 0.125), rtol=1e-12)
    # a zero crossing inside R ends the sum and clears the flag: lags before it only
    r = np.array([0.8, 0.4, 0.1, -0.2, 0.3, 0.3])
    s, tr = SS.integral_length_scale_of(r, 2.0)
    assert not tr and s == pytest.approx(2.0 * (0.5 + 1.3), rel=1e-15)
    s, tr = SS.integral_length_scale_of(np.array([[-0.1, 0.5], [0.5, np.nan], [np.nan, 0.5], [0.0, 0.1]]), 2.0)
    assert s[0] == 1.0 and not tr[0] and s[1] == 2.0 and tr[1] and np.isnan(s[2]) and tr[2] and s[3] == 1.0 and not tr[3]
    # the two ends of a masked pair set have their own means and variances
    sums, pairs = rho_sums([0.5])
    sums[..., M["F1"]] += 4096 * 1.0                                                   # shift the second end by +1
    sums[..., M["FF1"]] += 4096 * (2 * 0.25 + 1.0)
    sums[..., M["D2"]] += 4096 * 1.0                                                   # delta grows by 1: D2 + 2 D1 + 1, D1 = 0
    assert np.allclose(SS.autocorrelation(sums, pairs), 0.5, atol=1e-12)


def test_zero_pairs_and_zero_denominators_are_nan_never_an_exception(SS):
    R = 3
    sums, pairs = synthetic_sums(R, 10, [1.0, 1.0, 1.0], [1.0, 0.0, 1.0], [0.5, 0.5, 0.5])
    pairs[0, :, 2] = 0
    sums[0, :, 2] = 0
    with np.errstate(all="raise"):
        S2 = SS.structure_function(sums, pairs, STDS, 2)
        rel, ratio, corr = SS.relative_error(sums, pairs), SS.variance_ratio(sums, pairs), SS.increment_correlation(sums, pairs)
        skew, flat, rho = SS.increment_skewness(sums, pairs), SS.increment_flatness(sums, pairs), SS.autocorrelation(sums, pairs)
        scale, trunc = SS.integral_length_scale(sums, pairs)
        res = SS.resolved_lag(sums, pairs)
    assert np.isnan(S2[0, :, 2]).all() and not np.isnan(S2[0, :, :2]).any()
    assert np.isnan(rel[0, :, 1:]).all() and (rel[0, :, 0] == 0.5).all()              # S2_truth = 0 at lag 2, no pairs at lag 3
    assert np.isnan(ratio[0, :, 1:]).all() and np.isnan(corr[0, :, 1:]).all() and (corr[0, :, 0] == 0.75).all()
    assert np.isnan(skew[0, :, 2]).all() and np.isnan(flat[0, :, 2]).all() and np.isnan(rho).all()      # variances are 0 here
    assert np.isnan(scale).all() and trunc.all()
    assert (res == 1).all()


def test_meter_pools_in_any_order_on_exact_data(SS):
    shape = (1, 4, 4, 5, 11)
    batches = []
    for i in range(3):
        p, t = quantised_fields(shape, 30 + i)
        b = (torch.rand(1, 1, 4, 5, 11, generator=torch.Generator().manual_seed(40 + i)) > 0.15).float()
        batches.append(SR.scale_statistics_ref(p, t, b, 4)[:2])
    meter = SS.ScaleStatisticsMeter()
    with pytest.raises(RuntimeError):
        meter.result()
    results = []
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        meter.reset()
        for i in order:
            meter.update(torch.from_numpy(batches[i][0]), torch.from_numpy(batches[i][1]))
        results.append(meter.result())
    for s, n in results[1:]:
        assert np.array_equal(s.view(np.int64), results[0][0].view(np.int64)) and np.array_equal(n, results[0][1])
    assert results[0][0].dtype == np.float64 and results[0][1].dtype == np.int64
    assert np.array_equal(results[0][1], sum(b[1] for b in batches))
    with pytest.raises(ValueError):
        meter.update(batches[0][0][None], batches[0][1][None])          # the per-sample form
    with pytest.raises(ValueError):
        meter.update(batches[0][0][:, :, :2], batches[0][1][:, :, :2])  # another max_lag


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_cabi_symbols_signatures_and_index_maps(eng):
    L = eng._lib
    P, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    want = {"sr3d_eval_scale_statistics_workspace_bytes": (SZ, [I] * 5),
            "sr3d_eval_scale_statistics": (I, [P, P, P, I, I, I, I, I, I, P, P, P, P])}
    for name, (res, args) in want.items():
        assert hasattr(L.lib, name), name
        assert L.SYMBOLS[name][0] is res and L.SYMBOLS[name][1] == args, name
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr3d.h")).read(), flags=re.S)
    decl = re.search(r"\bint sr3d_eval_scale_statistics\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "p", "t", "b", "B", "Z", "Y", "X", "R", "unobstructed", "sums_out", "pairs_out", "workspace", "stream"]
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SR3D_SCALE_([A-Z_]+) (\d+)", text)}
    assert defs == {"MAX_LAG": 64, "SERIES": 12, "MOMENTS": 8, "DIRS": 3}
    assert (L.SCALE_MAX_LAG, L.SCALE_SERIES, L.SCALE_MOMENTS, len(L.SCALE_DIRS)) == (64, 12, 8, 3) == (
        SR.MAX_LAG, SR.NSERIES, SR.NMOMENTS, SR.NDIRS)
    moments = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSR3D_SCALE_MOMENT_([A-Z0-9]+) = (\d+)", text)}
    assert moments == L.SCALE_MOMENT_INDEX == SR.M
    first = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSR3D_SCALE_(PRED|TRUTH|ERR)_T = (\d+)", text)}
    assert first == {"PRED": 0, "TRUTH": 4, "ERR": 8}
    assert L.SCALE_SERIES_INDEX == {n: i for i, n in enumerate(SR.SERIES)} and L.SCALE_DIRS == SR.DIRS == ("x", "y", "z")
    for kind, base in first.items():
        assert [L.SCALE_SERIES_INDEX[f"{kind}_{c}"] for c in "TUVW"] == [base, base + 1, base + 2, base + 3]


def test_cabi_workspace_and_argument_errors(eng):
    L = eng._lib
    ws = L.lib.sr3d_eval_scale_statistics_workspace_bytes
    assert ws(1, 32, 320, 320, 32) >= 3 * 32 * 320 * 320 and ws(1, 1, 1, 1, 1) >= 3
    base = (2, 19, 23, 67, 5)
    for i in range(5):          # monotone in every argument
        more = list(base)
        more[i] += 1
        assert ws(*more) >= ws(*base) > 0, i
    assert ws(4, 19, 23, 67, 5) > ws(*base) and ws(2, 19, 23, 68, 5) > ws(*base)
    for bad in ((0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, -1, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 0), (1, 4, 4, 4, 65)):
        assert ws(*bad) == 0
    p = C.c_void_p(0x1000)      # never dereferenced: every call below fails its checks before a launch

    def call(**over):
        a = dict(p=p, t=p, b=p, B=1, Z=4, Y=6, X=8, R=4, unob=0, sums=p, pairs=p, ws=p)
        a.update(over)
        return L.lib.sr3d_eval_scale_statistics(a["p"], a["t"], a["b"], a["B"], a["Z"], a["Y"], a["X"], a["R"], a["unob"],
                                                a["sums"], a["pairs"], a["ws"], None)

    for over in (dict(p=None), dict(t=None), dict(b=None), dict(sums=None), dict(pairs=None), dict(ws=None),
                 dict(ws=None, unob=1), dict(R=0), dict(R=-1), dict(R=65), dict(R=65, unob=1), dict(B=0), dict(Z=0),
                 dict(Y=-3), dict(X=0), dict(Z=2048, Y=1024, X=1024), dict(B=65536), dict(p=C.c_void_p(0x1002)),
                 dict(sums=C.c_void_p(0x1004)), dict(pairs=C.c_void_p(0x1004))):
        assert call(**over) == -1, over
        assert L.lib.sr3d_last_error().decode().startswith("eval_scale_statistics: "), over
    assert call(R=65) == -1 and b"1 .. 64" in L.lib.sr3d_last_error()
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.check(call(Z=2048, Y=1024, X=1024), "sr3d_eval_scale_statistics")


def test_python_surface_refuses_before_any_launch(eng):
    ops = eng.ops
    b = torch.ones(1, 1, 4, 6, 8)
    p = torch.rand(1, 4, 4, 6, 8)
    with pytest.raises(ValueError, match="B,4,Z,Y,X"):
        ops.eval_scale_statistics(p, p, b[:, 0])
    with pytest.raises(ValueError, match="B,4,Z,Y,X"):
        ops.eval_scale_statistics(p[:, :3], p[:, :3], b)
    with pytest.raises(ValueError, match="B,4,Z,Y,X"):
        ops.eval_scale_statistics(p, p[..., :7], b)
    for R in (0, -2, 65):
        with pytest.raises(ValueError, match="max_lag"):
            ops.eval_scale_statistics(p, p, b, max_lag=R)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_scale_statistics(p, p, b)
    with pytest.raises(TypeError):
        ops.eval_scale_statistics(p, p, b, 8)           # max_lag is keyword-only


# ---- the script ------------------------------------------------------------------------------------------------------
def _stub_eval_scale_statistics(p, t, b, *, max_lag=32, unobstructed=False, per_sample=False):
    """ops.eval_scale_statistics on the CPU, from the restatement"""
    s, n, _ = SR.scale_statistics_ref(p, t, b, max_lag, unobstructed=unobstructed, per_sample=per_sample)
    return torch.from_numpy(s), torch.from_numpy(n)


@pytest.mark.parametrize("per_level", [False, True])
def test_script_table_layout_on_a_stubbed_ops_call(eng, SS, monkeypatch, tmp_path, per_level):
    import pandas as pd
    monkeypatch.setattr(eng.ops, "eval_scale_statistics", _stub_eval_scale_statistics)
    spec = importlib.util.spec_from_file_location("evaluate_scale_statistics", SCRIPT)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    assert script.MODEL_CSV == "scale_statistics_scores.csv"
    assert script.BASELINE_CSV == "interpolation_baseline_scale_statistics_scores.csv"

    Z, Y, X, R = 3, 9, 14, 5
    g = torch.Generator().manual_seed(50)
    loader = []
    for n in (1, 2):
        y = torch.rand(n, 4, Z, Y, X, generator=g)
        # a blurred prediction: the running mean of the truth along x (smooth: small-scale variance is lost)
        pred = (y + torch.roll(y, 1, -1) + torch.roll(y, -1, -1)) / 3
        b = torch.ones(n, Z, Y, X)
        b[:, :2, 2:4, 6] = 0
        loader.append((pred, b, y))

    class Identity(torch.nn.Module):
        def forward(self, X, bb):
            return X

    config = {"data": {"stds": STDS}}
    path, df = script.write_scale_statistics(dataloader=loader, model=Identity(), config=config, device="cpu",
                                             out_dir=str(tmp_path / "out"), file_name=script.MODEL_CSV, max_lag=R,
                                             unobstructed=True, per_level=per_level, delta_meter=5.0, save_sums=True)
    assert path == str(tmp_path / "out" / "scale_statistics_scores.csv")
    back = pd.read_csv(path)
    lead = (["level"] if per_level else []) + ["channel", "direction", "lag", "distance_m", "pairs", "longitudinal"]
    per_kind = ["S2", "S3", "S4", "skewness", "flatness", "rho"]
    cols = lead + [f"{q}_{k}" for k in SS.KINDS for q in per_kind] + ["variance_ratio", "increment_correlation", "relative_error"]
    cols += [f"integral_scale_{k}_{s}" for k in SS.KINDS for s in ("m", "truncated")] + ["resolved_lag", "resolved_distance_m"]
    assert list(back.columns) == cols
    blocks = Z if per_level else 1
    assert len(back) == blocks * 4 * 3 * R
    one = back[back["level"] == 0] if per_level else back
    assert list(one["channel"][::3 * R]) == ["T", "u", "v", "w"] and list(one["direction"][:3 * R:R]) == ["x", "y", "z"]
    assert list(one["lag"][:R]) == list(range(1, R + 1)) and list(one["distance_m"][:R]) == [5.0 * r for r in range(1, R + 1)]
    flagged = {(r.channel, r.direction) for r in back.itertuples() if r.longitudinal}
    assert flagged == {("u", "x"), ("v", "y"), ("w", "z")}
    # against the restatement on the same batches
    pooled = [SR.scale_statistics_ref(pr, y, b.unsqueeze(1), R, unobstructed=True) for pr, b, y in loader]
    sums, pairs = sum(x[0] for x in pooled), sum(x[1] for x in pooled)
    z = np.load(str(tmp_path / "out" / "scale_statistics_scores_sums.npz"))
    assert np.array_equal(z["sums"], sums) and np.array_equal(z["pairs"], pairs) and bool(z["unobstructed"])
    assert list(z["series"]) == list(SR.SERIES) and list(z["moments"]) == list(SR.MOMENTS) and list(z["directions"]) == ["x", "y", "z"]
    for row in back.itertuples():
        c, d, r = "Tuvw".index(row.channel), "xyz".index(row.direction), row.lag
        s, n = (sums[row.level], pairs[row.level]) if per_level else (sums.sum(axis=0), pairs.sum(axis=0))
        assert row.pairs == n[d, r - 1]
        if row.pairs == 0:                       # R = 5 > Z - 1: the lag does not fit along z from this level up
            assert row.direction == "z" and r >= Z - (row.level if per_level else 0)
            assert np.isnan(row.S2_pred) and np.isnan(row.relative_error) and np.isnan(row.rho_err)
            continue
        for k, kind in enumerate(SS.KINDS):
            want = s[d, r - 1, 4 * k + c, M["D2"]] / n[d, r - 1] * STDS[c] ** 2
            assert getattr(row, f"S2_{kind}") == pytest.approx(want, rel=1e-13)
        dp, dt, de = (s[d, r - 1, 4 * k + c, M["D2"]] for k in range(3))
        assert row.variance_ratio == pytest.approx(dp / dt, rel=1e-13)
        assert row.relative_error == pytest.approx(de / dt, rel=1e-13)
        assert row.increment_correlation == pytest.approx((dp + dt - de) / (2 * np.sqrt(dp * dt)), rel=1e-12)
    assert int((back["pairs"] == 0).sum()) == 4 * (3 + 4 + 5 if per_level else 3)
    # the blur: along x the prediction has lost most of the lag-1 variance, along y and z a third of the noise remains
    x1 = one[(one["direction"] == "x") & (one["lag"] == 1)]
    have = one[one["pairs"] > 0]
    assert bool((x1["variance_ratio"] < 0.5).all()) and bool((have["variance_ratio"] < 1.0).all())
    assert bool((have["flatness_truth"] > 1.0).all()) and bool((have["S2_err"] > 0).all()) and len(have) > 40
    # the wall at x = 6 of levels 0 and 1: fewer pairs along x than an empty domain has
    if not per_level:
        assert int(x1["pairs"].iloc[0]) == 3 * (Z * Y * (X - 1) - 2 * 2 * 2)
