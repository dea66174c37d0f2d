"""Wall-distance-resolved evaluation on the GPU (include/sr3d.h: sr3d_wall_distance, sr3d_eval_wall_distance_profiles;
ops.wall_distance, ops.near_wall_mask(b, n), ops.eval_wall_distance_profiles; the near-wall modules at any width)
against the fp64 restatement of tests/wall_distance_ref.py, the reference's own near-wall masks and modules at widths
1 .. 12 (tests/golden/wall_distance.npz) and the existing whole-volume and per-level passes.  The cases live on B = 2,
(Z, Y, X) = (19, 23, 67): against the profile kernel's 8 x 62 x 16 (y, x, z) tile that is one full and one partial
tile or more on every axis, against the distance kernel's 64-cell row chunks one full and one partial chunk, and
distances cross the edges of both.

Masks and distances are compared bit for bit.  The bound on values is the project's fp32 parity bound, relative 1e-5
per entry: every numerator is a sum of non-negative terms, so the relative error of a ratio is well-conditioned."""
import numpy as np
import pytest
import torch

import wall_distance_ref as WR
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
STDS = WR.STDS
D = 8
PROFILE_CASES = ("tower", "sparse", "fractional", "mixed")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("wall_distance.npz")


@pytest.fixture(scope="module")
def cases(gold):
    """{kind: (p, t, b)} on the CPU: made once, shared, never modified"""
    return {kind: WR.case(gold, kind) for kind in WR.CASES}


@pytest.fixture(scope="module")
def refs(cases):
    """{kind: (reference values, reference sums)} at D = 8 in fp64, for the cases the profiles are checked on + iid"""
    out = {}
    for kind in PROFILE_CASES + ("iid",):
        p, t, b = cases[kind]
        out[kind] = WR.wall_distance_profiles_ref(p.double(), t.double(), b.double(), STDS, D=D)
    return out


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def assert_rows_close(got, ref, index, what, tol=TOL):
    """every row of `got` (device tensor (N, bins)) against {name: (bins,) fp64}: same NaN pattern, relative `tol`
    elsewhere; returns (entries compared numerically, NaN entries)"""
    got = got.detach().cpu().double()
    n = nan = 0
    for name, i in index.items():
        g, r = got[i], ref[name].double()
        assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, name, g, r)
        ok = ~torch.isnan(r)
        err = (g[ok] - r[ok]).abs()
        print(what, name, "worst relative difference", float((err / r[ok].abs().clamp_min(1e-300)).max()) if err.numel() else 0.0)
        assert bool((err <= tol * r[ok].abs()).all()), (what, name, float((err / r[ok].abs().clamp_min(1e-300)).max()))
        n += int(ok.sum())
        nan += int((~ok).sum())
    return n, nan


def run(eng, p, t, b, **kw):
    return eng.ops.eval_wall_distance_profiles(p.to(DEV), t.to(DEV), b.to(DEV), STDS, **kw)


@pytest.mark.parametrize("kind", WR.CASES)
def test_distance_equals_the_restatement(eng, cases, kind):
    b = cases[kind][2]
    bd = b.to(DEV)
    for cap in (1, 3, 12):
        got = eng.ops.wall_distance(bd, cap)
        assert got.dtype == torch.uint8 and got.shape == b.shape
        assert torch.equal(got.cpu(), WR.wall_distance_ref(b, cap)), (kind, cap)
    if kind == "all_fluid":
        assert bool((eng.ops.wall_distance(bd, 254) == 255).all())


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 9, 20), (5, 2, 70), (5, 9, 2), (3, 9, 125)])
def test_distance_on_degenerate_grids(eng, shape):
    Z, Y, X = shape
    g = torch.Generator().manual_seed(43 + Z + Y + X)
    b = (torch.rand(2, 1, Z, Y, X, generator=g) > 0.03).float()
    b[0, 0, 0, 0, 0] = 0            # sample 0 always holds a built corner cell
    b[1] = 1.0 if X < 64 else b[1]  # ... and on the small grids sample 1 holds none
    for cap in (1, 4, 254):
        assert torch.equal(eng.ops.wall_distance(b.to(DEV), cap).cpu(), WR.wall_distance_ref(b, cap)), (shape, cap)


@pytest.mark.parametrize("kind", WR.GOLDEN_CASES)
def test_near_wall_masks_equal_the_reference_bit_for_bit(eng, gold, cases, kind):
    from sr3d_amd.src.loss_maker import calc_mask_near_build_wall
    b = cases[kind][2]
    bd = b.to(DEV)
    for n in WR.GOLDEN_WIDTHS:
        ref = WR.unpack(gold[f"near/{kind}/{n}"])
        for got in (eng.ops.near_wall_mask(bd, n), calc_mask_near_build_wall(bd, n)):
            assert got.dtype == torch.float32 and torch.equal(got.cpu(), ref), (kind, n)
    # width 1 is today's call, and the distance route agrees with it
    one = eng.ops.near_wall_mask(bd)
    assert torch.equal(one, eng.ops.near_wall_mask(bd, 1))
    assert torch.equal(one, ((eng.ops.wall_distance(bd, 1) <= 1) & (bd > 0)).float())
    # wider than any distance in the grid: every cell with b > 0, as soon as something is built
    assert torch.equal(eng.ops.near_wall_mask(bd, 300).cpu(), (b > 0).float())


@pytest.mark.parametrize("kind", WR.GOLDEN_CASES)
def test_near_wall_modules_at_every_stored_width(eng, gold, cases, kind):
    from sr3d_amd.src import loss_maker as lm
    p, t, b = (x.to(DEV) for x in cases[kind])
    for n in WR.GOLDEN_WIDTHS:
        ref = gold[f"module/{kind}/{n}"].astype(np.float64)
        got = (float(lm.MaskedL1LossNearWall(num_filter_applications=n)(p, t, b)),
               float(lm.MaskedL2LossNearWall(num_filter_applications=n)(p, t, b)))
        print(kind, n, got, ref)
        for g, r in zip(got, ref):
            assert r > 0 and abs(g - r) <= TOL * r, (kind, n, g, r)


@pytest.mark.parametrize("kind", PROFILE_CASES)
def test_profiles_vs_restatement(eng, cases, refs, kind):
    L = eng._lib
    p, t, b = cases[kind]
    V, S = refs[kind]
    values, sums = run(eng, p, t, b, max_distance=D)
    assert tuple(values.shape) == (L.WALLDIST_COUNT, D + 2) and tuple(sums.shape) == (L.WALLDIST_SUM_COUNT, D + 2)
    n, nan = assert_rows_close(values, V, L.WALLDIST_INDEX, kind)
    assert n + nan == 16 * (D + 2)
    if kind in ("tower", "sparse"):
        # exactly the interior rows at bins 0 and 1 (M = b (1 - near_1) is zero there) are NaN
        assert (n, nan) == (152, 8)
        v = values.cpu()
        for name in WR.INTERIOR:
            row = v[L.WALLDIST_INDEX[name]]
            assert [k for k in range(D + 2) if bool(torch.isnan(row[k]))] == [0, 1], (name, row)
    assert_rows_close(sums, S, L.WALLDIST_SUM_INDEX, kind)
    if kind != "fractional":
        # the counts are whole numbers below 2^24.  |d| is a multiple of 1 / 4096 below 1 and a row of a block adds at
        # most 62 * 16 * 4 of them: below 2^24 / 4096, exact in fp32 in any order; rows, blocks and samples are added
        # in double, so the total is exact and its one rounding to fp32 is the restatement's
        s = sums.cpu()
        for name in WR.COUNTS:
            assert torch.equal(s[L.WALLDIST_SUM_INDEX[name]].double(), S[name]), (kind, name)
        assert torch.equal(s[L.WALLDIST_SUM_INDEX["abs"]], S["abs"].float()), kind


@pytest.mark.parametrize("kind", ["tower", "fractional"])
def test_sums_over_bins_equal_the_per_level_sums_over_levels(eng, cases, kind):
    L = eng._lib
    p, t, b = (x.to(DEV) for x in cases[kind])
    _, by_bin = eng.ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D)
    _, by_level = eng.ops.eval_level_profiles(p, t, b, STDS)
    by_bin, by_level = by_bin.cpu().double().sum(dim=1), by_level.cpu().double().sum(dim=1)
    checked = 0
    for name, i in L.PROFILE_SUM_INDEX.items():
        if name.startswith("near") and name != "near_int":
            continue            # POS here, NEAR there
        got, ref = float(by_bin[L.WALLDIST_SUM_INDEX[name]]), float(by_level[i])
        assert ref > 0 and abs(got - ref) <= TOL * ref, (name, got, ref)
        checked += 1
    assert checked == 17
    assert float(by_bin[L.WALLDIST_SUM_INDEX["cells"]]) == float(b.numel())


@pytest.mark.parametrize("kind", WR.GOLDEN_CASES)
def test_cumulative_near_wall_rows_are_the_reference_modules(eng, gold, cases, kind):
    L = eng._lib
    p, t, b = (x.to(DEV) for x in cases[kind])
    values, _ = eng.ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D)
    v = values.cpu().double()
    for n in (1, 2, 3, 5, 8):
        ref = gold[f"module/{kind}/{n}"].astype(np.float64)
        for row, r in zip(("MaskedL1NearWall", "MaskedL2NearWall"), ref):
            g = float(v[L.WALLDIST_INDEX[row], n])
            assert abs(g - r) <= TOL * r, (kind, row, n, g, r)
    whole = eng.ops.eval_metrics(p, t, b, STDS).cpu().double()
    for row in ("MaskedL1NearWall", "MaskedL2NearWall"):
        g, r = float(v[L.WALLDIST_INDEX[row], 1]), float(whole[L.EVAL_INDEX[row]])
        assert r > 0 and abs(g - r) <= TOL * r, (kind, row, g, r)


def test_empty_bins(eng, cases, refs):
    """the iid mask leaves nothing farther than 2 cells from a building: bins 3 .. 9 are empty"""
    L = eng._lib
    p, t, b = cases["iid"]
    V, S = refs["iid"]
    values, sums = run(eng, p, t, b, max_distance=D)
    v, s = values.cpu(), sums.cpu()
    assert bool((s[L.WALLDIST_SUM_INDEX["cells"], :3] > 0).all()) and bool((s[:, 3:] == 0).all())
    for name in ("L1", "L2", "ChannelwiseMseT", "ChannelwiseMseW", *WR.INTERIOR):
        assert bool(torch.isnan(v[L.WALLDIST_INDEX[name], 3:]).all()), name
    for name in ("MaskedL1", "MaskedL2", "AbsDiffTemperature", "DiffVelocityNorm"):
        assert bool((v[L.WALLDIST_INDEX[name], 3:] == 0).all()), name
    assert_rows_close(values, V, L.WALLDIST_INDEX, "iid")
    assert_rows_close(sums, S, L.WALLDIST_SUM_INDEX, "iid")


def test_two_calls_are_bit_equal_and_a_wider_cap_changes_nothing(eng, cases):
    p, t, b = (x.to(DEV) for x in cases["tower"])
    ops = eng.ops
    first = ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D)
    second = ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D)
    d8, d12 = ops.wall_distance(b, 8), ops.wall_distance(b, 12)
    assert not torch.equal(d8, d12) and torch.equal(d8, d12.clamp(max=9))
    given = ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D, dist=d8)
    wider = ops.eval_wall_distance_profiles(p, t, b, STDS, max_distance=D, dist=d12)
    for other in (second, given, wider):
        for a, c in zip(first, other):
            assert a.data_ptr() != c.data_ptr() and torch.equal(bits(a), bits(c))
    from sr3d_amd.src.wall_distance_profiles import calc_wall_distance_profiles
    named = calc_wall_distance_profiles(p, t, b, STDS, max_distance=D, dist=d12)
    assert torch.equal(bits(named["DiffOmegaNorm"]), bits(first[0][eng._lib.WALLDIST_INDEX["DiffOmegaNorm"]]))


def test_argument_errors(eng):
    ops = eng.ops
    p = torch.rand(1, 4, 4, 6, 8, device=DEV)
    b = torch.ones(1, 1, 4, 6, 8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_wall_distance_profiles(p, p, b, STDS, dist=torch.zeros_like(b))
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_wall_distance_profiles(p, p, b, STDS, dist=torch.zeros(1, 1, 4, 6, 9, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.eval_wall_distance_profiles(p, p, b[:, 0], STDS)
    for cap in (0, 255):
        with pytest.raises(RuntimeError, match="cap"):
            ops.wall_distance(b, cap)
    with pytest.raises(RuntimeError, match="delta_meter"):
        ops.eval_wall_distance_profiles(p, p, b, STDS, delta_meter=0.0)
    # and the calls still work afterwards: nothing built, p == t
    values, sums = ops.eval_wall_distance_profiles(p, p, b, STDS, max_distance=2)
    L = eng._lib
    assert float(sums[L.WALLDIST_SUM_INDEX["cells"], 3]) == b.numel() and float(values[L.WALLDIST_INDEX["L1"], 3]) == 0.0
