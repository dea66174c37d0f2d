"""Height-resolved evaluation on the GPU (include/sr3d.h: sr3d_eval_level_profiles; ops.eval_level_profiles;
src/level_profiles.py) against the fp64 restatement of tests/level_profiles_ref.py, the reference's own ``lev=k``
modules (tests/golden/level_profiles.npz) and the existing whole-volume pass.  Shapes are chosen against the kernel's
8 x 62 x 16 (y, x, z) tile: the ragged case has one full and one partial tile on every axis.

The bound is the project's fp32 parity bound, relative 1e-5 per entry: every numerator is a sum of non-negative terms,
so the relative error of a ratio is well-conditioned."""
import ctypes as C

import numpy as np
import pytest
import torch

import level_profiles_ref as LR
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
STDS = LR.STDS


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("level_profiles.npz")


@pytest.fixture(scope="module")
def ragged(gold):
    """{kind: (p, t, b, reference values, reference sums)}: computed once, shared, never modified"""
    out = {}
    for kind in ("iid", "tower"):
        p, t, b = LR.ragged_case(gold, kind)
        V, S = LR.level_profiles_ref(p.double(), t.double(), b.double(), STDS)
        out[kind] = (p, t, b, V, S)
    return out


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def assert_rows_close(got, ref, index, what, tol=TOL):
    """every row of `got` (device tensor (N, Z)) against {name: (Z,) fp64}: same NaN pattern, relative `tol` elsewhere;
    returns the number of entries compared numerically"""
    got = got.detach().cpu().double()
    n = 0
    for name, i in index.items():
        g, r = got[i], ref[name].double()
        assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, name, g, r)
        ok = ~torch.isnan(r)
        err = (g[ok] - r[ok]).abs()
        assert bool((err <= tol * r[ok].abs()).all()), (what, name, float((err / r[ok].abs().clamp_min(1e-300)).max()))
        n += int(ok.sum())
    return n


def run(eng, p, t, b, stds=STDS, **kw):
    return eng.ops.eval_level_profiles(p.to(DEV), t.to(DEV), b.to(DEV), stds, **kw)


@pytest.mark.parametrize("kind", ["iid", "tower"])
def test_ragged_case_vs_restatement_and_reference_modules(eng, gold, ragged, kind):
    L = eng._lib
    p, t, b, V, S = ragged[kind]
    values, sums = run(eng, p, t, b)
    Z = p.shape[2]
    assert tuple(values.shape) == (L.PROFILE_COUNT, Z) and tuple(sums.shape) == (L.PROFILE_SUM_COUNT, Z)
    assert set(L.PROFILE_INDEX) == set(LR.PROFILES) and set(L.PROFILE_SUM_INDEX) == set(LR.SUMS)
    n = assert_rows_close(values, V, L.PROFILE_INDEX, kind)
    assert n >= 12 * Z + 4 * (Z - 4)      # beyond levels 0 and Z-1, the iid mask may empty an interior level or two
    assert_rows_close(sums, S, L.PROFILE_SUM_INDEX, kind)
    # the interior profiles are NaN at the bottom and the top level by construction
    v = values.cpu()
    for name in LR.INTERIOR:
        row = v[L.PROFILE_INDEX[name]]
        assert torch.isnan(row[0]) and torch.isnan(row[-1]) and int(torch.isfinite(row).sum()) >= Z - 4, (name, row)
    # the reference's own modules with lev = k, for every k
    for name in ("AbsDiffTemperature", "DiffVelocityNorm"):
        ref = torch.from_numpy(gold[f"ragged/{kind}/{name}"]).double()
        got = v[L.PROFILE_INDEX[name]].double()
        assert ref.shape == got.shape == (Z,)
        assert bool(((got - ref).abs() <= TOL * ref.abs()).all()), (name, got, ref)


@pytest.mark.parametrize("kind", ["iid", "tower"])
def test_agrees_with_the_whole_volume_pass(eng, ragged, kind):
    L = eng._lib
    p, t, b, _, _ = ragged[kind]
    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    values, sums = eng.ops.eval_level_profiles(pd, td, bd, STDS)
    values, sums = values.cpu().double(), sums.cpu().double()
    B, _, Z, Y, X = p.shape
    per_lev = torch.stack([eng.ops.eval_metrics(pd, td, bd, STDS, 5.0, k) for k in range(Z)]).cpu().double()
    for prof, entry in (("AbsDiffTemperature", "AbsDiffTemperatureLev"), ("DiffVelocityNorm", "DiffVelocityNormLev")):
        got, ref = values[L.PROFILE_INDEX[prof]], per_lev[:, L.EVAL_INDEX[entry]]
        assert bool(((got - ref).abs() <= TOL * ref.abs()).all()), (prof, got, ref)
    # the raw sums over all levels, turned into ratios, are the whole-volume metrics
    whole = per_lev[0]
    total = {name: sums[i].sum() for name, i in L.PROFILE_SUM_INDEX.items()}
    pooled = LR.ratios(total, B * Z * Y * X)
    checked = 0
    for name, i in L.EVAL_INDEX.items():
        if name.endswith("Lev"):
            continue
        got, ref = float(pooled[name]), float(whole[i])
        assert np.isfinite(ref) and abs(got - ref) <= TOL * abs(ref), (name, got, ref)
        checked += 1
    assert checked == 12


def test_exact_inputs_pin_both_passes_to_each_other_bit_for_bit(eng):
    """on inputs where every fp32 operation of the non-interior terms is exact, the order of summation cannot matter:
    the whole-volume pass and the per-level pass, which share their stencil and term formulas
    (csrc/sr3d_eval_march.h) and differ in how they add up, must agree bit for bit, and with the fp64 restatement.
    Fields are multiples of 1/4 in [0, 2) that differ in T and u only (|d| < 2, sqrt(dv^2) = |dv|), scales are powers
    of two: every term is a multiple of 1/16 of at most 4; a block adds at most 8 * 62 * 16 * 4 = 31744 of them and
    the whole case 2 * 18 * 11 * 70 * 4 = 110880, so every partial sum is an integer below 2^24 in units of 1/16."""
    L = eng._lib
    B, Z, Y, X = 2, 18, 11, 70           # two tiles on every axis, the second one partial
    stds, delta = (2.0, 1.0, 4.0, 0.5), 4.0
    g = torch.Generator().manual_seed(61)
    t = torch.randint(0, 8, (B, 4, Z, Y, X), generator=g).float() / 4
    p = t.clone()
    p[:, :2] = torch.randint(0, 8, (B, 2, Z, Y, X), generator=g).float() / 4
    b = (torch.rand(B, 1, Z, Y, X, generator=g) > 0.02).float()     # sparse: about half the open cells are not near a wall
    b[:, :, :7, 3:8, 20:40] = 0          # a built block: near-wall cells on its faces and roof
    interior = ("res_p", "res_t", "ddiv", "omega")      # divergence / vorticity terms are not exactly representable
    _, S = LR.level_profiles_ref(p.double(), t.double(), b.double(), stds, delta)
    for name in LR.SUMS:
        if name not in interior:
            units = torch.cat([S[name], S[name].sum()[None]]) * 16
            assert torch.equal(units, units.round()) and float(units.max()) < 2 ** 24, name
    assert 0.25 * float(S["mask_int"].sum()) < float(S["near_int"].sum()) < 0.75 * float(S["mask_int"].sum())

    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    values, sums = eng.ops.eval_level_profiles(pd, td, bd, stds, delta=delta)
    per_lev = torch.stack([eng.ops.eval_metrics(pd, td, bd, stds, delta, k) for k in range(Z)]).cpu()
    values, sums = values.cpu(), sums.cpu()
    for name, i in L.PROFILE_SUM_INDEX.items():
        if name in interior:
            assert_rows_close(sums, S, {name: i}, "exact")
        else:
            assert torch.equal(sums[i].double(), S[name]), name
    for name, i in L.EVAL_SUMS.items():
        total = sums[L.PROFILE_SUM_INDEX[name]].double().sum().float()
        for k in range(Z):
            assert torch.equal(bits(total), bits(per_lev[k, i])), (name, k)
    for prof, entry in (("AbsDiffTemperature", "AbsDiffTemperatureLev"), ("DiffVelocityNorm", "DiffVelocityNormLev")):
        got, ref = values[L.PROFILE_INDEX[prof]], per_lev[:, L.EVAL_INDEX[entry]]
        assert bool((got > 0).all()) and torch.equal(bits(got), bits(ref)), prof


def test_podium_case(eng):
    """two built levels under open air: which levels are empty, exactly zero or NaN is known in advance"""
    L = eng._lib
    B, Z, Y, X = 2, 6, 9, 70
    g = torch.Generator().manual_seed(31)
    p, t = torch.rand(B, 4, Z, Y, X, generator=g), torch.rand(B, 4, Z, Y, X, generator=g)
    b = torch.ones(B, 1, Z, Y, X)
    b[:, :, :2] = 0
    values, sums = run(eng, p, t, b)
    v = values.cpu()
    for name in ("MaskedL1", "MaskedL2", "AbsDiffTemperature", "DiffVelocityNorm"):
        row = v[L.PROFILE_INDEX[name]]
        assert float(row[0]) == 0.0 and float(row[1]) == 0.0 and bool((row[2:] > 0).all()), (name, row)
    for name in ("MaskedL1NearWall", "MaskedL2NearWall"):
        row = v[L.PROFILE_INDEX[name]]
        assert [k for k in range(Z) if float(row[k]) != 0.0] == [2], (name, row)
    for name in LR.INTERIOR:
        row = v[L.PROFILE_INDEX[name]]
        assert [k for k in range(Z) if bool(torch.isnan(row[k]))] == [0, 1, 2, 5], (name, row)
        assert bool(torch.isfinite(row[3:5]).all())
    V, S = LR.level_profiles_ref(p.double(), t.double(), b.double(), STDS)
    compared = assert_rows_close(values, V, L.PROFILE_INDEX, "podium")
    assert compared == 12 * Z + 4 * (Z - 4)     # every level of the other rows, levels 3 and 4 of the interior rows
    assert_rows_close(sums, S, L.PROFILE_SUM_INDEX, "podium")


@pytest.mark.parametrize("shape", [(2, 9, 20), (3, 9, 20), (5, 2, 70), (5, 9, 2)])
def test_degenerate_grids(eng, shape):
    L = eng._lib
    Z, Y, X = shape
    B = 2
    g = torch.Generator().manual_seed(41 + Z + Y)
    p, t = torch.rand(B, 4, Z, Y, X, generator=g), torch.rand(B, 4, Z, Y, X, generator=g)
    b = torch.ones(B, 1, Z, Y, X)
    b[:, :, 0, 0, 0] = 0        # one built corner cell: near-wall cells exist, most of the interior stays open
    values, sums = run(eng, p, t, b)
    V, S = LR.level_profiles_ref(p.double(), t.double(), b.double(), STDS)
    assert_rows_close(values, V, L.PROFILE_INDEX, shape)
    assert_rows_close(sums, S, L.PROFILE_SUM_INDEX, shape)
    v = values.cpu()
    for name in LR.INTERIOR:
        row = v[L.PROFILE_INDEX[name]]
        if shape == (3, 9, 20):
            assert bool(torch.isnan(row[0])) and bool(torch.isfinite(row[1])) and bool(torch.isnan(row[2])), (name, row)
        else:
            assert bool(torch.isnan(row).all()), (name, row)
    others = [i for n, i in L.PROFILE_INDEX.items() if n not in LR.INTERIOR]
    assert bool(torch.isfinite(v[others]).all())


def test_per_sample_equals_one_sample_calls_bit_for_bit(eng, ragged):
    L = eng._lib
    p, t, b, _, _ = ragged["iid"]
    B = p.shape[0]
    values, sums = run(eng, p, t, b, per_sample=True)
    assert tuple(values.shape) == (B, L.PROFILE_COUNT, p.shape[2]) and tuple(sums.shape) == (B, L.PROFILE_SUM_COUNT, p.shape[2])
    for i in range(B):
        v1, s1 = run(eng, p[i:i + 1], t[i:i + 1], b[i:i + 1])
        assert torch.equal(bits(values[i]), bits(v1)), i
        assert torch.equal(bits(sums[i]), bits(s1)), i
    _, batch = run(eng, p, t, b)
    got, ref = sums.cpu().double().sum(dim=0), batch.cpu().double()
    assert bool(((got - ref).abs() <= TOL * ref.abs()).all())
    assert not torch.equal(bits(sums[0]), bits(sums[1]))


def test_two_calls_are_bit_equal(eng, ragged):
    p, t, b, _, _ = ragged["tower"]
    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    first = eng.ops.eval_level_profiles(pd, td, bd, STDS)
    second = eng.ops.eval_level_profiles(pd, td, bd, STDS)
    for a, c in zip(first, second):
        assert a.data_ptr() != c.data_ptr() and torch.equal(bits(a), bits(c))
    # None scales count as 1.0
    ones = eng.ops.eval_level_profiles(pd, td, bd, (1.0, 1.0, 1.0, 1.0))
    none = eng.ops.eval_level_profiles(pd, td, bd, (None,) * 4)
    assert torch.equal(bits(ones[0]), bits(none[0])) and not torch.equal(bits(ones[0]), bits(first[0]))


def test_meter_equals_evaluate_with_lev_modules(eng):
    """over a three-batch loader (batch sizes 2, 1, 2) the meter's AbsDiffTemperature at level k is what
    optim_helper.evaluate reports for AbsDiffTemperature(lev=k); the pooled variant is the ratio of the summed sums"""
    from sr3d_amd.src import loss_maker as lm
    from sr3d_amd.src.level_profiles import LEVEL_PROFILE_NAMES, evaluate_level_profiles
    from sr3d_amd.src.optim_helper import evaluate
    L = eng._lib
    Z, Y, X = 6, 10, 70
    g = torch.Generator().manual_seed(51)
    loader = []
    for n in (2, 1, 2):
        y = torch.rand(n, 4, Z, Y, X, generator=g)
        pred = y + 0.3 * (torch.rand(n, 4, Z, Y, X, generator=g) - 0.5)
        b = (torch.rand(n, Z, Y, X, generator=g) > 0.2).float()
        loader.append((pred, b, y))     # the "model" below returns its input: the prediction rides in the LR slot

    class Identity(torch.nn.Module):
        def forward(self, X, bb):
            return X

    df = evaluate_level_profiles(dataloader=loader, model=Identity(), stds=STDS, device=DEV)
    assert list(df.columns) == ["level", "height_m", *LEVEL_PROFILE_NAMES, "FluidCells", "NearWallCells", "InteriorCells"]
    assert len(df) == Z and list(df["height_m"]) == [17.5 + 5.0 * k for k in range(Z)]
    fns = {f"T{k}": lm.AbsDiffTemperature(STDS[0], lev=k) for k in range(Z)}
    fns.update({f"V{k}": lm.DiffVelocityVectorNorm(STDS[1:], lev=k) for k in range(Z)})
    res = evaluate(dataloader=loader, model=Identity(), loss_fns=fns, device=DEV)
    for k in range(Z):
        for col, key in (("AbsDiffTemperature", f"T{k}"), ("DiffVelocityNorm", f"V{k}")):
            got, ref = float(df[col][k]), float(res[key].avg)
            assert ref > 0 and abs(got - ref) <= TOL * abs(ref), (col, k, got, ref)
    # pooled: the restatement's sums added over the batches, then the ratios
    tot, cells = None, 0
    for pred, b, y in loader:
        S = LR.level_sums(pred.double(), y.double(), b.unsqueeze(1).double(), STDS)
        tot = S if tot is None else {k: tot[k] + S[k] for k in S}
        cells += len(pred) * Y * X
    ref = LR.ratios(tot, cells)
    dfp = evaluate_level_profiles(dataloader=loader, model=Identity(), stds=STDS, device=DEV, pooled=True)
    for name in LEVEL_PROFILE_NAMES:
        got, r = torch.tensor(dfp[name].to_numpy()), ref[name]
        assert torch.equal(torch.isnan(got), torch.isnan(r)), name
        ok = ~torch.isnan(r)
        assert bool(((got[ok] - r[ok]).abs() <= TOL * r[ok].abs()).all()), name
    assert np.allclose(dfp["FluidCells"].to_numpy(), tot["mask"].numpy(), rtol=0, atol=0)


def test_argument_errors(eng):
    L = eng._lib
    ops = eng.ops
    p = torch.rand(1, 4, 4, 6, 8, device=DEV)
    b = torch.ones(1, 1, 4, 6, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.eval_level_profiles(p, p, b[:, 0], STDS)
    with pytest.raises(ValueError):
        ops.eval_level_profiles(p, p, torch.ones(1, 1, 4, 6, 9, device=DEV), STDS)
    with pytest.raises(ValueError):
        ops.eval_level_profiles(p[:, :3], p[:, :3], b, STDS)
    for delta in (0.0, -5.0):
        with pytest.raises(RuntimeError, match="delta_meter"):
            ops.eval_level_profiles(p, p, b, STDS, delta=delta)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_level_profiles(p.cpu(), p.cpu(), b.cpu(), STDS)
    # a grid of 2^31 voxels is refused before anything is launched (the pointers are never dereferenced), as by
    # sr3d_eval_metrics
    sc = (C.c_float * 4)(*STDS)
    out = torch.empty(64, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
    rc = L.lib.sr3d_eval_level_profiles(ptr(p), ptr(p), ptr(b), 1, 2048, 1024, 1024, sc, 5.0, 0, ptr(out), ptr(out),
                                        ptr(out), None)
    assert rc == -1 and b"2^31" in L.lib.sr3d_last_error()
    rc = L.lib.sr3d_eval_metrics(ptr(p), ptr(p), ptr(b), 1, 2048, 1024, 1024, sc, 5.0, 0, ptr(out), ptr(out), None)
    assert rc == -1 and b"2^31" in L.lib.sr3d_last_error()
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.check(L.lib.sr3d_eval_level_profiles(ptr(p), ptr(p), ptr(b), 1, 2048, 1024, 1024, sc, 5.0, 0, ptr(out),
                                               ptr(out), ptr(out), None), "sr3d_eval_level_profiles")
    # and the call still works afterwards
    values, _ = ops.eval_level_profiles(p, p, b, STDS)
    assert float(values[L.PROFILE_INDEX["L1"]].abs().max()) == 0.0
