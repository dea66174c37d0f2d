"""Error-distribution evaluation on the GPU (include/sr3d.h: sr3d_eval_distributions; ops.eval_distributions) against
the numpy restatement of tests/error_distributions_ref.py: counts, cell counts and min / max must be EQUAL, on every mask
kind, near-wall width, range set, with the distance given or not, per sample or not.  The cases live on B = 2,
(Z, Y, X) = (19, 23, 67): an odd voxel count, so the channel planes are misaligned (the dword path of the kernel), 8
workgroups per sample with a ragged last one; the fields are multiples of 1 / 4096, so many values sit exactly on bin
edges.  A second shape, (20, 24, 68), has 16-byte aligned planes and takes the kernel's 16-byte-load path."""
import numpy as np
import pytest
import torch

import error_distributions_ref as ER
import wall_distance_ref as WR
from helpers import load_golden, tower_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STDS = WR.STDS
MASKS = ("tower", "sparse", "fractional", "mixed", "all_fluid")
WIDTHS = (0, 1, 3)
# the default ranges (256 / (hi - lo) a power of two; p - t of two U[0, 1) fields leaves them on both sides), and ranges
# whose inverse width is no power of two, per channel, most of them narrow: under- and overflow are populated in every
# series but ERR_W, whose range holds everything
RANGES = {"default": {},
          "narrow": dict(err_range=[(-0.3, 0.7), (-0.25, 0.125), (-0.01, 0.013), (-2.0, 3.0)],
                         field_range=[(0.1, 0.9), (0.25, 0.75), (0.3, 0.30001), (0.2, 0.5)], vel_norm_range=(0.5, 3.0))}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def cases():
    """{kind: (p, t, b)} on the CPU: made once, shared, never modified"""
    gold = load_golden("wall_distance.npz")
    return {kind: WR.case(gold, kind) for kind in MASKS}


def assert_same(got, ref, what):
    """(counts, minmax, cells) from the device against the restatement's: equal, min / max included"""
    counts, minmax, cells = (x.cpu() for x in got)
    assert counts.dtype == torch.int64 and minmax.dtype == torch.float32 and cells.dtype == torch.int64, what
    assert torch.equal(cells, ref[2]), (what, cells, ref[2])
    assert torch.equal(counts, ref[0]), (what, (counts != ref[0]).nonzero()[:8])
    assert torch.equal(minmax, ref[1]), (what, minmax, ref[1])


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", MASKS)
def test_equals_the_restatement(eng, cases, kind):
    p, t, b = cases[kind]
    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    populated = 0
    for nw in WIDTHS:
        dist = eng.ops.wall_distance(bd, max(nw, 1) + 2)        # a wider cap changes nothing
        for rname, rng in RANGES.items():
            whole = ER.distributions_ref(p, t, b, STDS, near_width=nw, **rng)
            per = ER.distributions_ref(p, t, b, STDS, near_width=nw, per_sample=True, **rng)
            for given in (False, True):
                kw = dict(near_width=nw, dist=dist if given else None, **rng)
                assert_same(eng.ops.eval_distributions(pd, td, bd, STDS, **kw), whole, (kind, nw, rname, given))
                got = eng.ops.eval_distributions(pd, td, bd, STDS, per_sample=True, **kw)
                assert tuple(got[0].shape) == (2, 13, 2, 259) and tuple(got[1].shape) == (2, 13, 2, 2)
                assert tuple(got[2].shape) == (2, 3)
                assert_same(got, per, (kind, nw, rname, given, "per sample"))
            c = whole[0]
            if rname == "narrow":
                out = c[:, :, [ER.UNDER, ER.OVER]].sum(dim=1)
                assert bool((out[[i for i, n in enumerate(ER.SERIES) if n != "ERR_W"]] > 0).all()), out
            else:
                assert int(c[:4, :, [ER.UNDER, ER.OVER]].sum(dim=1).min()) > 0 and int(c[5:, :, [ER.UNDER, ER.OVER]].sum()) == 0
            populated += int((c[:, :, 1:257] > 0).sum())
        cells = whole[2]
        assert int(cells.sum()) == b.numel() and int(cells[0]) == int((~(b > 0)).sum())
        assert (int(cells[1]) > 0) == (nw > 0 and kind != "all_fluid")
    assert populated > 1000


def test_per_sample_equals_one_sample_calls_and_two_calls_are_bit_equal(eng, cases):
    p, t, b = (x.to(DEV) for x in cases["mixed"])
    ops = eng.ops
    first = ops.eval_distributions(p, t, b, STDS, near_width=3, per_sample=True)
    second = ops.eval_distributions(p, t, b, STDS, near_width=3, per_sample=True)
    for a, c in zip(first, second):
        assert a.data_ptr() != c.data_ptr() and torch.equal(a, c)
    assert torch.equal(bits(first[1]), bits(second[1]))
    for i in range(2):
        one = ops.eval_distributions(p[i:i + 1], t[i:i + 1], b[i:i + 1], STDS, near_width=3)
        assert torch.equal(one[0], first[0][i]) and torch.equal(one[2], first[2][i])
        assert torch.equal(bits(one[1]), bits(first[1][i]))
    whole = ops.eval_distributions(p, t, b, STDS, near_width=3)
    assert torch.equal(whole[0], first[0].sum(dim=0)) and torch.equal(whole[2], first[2].sum(dim=0))
    assert torch.equal(whole[1][..., 0], first[1][..., 0].min(dim=0).values)
    assert torch.equal(whole[1][..., 1], first[1][..., 1].max(dim=0).values)


def test_identical_fields_put_every_cell_into_one_bin(eng, cases):
    """p == t: every lane of every wave adds to the same counter -- the worst case for the LDS adds, exact by construction"""
    L = eng._lib
    _, t, b = cases["tower"]
    td, bd = t.to(DEV), b.to(DEV)
    counts, minmax, cells = (x.cpu() for x in eng.ops.eval_distributions(td, td.clone(), bd, STDS, near_width=1))
    assert int(cells[1]) > 0 and int(cells[2]) > 0 and int(cells.sum()) == b.numel()
    zero_slot = 1 + 128                     # floor((0 - (-0.5)) * 256) = 128
    for name in ("ERR_T", "ERR_U", "ERR_V", "ERR_W", "ERR_VEL_NORM"):
        s = L.DIST_SERIES_INDEX[name]
        slot = 1 if name == "ERR_VEL_NORM" else zero_slot
        want = torch.zeros(2, L.DIST_SLOTS, dtype=torch.int64)
        want[:, slot] = cells[1:]
        assert torch.equal(counts[s], want), name
        assert bool((minmax[s] == 0).all()), name
    for c in "TUVW":
        assert torch.equal(counts[L.DIST_SERIES_INDEX["PRED_" + c]], counts[L.DIST_SERIES_INDEX["TRUTH_" + c]])
    assert_same((counts, minmax, cells), ER.distributions_ref(t, t, b, STDS, near_width=1), "p == t")


def test_nan_and_infinities_are_counted_in_fluid_cells_only(eng, cases):
    L = eng._lib
    p, t, b = (x.clone() for x in cases["tower"])
    fluid = (b[0, 0] > 0).nonzero()
    built = (b[0, 0] == 0).nonzero()
    assert len(built) > 10
    nan, inf = float("nan"), float("inf")
    f = [tuple(int(v) for v in fluid[i]) for i in (0, 77, 5000, 9999, 20000, 25000)]
    w = [tuple(int(v) for v in built[i]) for i in (0, 5, 9)]
    p[0, 0][f[0]], p[0, 0][f[1]], t[0, 0][f[2]] = nan, nan, nan       # T: 2 NaN predictions, 1 NaN truth
    p[0, 1][f[3]], t[0, 2][f[4]], p[1, 3][f[5]] = inf, inf, -inf      # u: +inf prediction; v: +inf truth; w: -inf prediction
    p[0, 0][w[0]], t[0, 1][w[1]], p[0, 2][w[2]] = nan, inf, -inf      # in built cells: never seen
    ref = ER.distributions_ref(p, t, b, STDS, near_width=1)
    got = eng.ops.eval_distributions(p.to(DEV), t.to(DEV), b.to(DEV), STDS, near_width=1)
    assert_same(got, ref, "planted")
    counts, minmax = got[0].cpu().sum(dim=1), got[1].cpu()
    I = L.DIST_SERIES_INDEX
    assert int(counts[I["PRED_T"], ER.NAN]) == 2 and int(counts[I["TRUTH_T"], ER.NAN]) == 1
    assert int(counts[I["ERR_T"], ER.NAN]) == 3 and int(counts[:, ER.NAN].sum()) == 6
    assert int(counts[I["PRED_U"], ER.OVER]) >= 1 and int(counts[I["ERR_U"], ER.NAN]) == 0
    assert float(minmax[I["PRED_U"]].max()) == inf and float(minmax[I["ERR_U"]].max()) == inf
    assert float(minmax[I["TRUTH_V"]].max()) == inf and float(minmax[I["ERR_V"]].min()) == -inf
    assert float(minmax[I["PRED_W"]].min()) == -inf and float(minmax[I["ERR_VEL_NORM"]].max()) == inf
    assert int(counts[I["ERR_VEL_NORM"], ER.NAN]) == 0 and not bool(torch.isnan(minmax).any())
    assert 0.0 <= float(minmax[I["PRED_T"]].min()) and float(minmax[I["PRED_T"]].max()) < 1.0     # NaN ignored


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 2), (2, 3, 5)])
def test_degenerate_grids_and_a_mask_with_nothing_fluid(eng, shape):
    Z, Y, X = shape
    g = torch.Generator().manual_seed(7 + Z * Y * X)
    p, t = torch.rand(2, 4, Z, Y, X, generator=g), torch.rand(2, 4, Z, Y, X, generator=g)
    b = torch.ones(2, 1, Z, Y, X)
    b[0, 0, 0, 0, 0] = 0
    for mask in (b, torch.zeros_like(b)):
        for nw in (0, 1):
            for per in (False, True):
                ref = ER.distributions_ref(p, t, mask, STDS, near_width=nw, per_sample=per)
                got = eng.ops.eval_distributions(p.to(DEV), t.to(DEV), mask.to(DEV), STDS, near_width=nw, per_sample=per)
                assert_same(got, ref, (shape, nw, per))
    counts, minmax, cells = (x.cpu() for x in got)       # nothing fluid
    assert int(counts.sum()) == 0 and cells.tolist() == [[Z * Y * X, 0, 0]] * 2
    assert bool((minmax[..., 0] == float("inf")).all()) and bool((minmax[..., 1] == float("-inf")).all())


def test_views_and_odd_storage_offsets(eng, cases):
    p, t, b = (x.to(DEV) for x in cases["sparse"])
    ref = eng.ops.eval_distributions(p, t, b, STDS, near_width=1)
    # a non-contiguous view (channels last in memory) and tensors that start one float into their storage
    pv = p.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    assert not pv.is_contiguous() and torch.equal(pv, p)

    def shifted(x, k):
        buf = torch.empty(x.numel() + k, dtype=x.dtype, device=x.device)
        buf[k:] = x.flatten()
        v = buf[k:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == (x.data_ptr() + 4 * k) % 16
        return v

    for q in ((pv, t, b), (shifted(p, 1), shifted(t, 3), shifted(b, 1)), (p, shifted(t, 2), b)):
        got = eng.ops.eval_distributions(*q, STDS, near_width=1)
        for a, c in zip(got, ref):
            assert torch.equal(a, c)
        assert torch.equal(bits(got[1]), bits(ref[1]))


def test_aligned_planes_take_the_16_byte_loads_and_agree(eng):
    """Z * Y * X % 4 == 0 and fresh allocations: the 16-byte-load path (8 workgroups a sample);
    the same data one float into its storage goes down the dword path: both equal the restatement"""
    B, Z, Y, X = 2, 20, 24, 68
    g = torch.Generator().manual_seed(31)
    t = torch.randint(0, 4096, (B, 4, Z, Y, X), generator=g).float() / 4096
    p = t + torch.randint(-300, 301, (B, 4, Z, Y, X), generator=g).float() / 4096
    b = tower_mask(Z, Y, X).repeat(B, 1, 1, 1, 1)
    b[1] = (torch.rand(1, Z, Y, X, generator=g) > 0.01).float()
    b[1, 0, 3, 4, 5] = 0.5
    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    assert all(x.data_ptr() % 16 == 0 for x in (pd, td, bd)) and (Z * Y * X) % 4 == 0
    buf = torch.empty(p.numel() + 1, device=DEV)
    buf[1:] = pd.flatten()
    p_odd = buf[1:].view(p.shape)
    assert p_odd.data_ptr() % 16 == 4
    for nw in (0, 2):
        for per in (False, True):
            ref = ER.distributions_ref(p, t, b, STDS, near_width=nw, per_sample=per)
            assert_same(eng.ops.eval_distributions(pd, td, bd, STDS, near_width=nw, per_sample=per), ref, ("vec", nw, per))
            assert_same(eng.ops.eval_distributions(p_odd, td, bd, STDS, near_width=nw, per_sample=per), ref, ("dword", nw, per))
    assert int(ref[0][..., [ER.UNDER, ER.OVER]].sum()) == 0 and int(ref[2][:, 1].min()) > 0


def test_means_from_the_histograms_against_the_reference_modules(eng, cases):
    """sum counts x bin centre / cells of |ERR_T| std_T (the signed bins folded about 0) against eval_metrics'
    AbsDiffTemperature, and of ERR_VEL_NORM against DiffVelocityNorm, on the binary tower mask: a value sits within
    half a bin of its bin's centre, so the two means differ by at most half a bin (x std_T for the temperature).
    That needs empty under- and overflow slots, asserted first."""
    L = eng._lib
    from sr3d_amd.src.error_distributions import fold_counts
    _, t, b = cases["tower"]
    g = torch.Generator().manual_seed(5)
    p = t + 0.03 * torch.randn(t.shape, generator=g)
    pd, td, bd = p.to(DEV), t.to(DEV), b.to(DEV)
    counts, _, cells = (x.cpu().numpy() for x in eng.ops.eval_distributions(pd, td, bd, STDS, near_width=1))
    fluid = counts.sum(axis=1)
    n = int(cells[1] + cells[2])
    I = L.DIST_SERIES_INDEX
    for s in (I["ERR_T"], I["ERR_VEL_NORM"]):
        assert fluid[s, ER.UNDER] == 0 and fluid[s, ER.OVER] == 0 and fluid[s, ER.NAN] == 0 and fluid[s].sum() == n
    whole = eng.ops.eval_metrics(pd, td, bd, STDS).cpu().double()
    w = 1.0 / 256
    _, folded, over = fold_counts(fluid[I["ERR_T"]], -0.5, 0.5)
    assert over == 0
    got = float((folded * (np.arange(128) + 0.5) * w).sum() / n) * STDS[0]
    ref = float(whole[L.EVAL_INDEX["AbsDiffTemperature"]])
    print("AbsDiffTemperature", got, ref, "bound", 0.5 * w * STDS[0])
    assert ref > 0 and abs(got - ref) <= 0.5 * w * STDS[0]
    w = 8.0 / 256
    got = float((fluid[I["ERR_VEL_NORM"], 1:257] * (np.arange(256) + 0.5) * w).sum() / n)
    ref = float(whole[L.EVAL_INDEX["DiffVelocityNorm"]])
    print("DiffVelocityNorm", got, ref, "bound", 0.5 * w)
    assert ref > 0 and abs(got - ref) <= 0.5 * w


def test_meter_on_the_device_pools_exactly(eng, cases):
    from sr3d_amd.src.error_distributions import DistributionMeter
    p, t, b = (x.to(DEV) for x in cases["mixed"])
    meter = DistributionMeter()
    for i in range(2):
        meter.update(*eng.ops.eval_distributions(p[i:i + 1], t[i:i + 1], b[i:i + 1], STDS, near_width=1))
    counts, minmax, cells = meter.result()
    whole = [x.cpu().numpy() for x in eng.ops.eval_distributions(p, t, b, STDS, near_width=1)]
    assert np.array_equal(counts, whole[0]) and np.array_equal(cells, whole[2])
    assert np.array_equal(minmax.view(np.int32), whole[1].view(np.int32))


def test_argument_errors(eng):
    ops = eng.ops
    p = torch.rand(1, 4, 4, 6, 8, device=DEV)
    b = torch.ones(1, 1, 4, 6, 8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_distributions(p, p, b, STDS, dist=torch.zeros_like(b))
    with pytest.raises(ValueError, match="near_width"):
        ops.eval_distributions(p, p, b, STDS, near_width=255)
    with pytest.raises(ValueError, match="lo < hi"):
        ops.eval_distributions(p, p, b, STDS, err_range=(0.5, 0.5))
    with pytest.raises(RuntimeError, match="too narrow"):
        ops.eval_distributions(p, p, b, STDS, vel_norm_range=(0.0, 1e-44))
    # and the call still works afterwards
    counts, _, cells = ops.eval_distributions(p, p, b, STDS)
    assert cells.tolist() == [0, 0, b.numel()] and int(counts.sum()) == 13 * b.numel()
