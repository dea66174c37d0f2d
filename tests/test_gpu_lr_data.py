"""LR training data on the MI355X (csrc/sr3d_lrdata.hip): the kernel bit for bit against the numpy restatement
(tests/lr_data_ref.py, pinned to scipy by tests/golden/lr_data.npz) on every rule, at full size, on strided channel
views, twice in a row, its argument errors, and script/make_dl_data_using_outside_lr_builds.py end to end in both input
modes (the tree read back by the repo's Dataset)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lr_data_ref as R
from helpers import ROOT, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "make_dl_data_using_outside_lr_builds.py")


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def tdm(eng):
    from sr3d_amd.src import training_data_maker
    return training_data_maker


def assert_same(a, b):
    """bit-equal values, NaN in the same places"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN differs at {int((na != nb).sum())} cells"
    ok = a[~na].view(np.int32) == b[~nb].view(np.int32)
    assert ok.all(), f"{int((~ok).sum())} cells differ, max |diff| {float(np.abs(a[~na] - b[~nb]).max())}"


def run_op(eng, tdm, raw, hm, tz, ez, levs, lats=None, lons=None, margin=4, align_nan=True, raw_t=None):
    tops = torch.from_numpy(tdm.lr_building_tops(tz, ez, levs, 4)).to(DEV)
    rt = torch.from_numpy(np.ascontiguousarray(raw)).to(DEV) if raw_t is None else raw_t
    return eng.ops.coarse_grain_outside_buildings(rt, torch.from_numpy(np.asarray(hm, bool)).to(DEV), tops,
                                                  hr_margin=margin, lat=lats, lon=lons, lev=levs,
                                                  align_nan=align_nan)


def test_golden_step(eng, tdm):
    g = load_golden("lr_data.npz")
    hr, lr = run_op(eng, tdm, g["step/raw"], g["step/hr_mask"], g["step/lr_tz"], g["step/lr_ez"], g["step/levs"],
                    g["step/lats"], g["step/lons"], margin=int(g["step/margin"]))
    assert_same(hr, g["step/hr"])
    assert_same(lr, g["step/lr"])


@pytest.mark.parametrize("seed,coords,shape,margin,align", [
    (0, False, (4, 8, 24, 28), 4, True),
    (1, True, (4, 8, 24, 28), 4, True),
    (2, True, (4, 12, 32, 80), 8, False),      # a partial 64-column tile, three LR levels
    (3, False, (3, 8, 16, 20), 0, True),       # no margin, three channels
    (4, True, (4, 16, 36, 132), 4, True),
])
def test_rules_bit_exact(eng, tdm, seed, coords, shape, margin, align):
    raw, hm, tz, ez, levs, lats, lons = R.make_case(seed, *shape, coords=coords)
    want = R.lr_data_ref(raw, hm, tz, ez, levs, lats, lons, margin=margin, align_nan=align)
    hr, lr = run_op(eng, tdm, raw, hm, tz, ez, levs, lats, lons, margin=margin, align_nan=align)
    assert_same(hr, want[0])
    assert_same(lr, want[1])
    assert np.isnan(want[1]).any() and (~np.isnan(want[1])).any()


def test_near_ties_in_coordinates(eng, tdm):
    """lat / lon whose midpoints round onto a cell: the tie goes to the lower coordinate, in fp64"""
    raw, hm, tz, ez, levs, _, _ = R.make_case(5, 4, 8, 16, 16)
    raw[:, :, 4:7, 5] = np.nan                 # fully-NaN columns at x = 5, rows 4..6
    raw[:, :, :, 9] = np.nan                   # a fully-NaN x line
    lats = np.array([0.1, 0.2, 0.30000000000000004, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.6])
    lons = np.cumsum(np.r_[0.1, np.full(15, 0.1)])
    want = R.lr_data_ref(raw, hm, tz, ez, levs, lats, lons, margin=0)
    assert_same(run_op(eng, tdm, raw, hm, tz, ez, levs, lats, lons, margin=0)[1], want[1])


def full_size_case():
    rng = np.random.default_rng(7)
    C, Z, Y, X = 4, 40, 400, 400
    levs = 17.5 + 5.0 * np.arange(Z)
    raw = np.empty((C, Z, Y, X), np.float32)
    raw[0] = 300 + 3 * rng.standard_normal((Z, Y, X), dtype=np.float32)
    raw[1:] = 4 * rng.standard_normal((C - 1, Z, Y, X), dtype=np.float32)
    hr_tz = np.full((Y, X), 10.0)
    for _ in range(120):                       # buildings of odd widths, some taller than the domain
        y0, x0 = rng.integers(0, Y - 20, 2)
        h, w = rng.integers(1, 19, 2)
        hr_tz[y0:y0 + h, x0:x0 + w] = rng.choice([rng.uniform(20, 120), rng.uniform(150, 300)])
    hm = R.calc_is_in_building(hr_tz, np.full((Y, X), 15.0), levs) > 0
    tall = hr_tz > levs[-1]
    raw[0][:, tall] = np.nan                   # tm is undefined inside the tallest buildings: whole columns
    hm |= np.isnan(raw[0])
    lr_tz = hr_tz.reshape(Y // 4, 4, X // 4, 4).max(axis=(1, 3))
    lr_tz[rng.random(lr_tz.shape) < 0.02] = levs[Z - 3] + 1.0
    return raw, hm, lr_tz, np.full(lr_tz.shape, 15.0), levs


def test_full_size(eng, tdm):
    raw, hm, tz, ez, levs = full_size_case()
    want = R.lr_data_ref(raw, hm, tz, ez, levs, margin=40)
    hr, lr = run_op(eng, tdm, raw, hm, tz, ez, levs, margin=40)
    assert tuple(hr.shape) == (4, 40, 320, 320) and tuple(lr.shape) == (4, 10, 80, 80)
    assert_same(hr, want[0])
    assert_same(lr, want[1])


def test_strided_channel_view_and_repeat(eng, tdm):
    raw, hm, tz, ez, levs, lats, lons = R.make_case(6, 4, 8, 24, 28, coords=True)
    want = R.lr_data_ref(raw, hm, tz, ez, levs, lats, lons, margin=4)
    big = torch.full((9,) + raw.shape[1:], float("inf"), device=DEV)
    view = big[1::2]                           # offset and a channel stride of two volumes
    view.copy_(torch.from_numpy(raw))
    assert view.data_ptr() != big.data_ptr() and not view.is_contiguous()
    a = run_op(eng, tdm, raw, hm, tz, ez, levs, lats, lons, margin=4, raw_t=view)
    b = run_op(eng, tdm, raw, hm, tz, ez, levs, lats, lons, margin=4, raw_t=view)
    for x, y, w in zip(a, b, want):
        assert_same(x, w)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_dataset_function(eng, tdm):
    """the reference's function names: a mapping of variables in, LR arrays out, the pooling weights unused"""
    from sr3d_amd.src.building_height_helper import calc_ave_pooling_weights, make_resized_lr_tz
    raw, hm, tz, ez, levs, lats, lons = R.make_case(8, 4, 8, 16, 24, coords=True)
    resized = make_resized_lr_tz(tz, ez, np.zeros((4,) + hm.shape), levs) if tz.shape[0] == tz.shape[1] else None
    rz = R.resized_lr_mask(tz, ez, levs) if resized is None else resized[0]
    ds = {n: raw[i] for i, n in enumerate(["tm", "vl", "vp", "vr"])}
    out = tdm.make_coarse_grained_dataset_with_outside_lr_buildings(
        hr_ds=ds, lr_is_in_build=rz, hr_is_in_build=hm.astype(float), avg_pooling_weights=None, lev_window_width=4,
        lat_window_width=4, lon_window_width=4, levs=levs, lats=lats, lons=lons)
    for i, n in enumerate(ds):
        assert_same(out[n], R.coarse_grain_literal(raw[i], hm, rz, levs, lats, lons))
    one = tdm.make_coarse_grained_dataarray_with_outside_lr_buildings(
        da=torch.from_numpy(raw[2]), lr_is_in_build=rz, hr_is_in_build=hm, avg_pooling_weights=calc_ave_pooling_weights(
            rz, 4, 4, 4), lev_window_width=4, lat_window_width=4, lon_window_width=4, levs=levs, lats=lats, lons=lons)
    assert_same(one, out["vp"])


def test_argument_errors(eng, tdm):
    raw, hm, tz, ez, levs, _, _ = R.make_case(9, 4, 8, 16, 16)
    ops, L = eng.ops, eng._lib
    good = dict(raw=torch.from_numpy(raw).to(DEV), hr_mask=torch.from_numpy(hm).to(DEV),
                lr_tops=torch.from_numpy(tdm.lr_building_tops(tz, ez, levs)).to(DEV))
    for kw, exc in ((dict(scale=2), ValueError), (dict(hr_margin=6), ValueError), (dict(hr_margin=8), ValueError),
                    (dict(lat=np.arange(15.0)), ValueError), (dict(lon=np.arange(16.0)[::-1].copy()), ValueError)):
        with pytest.raises(exc):
            ops.coarse_grain_outside_buildings(**good, **kw)
    with pytest.raises(ValueError):
        ops.coarse_grain_outside_buildings(good["raw"][:, :, :, :12], good["hr_mask"], good["lr_tops"])
    with pytest.raises(RuntimeError):
        ops.coarse_grain_outside_buildings(good["raw"].cpu(), good["hr_mask"], good["lr_tops"])
    # the C ABI itself: every bad argument is an error code, nothing is launched
    hr = torch.empty(4, 8, 16, 16, device=DEV)
    lr = torch.empty(4, 2, 4, 4, device=DEV)
    ws = torch.empty(L.lib.sr3d_lrdata_workspace_bytes(4, 16, 16), dtype=torch.uint8, device=DEV)

    def params(**over):
        f = dict(raw=good["raw"].data_ptr(), channel_stride=8 * 16 * 16, C=4, Z=8, Y=16, X=16, scale=4, hr_margin=0,
                 align_nan=1, hr_mask=good["hr_mask"].data_ptr(), lr_tops=good["lr_tops"].data_ptr(), lat=None,
                 lon=None, lev=None, hr_out=hr.data_ptr(), lr_out=lr.data_ptr())
        f.update(over)
        return L.LrDataParams(**f)

    call = lambda p, n=ws.numel(): L.lib.sr3d_lrdata(C.byref(p), C.c_void_p(ws.data_ptr()), n, L.stream_ptr())  # noqa
    assert call(params()) == 0
    for over in (dict(scale=3), dict(Z=6), dict(Y=18), dict(hr_margin=2), dict(hr_margin=8), dict(Z=132),
                 dict(raw=None), dict(hr_mask=None), dict(lr_tops=None), dict(hr_out=None), dict(lr_out=None),
                 dict(channel_stride=100)):
        assert call(params(**over)) == -1, over
        assert L.lib.sr3d_last_error()
    assert call(params(), 16) == -3
    assert L.lib.sr3d_lrdata(None, C.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert_same(run_op(eng, tdm, raw, hm, tz, ez, levs, margin=0)[1], R.lr_data_ref(raw, hm, tz, ez, levs, margin=0)[1])


# ---------------------------------------------------------------- the script end to end
def write_eletopoz(path, tz_yx, ez_yx):
    with open(path, "w") as f:
        f.write("i j Ez Tz Tzl\n")
        for y in range(tz_yx.shape[0]):
            for x in range(tz_yx.shape[1]):
                f.write(f"{x + 1} {y + 1} {ez_yx[y, x]:.4f} {tz_yx[y, x]:.4f} 0.0\n")


def script_case(tmp_path):
    rng = np.random.default_rng(11)
    Z, Y, X, m = 8, 48, 48, 8
    levs = 17.5 + 5.0 * np.arange(Z)
    hr_tz = np.where(rng.random((Y, X)) < 0.15, rng.uniform(18.0, 40.0, (Y, X)), 10.0).round(2)
    hr_ez = np.full((Y, X), 15.0)
    lr_tz = rng.choice([10.0, 26.0, 31.0, 52.5], (Y // 4, X // 4))
    lr_tz[m // 4, 20 // 4] = 10.0              # no LR building over the block of the margin case below
    lr_ez = np.full((Y // 4, X // 4), 15.0)
    write_eletopoz(tmp_path / "hr.txt", hr_tz, hr_ez)
    write_eletopoz(tmp_path / "lr.txt", lr_tz, lr_ez)
    raw_dir = tmp_path / "raw"
    raw_dir.mkdir()
    stamps = [f"20150731T05{k:02d}00" for k in range(5)]
    raws = {}
    for k, s in enumerate(stamps):
        r = np.empty((4, Z, Y, X), np.float32)
        r[0] = 300 + rng.standard_normal((Z, Y, X))
        r[1:] = 3 * rng.standard_normal((3, Z, Y, X))
        r[0][:, m:m + 2, 20] = np.nan          # fully-NaN columns on the window's first rows: their nearest valid
        r[0][:, m - 1, 20] = 295.0 + k         # column (row m - 1) lies in the cut margin
        raws[s] = r
        np.save(raw_dir / f"{s}.npy", r)
    (raw_dir / "README.npy").write_bytes(b"")  # not a time stamp: ignored
    return dict(levs=levs, hr_tz=hr_tz, hr_ez=hr_ez, lr_tz=lr_tz, lr_ez=lr_ez, raw_dir=raw_dir, stamps=stamps,
                raws=raws, m=m)


def run_script(args, timeout=300):
    r = subprocess.run([sys.executable, SCRIPT] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_script_raw_dir_and_from_hr(eng, tmp_path):
    from sr3d_amd.src.dataset import DatasetWithoutAligningResolution
    k = script_case(tmp_path)
    m, levs, out = k["m"], k["levs"], tmp_path / "DL_data"
    run_script(["--raw_dir", k["raw_dir"], "--out_dir", out, "--hr_building_path", tmp_path / "hr.txt",
                "--lr_building_path", tmp_path / "lr.txt", "--hr_margin", m])
    group = out / "10"
    kept = k["stamps"][::-1][::2][::-1]
    assert kept == [k["stamps"][0], k["stamps"][2], k["stamps"][4]]
    made = sorted(p.name for p in (group / "20150731").iterdir())
    assert made == sorted([f"{s}_HR.npy" for s in kept] + [f"{s}_LR_x04.npy" for s in kept])

    hm = (R.calc_is_in_building(k["hr_tz"], k["hr_ez"], levs) + np.isnan(k["raws"][kept[0]][0])) > 0
    hr_mask = np.load(group / "hr_is_in_build.npy")
    lr_mask = np.load(group / "lr_is_in_build.npy")
    assert hr_mask.dtype == lr_mask.dtype == np.float64
    assert np.array_equal(hr_mask, np.tile(hm[None, :, m:-m, m:-m].astype(float), (4, 1, 1, 1)))
    lz = R.calc_is_in_building(k["lr_tz"], k["lr_ez"], levs[::4])
    assert np.array_equal(lr_mask, np.tile(lz[None, :, m // 4:-m // 4, m // 4:-m // 4], (4, 1, 1, 1)))
    for s in kept:
        want = R.lr_data_ref(k["raws"][s], hm, k["lr_tz"], k["lr_ez"], levs, margin=m)
        assert_same(np.load(group / "20150731" / f"{s}_HR.npy"), want[0])
        assert_same(np.load(group / "20150731" / f"{s}_LR_x04.npy"), want[1])

    ds = DatasetWithoutAligningResolution([group / "20150731"], group / "hr_is_in_build.npy",
                                          hr_org_size=(8, 32, 32), hr_crop_size=(8, 32, 32), use_cropping=False,
                                          max_height_index=8)
    assert len(ds) == 3
    lr_c, bldg, hr_c = ds[0]
    assert tuple(hr_c.shape) == (4, 8, 32, 32) and tuple(lr_c.shape) == (4, 2, 8, 8) and torch.isfinite(lr_c).all()

    before = {p: p.stat().st_mtime_ns for p in group.rglob("*.npy")}
    run_script(["--raw_dir", k["raw_dir"], "--out_dir", out, "--hr_building_path", tmp_path / "hr.txt",
                "--lr_building_path", tmp_path / "lr.txt", "--hr_margin", m])
    assert {p: p.stat().st_mtime_ns for p in group.rglob("*.npy")} == before     # existing files are skipped

    # --from_hr: the LR files again from the cut HR files, into a tree of its own
    out2 = tmp_path / "again"
    run_script(["--from_hr", out, "--out_dir", out2, "--lr_building_path", tmp_path / "lr.txt", "--hr_margin", m])
    ml = m // 4
    tz_c, ez_c = k["lr_tz"][ml:-ml, ml:-ml], k["lr_ez"][ml:-ml, ml:-ml]
    for s in kept:
        hr_cut = np.load(group / "20150731" / f"{s}_HR.npy")
        again = np.load(out2 / "10" / "20150731" / f"{s}_LR_x04.npy")
        want = R.lr_data_ref(hr_cut, np.isnan(hr_cut[0]), tz_c, ez_c, levs, margin=0)[1]
        assert_same(again, want)
        # the documented difference: the fully-NaN columns at window rows 0, 1 (x = 20) took row m - 1 of the margin
        # in the full domain, and take window row 2 here; only the LR blocks that hold them differ
        orig = np.load(group / "20150731" / f"{s}_LR_x04.npy")
        diff = ~((orig == again) | (np.isnan(orig) & np.isnan(again)))
        cols = {(int(yy), int(xx)) for yy, xx in zip(*np.nonzero(diff.any(axis=(0, 1))))}
        assert cols == {(0, (20 - m) // 4)}, cols
    assert np.array_equal(np.load(out2 / "10" / "lr_is_in_build.npy"), lr_mask)
