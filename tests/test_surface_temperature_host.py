"""CPU-side checks of the near-surface (2 m) temperature feature: the EleTopoZ parser against pandas and against the
reference's outputs, calc_is_in_building, the numpy restatement of the notebook's extrapolation (tests/surface_ref.py),
the RMSE / MAE definition, argument validation of the C ABI and no CPU path."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

import surface_ref as sr
from helpers import GOLDEN, load_golden

FIXTURE = os.path.join(GOLDEN, "EleTopoZ_fixture.txt")


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.fixture(scope="module")
def bhh(eng):
    from sr3d_amd.src import building_height_helper
    return building_height_helper


@pytest.fixture(scope="module")
def st(eng):
    from sr3d_amd.src import surface_temperature
    return surface_temperature


@pytest.fixture(scope="module")
def gold():
    return load_golden("surface_temperature.npz")


def pandas_pivot(path, col, margin):
    """an independent statement of the reference's parse: whitespace table, pivot_table(aggfunc="max")"""
    df = pd.read_csv(path, sep=r"\s+", skiprows=1, header=None, names=["i", "j", "Ez", "Tz", "Tzl"])
    ret = pd.pivot_table(df[["i", "j", col]], values=col, index="i", columns="j", aggfunc="max").values
    return ret if margin == 0 else ret[margin:-margin, margin:-margin]


@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("col", ["Tz", "Ez"])
def test_parser_matches_golden_and_pandas(bhh, gold, margin, col):
    got = bhh.read_building_height(FIXTURE, col, margin=margin)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, gold[f"{col.lower()}_m{margin}"])
    np.testing.assert_array_equal(got, pandas_pivot(FIXTURE, col, margin))
    if margin == 0:
        assert np.isnan(got[5, 7])                       # the missing (i, j) pair


def test_parser_default_margin_and_dropped_lines(bhh, tmp_path):
    """duplicates keep the max, missing pairs are NaN, all-NaN rows / columns disappear as in pandas"""
    rng = np.random.default_rng(3)
    lines = ["i j Ez Tz Tzl"]
    for i in range(50):
        for j in range(46):
            if i == 7 or j == 11:                         # whole row i = 7 and column j = 11 NaN -> dropped by pandas
                tz = "nan"
            elif rng.random() < 0.02:
                continue                                  # missing pair
            else:
                tz = f"{rng.uniform(0, 200):.3f}"
            lines.append(f"  {i} {j}   {rng.uniform(0, 20):.2f} {tz} 0.0")
            if tz != "nan" and rng.random() < 0.05:
                lines.append(f"{i}  {j} 1.0 {rng.uniform(0, 200):.3f} 1.0")
    p = tmp_path / "EleTopoZ.txt"
    p.write_text("\n".join(lines) + "\n")
    got = bhh.read_building_height(str(p), "Tz")          # default margin 20
    ref = pandas_pivot(str(p), "Tz", 20)
    assert got.shape == ref.shape == (50 - 1 - 40, 46 - 1 - 40)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(bhh.read_building_height(str(p), "Tz", margin=0), pandas_pivot(str(p), "Tz", 0))


def test_calc_is_in_building_matches_golden(bhh, gold):
    got = bhh.calc_is_in_building(gold["tz_m2"].T, gold["ez_m2"].T, gold["inb_levs"])
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, gold["inb_m2"])


def test_calc_is_in_building_quirks(bhh):
    levs = np.arange(4) * 5 + 17.5                            # 17.5 22.5 27.5 32.5
    tz = np.array([[20.0, 40.0, np.nan, 10.0, 22.5]])
    ez = np.array([[0.0, 0.0, 0.0, 10.0, 0.0]])
    got = bhh.calc_is_in_building(tz, ez, levs)
    np.testing.assert_array_equal(got[:, 0], [[1, 0, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])


def test_restatement_matches_notebook(gold):
    for k in ("true", "pred"):
        got = sr.t2m_ref(gold[k], gold["tz_m0"], gold["heights"])
        np.testing.assert_array_equal(got, gold[f"{k}_2m"])        # NaN in the same places, bits equal


def test_height_levels_and_dimensionalize(st, gold):
    np.testing.assert_array_equal(st.HEIGHT_LEVELS, gold["heights"])
    x = torch.rand(2, 4, 3, 5, 6)
    m = torch.Tensor([300.0, -6.5, -9.1, -3.5])[None, :, None, None, None]
    s = torch.Tensor([8.4, 14.4, 21.6, 7.0])[None, :, None, None, None]
    assert torch.equal(st.dimensionalize(x, m, s), x * s + m)


def test_error_definition(st, gold):
    """RMSE / MAE from (sum sq, sum abs, count) = the notebook's nanmean definition, in fp64"""
    p, t = gold["pred_2m"], gold["true_2m"]
    acc = sr.errors_ref(p, t)
    d = p.astype(np.float64) - t.astype(np.float64)
    e = st.calc_2m_temperature_errors(acc)
    assert abs(e["RMSE"] - np.sqrt(np.nanmean(d ** 2))) <= 1e-12 * e["RMSE"]
    assert abs(e["MAE"] - np.nanmean(np.abs(d))) <= 1e-12 * e["MAE"]
    assert abs(e["RMSE"] - float(gold["rmse"])) <= 1e-5 * e["RMSE"]     # the notebook's float32 nanmean
    assert abs(e["MAE"] - float(gold["mae"])) <= 1e-5 * e["MAE"]
    assert np.isnan(st.calc_2m_temperature_errors(torch.zeros(3, dtype=torch.float64))["RMSE"])


def test_c_abi_argument_errors(eng):
    L = eng._lib
    lib = L.lib
    assert lib.sr3d_surface_temperature_workspace_bytes(2, 320, 320) == 16 + 2 * 400 * 3 * 8
    assert lib.sr3d_surface_temperature_workspace_bytes(1, 3, 5) == 16 + 24
    assert lib.sr3d_surface_temperature_workspace_bytes(0, 3, 5) == 0
    h = (C.c_double * 3)(17.5, 22.5, 27.5)
    fake = C.c_void_p(16)                                       # never dereferenced: the checks fail first
    src = L.SurfaceSrc(16, 4, 3, 4, 3, 0, 1.0, 0.0)             # channel 4 of 4
    assert lib.sr3d_surface_temperature(C.byref(src), 1, 4, 4, fake, h, 3, fake, None) == -1
    assert b"channel" in lib.sr3d_last_error()
    src = L.SurfaceSrc(16, 4, 3, 0, 4, 0, 1.0, 0.0)             # 4 levels of 3
    assert lib.sr3d_surface_temperature(C.byref(src), 1, 4, 4, fake, h, 3, fake, None) == -1
    src = L.SurfaceSrc(16, 4, 3, 0, 3, 0, 1.0, 0.0)
    bad = (C.c_double * 3)(17.5, 17.5, 27.5)                    # not increasing
    assert lib.sr3d_surface_temperature(C.byref(src), 1, 4, 4, fake, bad, 3, fake, None) == -1
    assert b"increase" in lib.sr3d_last_error()
    assert lib.sr3d_surface_temperature(C.byref(src), 1, 4, 4, None, h, 3, fake, None) == -1
    rc = lib.sr3d_surface_temperature_errors(C.byref(src), C.byref(src), 1, 4, 4, fake, h, 3, None, None, fake, fake,
                                             8, None)
    assert rc == -3 and b"workspace" in lib.sr3d_last_error()
    rc = lib.sr3d_surface_temperature_errors(C.byref(src), C.byref(src), 1, 4, 4, fake, h, 3, None, None, None, fake,
                                             64, None)
    assert rc == -1 and b"accumulator" in lib.sr3d_last_error()


def test_no_cpu_path(eng):
    x = torch.rand(1, 4, 32, 5, 6)
    tz = torch.zeros(5, 6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.surface_temperature(x, tz)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.ops.surface_temperature_errors(x, x, tz)
