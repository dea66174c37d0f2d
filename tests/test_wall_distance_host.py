"""The wall-distance-resolved evaluation without a GPU: the restatement (tests/wall_distance_ref.py) against the golden
file made by the reference's own near-wall function and modules at widths 1 .. 12, the C ABI (symbols, signatures,
index maps, workspace sizes, argument errors: every one is returned before anything is launched) and the table
script/evaluate_wall_distance_profiles.py writes, on a stubbed ``ops.eval_wall_distance_profiles``."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import wall_distance_ref as WR
from helpers import ROOT, load_golden

TOL = 1e-5      # the project's fp32 parity bound
SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "evaluate_wall_distance_profiles.py")


@pytest.fixture(scope="module")
def gold():
    return load_golden("wall_distance.npz")


@pytest.fixture(scope="module")
def eng():
    import sr3d_amd
    return sr3d_amd


@pytest.mark.parametrize("kind", WR.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_masks_and_modules(gold, kind):
    p, t, b = WR.case(gold, kind)
    assert tuple(p.shape) == (WR.SHAPE[0], 4) + WR.SHAPE[1:] and p.dtype == torch.float32
    assert list(gold["stds"]) == WR.STDS
    dist = WR.wall_distance_ref(b, 12)
    assert dist.dtype == torch.uint8 and int(dist.min()) == 0 and int(dist.max()) <= 13
    V, S = WR.wall_distance_profiles_ref(p.double(), t.double(), b.double(), WR.STDS, D=12, dist=dist)
    for n in WR.GOLDEN_WIDTHS:
        near = WR.unpack(gold[f"near/{kind}/{n}"])
        assert torch.equal(((dist <= n) & (b > 0)).float(), near), n       # bit for bit
        assert torch.equal(WR.near_wall_ref(b, n), near), n
        assert float(S["pos"][:n + 1].sum()) == float(near.sum())
        for row, ref in zip(("MaskedL1NearWall", "MaskedL2NearWall"), gold[f"module/{kind}/{n}"].astype(np.float64)):
            assert ref > 0 and abs(float(V[row][n]) - ref) <= TOL * ref, (row, n, float(V[row][n]), ref)
    # width 1 is the oracle's near-wall mask
    from oracle import ref_cpu as R
    assert torch.equal(WR.near_wall_ref(b, 1), R.near_wall_mask(b))


def test_cases_are_what_they_claim(gold):
    B, Z, Y, X = WR.SHAPE
    frac = WR.case(gold, "fractional")[2]
    assert 0.0005 < float((frac == 0.5).float().mean()) < 0.002 and set(frac.unique().tolist()) == {0.0, 0.5, 1.0}
    assert 0.001 < 1.0 - float(WR.case(gold, "sparse")[2].mean()) < 0.003
    mixed, tower, sparse = (WR.case(gold, k)[2] for k in ("mixed", "tower", "sparse"))
    assert torch.equal(mixed[0], tower[0]) and torch.equal(mixed[1], sparse[1]) and not torch.equal(mixed[0], mixed[1])
    # iid: nothing is farther than 2 cells from a built cell; one_cell: the distance is known in closed form
    assert int(WR.wall_distance_ref(WR.case(gold, "iid")[2], 12).max()) == 2
    d = WR.wall_distance_ref(WR.case(gold, "one_cell")[2], 12)
    z, y, x = torch.meshgrid(torch.arange(Z), torch.arange(Y), torch.arange(X), indexing="ij")
    cheb = torch.maximum(torch.maximum(z, (y - 11).abs()), (x - 33).abs()).clamp(max=13)
    assert torch.equal(d[0, 0].long(), cheb) and torch.equal(d[1], d[0])
    assert bool((WR.wall_distance_ref(WR.case(gold, "all_fluid")[2], 254) == 255).all())
    # the interior rows of a binary mask are NaN at bins 0 and 1 only
    p, t, b = WR.case(gold, "tower")
    V, S = WR.wall_distance_profiles_ref(p.double(), t.double(), b.double(), WR.STDS, D=8)
    for name in WR.INTERIOR:
        assert [k for k in range(10) if bool(torch.isnan(V[name][k]))] == [0, 1], name
    assert int(S["cells"].sum()) == B * Z * Y * X and float(S["cells"][0]) == float((b == 0).sum())


def _header_enum(prefix):
    text = open(os.path.join(ROOT, "include", "sr3d.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"\b{prefix}([A-Z0-9_]+) = (\d+)", text)}


def test_cabi_symbols_signatures_and_index_maps(eng):
    L = eng._lib
    P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    want = {"sr3d_wall_distance_workspace_bytes": (SZ, [I] * 4),
            "sr3d_wall_distance": (I, [P, P, I, I, I, I, I, P, P]),
            "sr3d_eval_wall_distance_profiles_workspace_bytes": (SZ, [I] * 5),
            "sr3d_eval_wall_distance_profiles": (I, [P, P, P, P, I, I, I, I, C.POINTER(F), F, I, P, P, P, P])}
    for name, (res, args) in want.items():
        assert hasattr(L.lib, name), name
        assert L.SYMBOLS[name][0] is res and L.SYMBOLS[name][1] == args, name
    # the header declares exactly these parameters
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr3d.h")).read(), flags=re.S)

    def params(fn):
        decl = re.search(rf"\b{fn}\((.*?)\);", text, flags=re.S).group(1)
        return [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]

    assert params("int sr3d_wall_distance") == ["b", "dist_out", "B", "Z", "Y", "X", "cap", "workspace", "stream"]
    assert params("int sr3d_eval_wall_distance_profiles") == [
        "p", "t", "b", "dist", "B", "Z", "Y", "X", "stds", "delta_meter", "D", "sums_out", "values_out", "workspace",
        "stream"]
    # the name -> row maps are the header's enums
    sums = _header_enum("SR3D_WALLDIST_SUM_")
    assert sums.pop("COUNT") == L.WALLDIST_SUM_COUNT == len(L.WALLDIST_SUM_INDEX) == len(WR.SUMS) == 21
    assert {k.upper(): v for k, v in L.WALLDIST_SUM_INDEX.items()} == sums
    vals = {k: v for k, v in _header_enum("SR3D_WALLDIST_").items() if not k.startswith("SUM_")}
    assert vals.pop("COUNT") == L.WALLDIST_COUNT == len(L.WALLDIST_INDEX) == len(WR.PROFILES) == 16
    snake = {re.sub(r"(?<!^)(?=[A-Z])", "_", k).upper(): v for k, v in L.WALLDIST_INDEX.items()}
    assert snake == vals
    assert [n for n, _ in sorted(L.WALLDIST_SUM_INDEX.items(), key=lambda kv: kv[1])] == list(WR.SUMS)
    assert [n for n, _ in sorted(L.WALLDIST_INDEX.items(), key=lambda kv: kv[1])] == list(WR.PROFILES)
    # the per-bin sums are the per-level sums with POS in the NEAR slots, then CELLS
    for k, v in L.PROFILE_SUM_INDEX.items():
        assert L.WALLDIST_SUM_INDEX[k.replace("near", "pos") if k in ("near", "near_abs", "near_sq") else k] == v
    assert L.WALLDIST_INDEX == L.PROFILE_INDEX
    assert int(re.search(r"#define SR3D_WALLDIST_MAX_D (\d+)", text).group(1)) == L.WALLDIST_MAX_D == 30


def test_cabi_workspace_and_argument_errors(eng):
    L = eng._lib
    dws, pws = L.lib.sr3d_wall_distance_workspace_bytes, L.lib.sr3d_eval_wall_distance_profiles_workspace_bytes
    assert dws(1, 32, 320, 320) == 32 * 320 * 320 and dws(2, 19, 23, 67) == 2 * 19 * 23 * 67 and dws(3, 1, 1, 1) == 3
    # [sample][z tiles of 16][xy tiles of 8 x 62][D + 2 bins][21 sums] doubles
    assert pws(1, 32, 320, 320, 8) == 1 * 2 * (40 * 6) * 10 * 21 * 8
    assert pws(2, 19, 23, 67, 30) == 2 * 2 * (3 * 2) * 32 * 21 * 8
    assert pws(3, 1, 1, 1, 1) == 3 * 3 * 21 * 8
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0)):
        assert dws(*bad) == 0 and pws(*bad, 8) == 0
    assert pws(1, 4, 4, 4, 0) == 0 and pws(1, 4, 4, 4, 31) == 0
    p = C.c_void_p(0x1000)      # never dereferenced: every call below fails its checks before a launch
    sc = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)

    def distance(**over):
        a = dict(b=p, out=p, B=1, Z=4, Y=6, X=8, cap=8, ws=p)
        a.update(over)
        return L.lib.sr3d_wall_distance(a["b"], a["out"], a["B"], a["Z"], a["Y"], a["X"], a["cap"], a["ws"], None)

    for over in (dict(b=None), dict(out=None), dict(ws=None), dict(B=0), dict(Z=0), dict(Y=-3), dict(X=0), dict(cap=0),
                 dict(cap=255), dict(cap=-1), dict(Z=2048, Y=1024, X=1024), dict(B=65536)):
        assert distance(**over) == -1, over
        assert L.lib.sr3d_last_error().decode().startswith("wall_distance: "), over
    assert distance(cap=255) == -1 and b"1 .. 254" in L.lib.sr3d_last_error()

    def profiles(**over):
        a = dict(p=p, t=p, b=p, dist=p, B=1, Z=4, Y=6, X=8, stds=sc, delta=5.0, D=8, sums=p, values=p, ws=p)
        a.update(over)
        return L.lib.sr3d_eval_wall_distance_profiles(a["p"], a["t"], a["b"], a["dist"], a["B"], a["Z"], a["Y"], a["X"],
                                                      a["stds"], a["delta"], a["D"], a["sums"], a["values"], a["ws"], None)

    for over in (dict(p=None), dict(t=None), dict(b=None), dict(dist=None), dict(stds=None), dict(sums=None),
                 dict(values=None), dict(ws=None), dict(B=0), dict(Z=0), dict(Y=-3), dict(X=0), dict(delta=0.0),
                 dict(D=0), dict(D=31), dict(Z=2048, Y=1024, X=1024), dict(B=65536)):
        assert profiles(**over) == -1, over
        assert L.lib.sr3d_last_error().decode().startswith("eval_wall_distance_profiles: "), over
    assert profiles(D=31) == -1 and b"1 .. 30" in L.lib.sr3d_last_error()
    with pytest.raises(RuntimeError, match="max distance"):
        L.check(profiles(D=0), "sr3d_eval_wall_distance_profiles")


def test_python_surface_refuses_before_any_launch(eng):
    """shape, dtype and range errors of the ops are raised on the host (CPU tensors never reach a kernel)"""
    ops = eng.ops
    b = torch.ones(1, 1, 4, 6, 8)
    p = torch.rand(1, 4, 4, 6, 8)
    with pytest.raises(ValueError):
        ops.wall_distance(b[:, 0], 3)
    with pytest.raises(ValueError):
        ops.near_wall_mask(b, 0)
    with pytest.raises(NotImplementedError, match="254"):
        ops.near_wall_mask(torch.ones(1, 1, 1, 2, 300), 255)
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_wall_distance_profiles(p, p, b, WR.STDS, dist=torch.zeros(b.shape))
    with pytest.raises(ValueError, match="uint8"):
        ops.eval_wall_distance_profiles(p, p, b, WR.STDS, dist=torch.zeros(1, 1, 4, 6, 9, dtype=torch.uint8))
    for D in (0, 31):
        with pytest.raises(ValueError, match="max_distance"):
            ops.eval_wall_distance_profiles(p, p, b, WR.STDS, max_distance=D)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.wall_distance(b, 3)
    from sr3d_amd.src import loss_maker as lm
    assert lm.MaskedL1LossNearWall(num_filter_applications=5).num_filter_applications == 5
    assert lm.MaskedL2LossNearWall(num_filter_applications=12).entry == "MaskedL2NearWall"
    with pytest.raises(ValueError):
        lm.MaskedL1LossNearWall(num_filter_applications=0)
    with pytest.raises(RuntimeError, match="GPU"):
        lm.calc_mask_near_build_wall(b, 3)


def _stub_eval_wall_distance_profiles(L):
    """ops.eval_wall_distance_profiles on the CPU, from the restatement"""
    def stub(p, t, b, stds, delta_meter=5.0, max_distance=8, dist=None):
        V, S = WR.wall_distance_profiles_ref(p.double(), t.double(), b.double(), [1.0 if s is None else s for s in stds],
                                             delta_meter, max_distance, dist)
        values = torch.stack([V[n] for n, _ in sorted(L.WALLDIST_INDEX.items(), key=lambda kv: kv[1])]).float()
        sums = torch.stack([S[n] for n, _ in sorted(L.WALLDIST_SUM_INDEX.items(), key=lambda kv: kv[1])]).float()
        return values, sums
    return stub


@pytest.mark.parametrize("pooled", [False, True])
def test_script_table_layout_on_a_stubbed_ops_call(eng, monkeypatch, tmp_path, pooled):
    import pandas as pd
    L = eng._lib
    from sr3d_amd.src.wall_distance_profiles import WALL_DISTANCE_PROFILE_NAMES
    monkeypatch.setattr(eng.ops, "eval_wall_distance_profiles", _stub_eval_wall_distance_profiles(L))
    spec = importlib.util.spec_from_file_location("evaluate_wall_distance_profiles", SCRIPT)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    assert script.MODEL_CSV == "wall_distance_scores.csv"
    assert script.BASELINE_CSV == "interpolation_baseline_wall_distance_scores.csv"

    Z, Y, X, D = 7, 9, 12, 3
    g = torch.Generator().manual_seed(7)
    loader = []
    for n in (1, 2):
        y = torch.rand(n, 4, Z, Y, X, generator=g)
        b = torch.ones(n, Z, Y, X)
        b[:, :2, 2:4, 3:5] = 0
        loader.append((y + 0.1 * torch.rand(n, 4, Z, Y, X, generator=g), b, y))

    class Identity(torch.nn.Module):
        def forward(self, X, bb):
            return X

    path, df = script.write_profiles(dataloader=loader, model=Identity(), stds=WR.STDS, device="cpu",
                                     out_dir=str(tmp_path / "out"), file_name=script.MODEL_CSV, max_distance=D,
                                     pooled=pooled)
    assert path == str(tmp_path / "out" / "wall_distance_scores.csv")
    back = pd.read_csv(path)
    assert list(back.columns) == ["distance_cells", "distance_m", *WALL_DISTANCE_PROFILE_NAMES, "Cells", "FluidCells",
                                  "InteriorCells"]
    assert WALL_DISTANCE_PROFILE_NAMES == WR.PROFILES and len(back) == D + 2
    assert list(back["distance_cells"]) == list(range(D + 2))
    assert list(back["distance_m"]) == [0.0, 5.0, 10.0, 15.0, np.inf]
    assert int(back["Cells"].sum()) == 3 * Z * Y * X and back["Cells"][0] == 3 * 2 * 2 * 2
    assert back["FluidCells"][0] == 0 and list(back["FluidCells"][1:]) == list(back["Cells"][1:])
    assert back["InteriorCells"][0] == 0 and back["InteriorCells"][1] == 0 and back["InteriorCells"][2] > 0
    assert np.isnan(back["DiffOmegaNorm"][1]) and np.isfinite(back["DiffOmegaNorm"][2])
    # pooled: the restatement's sums added over the batches, then the ratios (cumulative rows re-derived)
    tot = None
    for pred, b, y in loader:
        bb = b.unsqueeze(1).double()
        S = WR.bin_sums(WR.voxel_terms(pred.double(), y.double(), bb, WR.STDS), WR.wall_distance_ref(bb, D), D)
        tot = S if tot is None else {k: tot[k] + S[k] for k in S}
    ref = WR.ratios(tot)
    if pooled:
        for name in WALL_DISTANCE_PROFILE_NAMES:
            got, r = back[name].to_numpy(), ref[name].numpy()
            assert np.array_equal(np.isnan(got), np.isnan(r)), name
            assert np.allclose(got[~np.isnan(r)], r[~np.isnan(r)], rtol=TOL, atol=0), name
    else:
        # every batch holds the same mask: the same denominators, so the sample-weighted mean is the pooled ratio
        assert np.allclose(back["L1"].to_numpy(), ref["L1"].numpy(), rtol=TOL, atol=0)
