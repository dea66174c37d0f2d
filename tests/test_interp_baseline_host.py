"""The interpolation baseline without a GPU: the numpy restatement (tests/interp_baseline_ref.py) bit for bit against the
scipy-made golden file, its fp32 form against its fp64 form, what each rule case claims to exercise, and the argument
errors of the C ABI (every one is returned before anything is launched, so the library answers on a CPU-only box)."""
import numpy as np
import pytest

import interp_baseline_ref as R
from helpers import load_golden

TOL = 1e-5      # the project's fp32 parity bound (README)
CASES = [(n, s) for s in sorted(R.RULE_SHAPES) for n in sorted(R.RULE_CASES)]


@pytest.fixture(scope="module")
def gold():
    return load_golden("interp_baseline.npz")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN differs at {int((na != nb).sum())} cells"
    assert np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)), float(np.abs(a[~na] - b[~nb]).max())


def test_lines_equal_scipy(gold):
    for i in range(int(gold["lines/n"])):
        y = gold[f"lines/{i}/y"]
        same_bits(R.fill_axis(y, 0), gold[f"lines/{i}/out"])
    assert np.isnan(gold["lines/3/out"]).all() and np.isnan(gold["lines/5/out"]).sum() == 4    # too few valid cells
    assert np.isnan(gold["lines/8/out"]).sum() == 1 and not np.isnan(gold["lines/9/out"]).any()


@pytest.mark.parametrize("name,scale", CASES)
def test_restatement_equals_scipy_golden(gold, name, scale):
    lr, mask = R.rule_case(name, scale)
    k = f"{name}_x{scale}"
    r = R.interp_baseline_ref(lr, mask, scale)
    # the file holds the cells that were NaN before the fill and a checksum of the others (torch's own upsample)
    blank = np.unpackbits(gold[f"{k}/blank"])[:r["out"].size].reshape(r["out"].shape).astype(bool)
    assert np.array_equal(blank, np.isnan(r["masked"]))
    same_bits(r["out"][blank], gold[f"{k}/values"])
    assert not np.isnan(r["out"][~blank]).any()
    assert np.bitwise_xor.reduce(r["out"][~blank].view(np.uint32)) == gold[f"{k}/checksum"]


@pytest.mark.parametrize("name,scale", CASES)
def test_rule_cases_exercise_what_they_claim(name, scale):
    lr, mask = R.rule_case(name, scale)
    r = R.interp_baseline_ref(lr, mask, scale)
    after_mask, after_z, after_y, after_x = r["n_nan"]
    assert after_mask > 0
    done = R.RULE_CASES[name]
    assert (after_z == 0) == (done == "z")
    assert (after_y == 0) == (done in ("z", "y"))
    assert (after_x == 0) == (done != "never")
    if done == "never":
        assert after_x == r["out"].size
    # a test column extrapolates over at most 16 HR levels, so that fp32 stays inside the parity bound
    assert scale * (mask.shape[0] - 1) <= 16


@pytest.mark.parametrize("name,scale", CASES + [("tower", 4)])
def test_fp32_restatement_within_bound_of_fp64(name, scale):
    lr, mask = R.tower_case() if name == "tower" else R.rule_case(name, scale)
    a = R.interp_baseline_ref(lr, mask, scale)
    b = R.interp_baseline_ref(lr, mask, scale, dtype=np.float64)
    assert a["out"].dtype == np.float32 and b["out"].dtype == np.float64 and a["n_nan"] == b["n_nan"]
    nan = np.isnan(b["out"])
    assert np.array_equal(np.isnan(a["out"]), nan)
    if (~nan).any():
        err = np.abs(a["out"][~nan] - b["out"][~nan]).max() / np.abs(b["out"][~nan]).max()
        assert err <= TOL, err


def test_tower_case_is_realistic():
    lr, mask = R.tower_case()
    built = mask[0].mean()
    assert 0.1 < built < 0.3 and mask.all(axis=0).any() and not mask[-1].all()
    n = R.interp_baseline_ref(lr, mask, 4)["n_nan"]
    assert n[0] > 0 and n[1] > 0 and n[3] == 0      # whole columns are left to the y pass; everything is filled


def test_cabi_argument_errors():
    import ctypes as C

    import sr3d_amd
    L = sr3d_amd._lib
    assert L.lib.sr3d_interp_baseline_workspace_bytes(1, 4, 8, 80, 80, 4) == 4 * (320 + 32) * 4
    assert L.lib.sr3d_interp_baseline_workspace_bytes(2, 3, 4, 6, 5, 2) == 6 * (10 + 8) * 4
    for bad in ((1, 4, 8, 80, 80, 3), (1, 4, 8, 80, 80, 8), (0, 4, 8, 80, 80, 4), (1, 4, 8, 0, 80, 4)):
        assert L.lib.sr3d_interp_baseline_workspace_bytes(*bad) == 0
    p = C.c_void_p(0x1000)      # never dereferenced: every call below fails its checks before a launch

    def call(**over):
        a = dict(lr=p, bs=4 * 105, cs=105, dtype=L.DTYPE_F32, B=1, C=4, z=3, y=5, x=7, mask=p, mz=3, my=5, mx=7,
                 scale=4, out=p, n=p, ws=p, wsb=1 << 20)
        a.update(over)
        return L.lib.sr3d_interp_baseline(a["lr"], a["bs"], a["cs"], a["dtype"], a["B"], a["C"], a["z"], a["y"],
                                          a["x"], a["mask"], a["mz"], a["my"], a["mx"], a["scale"], a["out"], a["n"],
                                          a["ws"], a["wsb"], None)

    for over in (dict(scale=3), dict(scale=1), dict(scale=8), dict(mz=4), dict(my=4), dict(mx=28), dict(lr=None),
                 dict(mask=None), dict(out=None), dict(n=None), dict(ws=None), dict(dtype=L.DTYPE_BF16), dict(dtype=7),
                 dict(B=0), dict(z=-1), dict(cs=100), dict(B=2, bs=100), dict(out=C.c_void_p(0x1002)),
                 dict(B=64, C=64, z=32, y=80, x=80, mz=32, my=80, mx=80, cs=32 * 80 * 80, bs=64 * 32 * 80 * 80)):
        assert call(**over) == -1, over
        assert L.lib.sr3d_last_error().decode().startswith("interp_baseline: "), over
    assert call(wsb=16) == -3
    assert b"workspace" in L.lib.sr3d_last_error()
