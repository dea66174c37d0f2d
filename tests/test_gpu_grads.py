"""GrADS decode on the MI355X (csrc/sr3d_grads.hip): ops.grads_decode bit for bit against the numpy restatement
(tests/grads_ref.py) on every layout rule, at the reference's full shape, twice in a row, its argument errors,
load_atmos_data(...).step(i), and script/make_dl_data_using_outside_lr_builds.py --grads_dir end to end against
--raw_dir on the same fields.  No tolerance anywhere: the feature is data movement plus an equality test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grads_ref as G
from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCRIPT = os.path.join(ROOT, "3d-sr-micrometeorology_amd", "script", "make_dl_data_using_outside_lr_builds.py")
UNDEF = -9.99e33          # not exact in fp32: the comparison is with (float)undef
NAMES = ("tm", "vl", "vp", "vr")


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
    assert ok.all(), f"{int((~ok).sum())} cells differ"


def file_bytes(seed, Zf, Y, X, *, big=True, sequential=False, yrev=False, zrev=False, file_nan=False, undef=UNDEF,
               lead=0):
    """four variables' single-time-step files as byte strings, laid out by the writer's rules (``lead`` extra bytes
    in front of each), and the fields they hold"""
    fields = G.make_fields(seed, 1, Zf, Y, X, undef=undef, file_nan=file_nan)
    dt = np.dtype(">f4" if big else "<f4")
    marker = np.array([Y * X * 4], dtype=">i4" if big else "<i4").tobytes() if sequential else b""
    bufs = []
    for n in NAMES:
        vol = fields[n][0]
        vol = vol[::-1] if zrev else vol
        vol = vol[:, ::-1] if yrev else vol
        bufs.append(b"\xa5" * lead + b"".join(marker + np.ascontiguousarray(s).astype(dt).tobytes() + marker
                                              for s in vol))
    return bufs, fields


def to_dev(bufs):
    return [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV) for b in bufs]


def run_both(eng, bufs, shape, off, pitch, undef, big, **kw):
    want, want_mask = G.decode_buffers(bufs, shape, off, pitch, undef, big, **kw)
    got, mask = eng.ops.grads_decode(to_dev(bufs), shape=shape, level_offset=off, level_pitch=pitch, undef=undef,
                                     byteswap=big, want_tm_mask=True, **kw)
    assert got.dtype == torch.float32 and got.is_contiguous() and mask.dtype == torch.uint8
    assert_same(got, want)
    assert np.array_equal(mask.cpu().numpy(), want_mask) and tuple(mask.shape) == tuple(shape)
    return got, want


@pytest.mark.parametrize("big", [True, False])
@pytest.mark.parametrize("sequential", [False, True])
@pytest.mark.parametrize("yrev,zrev", [(False, False), (True, False), (False, True), (True, True)])
def test_layouts(eng, big, sequential, yrev, zrev):
    Z, Y, X = 5, 9, 24
    bufs, fields = file_bytes(0, Z, Y, X, big=big, sequential=sequential, yrev=yrev, zrev=zrev, file_nan=True)
    pitch = Y * X * 4 + (8 if sequential else 0)
    got, want = run_both(eng, bufs, (Z, Y, X), 4 if sequential else 0, pitch, UNDEF, big, yrev=yrev, zrev=zrev)
    # the restatement itself against the fields that were written
    full = np.stack([np.where(fields[n][0] == np.float32(UNDEF), np.float32(np.nan), fields[n][0]) for n in NAMES])
    assert_same(want, np.stack([full[0]] + [np.where(np.isnan(full[0]), np.float32(np.nan), f) for f in full[1:]]))
    assert np.isnan(want).any() and np.isnan(fields["tm"]).any()          # a NaN in the file stays NaN


@pytest.mark.parametrize("align", [True, False])
def test_align_nan_on_and_off(eng, align):
    Z, Y, X = 3, 6, 16
    bufs, _ = file_bytes(1, Z, Y, X, file_nan=True)
    got, want = run_both(eng, bufs, (Z, Y, X), 0, Y * X * 4, UNDEF, True, align_nan=align)
    tm_nan = np.isnan(want[0])
    assert np.isnan(want[1:][:, tm_nan]).all() == align and tm_nan.any() and not tm_nan.all()


def test_undef_not_exact_in_fp32_and_per_variable(eng):
    """-9.99e33 is not a float32: the file holds float32(-9.99e33) and must match; each variable has its own undef,
    and a value one ulp away from it is kept"""
    Z, Y, X = 2, 4, 8
    undefs = [UNDEF, -999.0, 1.0e20, 0.0]
    assert float(np.float32(UNDEF)) != UNDEF
    rng = np.random.default_rng(2)
    bufs = []
    for u in undefs:
        a = rng.standard_normal((Z, Y, X)).astype(np.float32)
        a[rng.random(a.shape) < 0.3] = np.float32(u)
        a[0, 0, 0] = np.nextafter(np.float32(u), np.float32(np.inf))
        a[0, 0, 1] = np.float32(UNDEF)                    # tm's undef inside the other variables is a value
        a[0, 0, 2] = np.float32(-0.0)
        bufs.append(a.astype(">f4").tobytes())
    got, want = run_both(eng, bufs, (Z, Y, X), 0, Y * X * 4, undefs, True, align_nan=False)
    assert not np.isnan(want[1:, 0, 0, 1]).any() and np.isnan(want[0, 0, 0, 1]) and not np.isnan(want[:, 0, 0, 0]).any()
    assert np.isnan(want[3, 0, 0, 2]) and not np.isnan(want[:3, 0, 0, 2]).any()   # undef 0.0 matches -0.0, as numpy's ==


@pytest.mark.parametrize("X,lead", [(23, 0), (22, 0), (1, 0), (24, 4), (24, 8), (24, 0)])
def test_ragged_x_and_broken_alignment(eng, X, lead):
    """X % 4 != 0, and X % 4 == 0 with a slab offset that is a multiple of 4 but not of 16: the 4-byte path"""
    Z, Y = 4, 7
    bufs, _ = file_bytes(3, Z, Y, X, lead=lead)
    run_both(eng, bufs, (Z, Y, X), lead, Y * X * 4, UNDEF, True)


def test_mixed_alignment_between_variables(eng):
    """offsets and pitches per variable; one misaligned variable sends the whole call to the 4-byte path"""
    Z, Y, X = 3, 5, 16
    bufs, _ = file_bytes(4, Z, Y, X)
    slab = Y * X * 4
    wide = [b"".join(b[z * slab:(z + 1) * slab] + b"\0" * 32 for z in range(Z)) for b in bufs[:2]]
    lead = [b"\0" * 12 + b for b in bufs[2:]]
    run_both(eng, wide + lead, (Z, Y, X), [0, 0, 12, 12], [slab + 32, slab + 32, slab, slab], UNDEF, True)
    run_both(eng, wide + bufs[2:], (Z, Y, X), [0, 0, 0, 0], [slab + 32, slab + 32, slab, slab], UNDEF, True)


@pytest.mark.parametrize("z0,n", [(0, 4), (3, 4), (6, 4), (0, 10)])
@pytest.mark.parametrize("zrev,sequential", [(False, False), (True, True)])
def test_level_window(eng, z0, n, zrev, sequential):
    """a window at the bottom, in the middle and at the top of a 10-level file, given as a byte range of the file"""
    Zf, Y, X = 10, 6, 12
    bufs, fields = file_bytes(5, Zf, Y, X, zrev=zrev, sequential=sequential)
    pitch = Y * X * 4 + (8 if sequential else 0)
    first = Zf - (z0 + n) if zrev else z0
    win = [b[first * pitch:(first + n) * pitch] for b in bufs]
    got, want = run_both(eng, win, (n, Y, X), 4 if sequential else 0, pitch, UNDEF, True, zrev=zrev)
    tm = fields["tm"][0, z0:z0 + n]
    assert_same(want[0], np.where(tm == np.float32(UNDEF), np.float32(np.nan), tm))


def test_full_shape_and_repeat(eng):
    """the reference's shape: a 40-level window from level 4 of a taller big-endian file, 400 x 400; two calls on the
    same buffers give the same bits"""
    Zf, Z, Y, X = 48, 40, 400, 400
    rng = np.random.default_rng(6)
    slab = Y * X * 4
    bufs = []
    for k in range(4):
        a = ((300.0 if k == 0 else 0.0) + 3 * rng.standard_normal((Zf, Y, X), dtype=np.float32))
        a[rng.random((Zf, Y, X), dtype=np.float32) < 0.1] = np.float32(UNDEF)
        bufs.append(a.astype(">f4").tobytes()[4 * slab:(4 + Z) * slab])
    dev = to_dev(bufs)
    kw = dict(shape=(Z, Y, X), level_offset=0, level_pitch=slab, undef=UNDEF, byteswap=True, want_tm_mask=True)
    a, ma = eng.ops.grads_decode(dev, **kw)
    b, mb = eng.ops.grads_decode(dev, **kw)
    want, want_mask = G.decode_buffers(bufs, (Z, Y, X), 0, slab, UNDEF, True)
    assert tuple(a.shape) == (4, 40, 400, 400)
    assert_same(a, want)
    assert np.array_equal(ma.cpu().numpy(), want_mask)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ma, mb)
    assert eng.ops.grads_decode(dev, **dict(kw, want_tm_mask=False)).view(torch.int32).equal(a.view(torch.int32))


def test_argument_errors(eng):
    ops, L = eng.ops, eng._lib
    Z, Y, X = 2, 4, 8
    bufs, _ = file_bytes(7, Z, Y, X)
    dev = to_dev(bufs)
    slab = Y * X * 4
    good = dict(shape=(Z, Y, X), level_offset=0, level_pitch=slab, undef=UNDEF, byteswap=True)
    ops.grads_decode(dev, **good)
    for over in (dict(level_offset=2), dict(level_pitch=slab - 4), dict(level_pitch=slab + 2), dict(shape=(3, Y, X)),
                 dict(shape=(0, Y, X)), dict(level_offset=4), dict(undef=[1.0, 2.0])):
        with pytest.raises(ValueError):
            ops.grads_decode(dev, **dict(good, **over))
    with pytest.raises(ValueError):
        ops.grads_decode(dev[:3], **good)
    with pytest.raises(ValueError):
        ops.grads_decode([d.view(torch.int8) for d in dev], **good)
    with pytest.raises(ValueError):
        ops.grads_decode([torch.cat([d, d])[::2] for d in dev], **good)          # not contiguous
    with pytest.raises(RuntimeError):
        ops.grads_decode([d.cpu() for d in dev], **good)

    # the C ABI itself: every bad argument is SR3D_E_ARG with a message, nothing is launched
    out = torch.empty(4, Z, Y, X, device=DEV)
    mask = torch.empty(Z, Y, X, dtype=torch.uint8, device=DEV)
    i4, d4, q4 = C.c_longlong * 4, C.c_double * 4, C.c_void_p * 4

    def call(srcs=None, null_params=False, null_table=False, **over):
        f = dict(X=X, Y=Y, Z=Z, byteswap=1, yrev=0, zrev=0, align_nan=1, level_offset=i4(0, 0, 0, 0),
                 level_pitch=i4(*[slab] * 4), src_bytes=i4(*[d.numel() for d in dev]), undef=d4(*[UNDEF] * 4),
                 out=out.data_ptr(), tm_is_nan=mask.data_ptr())
        f.update(over)
        table = q4(*(srcs if srcs is not None else [d.data_ptr() for d in dev]))
        return L.lib.sr3d_grads_decode(None if null_table else table,
                                       None if null_params else C.byref(L.GradsParams(**f)), L.stream_ptr())

    assert call() == 0
    ptrs = [d.data_ptr() for d in dev]
    bad = [dict(null_params=True), dict(null_table=True), dict(srcs=ptrs[:2] + [None] + ptrs[3:]), dict(out=None),
           dict(X=0), dict(Y=-1), dict(Z=0), dict(level_pitch=i4(slab, slab, slab - 4, slab)),
           dict(level_offset=i4(0, 2, 0, 0)), dict(level_offset=i4(0, 0, 0, 4)), dict(level_pitch=i4(slab + 2, *[slab] * 3)),
           dict(src_bytes=i4(*[Z * slab - 1] * 4)), dict(srcs=[ptrs[0] + 1] + ptrs[1:])]
    for over in bad:
        assert call(**over) == -1, over
        assert L.lib.sr3d_last_error()
    assert call(tm_is_nan=None) == 0
    torch.cuda.synchronize()
    assert_same(out, G.decode_buffers(bufs, (Z, Y, X), 0, slab, UNDEF, True)[0])


# ---------------------------------------------------------------- load_atmos_data(...).step(i)
def write_case(d, fields, lev=None, **kw):
    for n in NAMES:
        G.write_grads(d / f"atmos_0n_{n}.ctl", {n: fields[n]}, undef=UNDEF, lev=lev, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(sequential=True, zrev=True, yrev=True, big_endian=False, fileheader=16)])
def test_load_atmos_data_step(eng, tdm, tmp_path, kw):
    T, Zf, Y, X = 13, 12, 8, 8
    fields = G.make_fields(8, T, Zf, Y, X, file_nan=True)
    write_case(tmp_path, fields, **kw)
    data = tdm.load_atmos_data(tmp_path, data_shape=(3, 8, 8, 8))
    flags = {k: v for k, v in kw.items()}
    full = {n: G.read_full(tmp_path / f"atmos_0n_{n}.dat", [(n, Zf)], T, Y, X, undef=UNDEF,
                           **{"big_endian": True, **flags})[n] for n in NAMES}
    want = G.align({n: full[n][10:, 4:12] for n in NAMES})
    for i in range(3):
        got = data.step(i, DEV)
        assert got.device == DEV and tuple(got.shape) == (4, 8, 8, 8)
        assert_same(got, want[i])
    got, mask = data.step(1, DEV, want_tm_mask=True)
    assert np.array_equal(mask.cpu().numpy(), np.isnan(want[1][0]).astype(np.uint8))
    # a cut margin (read_array's margin > 0) is cut from the decoded planes
    from sr3d_amd.src.io_grads import read_array
    vs = [read_array(tmp_path, n, margin=2, nx=8, ny=8, min_index_height=2, max_index_height=6)
          for n in ("vl", "vp", "vr", "tm")]
    got = type(data)(*vs).step(2, DEV)
    assert_same(got, G.align({n: full[n][12, 2:6, 2:6, 2:6] for n in NAMES}))


# ---------------------------------------------------------------- the script end to end
def write_eletopoz(path, tz_yx, ez_yx):
    with open(path, "w") as f:
        f.write("i j Ez Tz Tzl\n")
        for y in range(tz_yx.shape[0]):
            for x in range(tz_yx.shape[1]):
                f.write(f"{x + 1} {y + 1} {ez_yx[y, x]:.4f} {tz_yx[y, x]:.4f} 0.0\n")


def run_script(args, timeout=300):
    r = subprocess.run([sys.executable, SCRIPT] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_script_grads_dir_equals_raw_dir(eng, tmp_path):
    """the same fields as big-endian GrADS (extra levels below the window, extra time steps before the kept period,
    undef inside the buildings) and as --raw_dir .npy steps: the two trees are equal bit for bit, masks included"""
    rng = np.random.default_rng(12)
    Zf, z_lo, Z, Y, X, m = 11, 3, 8, 48, 48, 8
    T, discarded = 7, 2                                     # 5 steps after the discarded period, 3 of them kept
    lev_file = 2.5 + 5.0 * np.arange(Zf)                    # level z_lo = 3 is 17.5 m
    levs = lev_file[z_lo:z_lo + Z]
    hr_tz = np.where(rng.random((Y, X)) < 0.15, rng.uniform(18.0, 40.0, (Y, X)), 10.0).round(2)
    hr_ez = np.full((Y, X), 15.0)
    lr_tz = rng.choice([10.0, 26.0, 31.0, 52.5], (Y // 4, X // 4))
    lr_ez = np.full((Y // 4, X // 4), 15.0)
    write_eletopoz(tmp_path / "hr.txt", hr_tz, hr_ez)
    write_eletopoz(tmp_path / "lr.txt", lr_tz, lr_ez)
    in_building = lev_file[:, None, None] < hr_tz[None]     # the LES writes undef inside the buildings
    fields = {}
    for k, n in enumerate(NAMES):
        a = ((300.0 if k == 0 else 0.0) + 3 * rng.standard_normal((T, Zf, Y, X))).astype(np.float32)
        a[:, in_building] = np.float32(UNDEF)
        if k == 0:
            a[:, :, m:m + 2, 20] = np.float32(UNDEF)        # tm undefined on whole columns outside any building
        fields[n] = a
    fields["vl"][discarded + 2, z_lo + 5, 30, 30] = np.float32(UNDEF)       # undef in one velocity component only
    grads = tmp_path / "2015-07-31T05:00:00" / "micro-meteorology" / "out" / "grads"
    grads.mkdir(parents=True)
    write_case(grads, fields, lev=lev_file, big_endian=True, tdef="05:00Z31jul2015 1mn")

    raw_dir = tmp_path / "raw"
    raw_dir.mkdir()
    for t in range(discarded, T):
        step = {n: np.where(fields[n][t, z_lo:z_lo + Z] == np.float32(UNDEF), np.float32(np.nan),
                            fields[n][t, z_lo:z_lo + Z]) for n in NAMES}
        np.save(raw_dir / f"20150731T05{t:02d}00.npy", G.align(step))

    common = ["--hr_building_path", tmp_path / "hr.txt", "--lr_building_path", tmp_path / "lr.txt", "--hr_margin", m]
    out_raw, out_grads, out_named = tmp_path / "from_raw", tmp_path / "from_grads", tmp_path / "from_named"
    run_script(["--raw_dir", raw_dir, "--out_dir", out_raw, "--z0", 17.5, "--dz", 5.0] + common)
    grads_args = ["--discarded_initial_period", discarded, "--min_index_height", z_lo, "--num_levels", Z] + common
    run_script(["--grads_dir", grads, "--out_dir", out_grads] + grads_args)

    names = sorted(str(p.relative_to(out_raw)) for p in out_raw.rglob("*") if p.is_file())
    kept = [f"20150731T05{t:02d}00" for t in (2, 4, 6)]
    assert names == sorted([f"10/20150731/{s}_{k}.npy" for s in kept for k in ("HR", "LR_x04")]
                           + ["10/hr_is_in_build.npy", "10/lr_is_in_build.npy"])
    assert names == sorted(str(p.relative_to(out_grads)) for p in out_grads.rglob("*") if p.is_file())
    for n in names:
        a, b = np.load(out_raw / n), np.load(out_grads / n)
        assert a.dtype == b.dtype and a.shape == b.shape, n
        if a.dtype == np.float32:
            assert_same(b, a)
            assert np.isnan(a).any() and (~np.isnan(a)).any()
        else:
            assert np.array_equal(a, b), n

    # rerunning on the finished tree writes nothing
    before = {p: p.stat().st_mtime_ns for p in out_grads.rglob("*.npy")}
    run_script(["--grads_dir", grads, "--out_dir", out_grads] + grads_args)
    assert {p: p.stat().st_mtime_ns for p in out_grads.rglob("*.npy")} == before

    # --root_result_dir + --target_datetime name the same directory; a missing LR file is made again, alone
    run_script(["--root_result_dir", tmp_path, "--target_datetime", "2015-07-31T05:00:00", "--out_dir", out_named]
               + grads_args)
    assert names == sorted(str(p.relative_to(out_named)) for p in out_named.rglob("*") if p.is_file())
    victim = out_named / "10" / "20150731" / f"{kept[1]}_LR_x04.npy"
    victim.unlink()
    before = {p: p.stat().st_mtime_ns for p in out_named.rglob("*.npy")}
    run_script(["--grads_dir", grads, "--out_dir", out_named] + grads_args)
    assert {p: p.stat().st_mtime_ns for p in out_named.rglob("*.npy") if p != victim} == before
    assert_same(np.load(victim), np.load(out_raw / "10" / "20150731" / f"{kept[1]}_LR_x04.npy"))
    for bad in (["--grads_dir", grads, "--raw_dir", raw_dir], ["--root_result_dir", tmp_path]):
        r = subprocess.run([sys.executable, SCRIPT, "--out_dir", out_named] + [str(a) for a in bad + common],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2, r.stderr[-500:]
