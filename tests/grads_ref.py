"""GrADS in numpy: a writer of synthetic descriptor + data pairs and the decode restated, for the tests of
src/io_grads.py and ops.grads_decode (tests/test_grads_host.py, tests/test_gpu_grads.py).

The writer lays the file out from the GrADS descriptor grammar: ``fileheader`` bytes, then per time step, per variable
in ``vars`` order, per level one (y, x) slab of 4-byte floats; with ``options sequential`` each slab is a Fortran
record (its byte count as a 4-byte integer before and after it); ``yrev`` / ``zrev`` store rows / levels from the last
to the first.  The decode is ``np.fromfile`` with an explicit dtype, a reshape, ``== np.float32(undef)`` -> NaN, the
window, the flips and the NaN alignment to tm -- what the reference's read_xarray + align_nan_grids give.
"""
import os

import numpy as np

MONTHS = "jan feb mar apr may jun jul aug sep oct nov dec".split()


def tdef_start(t, form="hh:mm"):
    """a datetime as ``hh:mmZddmmmyyyy`` ("hh:mm"), ``hhZddmmmyyyy`` ("hh") or ``ddmmmyyyy`` ("date")"""
    date = f"{t.day:02d}{MONTHS[t.month - 1]}{t.year:04d}"
    return {"hh:mm": f"{t.hour:02d}:{t.minute:02d}Z{date}", "hh": f"{t.hour:02d}Z{date}", "date": date}[form]


def write_grads(ctl_path, fields, *, undef=-9.99e33, big_endian=True, sequential=False, yrev=False, zrev=False,
                fileheader=0, lev=None, lat=None, lon=None, zdef_levels_per_line=None, tdef="05:00Z31jul2015 1mn",
                endian_option=None, dset=None, upper=False, extra_lines=()):
    """``fields``: {name: (T, Z_v, Y, X) float32 with the undef value already in place}, in record order; every
    variable shares T, Y, X; zdef has max Z_v levels.  Writes <ctl_path> and its data file (``dset``: the dset record,
    default ``^<stem>.dat``).  ``lev`` etc.: coordinates (default lev 17.5 + 5 k from k = -4, lat / lon linear);
    ``zdef_levels_per_line``: write zdef as ``levels`` continued over lines of that many values, else linear when
    the spacing allows.  Returns the data file's path."""
    ctl_path = os.fspath(ctl_path)
    names = list(fields)
    T, _, Y, X = fields[names[0]].shape
    Z = max(f.shape[1] for f in fields.values())
    lev = -2.5 + 5.0 * np.arange(Z) if lev is None else np.asarray(lev, float)
    dt = np.dtype(">f4" if big_endian else "<f4")
    dset = f"^{os.path.splitext(os.path.basename(ctl_path))[0]}.dat" if dset is None else dset
    data_path = os.path.join(os.path.dirname(ctl_path), dset[1:]) if dset.startswith("^") else dset
    marker = np.array([Y * X * 4], dtype=">i4" if big_endian else "<i4").tobytes()
    with open(data_path, "wb") as f:
        f.write(bytes((7 * k + 1) % 256 for k in range(fileheader)))
        for t in range(T):
            for n in names:
                vol = np.asarray(fields[n][t], np.float32)
                vol = vol[::-1] if zrev else vol
                vol = vol[:, ::-1] if yrev else vol
                for slab in vol:
                    if sequential:
                        f.write(marker)
                    f.write(np.ascontiguousarray(slab).astype(dt).tobytes())
                    if sequential:
                        f.write(marker)
    opts = [endian_option if endian_option is not None else ("big_endian" if big_endian else "little_endian")]
    opts += [o for o, on in (("sequential", sequential), ("yrev", yrev), ("zrev", zrev)) if on]
    k = (lambda s: s.upper()) if upper else (lambda s: s)
    out = [f"{k('dset')} {dset}", f"{k('title')} synthetic LES output", f"{k('undef')} {undef!r}"]
    if fileheader:
        out.append(f"{k('fileheader')} {fileheader}")
    out.append(f"{k('options')} " + " ".join(k(o) for o in opts if o))
    lon = 139.0 + 0.001 * np.arange(X) if lon is None else np.asarray(lon, float)
    lat = 35.0 + 0.001 * np.arange(Y) if lat is None else np.asarray(lat, float)
    out.append(f"{k('xdef')} {X} {k('linear')} {float(lon[0])!r} {0.001 if X == 1 else float(lon[1] - lon[0])!r}")
    out.append(f"{k('ydef')} {Y} {k('levels')} " + " ".join(repr(float(v)) for v in lat))
    if zdef_levels_per_line:
        rows = [lev[i:i + zdef_levels_per_line] for i in range(0, Z, zdef_levels_per_line)]
        out.append(f"{k('zdef')} {Z} {k('levels')} " + " ".join(repr(float(v)) for v in rows[0]))
        out += ["  " + " ".join(repr(float(v)) for v in r) for r in rows[1:]]
    else:
        out.append(f"{k('zdef')} {Z} {k('linear')} {float(lev[0])!r} {5.0 if Z == 1 else float(lev[1] - lev[0])!r}")
    out.append(f"{k('tdef')} {T} {k('linear')} {tdef}")
    out += list(extra_lines)
    out.append(f"{k('vars')} {len(names)}")
    out += [f"{n} {0 if fields[n].shape[1] == 1 else fields[n].shape[1]} 99 the field {n}" for n in names]
    out.append(k("endvars"))
    with open(ctl_path, "w") as f:
        f.write("* a comment line\n" + "\n".join(out) + "\n")
    return data_path


def read_full(data_path, fields_levels, T, Y, X, *, undef, big_endian=True, sequential=False, yrev=False, zrev=False,
              fileheader=0):
    """the whole data file restated: {name: (T, Z_v, Y, X) float32 with NaN for the undef}; ``fields_levels``:
    [(name, Z_v)] in record order"""
    dt = np.dtype(">f4" if big_endian else "<f4")
    words = np.fromfile(data_path, dtype=dt, offset=fileheader)
    pad = 2 if sequential else 0                       # the two record markers, one word each
    total = sum(z for _, z in fields_levels)
    rec = words.reshape(T, total, Y * X + pad)
    out, k = {}, 0
    for name, z in fields_levels:
        a = rec[:, k:k + z, pad // 2:pad // 2 + Y * X].reshape(T, z, Y, X).astype(np.float32)
        k += z
        a = np.where(a == np.float32(undef), np.float32(np.nan), a)
        a = a[:, ::-1] if zrev else a
        a = a[:, :, ::-1] if yrev else a
        out[name] = np.ascontiguousarray(a)
    return out


def align(fields, order=("tm", "vl", "vp", "vr")):
    """(…, 4, Z, Y, X) stacked in ``order`` with the reference's align_nan_grids: NaN wherever tm is NaN"""
    tm = fields[order[0]]
    return np.stack([tm] + [np.where(np.isnan(tm), np.float32(np.nan), fields[n]) for n in order[1:]], axis=-4)


def decode_buffers(buffers, shape, level_offset, level_pitch, undef, byteswap, yrev=False, zrev=False,
                   align_nan=True):
    """ops.grads_decode restated on host byte strings: four buffers -> ((4, Z, Y, X) float32, isnan(tm) uint8)"""
    Z, Y, X = shape
    dt = np.dtype(">f4" if byteswap else "<f4")
    undefs = list(undef) if isinstance(undef, (list, tuple)) else [undef] * 4
    offs = list(level_offset) if isinstance(level_offset, (list, tuple)) else [level_offset] * 4
    pitches = list(level_pitch) if isinstance(level_pitch, (list, tuple)) else [level_pitch] * 4
    out = []
    for b, u, o, p in zip(buffers, undefs, offs, pitches):
        b = np.frombuffer(bytes(b), dtype=np.uint8)
        slabs = np.stack([np.frombuffer(b[o + z * p:o + z * p + Y * X * 4].tobytes(), dtype=dt) for z in range(Z)])
        a = slabs.reshape(Z, Y, X).astype(np.float32)
        with np.errstate(over="ignore"):
            a = np.where(a == np.float32(u), np.float32(np.nan), a)
        a = a[::-1] if zrev else a
        a = a[:, ::-1] if yrev else a
        out.append(a)
    if align_nan:
        out = [out[0]] + [np.where(np.isnan(out[0]), np.float32(np.nan), a) for a in out[1:]]
    return np.ascontiguousarray(np.stack(out)), np.isnan(out[0]).astype(np.uint8)


def make_fields(seed, T, Z, Y, X, *, undef=-9.99e33, names=("tm", "vl", "vp", "vr"), undef_frac=0.1, file_nan=False,
                levels=None):
    """random fields with the undef value (as float32) at random cells of every variable, independently; with
    ``file_nan`` a few true NaNs as well; ``levels``: {name: Z_v} overrides"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, n in enumerate(names):
        z = (levels or {}).get(n, Z)
        a = (300.0 if k == 0 else 0.0) + 3 * rng.standard_normal((T, z, Y, X))
        a = a.astype(np.float32)
        a[rng.random(a.shape) < undef_frac] = np.float32(undef)
        if file_nan:
            a[rng.random(a.shape) < 0.03] = np.nan
        out[n] = a
    return out
