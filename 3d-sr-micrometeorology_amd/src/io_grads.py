"""The LES's GrADS output without xgrads / xarray / dask (reference datascience/src/io_grads.py).

A GrADS data set is a text descriptor (``.ctl``) and a flat binary file of 4-byte floats: per time step, per variable,
per level one (y, x) slab.  ``parse_ctl`` reads the descriptor, written from the GrADS descriptor grammar;
``GradsVariable`` is a lazy view of one variable (a read-only ``np.memmap`` plus a time / level / margin selection)
that can return the byte range of one time step's level window -- what ``ops.grads_decode`` turns into fields on the
GPU -- or decode it on the host with numpy.  ``read_array`` is the reference's ``read_xarray`` with its file-name,
margin, time and level rules.

Supported: dset (``^`` = the descriptor's directory), undef, title, fileheader, options big_endian / little_endian /
byteswapped / sequential / yrev / zrev, xdef / ydef / zdef linear or levels (continued over lines), linear tdef with
mn / hr / dy increments, vars .. endvars with one or several variables per file.  Everything else raises
NotImplementedError naming the keyword.  The parser is pinned to the grammar and to the numpy restatement in
tests/grads_ref.py, not to xgrads or to a real MSSG descriptor: parity with xgrads is unpinned.
"""
from __future__ import annotations

import datetime
import os
import pathlib
import re
import sys
import typing
from logging import getLogger

import numpy as np

logger = getLogger()

_MONTHS = {m: i + 1 for i, m in enumerate("jan feb mar apr may jun jul aug sep oct nov dec".split())}
_OPTIONS = {"big_endian", "little_endian", "byteswapped", "sequential", "yrev", "zrev"}
_IGNORED = {"title"}
_TIME = re.compile(r"^(?:(\d{1,2})(?::(\d{2}))?z)?(\d{1,2})([a-z]{3})(\d{4})$")
_INCR = re.compile(r"^(\d+)(mn|hr|dy|mo|yr)$")


def get_grads_dir_micro_meteorology(root_dir: pathlib.Path, dt: datetime.datetime) -> pathlib.Path:
    str_dt = f"{dt:%Y-%m-%dT%H:%M:%S}"
    return pathlib.Path(root_dir) / str_dt / "micro-meteorology" / "out" / "grads"


def get_grads_dir_meteorology(root_dir: pathlib.Path, dt: datetime.datetime, offset_hours: int = 5) -> pathlib.Path:
    _dt = dt - datetime.timedelta(hours=offset_hours)
    str_dt = f"{dt:%Y-%m-%dT%H:%M:%S}"
    case_dir = f"1km_300m_100m-tokyo-many-grids_{_dt:%Y%m%d}_{_dt:%H}_{_dt:%M}UTC.000"
    return pathlib.Path(root_dir) / str_dt / "mssg-auto" / "MSSG" / case_dir / "out" / "grads"


# ---------------------------------------------------------------- the descriptor
class GradsDescriptor(typing.NamedTuple):
    path: str                     # the .ctl file
    dset: str                     # the data file, resolved
    undef: float
    fileheader: int               # bytes before the first record
    byteswap: bool                # the file's byte order is not this host's
    sequential: bool              # every (y, x) slab is a Fortran record: 4-byte marker, data, 4-byte marker
    yrev: bool
    zrev: bool
    lon: np.ndarray               # (X) float64
    lat: np.ndarray               # (Y)
    lev: np.ndarray               # (Z)
    time: np.ndarray              # (T) datetime64[s]
    variables: typing.Tuple[typing.Tuple[str, int], ...]   # (name, levels in the file), in record order

    @property
    def slab_bytes(self) -> int:
        """bytes from one (y, x) slab to the next"""
        return len(self.lat) * len(self.lon) * 4 + (8 if self.sequential else 0)

    @property
    def step_bytes(self) -> int:
        """bytes of one time step: every level of every variable"""
        return sum(n for _, n in self.variables) * self.slab_bytes

    def variable_offset(self, name: str) -> typing.Tuple[int, int]:
        """(bytes from the start of a time step to the variable's first slab, its levels in the file)"""
        before = 0
        for n, levels in self.variables:
            if n.lower() == name.lower():
                return before * self.slab_bytes, levels
            before += levels
        raise KeyError(f"{self.path}: no variable {name!r} (it has {[n for n, _ in self.variables]})")


def _parse_time(start: str, path: str) -> np.datetime64:
    m = _TIME.match(start.lower())
    if not m or m.group(4) not in _MONTHS:
        raise ValueError(f"{path}: tdef start {start!r} is not hh:mmZddmmmyyyy, hhZddmmmyyyy or ddmmmyyyy")
    hh, mn, dd, mon, yy = m.groups()
    t = datetime.datetime(int(yy), _MONTHS[mon], int(dd), int(hh or 0), int(mn or 0))
    return np.datetime64(t, "s")


def _axis(words, more, key: str, path: str) -> np.ndarray:
    """``n linear start step`` or ``n levels v0 v1 ...`` (``more``: an iterator over the following lines)"""
    if len(words) < 2:
        raise ValueError(f"{path}: {key}: count and mapping expected")
    n, kind = int(words[0]), words[1].lower()
    if n <= 0:
        raise ValueError(f"{path}: {key}: {n} points")
    if kind == "linear":
        if len(words) < 4:
            raise ValueError(f"{path}: {key} linear: start and step expected")
        return float(words[2]) + float(words[3]) * np.arange(n, dtype=np.float64)
    if kind == "levels":
        vals = [float(w) for w in words[2:]]
        while len(vals) < n:
            line = next(more, None)
            if line is None:
                raise ValueError(f"{path}: {key} levels: {len(vals)} of {n} values")
            vals += [float(w) for w in line.split()]
        if len(vals) != n:
            raise ValueError(f"{path}: {key} levels: {len(vals)} values for {n} points")
        return np.asarray(vals, dtype=np.float64)
    raise NotImplementedError(f"{path}: {key} {kind}: only linear and levels are implemented")


def parse_ctl(path) -> GradsDescriptor:
    """a GrADS descriptor file -> GradsDescriptor; checks the data file's size against it"""
    path = os.fspath(path)
    with open(path) as f:
        lines = (ln.strip() for ln in f.read().splitlines())
    lines = iter([ln for ln in lines if ln and not ln.startswith("*")])
    dset = undef = lon = lat = lev = time = variables = None
    fileheader, options = 0, set()
    for line in lines:
        words = line.split()
        key, args = words[0].lower(), words[1:]
        if key in _IGNORED:
            continue
        if key == "dset":
            name = line.split(None, 1)[1].strip() if args else ""
            if "%" in name:
                raise NotImplementedError(f"{path}: dset with % substitution (templates) is not implemented")
            dset = os.path.join(os.path.dirname(path), name[1:]) if name.startswith("^") else name
        elif key == "undef":
            undef = float(args[0])
        elif key == "fileheader":
            fileheader = int(args[0])
        elif key == "options":
            for o in (a.lower() for a in args):
                if o not in _OPTIONS:
                    raise NotImplementedError(f"{path}: options {o} is not implemented")
                options.add(o)
        elif key in ("xdef", "ydef", "zdef"):
            ax = _axis(args, lines, key, path)
            lon, lat, lev = (ax if key == "xdef" else lon), (ax if key == "ydef" else lat), (ax if key == "zdef" else lev)
        elif key == "tdef":
            if len(args) < 4 or args[1].lower() != "linear":
                raise NotImplementedError(f"{path}: tdef {' '.join(args[1:2])}: only linear tdef is implemented")
            m = _INCR.match(args[3].lower())
            if not m:
                raise ValueError(f"{path}: tdef increment {args[3]!r}")
            if m.group(2) in ("mo", "yr"):
                raise NotImplementedError(f"{path}: tdef increment {m.group(2)} is not implemented")
            secs = int(m.group(1)) * {"mn": 60, "hr": 3600, "dy": 86400}[m.group(2)]
            time = _parse_time(args[2], path) + np.arange(int(args[0])) * np.timedelta64(secs, "s")
        elif key == "vars":
            variables = []
            for _ in range(int(args[0])):
                vw = next(lines, "").split()
                if len(vw) < 3 or vw[0].lower() == "endvars":
                    raise ValueError(f"{path}: vars {args[0]}: {len(variables)} variable records")
                if "," in vw[1] or "," in vw[2] or vw[2].startswith("-"):
                    raise NotImplementedError(f"{path}: variable {vw[0]}: units {vw[2]} / levels {vw[1]} (special "
                                              "data layouts) are not implemented")
                variables.append((vw[0].split("=>")[-1], max(int(vw[1]), 1)))   # 0 levels: one level
            if next(lines, "").lower().split()[:1] != ["endvars"]:
                raise ValueError(f"{path}: endvars expected after {args[0]} variable records")
        else:
            raise NotImplementedError(f"{path}: {key} is not implemented")
    missing = [k for k, v in (("dset", dset), ("undef", undef), ("xdef", lon), ("ydef", lat), ("zdef", lev),
                              ("tdef", time), ("vars", variables)) if v is None]
    if missing:
        raise ValueError(f"{path}: no {', '.join(missing)} record")
    if sum(o in options for o in ("big_endian", "little_endian", "byteswapped")) > 1:
        raise ValueError(f"{path}: options name more than one byte order")
    big = "big_endian" in options or ("byteswapped" in options and sys.byteorder == "little")
    little = "little_endian" in options or ("byteswapped" in options and sys.byteorder == "big")
    file_order = "big" if big else "little" if little else sys.byteorder
    for name, levels in variables:
        if levels > len(lev):
            raise ValueError(f"{path}: variable {name} has {levels} levels, zdef {len(lev)}")
    d = GradsDescriptor(path, dset, undef, fileheader, file_order != sys.byteorder, "sequential" in options,
                        "yrev" in options, "zrev" in options, lon, lat, lev, time, tuple(variables))
    want, have = fileheader + len(time) * d.step_bytes, os.path.getsize(dset)
    if want != have:
        raise ValueError(f"{path}: the descriptor describes {want} bytes, {dset} holds {have}")
    return d


# ---------------------------------------------------------------- one variable, lazily
class GradsVariable:
    """one variable of a GrADS data set: (time, lev, lat, lon) float32 with the undef as NaN, never read as a whole.
    ``lev`` / ``lat`` / ``lon`` / ``time`` are the coordinates of the current selection; ``isel`` narrows it.
    A variable with fewer levels than zdef has the first of them."""

    def __init__(self, ctl: GradsDescriptor, name: str, memmap: np.memmap = None, t=None, z=None, y=None, x=None):
        self.ctl, self.name = ctl, name
        self._var_offset, self.file_levels = ctl.variable_offset(name)
        self.memmap = np.memmap(ctl.dset, dtype=np.uint8, mode="r") if memmap is None else memmap
        full = (len(ctl.time), self.file_levels, len(ctl.lat), len(ctl.lon))
        self._sel = tuple(range(n) if s is None else s for n, s in zip(full, (t, z, y, x)))

    undef = property(lambda self: self.ctl.undef)
    byteswap = property(lambda self: self.ctl.byteswap)
    sequential = property(lambda self: self.ctl.sequential)
    yrev = property(lambda self: self.ctl.yrev)
    zrev = property(lambda self: self.ctl.zrev)
    time = property(lambda self: self.ctl.time[self._sel[0].start:self._sel[0].stop])
    lev = property(lambda self: self.ctl.lev[self._sel[1].start:self._sel[1].stop])
    lat = property(lambda self: self.ctl.lat[self._sel[2].start:self._sel[2].stop])
    lon = property(lambda self: self.ctl.lon[self._sel[3].start:self._sel[3].stop])
    shape = property(lambda self: tuple(len(s) for s in self._sel))
    dims = ("time", "lev", "lat", "lon")

    def isel(self, time=None, lev=None, lat=None, lon=None) -> "GradsVariable":
        """a narrower view; each argument is a unit-step slice of the current selection"""
        sel = []
        for cur, s, dim in zip(self._sel, (time, lev, lat, lon), self.dims):
            new = cur if s is None else cur[s]
            if new.step != 1:
                raise ValueError(f"GradsVariable.isel: {dim} must be a unit-step slice (got {s})")
            sel.append(new)
        return GradsVariable(self.ctl, self.name, self.memmap, *sel)

    # ---- layout of the selection in the file
    @property
    def full_plane_shape(self) -> typing.Tuple[int, int]:
        return len(self.ctl.lat), len(self.ctl.lon)

    @property
    def window(self) -> typing.Tuple[slice, slice]:
        """the (lat, lon) selection inside a decoded full plane"""
        return (slice(self._sel[2].start, self._sel[2].stop), slice(self._sel[3].start, self._sel[3].stop))

    @property
    def level_offset(self) -> int:
        """bytes from the start of step_range's range to the first value of its first slab"""
        return 4 if self.sequential else 0

    @property
    def level_pitch(self) -> int:
        return self.ctl.slab_bytes

    def step_range(self, i: int) -> typing.Tuple[int, int]:
        """(first byte, one past the last byte) in the data file of the selected levels of the i-th selected time
        step: whole slabs, markers included"""
        t = self._sel[0][i]
        z = self._sel[1]
        n = len(z)
        first = self.file_levels - z.stop if self.zrev else z.start     # zrev: the file's first level is the top
        begin = self.ctl.fileheader + t * self.ctl.step_bytes + self._var_offset + first * self.level_pitch
        return begin, begin + n * self.level_pitch

    def step_bytes(self, i: int) -> np.ndarray:
        """the raw bytes of step_range(i): a uint8 view of the memmap (no copy)"""
        a, b = self.step_range(i)
        return self.memmap[a:b]

    # ---- host decode (numpy): what ops.grads_decode computes for this variable alone
    def step_numpy(self, i: int) -> np.ndarray:
        """(lev, lat, lon) float32 of the i-th selected time step, the undef as NaN"""
        Y, X = self.full_plane_shape
        n = len(self._sel[1])
        raw = np.asarray(self.step_bytes(i)).reshape(n, self.level_pitch)
        raw = raw[:, self.level_offset:self.level_offset + Y * X * 4]
        a = np.ascontiguousarray(raw).view(np.dtype(np.float32).newbyteorder("S" if self.byteswap else "="))
        a = a.astype(np.float32).reshape(n, Y, X)
        a = np.where(a == np.float32(self.undef), np.float32(np.nan), a)
        if self.zrev:
            a = a[::-1]
        if self.yrev:
            a = a[:, ::-1]
        return np.ascontiguousarray(a[(slice(None),) + self.window])

    @property
    def values(self) -> np.ndarray:
        """the whole selection (time, lev, lat, lon) on the host"""
        return np.stack([self.step_numpy(i) for i in range(len(self._sel[0]))])

    def __repr__(self):
        return f"GradsVariable({self.name!r}, shape={self.shape}, file={self.ctl.dset!r})"


def read_array(dir_path: pathlib.Path, variable_name: str, margin: int = 20, nx: int = 400, ny: int = 400,
               discarded_initial_period: int = 10, min_index_height: int = 0, max_index_height: int = None,
               nest_level: str = "0n") -> GradsVariable:
    """the reference's read_xarray without xarray: ``atmos_<nest_level>_<variable_name>.ctl`` of ``dir_path`` as a
    lazy GradsVariable with the margin cut (lon / lat indices margin .. nx - margin), the first
    ``discarded_initial_period`` time steps dropped and, if ``max_index_height`` is given, the levels
    [min_index_height, max_index_height)"""
    if min_index_height != 0 and max_index_height is None:
        logger.warning("min_index_height is not used.")
    ctl = parse_ctl(pathlib.Path(dir_path) / f"atmos_{nest_level}_{variable_name}.ctl")
    assert isinstance(ctl.undef, float)
    logger.debug(f"{variable_name}: undef = {ctl.undef}")
    da = GradsVariable(ctl, variable_name)
    if margin > 0:
        _, _, Y, X = da.shape
        if nx - margin > X or ny - margin > Y or 2 * margin >= min(nx, ny):
            raise IndexError(f"margin {margin} with nx, ny = {nx}, {ny}: outside the grid of {(Y, X)}")
        da = da.isel(lon=slice(margin, nx - margin), lat=slice(margin, ny - margin))
    da = da.isel(time=slice(discarded_initial_period, None))
    if max_index_height is not None:
        da = da.isel(lev=slice(min_index_height, max_index_height))
        if len(da.lev):
            logger.debug(f"{variable_name}, height range = {da.lev[0]} - {da.lev[-1]} m")
    return da


# ---------------------------------------------------------------- the reference's array helpers
def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def align_nan_grids(target_da, source_da):
    """``target_da`` with NaN wherever ``source_da`` is NaN (numpy arrays or torch tensors)"""
    if _is_tensor(target_da):
        import torch
        return target_da.masked_fill(torch.isnan(source_da), float("nan"))
    target = np.asarray(target_da)
    return np.where(np.isnan(np.asarray(source_da)), np.asarray(np.nan, dtype=target.dtype), target)


def calc_std_fields(ave_1st_moment, ave_2nd_moment, names: typing.Tuple[str, str] = None):
    """sqrt(<x^2> - <x>^2), 0 where that is not positive (a negative variance included), NaN where <x> is NaN.
    ``names`` (first-moment name, second-moment name), if given, must share the two-letter header, as the reference
    asserts of its DataArrays' names."""
    if names is not None:
        assert names[0] == names[1][:2], "Variable name header is different"
    if _is_tensor(ave_1st_moment):
        import torch
        stds = torch.sqrt(ave_2nd_moment - ave_1st_moment ** 2)
        stds = torch.where(stds > 0.0, stds, torch.zeros_like(stds))
        return stds.masked_fill(torch.isnan(ave_1st_moment), float("nan"))
    m1, m2 = np.asarray(ave_1st_moment), np.asarray(ave_2nd_moment)
    with np.errstate(invalid="ignore"):
        stds = np.sqrt(m2 - m1 ** 2)
    stds = np.where(stds > 0.0, stds, np.asarray(0, dtype=stds.dtype))
    return np.where(np.isnan(m1), np.asarray(np.nan, dtype=stds.dtype), stds)
