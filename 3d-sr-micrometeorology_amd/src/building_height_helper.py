"""Building and ground heights of the simulation domain (reference src/building_height_helper.py).

``read_building_height`` parses an ``EleTopoZ`` text file -- a header line, then whitespace-separated rows
``i j Ez Tz Tzl`` (x index, y index, ground height, building-top height, ...) -- into the (i, j) = (x, y) grid of one
column, as the reference's ``pandas.pivot_table(..., aggfunc="max")`` does: duplicate (i, j) rows keep their maximum,
a missing pair is NaN, and a row or column whose values are all NaN is dropped.  ``calc_is_in_building`` marks the
levels below each building top; ``make_resized_lr_tz`` and ``calc_ave_pooling_weights`` serve the LR data maker
(training_data_maker).  All run once per dataset, on the host, without OpenCV.
"""
import numpy as np
import pandas as pd

COLUMNS = ["i", "j", "Ez", "Tz", "Tzl"]


def read_building_height(building_path: str, target_col: str, margin: int = 20) -> np.ndarray:
    """the ``target_col`` column of the file as an (i, j) array, ``margin`` cells cut from every lateral edge"""
    with open(building_path, "r") as f:
        rows = [line.split() for line in f.readlines()[1:]]   # the first line is a header
    df = pd.DataFrame([dict(zip(COLUMNS, r)) for r in rows if r], columns=COLUMNS)
    for col in COLUMNS:
        df[col] = df[col].astype(int if col in ("i", "j") else float)
    grid = pd.pivot_table(data=df[["i", "j", target_col]], values=target_col, index="i", columns="j",
                          aggfunc="max").values
    return grid if margin == 0 else grid[margin:-margin, margin:-margin]


def calc_is_in_building(tz: np.ndarray, ez: np.ndarray, actual_levs: np.ndarray) -> np.ndarray:
    """(z, y, x) float64, 1 below the building top: for each column with tz > ez (a building: heights from the sea
    surface), the levels before the first one with ``actual_levs >= tz``.  As in the reference, ``argmin`` of
    ``actual_levs < tz`` is 0 when every level is below the top or when tz is NaN, so such a column marks nothing."""
    assert tz.shape == ez.shape
    assert len(tz.shape) == 2  # y and x
    assert len(actual_levs.shape) == 1  # z
    levs = np.asarray(actual_levs)
    top = (levs[:, None, None] < tz[None]).argmin(axis=0)          # (y, x): index of the first level >= tz
    building = ~(tz <= ez)                                          # NaN compares False: not skipped
    marked = np.arange(len(levs))[:, None, None] < np.where(building, top, 0)[None]
    return marked.astype(np.float64)


def make_resized_lr_tz(lr_tz: np.ndarray, lr_ez: np.ndarray, hr_is_in_build: np.ndarray, actual_hr_levs) -> np.ndarray:
    """the LR buildings on the HR grid: (channel, z, y, x) float64, broadcast over hr_is_in_build's channels.  The
    reference resizes with cv2.resize(..., dsize=hr_is_in_build.shape[-2:], INTER_NEAREST); cv2 reads dsize as
    (width, height), so only a square grid means what it says, and at an integer factor f its nearest neighbour of HR
    cell i is LR cell i // f.  Both are asserted here; then calc_is_in_building at the HR levels."""
    assert lr_tz.ndim == lr_ez.ndim == 2  # y and x
    assert hr_is_in_build.ndim == 4  # channel, z, y, x
    assert lr_tz.shape == lr_ez.shape
    Y, X = hr_is_in_build.shape[-2:]
    assert Y == X and lr_tz.shape[0] == lr_tz.shape[1], "cv2.resize(dsize=(Y, X)) needs a square grid"
    assert Y % lr_tz.shape[0] == 0, "the HR grid must be an integer multiple of the LR grid"
    f = Y // lr_tz.shape[0]
    resized_lr_tz = np.repeat(np.repeat(np.asarray(lr_tz), f, axis=0), f, axis=1)
    resized_lr_ez = np.repeat(np.repeat(np.asarray(lr_ez), f, axis=0), f, axis=1)
    resized_lr_is_in_build = calc_is_in_building(tz=resized_lr_tz, ez=resized_lr_ez,
                                                 actual_levs=np.asarray(actual_hr_levs))
    return np.broadcast_to(resized_lr_is_in_build[None, ...], shape=hr_is_in_build.shape)


def calc_ave_pooling_weights(lr_is_in_build: np.ndarray, lev_window_width: int, lat_window_width: int,
                             lon_window_width: int) -> np.ndarray:
    """the reference's masked average-pooling weights of every (lev, lat, lon) window: (1 - m) / sum(1 - m), NaN
    where the window is fully masked; shape (Z-w+1, Y-w+1, X-w+1, w, w, w) float64.  Kept for the reference's
    interface: the LR data does not depend on it (training_data_maker, module docstring)."""
    assert lr_is_in_build.ndim == 3  # z, y, x
    free = np.where(np.asarray(lr_is_in_build) == 1, 0.0, 1.0)
    win = np.lib.stride_tricks.sliding_window_view(
        free, (lev_window_width, lat_window_width, lon_window_width), axis=(0, 1, 2))
    count = win.sum(axis=(-3, -2, -1))[..., None, None, None]
    with np.errstate(invalid="ignore"):   # 0 / 0 of fully masked windows: NaN, as in the reference
        return np.where(count != 0, win / count, np.nan)
