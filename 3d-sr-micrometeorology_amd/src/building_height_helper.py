"""Building and ground heights of the simulation domain (reference src/building_height_helper.py).

``read_building_height`` parses an ``EleTopoZ`` text file -- a header line, then whitespace-separated rows
``i j Ez Tz Tzl`` (x index, y index, ground height, building-top height, ...) -- into the (i, j) = (x, y) grid of one
column, as the reference's ``pandas.pivot_table(..., aggfunc="max")`` does: duplicate (i, j) rows keep their maximum,
a missing pair is NaN, and a row or column whose values are all NaN is dropped.  ``calc_is_in_building`` marks the
levels below each building top.  Both run once per dataset, on the host.
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
