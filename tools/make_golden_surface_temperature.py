"""Generate tests/golden/surface_temperature.npz and tests/golden/EleTopoZ_fixture.txt (build machine only).

Run from anywhere:   python tools/make_golden_surface_temperature.py
Like tools/make_golden_equivariance.py it runs the reference's own code on seeded inputs: it imports the reference's
pytorch/src/building_height_helper.py (read-only, no bytecode written) and executes, from the reference's
make_2m_temperature notebook, the cell that defines HEIGHT_LEVELS and the cell that defines read_building_height and
infer_2m_height_temperature.  Only data is stored:
  EleTopoZ_fixture.txt   a synthetic EleTopoZ file: header line, rows "i j Ez Tz Tzl" on a 17 x 13 (i, j) grid,
                         some (i, j) pairs repeated with other values (the pivot keeps the maximum), one pair missing
                         (NaN).  Tz covers every branch of the extrapolation: below H[0], exactly on a level (H[0] and
                         H[31] included), strictly between two levels, in (H[30], H[31]] (t1 used), above H[31] (NaN).
  surface_temperature.npz
      heights             the notebook's HEIGHT_LEVELS
      tz_m<k>, ez_m<k>    read_building_height(fixture, "Tz" / "Ez", margin=k), k = 0, 1, 2 (helper module)
      tz_nb_m0            the same through the notebook's own copy of read_building_height
      inb_levs, inb_m2    calc_is_in_building(tz_m2.T, ez_m2.T, inb_levs) (helper module; (y, x) inputs)
      true, pred          (2, 32, 17, 13) float32 temperature in the notebook's (N, Z, X, Y) order: true has NaN inside
                          buildings and NaN voxels just above some building tops (the first level at or above it, or
                          the next); pred is finite
      true_2m, pred_2m    infer_2m_height_temperature(true / pred, tz_m0): (2, 17, 13) float32
      rmse, mae           the notebook's float32 sqrt(nanmean((pred_2m - true_2m) ** 2)) and nanmean(|...|)
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("SR3D_REFERENCE", "/root/reference/pytorch")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from src import building_height_helper as bhh  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
NI, NJ = 17, 13
MISSING = (5, 7)


def notebook_namespace():
    nb = json.load(open(os.path.join(REF, "notebook", "make_2m_temperature.ipynb")))
    cells = ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]
    ns = {"np": np, "pd": pd, "tqdm": lambda it, **kw: it}
    for src in cells:
        if src.startswith("HEIGHT_LEVELS =") or "def infer_2m_height_temperature" in src:
            exec(compile(src, "make_2m_temperature.ipynb", "exec"), ns)
    assert "HEIGHT_LEVELS" in ns and "infer_2m_height_temperature" in ns and "read_building_height" in ns
    return ns


def tz_values(rng, H, n):
    """building-top heights cycling through every branch of the extrapolation"""
    kinds = rng.permutation(np.arange(n) % 6)
    v = np.empty(n)
    for idx, k in enumerate(kinds):
        if k == 0:
            v[idx] = round(rng.uniform(0.0, H[0] - 0.01), 2)                  # below H[0]
        elif k == 1:
            v[idx] = H[rng.integers(0, len(H))]                                # exactly on a level
        elif k == 2:
            j = rng.integers(0, len(H) - 1)
            v[idx] = round(H[j] + rng.uniform(0.01, 4.99), 2)                 # strictly between
        elif k == 3:
            v[idx] = [H[-2] + 0.01, H[-2] + 2.5, H[-1]][rng.integers(0, 3)]  # (H[30], H[31]]: t1
        elif k == 4:
            v[idx] = round(rng.uniform(H[-1] + 0.01, H[-1] + 40.0), 2)       # above H[31]: NaN
        else:
            v[idx] = H[rng.integers(0, 3)] if rng.random() < 0.5 else round(rng.uniform(H[0], H[6]), 2)
    return v


def write_fixture(path, rng, H):
    tz = tz_values(rng, H, NI * NJ)
    tz[0], tz[1] = H[0], H[-1]
    rows = []
    for n, (i, j) in enumerate((i, j) for i in range(NI) for j in range(NJ)):
        if (i, j) == MISSING:
            continue
        ez = round(rng.uniform(0.0, 20.0), 2)
        rows.append((i, j, ez, tz[n], round(rng.uniform(0.0, 30.0), 2)))
    for n in rng.choice(len(rows), 12, replace=False):      # duplicate pairs: lower and higher values
        i, j, ez, t, tl = rows[n]
        rows.append((i, j, round(ez + rng.uniform(-3, 3), 2), round(t + rng.choice([-7.5, -2.0, 1.25, 6.0]), 2),
                     round(tl + 1.0, 2)))
    order = rng.permutation(len(rows))
    with open(path, "w") as f:
        f.write("    i    j        Ez        Tz       Tzl\n")
        for n in order:
            i, j, ez, t, tl = rows[n]
            f.write(f"{i:5d}{j:5d} {ez:9.2f} {t:9.2f} {tl:9.2f}\n")


def temperature(rng, N, tz, H, with_nan):
    Z = len(H)
    t = (300.0 + rng.normal(0.0, 1.5, size=(N, 1, NI, NJ)) - 0.006 * H[None, :, None, None]
         + rng.normal(0.0, 0.4, size=(N, Z, NI, NJ))).astype(np.float32)
    if with_nan:
        inside = H[None, :, None, None] < tz[None, None]                 # levels below the building top
        t[np.broadcast_to(inside, t.shape)] = np.nan
        for n in range(N):                                               # NaN just above some tops
            for _ in range(25):
                i, j = rng.integers(0, NI), rng.integers(0, NJ)
                b = tz[i, j]
                if not np.isfinite(b) or b > H[-1]:
                    continue
                first = 0 if b <= H[0] else int(np.nonzero(H >= b)[0][0])
                t[n, min(first + int(rng.integers(0, 2)), Z - 1), i, j] = np.nan
    return t


def main():
    rng = np.random.default_rng(20261016)
    ns = notebook_namespace()
    H = np.asarray(ns["HEIGHT_LEVELS"], dtype=np.float64)
    path = os.path.join(OUT, "EleTopoZ_fixture.txt")
    write_fixture(path, rng, H)

    g = {"heights": H}
    for m in (0, 1, 2):
        g[f"tz_m{m}"] = bhh.read_building_height(path, "Tz", margin=m)
        g[f"ez_m{m}"] = bhh.read_building_height(path, "Ez", margin=m)
    g["tz_nb_m0"] = ns["read_building_height"](path, "Tz", margin=0)
    assert g["tz_m0"].shape == (NI, NJ) and np.isnan(g["tz_m0"][MISSING])
    np.testing.assert_array_equal(g["tz_nb_m0"], g["tz_m0"])
    g["inb_levs"] = H
    g["inb_m2"] = bhh.calc_is_in_building(g["tz_m2"].T, g["ez_m2"].T, H)

    tz = g["tz_m0"]
    g["true"] = temperature(rng, 2, tz, H, with_nan=True)
    g["pred"] = temperature(rng, 2, tz, H, with_nan=False)
    g["true_2m"] = ns["infer_2m_height_temperature"](g["true"], tz)
    g["pred_2m"] = ns["infer_2m_height_temperature"](g["pred"], tz)
    d = g["pred_2m"] - g["true_2m"]
    g["rmse"] = np.sqrt(np.nanmean(d ** 2))
    g["mae"] = np.nanmean(np.abs(d))

    # every branch is present
    b = tz[np.isfinite(tz)]
    assert (b < H[0]).any() and np.isin(b, H).any() and (b > H[-1]).any()
    assert ((b > H[-2]) & (b <= H[-1])).any() and (~np.isin(b, H) & (b > H[0]) & (b < H[-1])).any()
    assert np.isnan(g["true_2m"]).any() and np.isfinite(g["true_2m"]).any()
    np.savez_compressed(os.path.join(OUT, "surface_temperature.npz"), **g)
    print("wrote", path, os.path.getsize(path), "bytes; surface_temperature.npz",
          os.path.getsize(os.path.join(OUT, "surface_temperature.npz")), "bytes; rmse", g["rmse"], "mae", g["mae"])


if __name__ == "__main__":
    main()
