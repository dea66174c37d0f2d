"""numpy restatement of the notebook's infer_2m_height_temperature (make_2m_temperature), vectorised over columns.
Pinned to the notebook's own outputs in tests/golden/surface_temperature.npz (tests/test_surface_temperature_host.py);
the GPU tests use it for shapes and inputs the golden file does not hold."""
import numpy as np

HEIGHTS = np.arange(32) * 5 + 17.5


def t2m_ref(temperature: np.ndarray, building: np.ndarray, heights: np.ndarray = HEIGHTS) -> np.ndarray:
    """temperature (N, Z, X, Y) float32, building (X, Y) float64 -> (N, X, Y) float32 with numpy >= 2's rounding of
    t1 + (b - h1) * (t2 - t1) / (h2 - h1): t2 - t1 in float32, the rest in float64, one rounding to float32"""
    Z = temperature.shape[1]
    H = np.asarray(heights, dtype=np.float64)[:Z]
    b = np.asarray(building, dtype=np.float64)
    above = b > H[-1]
    first = np.where(b > H[0], np.argmax(H[:, None, None] >= b[None], axis=0), 0)
    first = np.where(above, 0, first)
    second = np.minimum(first + 1, Z - 1)
    t1 = np.take_along_axis(temperature, first[None, None], axis=1)[:, 0]
    t2 = np.take_along_axis(temperature, second[None, None], axis=1)[:, 0]
    h1, h2 = H[first], H[second]
    with np.errstate(all="ignore"):
        t = (t1.astype(np.float64) + ((b - h1) * (t2 - t1).astype(np.float64)) / (h2 - h1)).astype(np.float32)
    t = np.where(first == Z - 1, t1, t)
    return np.where(above, np.float32(np.nan), t).astype(np.float32)


def errors_ref(pred_2m: np.ndarray, true_2m: np.ndarray):
    """(sum (p - t)^2, sum |p - t|, count) over the columns where both are finite, in fp64"""
    ok = np.isfinite(pred_2m) & np.isfinite(true_2m)
    d = pred_2m[ok].astype(np.float64) - true_2m[ok].astype(np.float64)
    return float((d * d).sum()), float(np.abs(d).sum()), float(ok.sum())
