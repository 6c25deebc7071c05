"""numpy twin of OpenCV's normalised cv::boxFilter on f32 as aggregations "BF" and "GFNL" use it.

boxFilter(src, dst, -1, Size(ku, kv)) with the defaults: anchor (-1, -1) -> (ku / 2, kv / 2),
normalize = true, BORDER_REFLECT_101, evaluated as RowSum<float, double> followed by
ColumnSum<double, float> (the generic path) with literal running sums in float64:

  row sums     s = src[r(x - au)] + ... (ku values, left to right); then per column
               s += (double)src[r(x + ku - au)] - (double)src[r(x - au)]
  column sums  SUM = the first kv - 1 reflected rows' row sums (top to bottom); then per row
               s0 = SUM + row[r(y + kv - 1 - av)], out = (float)(s0 * scale), SUM = s0 - row[r(y - av)]
  scale        1.0 / (kv * ku)

r is cv::borderInterpolate for BORDER_REFLECT_101 (p < 0 -> -p, p >= n -> 2n - 2 - p, repeated; 0
for n == 1).  An even window is not centred: 12 covers the offsets -6 .. +5.  Trailing axes of the
input (the disparities of a volume) are filtered independently.

gfnl() is GFNL()'s blend (stereoMatching.cpp:4449-4487) on top of it.
"""
import numpy as np


def reflect101(p: int, n: int) -> int:
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def box_filter(src: np.ndarray, kv: int = 12, ku: int = 12) -> np.ndarray:
    """H x W [x ...] float32 -> the same shape, window kv rows x ku columns."""
    a = np.ascontiguousarray(src, np.float32)
    H, W = a.shape[:2]
    av, au = kv // 2, ku // 2
    x64 = a.astype(np.float64)
    cols = [reflect101(i - au, W) for i in range(W + ku - 1)]     # ext column i
    rs = np.empty_like(x64)
    s = np.zeros_like(x64[:, 0])
    for i in range(ku):
        s = s + x64[:, cols[i]]
    rs[:, 0] = s
    for x in range(W - 1):
        s = s + (x64[:, cols[x + ku]] - x64[:, cols[x]])
        rs[:, x + 1] = s
    rows = [reflect101(i - av, H) for i in range(H + kv - 1)]     # ext row i
    scale = 1.0 / (kv * ku)
    out = np.empty_like(a)
    SUM = np.zeros_like(rs[0])
    for i in range(kv - 1):
        SUM = SUM + rs[rows[i]]
    for y in range(H):
        s0 = SUM + rs[rows[y + kv - 1]]
        out[y] = (s0 * scale).astype(np.float32)
        SUM = s0 - rs[rows[y]]
    return out


def box_filter_direct(src: np.ndarray, kv: int = 12, ku: int = 12) -> np.ndarray:
    """The same window as an explicitly padded direct sum in float64 (taps in raster order): equal
    to box_filter wherever the sums are exact."""
    a = np.ascontiguousarray(src, np.float32).astype(np.float64)
    H, W = a.shape[:2]
    av, au = kv // 2, ku // 2
    ri = [reflect101(y, H) for y in range(-av, H + kv - 1 - av)]
    ci = [reflect101(x, W) for x in range(-au, W + ku - 1 - au)]
    pad = a[ri][:, ci]
    acc = np.zeros_like(a)
    for i in range(kv):
        for j in range(ku):
            acc = acc + pad[i:i + H, j:j + W]
    return (acc * (1.0 / (kv * ku))).astype(np.float32)


def variance_plane(gray: np.ndarray) -> np.ndarray:
    """GFNL()'s I_var (cpp:4450-4457): box19(I I) - box19(I) box19(I) in f32."""
    I = np.ascontiguousarray(gray, np.uint8).astype(np.float32)
    m2 = box_filter(I * I, 19, 19)
    m = box_filter(I, 19, 19)
    mm = (m * m).astype(np.float32)
    return (m2 - mm).astype(np.float32)


def gfnl(nl: np.ndarray, gf: np.ndarray, gray: np.ndarray, thresh: float = 400.0):
    """(vm[0], arm_Mask) of GFNL() from the NL and GF volumes and the left gray image."""
    mask = variance_plane(gray) < np.float32(thresh)
    blend = (0.5 * nl.astype(np.float64) + 0.5 * gf.astype(np.float64)).astype(np.float32)
    return np.where(mask[:, :, None], np.asarray(nl, np.float32), blend), mask.astype(np.uint8)
