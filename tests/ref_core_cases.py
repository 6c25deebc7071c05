"""The case list of the reference-core pin: inputs for tests/test_ref_core.py, tests/test_gpu_ref_core.py and
tests/golden/make_ref_core.py, and the reference build's chain of stages on them (oracle/ref_core.py).

Three image families:
  make_pair  synthetic.make_pair: fine texture, arms of length 1-3;
  flat       blocks of 40 x 48 pixels of one colour each (+-1 of noise): arms up to the cap L_out = 34, long cross regions;
  binary     0 / 255 blocks of random size: gray differences of +-255, the gradients at their bounds.
"""
import functools
import hashlib

import numpy as np

from mystereomatching_amd import synthetic as S
from oracle import ref_core as R

KINDS = ("make_pair", "flat", "binary")
VARIANTS = ("so", "so_R2L", "so_T2D")
REG_LAMBDA = 0.3

# (kind, H, W, D): H from 2 to 75 (the CBCA lag is 34), W across 64 and 256, every D of the issue's list
CPU_CASES = [("make_pair", 2, 70, 16), ("make_pair", 3, 5, 1), ("make_pair", 7, 66, 65), ("make_pair", 23, 97, 24),
             ("make_pair", 36, 63, 64), ("make_pair", 75, 40, 128), ("make_pair", 5, 260, 200),
             ("make_pair", 12, 258, 256), ("flat", 40, 90, 32), ("flat", 75, 70, 130), ("binary", 11, 33, 16)]
# so_T2D is defined for every fill byte only with W = 1 (oracle/ref_core.py): volumes alone, no cost stage
T2D_W1_CASES = [(9, 1, 8), (40, 1, 33), (75, 1, 200)]
# the cases recorded in tests/golden/ref_core.npz for machines without the binary (small: the file holds every array)
GOLDEN_CASES = [("make_pair", 9, 21, 6), ("flat", 12, 40, 9), ("binary", 6, 18, 130)]


def sha256(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def pair(kind, H, W, D, idx=0):
    if kind == "make_pair":
        p = S.make_pair(H, W, D, 900 + idx)
    else:
        rng = np.random.default_rng(4100 + idx + 7 * H + 13 * W)
        if kind == "flat":
            base = rng.integers(30, 226, (H // 40 + 1, W // 48 + 1, 3))
            left = np.kron(base, np.ones((40, 48, 1), np.int64))[:H, :W] + rng.integers(-1, 2, (H, W, 3))
        else:
            base = rng.integers(0, 2, (H // 3 + 1, W // 5 + 1, 1)) * 255
            left = np.repeat(np.kron(base, np.ones((3, 5, 1), np.int64))[:H, :W], 3, axis=2)
        left = left.astype(np.uint8)
        shift = max(1, min(D - 1, W // 4, 5))
        right = np.roll(left, -shift, axis=1)
        right[:, W - shift:] = rng.integers(0, 256, (H, shift, 3)).astype(np.uint8) if kind == "flat" else 255 - left[:, :shift]
        p = {"lbgr": left, "rbgr": np.ascontiguousarray(right), "lgray": S.bgr_to_gray(left), "rgray": S.bgr_to_gray(right)}
    out = {k: np.ascontiguousarray(p[k], np.uint8) for k in R.KEYS}
    for a in out.values():
        a.setflags(write=False)
    return out


def solve_all_weight(lam=REG_LAMBDA):
    """SolveAll's 1 x 1 inverse as OpenCV computes it, (float)(1. / (double)(1 + lambda)) (oracle.solve_all_weight is
    pinned to this in tests/test_ref_core.py)."""
    return float(np.float32(1.0 / float(np.float32(1) + np.float32(lam))))


@functools.lru_cache(maxsize=None)
def chain(kind, H, W, D, cost="censusGrad", iters=2, intersect=True, paths=4):
    """The reference build's default pipeline on one pair, every stage read back:
    census, arms, cost (both views), agg (both), scaled (both), sgm0, sgm1 (leftFirst false), disp0, disp1."""
    ops = [("census",), ("arms",), ("cost", cost), ("cbca", iters), ("scale", solve_all_weight()),
           ("sgm", 0, paths, True), ("sgm", 1, paths, False), ("wta", 0), ("wta", 1)]
    o = R.run_defined(pair(kind, H, W, D), D, ops, intersect=intersect)
    out = {"census": o[0], "arms": o[1], "cost": o[2], "agg": o[3], "scaled": o[4], "sgm": (o[5][0], o[6][0]),
           "disp": (o[7][0], o[8][0])}
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def so_chain(kind, H, W, D, variant):
    """so* of the reference build on its own scaled CBCA volumes, both views with I[0] = the left image
    (cpp:1093-1104): ((DP[0], acc[0]), (DP[1], acc[1]))."""
    c = chain(kind, H, W, D)
    ops = [("setvm", 0, c["scaled"][0]), ("setvm", 1, c["scaled"][1]), ("so", 0, variant), ("so", 1, variant)]
    o = R.run_defined(pair(kind, H, W, D), D, ops)
    return o[2], o[3]


def t2d_w1_volume(H, D, seed=0):
    rng = np.random.default_rng(7700 + seed + H + D)
    vol = rng.random((H, 1, D), dtype=np.float32) * np.float32(4)
    img = rng.integers(0, 256, (H, 1, 3)).astype(np.uint8)
    return vol, img


def wta_volume(H, W, D, seed=0):
    """A volume for gen_dispFromVm's rule alone (`if (minC > vmP[d])` from FLT_MAX, cpp:3940-3952: the FIRST of equal
    minima, a NaN never taken, -1 where nothing is below FLT_MAX): costs quantised to {-1, -0, +0, 1, 2} (nearly
    every pixel has tied minima, -0 against +0 among them), constant pixels, NaN at d = 0, NaN at one d > 0, pixels
    of NaN only, one whole row of NaN, and pixels of FLT_MAX only."""
    rng = np.random.default_rng(9300 + seed + 3 * H + 5 * W + 7 * D)
    levels = np.array([-1.0, -0.0, 0.0, 1.0, 2.0], np.float32)
    vol = levels[rng.integers(0, len(levels), (H, W, D))]
    u = rng.random((H, W))
    vol[u < 0.10] = levels[rng.integers(0, len(levels), (H, W))][u < 0.10][:, None]      # constant pixels
    vol[(u >= 0.10) & (u < 0.25), 0] = np.nan
    if D >= 2:
        for v, x in zip(*np.nonzero((u >= 0.25) & (u < 0.40))):
            vol[v, x, rng.integers(1, D)] = np.nan
    vol[(u >= 0.40) & (u < 0.46)] = np.nan
    vol[(u >= 0.46) & (u < 0.50)] = np.finfo(np.float32).max
    vol[H // 2] = np.nan
    return np.ascontiguousarray(vol, np.float32)


def so_tie_volume(H, W, D, seed=0):
    """Costs on the grid of so()'s own penalties -- sums of 0, fl(0.6), fl(1.2), fl(1.8), fl(3.6) -- so that at the first
    step prev[d], prev[d - 1] + Pn2, prev[d + 1] + Pn2 and min + Pn3 tie (with and without the halving), and the order
    of so()'s strict compares decides the trace."""
    rng = np.random.default_rng(9500 + seed + H + W + D)
    grid = np.array([0.0, 0.6, 1.2, 1.8, 3.6], np.float32)
    return np.ascontiguousarray(grid[rng.integers(0, len(grid), (H, W, D))] + grid[rng.integers(0, 3, (H, W, D))])


# ---- what tests/test_gpu_ref_core.py runs (shapes from the kernels' layouts) -------------------------------------
GPU_COST = [(23, 97, 24), (23, 97, 100), (67, 257, 16)]                 # census words, cost and prep tiles
GPU_CBCA = [(2, 96, 256), (68, 96, 256), (40, 80, 128), (200, 90, 64)]  # fast sweeps both views; steady tiles
GPU_SGM = [(9, 17, 64, 4), (17, 33, 256, 4), (23, 7, 200, 4), (12, 19, 256, 8)]   # row / dwordx4 / scalar layouts, 8 paths
GPU_SO = (33, 71, 32)
GPU_WTA = [(7, 9, 1), (9, 11, 70), (6, 10, 200)]     # wta_volume(): one, two and four disparities per lane of k_wta
GPU_KIND = {(40, 80, 128): "flat"}       # one CBCA shape on long arms; everything else on make_pair
SMALL = 160 * 1024                       # a recorded array is kept in full up to this many bytes


def gpu_kind(H, W, D):
    return GPU_KIND.get((H, W, D), "make_pair")


def gpu_keys():
    """{key: (function making {name: array} from the reference build, input pair)} of every GPU expectation."""
    out = {}
    for H, W, D in GPU_COST:
        for cost in ("censusGrad", "Census"):
            out[f"cost_{cost}_{H}x{W}x{D}"] = ("cost", gpu_kind(H, W, D), H, W, D, cost)
    for H, W, D in GPU_CBCA:
        out[f"cbca_{H}x{W}x{D}"] = ("cbca", gpu_kind(H, W, D), H, W, D, "censusGrad")
    for H, W, D, paths in GPU_SGM:
        out[f"sgm{paths}_{H}x{W}x{D}"] = ("sgm", gpu_kind(H, W, D), H, W, D, paths)
    H, W, D = GPU_SO
    for variant in VARIANTS:
        out[f"{variant}_{H}x{W}x{D}"] = ("so", gpu_kind(H, W, D), H, W, D, variant)
    for H, W, D in GPU_WTA:
        out[f"wta_{H}x{W}x{D}"] = ("wta", "make_pair", H, W, D, 0)
    return out


def gpu_expected(spec):
    """The reference build's arrays for one GPU case, by name."""
    what, kind, H, W, D, arg = spec
    if what == "cost":
        c = chain(kind, H, W, D, cost=arg)
        return {"census0": c["census"][0], "census1": c["census"][1], "arms0": c["arms"][0], "arms1": c["arms"][1],
                "cost0": c["cost"][0], "cost1": c["cost"][1]}
    if what == "cbca":
        c = chain(kind, H, W, D)
        return {"arms0": c["arms"][0], "arms1": c["arms"][1], "agg0": c["agg"][0], "agg1": c["agg"][1]}
    if what == "sgm":
        c = chain(kind, H, W, D, paths=arg)
        return {"scaled0": c["scaled"][0], "sgm0": c["sgm"][0], "sgm1": c["sgm"][1], "disp0": c["disp"][0], "disp1": c["disp"][1]}
    if what == "wta":
        return {"disp0": R.wta(wta_volume(H, W, D, arg))}
    (d0, a0), (d1, a1) = so_chain(kind, H, W, D, arg)
    return {"disp0": d0, "acc0": a0, "disp1": d1, "acc1": a1}


def gpu_input_digest(spec):
    what, kind, H, W, D, arg = spec
    p = pair(kind, H, W, D)
    extra = [wta_volume(H, W, D, arg).view(np.uint32)] if what == "wta" else []
    return sha256(*(p[k] for k in R.KEYS), np.array([H, W, D]), np.frombuffer(str(arg).encode(), np.uint8), *extra)
