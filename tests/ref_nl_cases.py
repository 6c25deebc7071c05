"""Inputs shared by tests/test_ref_nl.py, tests/test_gpu_ref_nl.py and tests/golden/make_ref_nl.py:
image families and volumes for the comparisons with the reference's own NL/ code (oracle/ref_nl.py).

The spanning tree of an 8-bit image is far from unique: which one the reference picks depends on
the counting sort's tie order, the edge enumeration order, the union direction and the neighbour-list
order of the breadth-first walk.  The families below go from no ties at all that matter (uniform
random) to nothing but ties (2-level stripes and checkers, flat)."""
import hashlib

import numpy as np

from mystereomatching_amd import synthetic as S

FAMILIES = ("random", "levels4", "stripes", "checkers", "make_pair", "ramp", "flat")
NON_FLAT = tuple(f for f in FAMILIES if f != "flat")

# rows x cols outside 363..543 px, the window in which the reference's ctmf call cannot work
# (oracle/ref_nl.py): 19 x 19 = 361 and 17 x 32 = 544 are its two neighbours
SHAPES = ((3, 3), (3, 90), (90, 3), (4, 257), (130, 5), (19, 19), (17, 32), (24, 30), (40, 61))
SIGMAS = (0.1, 0.5, 0.005)     # 0.005 lies below update_table's 0.01 clamp


def image(family: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """An H x W x 3 uint8 image of the family."""
    rng = np.random.default_rng([seed, H, W, FAMILIES.index(family)])
    y, x = np.mgrid[0:H, 0:W]
    if family == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if family == "levels4":
        return (rng.integers(0, 4, (H, W, 3)) * 85).astype(np.uint8)
    if family == "stripes":
        # 2 levels, bands 3 px wide (they survive the 3 x 3 median): vertical bands in two channels,
        # horizontal ones in the third.  Inside a weight-0 cell the choice among tied edges cannot
        # show (all tree distances are 0), so what the order decides is which CELLS get linked; the
        # crossing bands make the cells a grid whose every link weighs 20 (table[20] = 0.46 at sigma
        # 0.1), i.e. all of them tie.
        a = 100 + ((x // 3) % 2) * 20
        b = 100 + ((y // 3) % 2) * 20
        return np.stack([a, a, b], -1).astype(np.uint8)
    if family == "checkers":     # 2 levels, 3 x 3 squares, plus 1-px checkers in one channel (the median eats them)
        a = (((x // 3) + (y // 3)) % 2) * 255
        b = ((x + y) % 2) * 255
        return np.stack([a, b, a], -1).astype(np.uint8)
    if family == "make_pair":
        return np.ascontiguousarray(S.make_pair(H, W, 8, 900 + seed)["lbgr"])
    if family == "ramp":         # a different slope in each direction and channel, wrapping at 256
        return np.stack([(3 * x + 5 * y) % 256, (7 * x + 2 * y) % 256, (x * y) % 256], -1).astype(np.uint8)
    if family == "flat":
        return np.full((H, W, 3), 77, np.uint8)
    raise KeyError(family)


def volume(H: int, W: int, P: int, seed: int = 0) -> np.ndarray:
    """H x W x P float32 costs in [0, 64): the magnitudes of the census / gradient costs."""
    rng = np.random.default_rng([seed, H, W, P, 17])
    return (rng.random((H, W, P), dtype=np.float32) * np.float32(64)).astype(np.float32)


def sha256(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the GPU tests' cases (tests/test_gpu_ref_nl.py), recorded in tests/golden/ref_nl_gpu.npz -----------------
# The GPU machine may hold neither a reference checkout nor oracle/_ref/: the expected volumes of
# every GPU case -- outputs of the reference build -- are therefore recorded (tests/golden/
# make_ref_nl.py): the sha256 of each volume's bits, the volume itself where it is small, and the
# sha256 of its inputs.  A bit-for-bit comparison needs no more than the digest.

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
GPU_SHAPES = ((24, 30, 8), (40, 61, 64), (3, 90, 16), (90, 3, 16), (4, 257, 64), (130, 5, 71), (33, 70, 131))
GPU_KINDS = ("make_pair", "levels4", "stripes")
GPU_BOTH = (40, 61, 24, 601)                # do_refine: H, W, D, index
GPU_SIGMA = (24, 30, 8, 602)                # nl_sigma 0.5 and 0.005 (and 0.1, to tell them from)
GPU_GFNL = (24, 30, 8, 900)
GPU_BATCH = (29, 41, 16, (("make_pair", 610), ("levels4", 611), ("make_pair", 612)))
FULL_VOLUME_BYTES = 100 * 1024              # recorded in full up to this size, else by digest alone


def gpu_pair(kind, H, W, D, idx):
    """make_pair, or a pair whose colour images are of a tie-heavy family (the right image is the
    left one moved 2 px: the raw costs only have to be some costs)."""
    if kind == "make_pair":
        p = S.make_pair(H, W, D, idx)
        return {k: np.ascontiguousarray(p[k]) for k in KEYS}
    l = image(kind, H, W, seed=idx)
    r = np.ascontiguousarray(np.roll(l, -2, axis=1))
    return {"lbgr": l, "rbgr": r, "lgray": S.bgr_to_gray(l), "rgray": S.bgr_to_gray(r)}


def gfnl_pair():
    """test_gpu_gfnl's input: make_pair with the right half stretched, so that both GFNL classes occur."""
    from test_gpu_gfnl import stretched
    H, W, D, idx = GPU_GFNL
    p = S.make_pair(H, W, D, idx)
    return stretched({k: p[k] for k in KEYS})


def gpu_raw(pair, D, view=0):
    """The raw cost volume the aggregation starts from: the oracle's (censusGrad; no NL code in it)."""
    from oracle import oracle as O
    H, W = pair["lgray"].shape
    return O.cost_volume(pair, O.config(H, W, D - 1), view=view)


def gpu_cases():
    """key -> (raw volume, guide image, sigma): everything the reference build is asked for by the GPU tests."""
    out = {}
    for kind in GPU_KINDS:
        for H, W, D in GPU_SHAPES:
            p = gpu_pair(kind, H, W, D, 600)
            out[f"left_{kind}_{H}x{W}x{D}"] = (gpu_raw(p, D), p["lbgr"], 0.1)
    H, W, D, idx = GPU_BOTH
    p = gpu_pair("make_pair", H, W, D, idx)
    out["both_view0"] = (gpu_raw(p, D), p["lbgr"], 0.1)
    out["both_view1_if_filtered"] = (gpu_raw(p, D, view=1), p["rbgr"], 0.1)   # what vm[1] must NOT be
    H, W, D, idx = GPU_SIGMA
    p = gpu_pair("make_pair", H, W, D, idx)
    for sigma in (0.1, 0.5, 0.005):
        out[f"sigma_{sigma}"] = (gpu_raw(p, D), p["lbgr"], sigma)
    p = gfnl_pair()
    out["gfnl"] = (gpu_raw(p, GPU_GFNL[2]), p["lbgr"], 0.1)
    H, W, D, members = GPU_BATCH
    for i, (kind, idx) in enumerate(members):
        p = gpu_pair(kind, H, W, D, idx)
        out[f"batch_{i}"] = (gpu_raw(p, D), p["lbgr"], 0.1)
    return out


def input_digest(raw, bgr, sigma) -> str:
    return sha256(raw, bgr, np.float64(sigma))
