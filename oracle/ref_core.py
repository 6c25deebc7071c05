"""Runs oracle/_ref/ref_core_driver, the reference's own cost / arms / CBCA / SGM / WTA / scan-line functions
behind our driver -- TEST INFRASTRUCTURE ONLY.

The binary is built by oracle/ref_core.mk from a reference checkout; oracle/_ref/ is not in git.  Each call
runs it once in a child process, with a time limit: one StereoMatching object, a list of ops on it, every
op's outputs read back (oracle/ref_core_driver.cpp has the list).

Mat::create does not zero memory, so every new buffer of the build is filled with a byte the caller chooses
(`fill`); run_defined() runs a case with both FILLS and refuses it unless the outputs are equal bit for bit.

The accepted domain, and why:
  * H, W >= 2: calGrad and calGrad_y read column 1 and row 1 unconditionally (cpp:284, 342).
  * D <= 512: the constructor makes vm[i] a 2-D Mat of D channels (cpp:2080), and CV_CN_MAX is 512.
  * so_T2D with W > 1 only with fill = 0: its backtrack sits INSIDE the column loop (cpp:6650-6680 within
    cpp:6586), so after column u it walks every column's trace, those of columns > u before anything has
    written them, and indexes the next row's trace with what it read.  The last pass (u = W - 1) rewrites
    the whole map from a fully written trace, so the result does not depend on those reads -- provided they
    stay inside the trace, which only a zeroed buffer (index 0) guarantees.  With any other fill byte the
    index is out of range and the wrapper refuses; with W = 1 there is no such read and any fill is accepted.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BINARY = os.path.join(HERE, "_ref", "ref_core_driver")
BINARY_ASAN = os.path.join(HERE, "_ref", "ref_core_driver_asan")
MAGIC = 0x524F4352
FILLS = (0x00, 0xFF)         # unwritten floats read as +0 and as NaN, unwritten arm lengths as 0 and 65535
TIMEOUT_S = 120.0
KEYS = ("lbgr", "rbgr", "lgray", "rgray")
OPS = {"census": 1, "arms": 2, "cost": 3, "setvm": 4, "cbca": 5, "scale": 6, "sgm": 7, "wta": 8, "so": 9}
COST = {"censusGrad": 0, "Census": 1}
SO = {"so": 0, "so_R2L": 1, "so_T2D": 2}
CENSUS_WORDS = 2             # ceil((7 * 9 + 8) / 64.), cpp:829-832


class RefCoreError(RuntimeError):
    pass


def available(binary: str = BINARY) -> bool:
    return os.path.isfile(binary) and os.access(binary, os.X_OK)


def reference_dir() -> str:
    """The reference checkout oracle/ref_core.mk builds from (SM_REFERENCE_DIR, or ../reference)."""
    return os.environ.get("SM_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference")


def checkout_present() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "stereoMatching.cpp"))


def blank_pair(H: int, W: int, bgr: np.ndarray | None = None) -> dict:
    """Images for the ops that read none (wta) or the colour images only (sgm, so)."""
    z3, z1 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    b = z3 if bgr is None else np.ascontiguousarray(bgr, np.uint8)
    return {"lbgr": b, "rbgr": b, "lgray": z1, "rgray": z1}


def _check_domain(H, W, D, ops, fill):
    if H < 2 or W < 2:
        if any(op[0] in ("cost",) for op in ops):
            raise RefCoreError(f"{H}x{W}: calGrad / calGrad_y read column 1 and row 1 (needs H, W >= 2)")
    if not 1 <= D <= 512:
        raise RefCoreError(f"D = {D}: vm[i] is a 2-D Mat of D channels, at most 512")
    for op in ops:
        if op[0] == "so" and SO[op[2]] == 2 and W > 1 and fill != 0:
            raise RefCoreError("so_T2D with W > 1 reads its trace before writing it: defined with fill = 0 only")


def run(pair: dict, D: int, ops, fill: int = 0, intersect: bool = True, timeout: float = TIMEOUT_S,
        binary: str = BINARY) -> list:
    """One run of the binary.  ops: ("census",), ("arms",), ("cost", "censusGrad" | "Census"),
    ("setvm", view, volume), ("cbca", iterations), ("scale", weight), ("sgm", view, paths, left_first),
    ("wta", view), ("so", view, "so" | "so_R2L" | "so_T2D").  Returns one entry per op: a tuple of arrays
    (both views where the op makes both), None for setvm."""
    if not available(binary):
        raise RefCoreError(f"{binary} is missing: build it with 'make -C oracle -f ref_core.mk' beside a "
                           "reference checkout (or set SM_REFERENCE_DIR)")
    img = {k: np.ascontiguousarray(pair[k], np.uint8) for k in KEYS}
    H, W = img["lgray"].shape
    if img["lbgr"].shape != (H, W, 3) or img["rbgr"].shape != (H, W, 3) or img["rgray"].shape != (H, W):
        raise ValueError("the four images must be H x W x 3, H x W x 3, H x W, H x W")
    _check_domain(H, W, D, ops, fill)
    vol, u16, i16 = (H, W, D), (H, W, 5), (H, W)
    body, layout = [], []
    for op in ops:
        name = op[0]
        a = b = c = 0
        payload = b""
        if name == "cost":
            a = COST[op[1]]
        elif name == "setvm":
            a = int(op[1])
            v = np.ascontiguousarray(op[2], np.float32)
            if v.shape != vol:
                raise ValueError("setvm needs an H x W x D volume")
            payload = v.tobytes()
        elif name == "cbca":
            a = int(op[1])
        elif name == "scale":
            a = struct.unpack("<i", struct.pack("<f", float(op[1])))[0]
        elif name == "sgm":
            a, b, c = int(op[1]), int(op[2]), int(bool(op[3]))
        elif name == "wta":
            a = int(op[1])
        elif name == "so":
            a, b = int(op[1]), SO[op[2]]
        body.append(struct.pack("<iiii", OPS[name], a, b, c) + payload)
        layout.append({"census": [(np.uint64, (H, W, CENSUS_WORDS))] * 2, "arms": [(np.uint16, u16)] * 2,
                       "cost": [(np.float32, vol)] * 2, "setvm": None, "cbca": [(np.float32, vol)] * 2,
                       "scale": [(np.float32, vol)] * 2, "sgm": [(np.float32, vol)], "wta": [(np.int16, i16)],
                       "so": [(np.int16, i16), (np.float32, vol)]}[name])
    with tempfile.TemporaryDirectory(prefix="ref_core_") as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<iiiiiii", MAGIC, H, W, D, int(fill), int(bool(intersect)), len(ops)))
            for k in KEYS:
                f.write(img[k].tobytes())
            for rec in body:
                f.write(rec)
        what = f"{[op[0] for op in ops]} at {H}x{W}x{D}, fill {fill:#04x}"
        try:
            r = subprocess.run([binary, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               stdin=subprocess.DEVNULL, timeout=timeout)
        except subprocess.TimeoutExpired as e:
            raise RefCoreError(f"reference core binary did not finish {what} in {timeout} s") from e
        if r.returncode != 0:
            raise RefCoreError(f"reference core binary failed ({r.returncode}) in {what}: "
                               f"{r.stderr.decode(errors='replace').strip()[-1500:]}")
        with open(fout, "rb") as f:
            raw = f.read()
    out, off = [], 0
    for lay in layout:
        if lay is None:
            out.append(None)
            continue
        arrs = []
        for dt, shape in lay:
            n = int(np.prod(shape))
            if off + n * np.dtype(dt).itemsize > len(raw):
                raise RefCoreError(f"output of {what} is short")
            arrs.append(np.frombuffer(raw, dt, n, off).reshape(shape).copy())
            off += n * np.dtype(dt).itemsize
        out.append(tuple(arrs))
    if off != len(raw):
        raise RefCoreError(f"output of {what} has {len(raw) - off} bytes too many")
    return out


def same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_defined(pair: dict, D: int, ops, intersect: bool = True, fills=FILLS, **kw) -> list:
    """run() with every fill byte; RefCoreError unless all outputs are equal bit for bit (then the result does
    not depend on memory the reference never wrote).  A case the domain allows with fill 0 only (so_T2D, W > 1)
    is run once."""
    H, W = np.asarray(pair["lgray"]).shape
    if any(op[0] == "so" and SO[op[2]] == 2 for op in ops) and W > 1:
        fills = (0,)
    first = run(pair, D, ops, fill=fills[0], intersect=intersect, **kw)
    for fill in fills[1:]:
        other = run(pair, D, ops, fill=fill, intersect=intersect, **kw)
        for i, (x, y) in enumerate(zip(first, other)):
            if x is None:
                continue
            for j, (p, q) in enumerate(zip(x, y)):
                if not same_bits(p, q):
                    raise RefCoreError(f"op {i} ({ops[i][0]}), output {j}: the reference's result depends on memory it "
                                       f"never wrote (fill {fills[0]:#04x} against {fill:#04x})")
    return first


# One function per stage ---------------------------------------------------------------------------------------

def census(pair: dict, **kw):
    """genCensusCode_NC_Sur (h:867-934) as censusCal calls it: (code[0], code[1]), H x W x 2 uint64."""
    return run_defined(pair, 1, [("census",)], **kw)[0]


def arms(pair: dict, **kw):
    """initArm + calArms<uchar> with window 0 (cpp:5675-5678): (HVL[0], HVL[1]), H x W x 5 uint16 (L, R, U, D, sum)."""
    return run_defined(pair, 1, [("arms",)], **kw)[0]


def cost(pair: dict, D: int, kind: str = "censusGrad", **kw):
    """censusGrad(vm) or censusCal(vm, 1): (vm[0], vm[1])."""
    return run_defined(pair, D, [("cost", kind)], **kw)[0]


def cbca(pair: dict, vm0: np.ndarray, vm1: np.ndarray, iterations: int = 2, intersect: bool = True, **kw):
    """cbca_aggregate(0, vm) with cbca_iterationNum = iterations on the given volumes: (vm[0], vm[1])."""
    D = vm0.shape[2]
    return run_defined(pair, D, [("setvm", 0, vm0), ("setvm", 1, vm1), ("cbca", iterations)], intersect=intersect, **kw)[2]


def solve_all(vm0: np.ndarray, vm1: np.ndarray, weight: float, **kw):
    """SolveAll's one-level sum with the given inverse weight: (vm[0], vm[1])."""
    H, W, D = vm0.shape
    return run_defined(blank_pair(H, W), D, [("setvm", 0, vm0), ("setvm", 1, vm1), ("scale", weight)], **kw)[2]


def sgm(vm: np.ndarray, bgr: np.ndarray, paths: int = 4, left_first: bool = True, **kw) -> np.ndarray:
    """sgm(vm, leftFirst): `bgr` is the image updateCost's D1 reads -- I_c[0] with leftFirst, else I_c[1]; it is
    given as both, so a wrong choice inside the build could not show here (tests/test_ref_core.py has a case
    with two different images for that)."""
    H, W, D = vm.shape
    return run_defined(blank_pair(H, W, bgr), D, [("setvm", 0, vm), ("sgm", 0, paths, left_first)], **kw)[1][0]


def wta(vm: np.ndarray, **kw) -> np.ndarray:
    """gen_dispFromVm: H x W int16."""
    H, W, D = vm.shape
    return run_defined(blank_pair(H, W), D, [("setvm", 0, vm), ("wta", 0)], **kw)[1][0]


def so(vm: np.ndarray, bgr: np.ndarray, variant: str = "so", **kw):
    """so / so_R2L / so_T2D on the volume with I[0] = bgr: (DP, accumulated volume)."""
    H, W, D = vm.shape
    return run_defined(blank_pair(H, W, bgr), D, [("setvm", 0, vm), ("so", 0, variant)], **kw)[1]
