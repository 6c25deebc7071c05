"""Runs oracle/_ref/ref_nl_driver, the reference's own NL/ code behind our driver -- TEST INFRASTRUCTURE ONLY.

The binary is built by oracle/ref_nl.mk from a reference checkout; oracle/_ref/ is not in git.  Each
call runs it once in a child process, with a time limit.

ctmf's domain, as qx_mst_kruskals_image::mst calls it (r = 1, memsize = rows * cols * 3): rows, cols >= 3,
and rows * cols outside 363..543.  Inside that window memsize / sizeof(Histogram) is 2, the stripe
divisor (ctmf.c:414) is 0, and the reference aborts on its own assertion (or, built without
assertions, never returns).  The wrapper refuses such sizes instead of starting the binary.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BINARY = os.path.join(HERE, "_ref", "ref_nl_driver")
MODES = {"median": 0, "tree": 1, "filter": 2}
WINDOW = (363, 543)          # rows * cols for which the reference's ctmf call cannot work
TIMEOUT_S = 60.0


class RefNLError(RuntimeError):
    pass


def available() -> bool:
    return os.path.isfile(BINARY) and os.access(BINARY, os.X_OK)


def reference_dir() -> str:
    """The reference checkout oracle/ref_nl.mk builds from (SM_REFERENCE_DIR, or ../reference)."""
    return os.environ.get("SM_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference")


def checkout_present() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "NL", "qx_tree_filter.cpp"))


def in_window(H: int, W: int) -> bool:
    return WINDOW[0] <= H * W <= WINDOW[1]


def run_raw(bgr: np.ndarray, mode: str, vol: np.ndarray | None = None, sigma: float = 0.1,
            timeout: float = TIMEOUT_S) -> bytes:
    """One run of the binary, no size check: returns its output file, raises RefNLError when it fails."""
    if not available():
        raise RefNLError(f"{BINARY} is missing: build it with 'make -C oracle -f ref_nl.mk' beside a "
                         "reference checkout (or set SM_REFERENCE_DIR)")
    img = np.ascontiguousarray(bgr, np.uint8)
    H, W = img.shape[:2]
    if img.shape != (H, W, 3):
        raise ValueError("bgr must be H x W x 3")
    if vol is None:
        vol = np.empty((H, W, 0), np.float32)
    v = np.ascontiguousarray(vol, np.float32)
    if v.shape[:2] != (H, W) or v.ndim != 3:
        raise ValueError("vol must be H x W x P")
    with tempfile.TemporaryDirectory(prefix="ref_nl_") as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<iiiid", H, W, v.shape[2], MODES[mode], float(sigma)))
            f.write(img.tobytes())
            f.write(v.tobytes())
        try:
            r = subprocess.run([BINARY, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               stdin=subprocess.DEVNULL, timeout=timeout)
        except subprocess.TimeoutExpired as e:
            raise RefNLError(f"reference NL binary did not finish {mode} at {H}x{W} in {timeout} s") from e
        if r.returncode != 0:
            raise RefNLError(f"reference NL binary failed ({r.returncode}) in {mode} at {H}x{W}: "
                             f"{r.stderr.decode(errors='replace').strip()[-300:]}")
        with open(fout, "rb") as f:
            return f.read()


def _run(bgr, mode, vol=None, sigma=0.1):
    H, W = np.asarray(bgr).shape[:2]
    if in_window(H, W):
        raise RefNLError(f"{H}x{W} = {H * W} px lies in {WINDOW[0]}..{WINDOW[1]}, where the reference's ctmf call "
                         "aborts or hangs")
    return run_raw(bgr, mode, vol, sigma)


def median(bgr: np.ndarray) -> np.ndarray:
    H, W = bgr.shape[:2]
    return np.frombuffer(_run(bgr, "median"), np.uint8).reshape(H, W, 3).copy()


def tree(bgr: np.ndarray) -> dict:
    """parent, nchild, child[n, 3] (-1 past nchild), weight, order (the BFS order), rank."""
    H, W = bgr.shape[:2]
    n = H * W
    raw = _run(bgr, "tree")
    if len(raw) != n * (4 + 4 + 12 + 1 + 4 + 4):
        raise RefNLError(f"tree output has {len(raw)} bytes")
    out, off = {}, 0
    for key, dt, cnt in (("parent", np.int32, n), ("nchild", np.int32, n), ("child", np.int32, 3 * n),
                         ("weight", np.uint8, n), ("order", np.int32, n), ("rank", np.int32, n)):
        out[key] = np.frombuffer(raw, dt, cnt, off).copy()
        off += cnt * np.dtype(dt).itemsize
    out["child"] = out["child"].reshape(n, 3)
    return out


def filter(vol: np.ndarray, bgr: np.ndarray, sigma: float = 0.1) -> np.ndarray:  # noqa: A001
    """NLCCA::aggreCV on an H x W x P float32 volume: (float) of the tree filter of the doubles."""
    v = np.ascontiguousarray(vol, np.float32)
    return np.frombuffer(_run(bgr, "filter", v, sigma), np.float32).reshape(v.shape).copy()


def nl(vol: np.ndarray, bgr: np.ndarray, sigma: float = 0.1) -> np.ndarray:
    """NL() (stereoMatching.cpp:4892-4917): aggreCV on the volume, aggreCV on a volume of ones, and
    the float quotient of the two float volumes."""
    v = np.ascontiguousarray(vol, np.float32)
    num = filter(v, bgr, sigma)
    # every plane of the ones volume filters alike, but NL() filters all of them: so do we
    den = filter(np.ones_like(v), bgr, sigma)
    return (num / den).astype(np.float32)
