"""Seeded degenerate stereo pairs: inputs on which the kernels' special cases decide the result.

synthetic.make_pair gives blurred random colour texture, whose costs are positive, distinct and
finite.  The pairs here are the opposite: constant or periodic images (most pixels have several
equal cost minima, so first-minimum tie-breaking decides the map), sparse high-contrast colour
blocks (the guided filter's output goes negative) and high-contrast grey images stored as colour
(the guided filter's per-pixel 3 x 3 float determinant cancels to 0 and the volume is NaN).
Every function returns the usual dict(lbgr, rbgr, lgray, rgray); gray is synthetic.bgr_to_gray.
"""
from __future__ import annotations

import numpy as np

from mystereomatching_amd import synthetic as S

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
GREY_KINDS = ("noise", "blocks")


def _pair(left, right):
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    return {"lbgr": left, "rbgr": right, "lgray": S.bgr_to_gray(left), "rgray": S.bgr_to_gray(right)}


def _colour(gray):
    return np.repeat(np.asarray(gray, np.uint8)[:, :, None], 3, axis=2)


def _shift_left(img, shift, fill):
    """The right view of a fronto-parallel plane at disparity `shift`: right[u] = left[u + shift];
    the `shift` columns that have no source take `fill` (same shape as those columns)."""
    out = np.empty_like(img)
    W = img.shape[1]
    s = min(shift, W)
    out[:, :W - s] = img[:, s:]
    out[:, W - s:] = fill
    return out


def constant(H, W, level=97):
    img = np.full((H, W, 3), level, np.uint8)
    return _pair(img, img.copy())


def identical(H, W, seed):
    img = S._texture(np.random.default_rng(seed), H, W)
    return _pair(img, img.copy())


def vstripes(H, W, period=6, shift=2):
    """0 / 255 columns, `period` wide in all (half dark, half bright); the right image is the same
    pattern moved by `shift` columns, so every multiple of the period off `shift` matches as well."""
    u = np.arange(W + shift)
    row = np.where((u % period) < period // 2, 0, 255).astype(np.uint8)
    left = np.broadcast_to(row[None, :W], (H, W))
    right = np.broadcast_to(row[None, shift:shift + W], (H, W))
    return _pair(_colour(left), _colour(right))


def hstripes(H, W, period=6):
    v = np.arange(H)
    col = np.where((v % period) < period // 2, 0, 255).astype(np.uint8)
    img = _colour(np.broadcast_to(col[:, None], (H, W)))
    return _pair(img, img.copy())


def checker(H, W, cell=3):
    v, u = np.mgrid[0:H, 0:W]
    img = _colour(np.where(((v // cell) + (u // cell)) % 2 == 0, 0, 255))
    return _pair(img, img.copy())


def step_edge(H, W, shift=5):
    """One vertical edge (40 left of it, 215 right), at column W / 2 in the left image and `shift`
    columns earlier in the right one."""
    u = np.arange(W)
    left = np.broadcast_to(np.where(u < W // 2, 40, 215)[None, :], (H, W))
    right = np.broadcast_to(np.where(u < W // 2 - shift, 40, 215)[None, :], (H, W))
    return _pair(_colour(left), _colour(right))


def left_constant_right_texture(H, W, seed):
    left = np.full((H, W, 3), 97, np.uint8)
    return _pair(left, S._texture(np.random.default_rng(seed), H, W))


def signed_blocks(H, W, seed):
    """Dim texture (make_pair's left image // 8) plus 200 on a random half of the 8 x 8 blocks,
    chosen per channel; the right image is the left one at disparity 5 with fresh dim noise in the
    vacated columns.  The guided filter's linear model overshoots around the isolated bright
    blocks, which drives aggregated costs below zero."""
    rng = np.random.default_rng(seed)
    base = S.make_pair(H, W, 8, seed=seed)["lbgr"].astype(np.int32) // 8
    on = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8, 3))
    on = np.repeat(np.repeat(on, 8, axis=0), 8, axis=1)[:H, :W]
    left = np.clip(base + 200 * on, 0, 255).astype(np.uint8)
    fill = rng.integers(0, 32, (H, min(5, W), 3)).astype(np.uint8)
    return _pair(left, _shift_left(left, 5, fill))


def grey_contrast(H, W, seed, kind="noise"):
    """B = G = R with levels 0 / 255 only: per-pixel noise or 6 x 6 blocks.  The right image is the
    left one at disparity 5 with fresh 0 / 255 noise in the vacated columns."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        g = rng.integers(0, 2, (H, W)) * 255
    elif kind == "blocks":
        on = rng.integers(0, 2, ((H + 5) // 6, (W + 5) // 6))
        g = np.repeat(np.repeat(on, 6, axis=0), 6, axis=1)[:H, :W] * 255
    else:
        raise ValueError(f"kind must be one of {GREY_KINDS}")
    left = _colour(g)
    fill = _colour(rng.integers(0, 2, (H, min(5, W))) * 255)
    return _pair(left, _shift_left(left, 5, fill))


def batch(pairs):
    """Stack pairs of one shape for StereoBatch.upload."""
    return {k: np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in KEYS}


# one size of each SGM / WTA kernel layout: rows of 16 lanes (D <= 64), two disparities per lane,
# scalar lanes (D % 4 != 0), checkpointed dwordx4 lanes; GF's MY_GUIDE form needs H, W >= 19
SHAPES = [(24, 30, 7), (40, 61, 23), (33, 80, 69), (23, 31, 130), (21, 30, 199)]
# the inputs of the tie tests, by name: (H, W) -> pair
TIE_INPUTS = {
    "constant": lambda H, W: constant(H, W),
    "identical": lambda H, W: identical(H, W, 3),
    "vstripes": lambda H, W: vstripes(H, W),
    "hstripes": lambda H, W: hstripes(H, W),
    "checker": lambda H, W: checker(H, W),
    "step_edge": lambda H, W: step_edge(H, W),
    "left_constant_right_texture": lambda H, W: left_constant_right_texture(H, W, 4),
}
