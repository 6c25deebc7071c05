"""numpy restatement of the reference's "FIF" aggregation, for SMALL inputs only.

FIF_Improve (stereoMatching.cpp:4707-4890, what costCalculate calls) and the plain form FIF
(cpp:4541-4705), written from the reference text.  float32 numpy ufuncs round every operation on
its own (no FMA contraction), as the reference's scalar loops do; the squares of the colour
differences are taken and added in float64 (std::pow(float, int) returns double) and rounded to
float32 on assignment; expf is the host libm's (pyref.expf).
PARITY UNPINNED: the guide is OpenCV's convertTo(CV_32F, 1 / 255.0), restated as
(float)u8 * (float)(1 / 255.0).
"""
from __future__ import annotations

import numpy as np

from pyref import expf, f32

BIG = np.finfo(f32).max
EPS = f32(0.08)   # cpp:4713
PN = f32(2)       # cpp:4714


def weights(bgr, eps=EPS):
    """wgt_hor, wgt_ver (cpp:4719-4746): w[v, u] joins (v, u) with (v, u + 1) resp. (v + 1, u).
    The last column of wgt_hor and the last row of wgt_ver are never read (left 0 here)."""
    H, W = bgr.shape[:2]
    If = (np.asarray(bgr, np.uint8).astype(f32) * f32(1 / 255.0)).astype(f32)

    def w(cur, nxt):
        d = (nxt - cur).astype(f32).astype(np.float64)
        s = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)
        ee = f32(f32(eps) * f32(eps))
        return expf(((-s).astype(f32) / ee).astype(f32))

    wh = np.zeros((H, W), f32)
    wv = np.zeros((H, W), f32)
    if W > 1:
        wh[:, :-1] = w(If[:, :-1], If[:, 1:])
    if H > 1:
        wv[:-1] = w(If[:-1], If[1:])
    return wh, wv


def step(prev, add, w, pn=PN, plain=False):
    """One sweep step over the last axis (d): add + min(prev[d-1] + Pn, prev[d+1] + Pn, prev[d]) * w
    (cpp:4767-4770); plain: add + prev * w (cpp:4601)."""
    w = np.asarray(w, f32)[..., None]
    if plain:
        return (add + (prev * w).astype(f32)).astype(f32)
    P = (prev + f32(pn)).astype(f32)
    lo = np.full_like(prev, BIG)
    up = np.full_like(prev, BIG)
    lo[..., 1:] = P[..., :-1]
    up[..., :-1] = P[..., 1:]
    m = np.minimum(np.minimum(lo, up), prev)
    return (add + (m * w).astype(f32)).astype(f32)


def _both_ways(vol, wgt, pn, plain):
    """Forward and backward sweeps along axis 1 of vol [lines, steps, D] with wgt [lines, steps],
    then (fwd + bwd) - vol."""
    n = vol.shape[1]
    fwd = np.empty_like(vol)
    bwd = np.empty_like(vol)
    fwd[:, 0] = vol[:, 0]
    for j in range(1, n):
        fwd[:, j] = step(fwd[:, j - 1], vol[:, j], wgt[:, j - 1], pn, plain)
    bwd[:, n - 1] = vol[:, n - 1]
    for j in range(n - 2, -1, -1):
        bwd[:, j] = step(bwd[:, j + 1], vol[:, j], wgt[:, j], pn, plain)
    return ((fwd + bwd).astype(f32) - vol).astype(f32)


def fif(vm, bgr, plain=False, eps=EPS, pn=PN):
    """The aggregated volume of one view: vm H x W x D float32, bgr that view's colour image."""
    vm = np.ascontiguousarray(vm, f32)
    wh, wv = weights(bgr, eps)
    A = _both_ways(vm, wh, pn, plain)                                      # rows
    out = _both_ways(A.transpose(1, 0, 2), wv.transpose(1, 0), pn, plain)  # columns
    return np.ascontiguousarray(out.transpose(1, 0, 2))
