"""numpy restatement of the reference's "AWS" aggregation (adaptive support weights, Yoon and
Kweon), for SMALL inputs only.

AWS(), the branch without JBF_STANDARD (stereoMatching.cpp:5711-5792), with genWeight_AWS /
calW4_AWS / calvm_AWS (stereoMatching.h:1305-1350, 1472-1493, 1533-1548).  float32 numpy ufuncs
round every operation on its own (no FMA contraction), as the reference's scalar loops do; the
colour distance is summed in float64 and rounded to float32, the square root is the correctly
rounded one, expf is the host libm's (pyref.expf).  The loops run over the taps in raster order
(dv outer, du inner) and are vectorised over (v, u, d): the accumulation order over the taps is
part of the result.
PARITY UNPINNED: the Lab planes are OpenCV's 8-bit BGR2Lab, restated here as its fixed-point path.
"""
from __future__ import annotations

import functools

import numpy as np

from pyref import expf, f32

RV, RU = 17, 17        # W_V_AWS, W_U_AWS (cpp:5715)
GAMMA_C = f32(5)       # r_c (h:1478)
L_SCALE = 0.153787     # calW4_AWS's weight of the squared L difference

COEFFS = ((1777, 1541, 778), (871, 2929, 296), (73, 448, 3575))   # round(4096 M / white); X, Y, Z over R, G, B


@functools.lru_cache(maxsize=None)
def tables():
    """gam[256]: round(255 * 8 * sRGB-inverse(i / 255)); cb[3072]: round(32768 * f(i / (255 * 8)))."""
    x = np.arange(256, dtype=np.float64) / 255.0
    g = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    gam = np.rint(255.0 * 8.0 * g).astype(np.int64)
    t = np.arange(3072, dtype=np.float64) / (255.0 * 8.0)
    f = np.where(t < 0.008856, 7.787 * t + 0.13793103448275862, np.cbrt(t))
    cb = np.rint(32768.0 * f).astype(np.int64)
    return gam, cb


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def bgr2lab(bgr):
    """u8 [..., 3] BGR -> u8 [..., 3] (L, a, b)."""
    gam, cb = tables()
    bgr = np.asarray(bgr, np.uint8)
    B, G, R = (gam[bgr[..., i]] for i in range(3))
    fx, fy, fz = (cb[_descale(R * c[0] + G * c[1] + B * c[2], 12)] for c in COEFFS)
    L = _descale(296 * fy - 1336934, 15)
    a = _descale(500 * (fx - fy) + 128 * 32768, 15)
    b = _descale(200 * (fy - fz) + 128 * 32768, 15)
    return np.clip(np.stack([L, a, b], axis=-1), 0, 255).astype(np.uint8)


def refl(i, n):
    """BORDER_REFLECT_101 index of an integer array i into [0, n), reflecting as often as needed."""
    i = np.array(i, dtype=np.int64, copy=True)
    if n == 1:
        return np.zeros_like(i)
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i[lo] = -i[lo]
        hi = i >= n
        i[hi] = 2 * (n - 1) - i[hi]


def taps(rv=RV, ru=RU):
    return [(dv, du) for dv in range(-rv, rv + 1) for du in range(-ru, ru + 1)]


def weights(lab, rv=RV, ru=RU, gamma_c=GAMMA_C):
    """wt[v, u, tap] of one image's Lab plane (genWeight_AWS, calW4_AWS)."""
    lab = np.asarray(lab, np.uint8).astype(f32)
    H, W = lab.shape[:2]
    vv, uu = np.arange(H), np.arange(W)
    out = np.empty((H, W, (2 * rv + 1) * (2 * ru + 1)), f32)
    for t, (dv, du) in enumerate(taps(rv, ru)):
        q = lab[refl(vv + dv, H)][:, refl(uu + du, W)]
        d = (lab - q).astype(f32)
        sq = (d * d).astype(f32).astype(np.float64)
        s = ((sq[..., 0] * L_SCALE + sq[..., 1]) + sq[..., 2]).astype(f32)
        dif = np.sqrt(s.astype(np.float64)).astype(f32)
        out[..., t] = expf(((-dif).astype(f32) / f32(gamma_c)).astype(f32))
    return out


def aggregate(vm, wt0, wt1, lor, rv=RV, ru=RU):
    """calvm_AWS<LOR>: vm H x W x D raw costs of view LOR, wt0 / wt1 the left / right image's weights."""
    vm = np.ascontiguousarray(vm, f32)
    H, W, D = vm.shape
    u = np.arange(W)[:, None]
    d = np.arange(D)[None, :]
    u1 = u + d * lor            # [W, D]
    u2 = u - d * (1 - lor)
    ok = (u1 < W) & (u2 >= 0)
    u1c, u2c = np.clip(u1, 0, W - 1), np.clip(u2, 0, W - 1)
    numer = np.zeros((H, W, D), f32)
    denom = np.zeros((H, W, D), f32)
    vv, uu = np.arange(H), np.arange(W)
    for t, (dv, du) in enumerate(taps(rv, ru)):
        ele = (wt0[:, :, t][:, u1c] * wt1[:, :, t][:, u2c]).astype(f32)   # [H, W, D]
        denom = (denom + ele).astype(f32)
        c = vm[refl(vv + dv, H)][:, refl(uu + du, W)]
        numer = (numer + (ele * c).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (numer / denom).astype(f32)
    return np.where(ok[None], out, vm).astype(f32), ok


def aws(cost, lbgr, rbgr, rv=RV, ru=RU, gamma_c=GAMMA_C):
    """Both views: cost = [vm0, vm1] raw volumes (vm1 may be None) -> (volumes, in-range masks,
    weights of both images)."""
    wt = [weights(bgr2lab(img), rv, ru, gamma_c) for img in (lbgr, rbgr)]
    vols, oks = [], []
    for lor, vm in enumerate(cost):
        if vm is None:
            vols.append(None)
            oks.append(None)
            continue
        o, ok = aggregate(vm, wt[0], wt[1], lor, rv, ru)
        vols.append(o)
        oks.append(ok)
    return vols, oks, wt
