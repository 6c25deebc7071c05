"""Numpy twin of the cost measures "SD", "BT", "grad", "TruncAD", "adGrad" and "ADCensusGrad"
(costCalculate, stereoMatching.cpp:954-987), for SMALL inputs only.

One function per measure, written from the reference text: float32 numpy ufuncs round every
operation on its own (no contraction), ADCensusGrad's blend runs in float64 as the reference's
double literals make it, and expf is the host libm's (pyref.expf).  The gradient images, the cross
arms and the census bits are pyref's.  view 0 pairs left u with right u - d, view 1 left u + d
with right u, as every measure's leftCoefficient / rightCoefficient do.
"""
from __future__ import annotations

import numpy as np

import pyref

f32 = np.float32
f64 = np.float64

METHODS = {"SD": 4, "BT": 5, "grad": 6, "TruncAD": 8, "adGrad": 9, "ADCensusGrad": 10}
W_AD = f32(0.11)            # adGrad (cpp:66): float parameters of gen_vm_from2vm_fixWgt
W_GRAD = f32(1 - 0.11)


def _pairs(W, D, view):
    """(d, u, uL, uR) with column slices: the in-range elements of disparity d pair the left columns
    [d, W) with the right columns [0, W - d) and belong to the focus pixels u = uL (view 0) or
    u = uR (view 1); the others keep the measure's default."""
    for d in range(min(D, W)):
        sl, sr = slice(d, W), slice(0, W - d)
        yield d, (sr if view == 1 else sl), sl, sr


def sd_cost(bgrL, bgrR, D, trunc=20, view=0):
    """gen_ad_sd_vm(.., AOS = 1, trunc) (cpp:2468-2509): sum += pow(abs(l - r), 2) in float."""
    H, W, _ = bgrL.shape
    L, R = bgrL.astype(f32), bgrR.astype(f32)
    out = np.full((H, W, D), f32(trunc), f32)
    for d, u, uL, uR in _pairs(W, D, view):
        a = np.abs(L[:, uL] - R[:, uR])
        s = np.zeros(a.shape[:2], f32)
        for c in range(3):
            s = (s + (a[..., c] * a[..., c]).astype(f32)).astype(f32)
        out[:, u, d] = np.minimum((s / f32(3)).astype(f32), f32(trunc))
    return out


def trunc_ad_cost(bgrL, bgrR, D, view=0):
    """gen_truncAD_vm (cpp:2511-2548): min(int sum, 60) stored as float."""
    H, W, _ = bgrL.shape
    L, R = bgrL.astype(np.int32), bgrR.astype(np.int32)
    out = np.full((H, W, D), f32(60), f32)
    for d, u, uL, uR in _pairs(W, D, view):
        out[:, u, d] = np.minimum(np.abs(L[:, uL] - R[:, uR]).sum(axis=-1), 60).astype(f32)
    return out


def nei_min_max(gray):
    """calNeiMaxMin (cpp:197-227): per pixel the min and max of I(u) and the half-way values to
    its neighbours; the edge columns have one neighbour."""
    I = gray.astype(f32)
    H, W = I.shape
    lo, hi = np.empty((H, W), f32), np.empty((H, W), f32)
    for u in range(W):
        cand = [I[:, u]]
        if u > 0:
            cand.append((0.5 * (gray[:, u - 1].astype(f64) + I[:, u])).astype(f32))
        if u < W - 1:
            cand.append((0.5 * (gray[:, u + 1].astype(f64) + I[:, u])).astype(f32))
        lo[:, u] = np.minimum.reduce(cand)
        hi[:, u] = np.maximum.reduce(cand)
    return lo, hi


def bt_cost(grayL, grayR, D, view=0):
    """bt (cpp:90-114) -> calCostForBT (cpp:142-195) on the gray images (cha = 1), trunc 20."""
    H, W = grayL.shape
    loL, hiL = nei_min_max(grayL)
    loR, hiR = nei_min_max(grayR)
    IL, IR = grayL.astype(f32), grayR.astype(f32)
    out = np.full((H, W, D), f32(20), f32)
    for d, u, uL, uR in _pairs(W, D, view):
        zero = np.zeros((H, W - d), f32)
        v0 = np.maximum(zero, np.maximum(loR[:, uR] - IL[:, uL], IL[:, uL] - hiR[:, uR]))
        v1 = np.maximum(zero, np.maximum(loL[:, uL] - IR[:, uR], IR[:, uR] - hiL[:, uL]))
        s = (zero + np.minimum(v0, v1)).astype(f32)
        out[:, u, d] = np.minimum((s / f32(1)).astype(f32), f32(20))
    return out


def grad_cost(grayL, grayR, arm_focus, D, trunc=500, view=0, adaptive=True):
    """grad(vm, trunc) (cpp:603-656) -> calgradvm: a min(|dgx|, T) + (1 - a) min(|dgy|, T) with
    the focus view's arm weights; (float)sqrt(2 T^2) out of range."""
    gx0, gy0 = pyref.grads(grayL)
    gx1, gy1 = pyref.grads(grayR)
    H, W = grayL.shape
    T = f32(trunc)
    out = np.full((H, W, D), f32(np.sqrt(float(T) ** 2 * 2)), f32)
    if adaptive:
        sH = np.minimum(arm_focus[..., 0], arm_focus[..., 1]).astype(f32)
        sV = np.minimum(arm_focus[..., 2], arm_focus[..., 3]).astype(f32)
        sH[sH == 0] = 1
        sV[sV == 0] = 1
        a = (sH / (sH + sV)).astype(f32)
        b = (f32(1) - a).astype(f32)
    else:
        a = b = np.ones((H, W), f32)
    for d, u, uL, uR in _pairs(W, D, view):
        dx = np.minimum(np.abs(gx0[:, uL] - gx1[:, uR]), T).astype(f32)
        dy = np.minimum(np.abs(gy0[:, uL] - gy1[:, uR]), T).astype(f32)
        out[:, u, d] = ((a[:, u] * dx).astype(f32) + (b[:, u] * dy).astype(f32)).astype(f32)
    return out


def ad_grad_parts(pair, D, view=0, arm_focus=None):
    """adGrad's two volumes (cpp:59-62): AD truncated at 7, grad truncated at 2."""
    if arm_focus is None:
        arm_focus = pyref.arms(pair["rbgr" if view else "lbgr"])
    A = pyref.ad_cost(pair["lbgr"], pair["rbgr"], D, 7, view=view)
    G = grad_cost(pair["lgray"], pair["rgray"], arm_focus, D, trunc=2, view=view)
    return A, G


def ad_grad_cost(pair, D, view=0, arm_focus=None):
    """gen_vm_from2vm_fixWgt (cpp:3767-3796): vm0 * wgt0 + vm1 * wgt1, float throughout."""
    A, G = ad_grad_parts(pair, D, view, arm_focus)
    return ((A * W_AD).astype(f32) + (G * W_GRAD).astype(f32)).astype(f32)


def census_bits(gray):
    """pyref.census's bit lists as one uint8 array [H, W, length]."""
    b = pyref.census(gray)
    return np.array([[b[v, u] for u in range(b.shape[1])] for v in range(b.shape[0])], np.uint8)


def census_cost(bitsL, bitsR, D, view=0):
    """censusCal(vm, 1) (gen_cenVM_XOR, h:936-981): the Hamming distance of the two bit strings, the
    code length out of range (pyref.census_cost, one disparity at a time)."""
    H, W, n = bitsL.shape
    out = np.full((H, W, D), f32(n), f32)
    for d, u, uL, uR in _pairs(W, D, view):
        out[:, u, d] = (bitsL[:, uL] != bitsR[:, uR]).sum(axis=-1).astype(f32)
    return out


def prepare(pair, census=False):
    """What the measures share per pair (computed once per test case): both images' cross arms and,
    for ADCensusGrad, their census bits."""
    pre = {"arms": (pyref.arms(pair["lbgr"]), pyref.arms(pair["rbgr"]))}
    if census:
        pre["census"] = (census_bits(pair["lgray"]), census_bits(pair["rgray"]))
    return pre


def ad_census_grad_parts(pair, D, view=0, arm_focus=None, census=None):
    """ADCensusGrad's three volumes (cpp:930-935): AD truncated at 255, census, grad at 500."""
    if arm_focus is None:
        arm_focus = pyref.arms(pair["rbgr" if view else "lbgr"])
    A = pyref.ad_cost(pair["lbgr"], pair["rbgr"], D, 255, view=view)
    bL, bR = census if census is not None else (census_bits(pair["lgray"]), census_bits(pair["rgray"]))
    Cn = census_cost(bL, bR, D, view=view)
    G = grad_cost(pair["lgray"], pair["rgray"], arm_focus, D, trunc=500, view=view)
    return A, Cn, G


def ad_census_grad_blend(A, Cn, G):
    """The live line of gen_vm_from3vm_exp (cpp:3635, 3640): float adCenv = 0.5 * A + 0.5 * C
    (double), then 0.7 * (1 - exp(-adCenv / 1)) + 0.3 * (1 - exp(-G / 2)): the exponentials and
    1 - e are float, the two products and their sum double."""
    m = (0.5 * A.astype(f64) + 0.5 * Cn.astype(f64)).astype(f32)
    e0 = (f32(1) - pyref.expf((-m / f32(1)).astype(f32))).astype(f32)
    e1 = (f32(1) - pyref.expf((-G / f32(2)).astype(f32))).astype(f32)
    return (0.7 * e0.astype(f64) + 0.3 * e1.astype(f64)).astype(f32)


def ad_census_grad_cost(pair, D, view=0, arm_focus=None, census=None):
    return ad_census_grad_blend(*ad_census_grad_parts(pair, D, view, arm_focus, census))


def cost_volume(pair, D, method, view=0, arm_focus=None, census=None):
    """The raw volume of `method` (a costcalculation string) with the reference's call-site constants.
    arm_focus: the focus view's arms, census: both images' census_bits (computed here when absent)."""
    if method == "SD":
        return sd_cost(pair["lbgr"], pair["rbgr"], D, 20, view)
    if method == "TruncAD":
        return trunc_ad_cost(pair["lbgr"], pair["rbgr"], D, view)
    if method == "BT":
        return bt_cost(pair["lgray"], pair["rgray"], D, view)
    if arm_focus is None:
        arm_focus = pyref.arms(pair["rbgr" if view else "lbgr"])
    if method == "grad":
        return grad_cost(pair["lgray"], pair["rgray"], arm_focus, D, 500, view)
    if method == "adGrad":
        return ad_grad_cost(pair, D, view, arm_focus)
    if method == "ADCensusGrad":
        return ad_census_grad_cost(pair, D, view, arm_focus, census)
    raise KeyError(method)


def pipeline(pair, D, method, iters=2, solve=True, opt="sgm", paths=4, refine=False, pre=None):
    """cost -> CBCA (iters) -> SolveAll -> sgm / so / WTA [-> refine()]; returns the map (and keeps
    to pyref's stages throughout).  so runs on the left view only here (DP[0])."""
    pre = pre or prepare(pair, census=method == "ADCensusGrad")
    aL, aR = pre["arms"]

    def view_map(v):
        vm = cost_volume(pair, D, method, v, aR if v else aL, pre.get("census"))
        if iters:
            vm = pyref.cbca(vm, aL, aR, iters=iters, view=v)
        if solve:
            vm = pyref.solve_all(vm)
        if opt == "sgm":
            vm = pyref.sgm(vm, pair["rbgr" if v else "lbgr"], paths=paths)
        elif opt == "so":
            return pyref.so(vm, pair["lbgr"])[1]
        return pyref.wta(vm)

    d0 = view_map(0)
    if refine:
        d0 = pyref.refine(d0, view_map(1), aL, pair["lbgr"], D)
    return d0
