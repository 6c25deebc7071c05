"""Restatement of three stages of the reference's refine() (stereoMatching.cpp:1347-1510) -- TEST INFRASTRUCTURE.

  cal_pkr + sign_dp   Do_calPKR: calPKR (cpp:4087-4126) and signDp_UsingPKR (cpp:4128-4140)
  bg_ipol             Do_bgIpol: BGIpol (cpp:7323-7338) over backgroundInterpolateCore (cpp:7011-7043)
  subpixel + median3_f32   Do_subpixelEnhancement: subpixelEnhancement (cpp:6138-6167), medianBlur(SE, SE, 3) (cpp:1490)

Written from the reference's text as plain loops (the masked-slot second search, the sequential in-place row walk,
the round trip through int16), in float32 throughout.  The reference cannot be built here (no OpenCV), so this is
what the GPU stages are compared against; refine_ext composes it with the C oracle's LR check, region vote,
properIpol and median in refine()'s order.  bg_ipol_scan is the recurrence the kernel uses, kept apart
so that the host tests can compare the two.
"""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
RATIO_PKR = f32(0.1)       # cpp:4093
DISP_PKR = -4 * 16         # h:218
BG_IPL_DEPTH = 1000        # h:311
SE_REFERENCE, SE_FLOAT = 0, 1


def two_minima(costs):
    """calPKR's inner loops (cpp:4103-4117) on one pixel's costs: the first strict minimum, its slot overwritten with
    FLT_MAX, the first strict minimum again.  Returns (cost[0], cost[1])."""
    vmP = np.array(costs, f32)
    if vmP.size < 2:
        raise ValueError("calPKR is undefined for one cost: the second search writes slot -1")
    cost = []
    for _ in range(2):
        mn, disp = FLT_MAX, -1
        for d in range(vmP.size):
            if vmP[d] < mn:
                mn, disp = vmP[d], d
        cost.append(f32(mn))
        if disp < 0:
            raise ValueError("calPKR is undefined when no cost is below FLT_MAX")
        vmP[disp] = FLT_MAX
    return cost[0], cost[1]


def pkr_bad(c0, c1, ratio=RATIO_PKR):
    """cpp:4118: (cost[1] - cost[0]) / cost[1] < ratio_PKR, every step a float; NaN compares false."""
    with np.errstate(all="ignore"):
        return bool(f32(f32(c1) - f32(c0)) / f32(c1) < f32(ratio))


def cal_pkr(vm, ratio=RATIO_PKR):
    """PKR_Err_Mask (uint8 H x W) of a volume H x W x D."""
    H, W, _ = vm.shape
    mask = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            c0, c1 = two_minima(vm[v, u])
            if pkr_bad(c0, c1, ratio):
                mask[v, u] = 1
    return mask


def sign_dp(dp, mask, disp_pkr=DISP_PKR):
    """signDp_UsingPKR (cpp:4128-4140)."""
    out = np.array(dp, np.int16)
    out[(mask > 0) & (out >= 0)] = disp_pkr
    return out


def bg_core(row, u, depth):
    """backgroundInterpolateCore (cpp:7011-7043) on one row (a list of ints, read as it stands)."""
    W = len(row)
    vec = [-1, -1]
    coeffi = 1
    for k in range(2):   # +u first, then -u
        for d in range(1, depth + 1):
            un = u + d * coeffi
            if 0 <= un < W:
                if row[un] >= 0:
                    vec[k] = row[un]
                    break
            else:
                break
        coeffi *= -1
    if vec[0] != -1 and vec[1] == -1:
        return vec[0]
    if vec[0] == -1 and vec[1] != -1:
        return vec[1]
    return vec[0] if vec[0] < vec[1] else vec[1]


def bg_ipol(dp, depth=BG_IPL_DEPTH):
    """BGIpol (cpp:7323-7338): raster order, in place -- the left search sees this pass's fills."""
    out = np.array(dp, np.int16)
    for v in range(out.shape[0]):
        row = [int(x) for x in out[v]]
        for u in range(len(row)):
            if row[u] < 0:
                d = bg_core(row, u, depth)
                if d >= 0:
                    row[u] = d
        out[v] = row
    return out


def bg_ipol_scan(dp, depth=BG_IPL_DEPTH):
    """The same map as a first-order recurrence: y(u) = valid ? old(u) : min'(r(u), y(u - 1)), r(u) the nearest
    input-valid value in (u, u + depth], "none" = +infinity; a hole whose y is none keeps its value."""
    out = np.array(dp, np.int16)
    if depth < 1:
        return out
    NONE = 1 << 30
    for v in range(out.shape[0]):
        old = [int(x) for x in out[v]]
        W = len(old)
        r = [NONE] * W
        pos = -1
        for u in range(W - 1, -1, -1):
            if pos >= 0 and pos - u <= depth:
                r[u] = old[pos]
            if old[u] >= 0:
                pos = u
        y = NONE
        for u in range(W):
            y = old[u] if old[u] >= 0 else min(r[u], y)
            if y != NONE:
                out[v, u] = y
    return out


def subpixel_px(d, costs, mode=SE_REFERENCE):
    """subpixelEnhancement's body (cpp:6148-6164) for one pixel: d its disparity, costs its D costs."""
    D = len(costs)
    disp = int(d)
    out = f32(disp)
    if 0 < disp < D - 1:
        cost, cp, cm = f32(costs[disp]), f32(costs[disp + 1]), f32(costs[disp - 1])
        with np.errstate(all="ignore"):
            denom = f32(f32(2) * f32(f32(cp + cm) - f32(f32(2) * cost)))
            if denom != 0:
                diff = f32(f32(cp - cm) / denom)
                if diff > -1 and diff < 1:
                    val = f32(f32(disp) - diff)
                    # cpp:6161 `disp -= diff` on a short: the float difference converted back, truncating toward zero
                    out = val if mode == SE_FLOAT else f32(np.int16(np.trunc(val)))
    return out


def subpixel(dp, vm, mode=SE_REFERENCE):
    H, W = dp.shape
    se = np.empty((H, W), f32)
    for v in range(H):
        for u in range(W):
            se[v, u] = subpixel_px(dp[v, u], vm[v, u], mode)
    return se


def median3_f32(se):
    """cv::medianBlur(SE, SE, 3) on CV_32F: replicated borders, a copy is filtered."""
    p = np.pad(np.asarray(se, f32), 1, mode="edge")
    H, W = se.shape
    win = np.stack([p[i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=-1)
    return np.ascontiguousarray(np.sort(win, axis=-1)[:, :, 4])


def refine_ext(O, cfg, d0, d1, arms_l, bgr, vm, do_pkr=False, ratio=RATIO_PKR, disp_pkr=DISP_PKR, do_bg=False,
               depth=BG_IPL_DEPTH, do_se=False, mode=SE_REFERENCE):
    """refine() (cpp:1364-1506) with the oracle module O's stages around the three above.  vm is vm[0] as
    dispOptimize left it.  Returns dict(disp, mask, se) (mask / se None when their stage is off)."""
    d = O.lr_check(d0, d1, cfg)
    mask = se = None
    if do_pkr:
        mask = cal_pkr(vm, ratio)
        d = sign_dp(d, mask, disp_pkr)
    if cfg.do_region_vote:
        for _ in range(cfg.region_vote_nums):
            d = O.region_vote(d, arms_l, cfg)
    if cfg.do_proper_ipol:
        for _ in range(cfg.region_vote_nums):
            d = O.proper_ipol(d, bgr, cfg)
    if do_bg:
        d = bg_ipol(d, depth)
    if do_se:
        se = median3_f32(subpixel(d, vm, mode))
    if cfg.do_last_median:
        d = O.median3(d)
    return {"disp": d, "mask": mask, "se": se}
