"""Plain-loop restatement of refine()'s outlier classification, written from the reference's arithmetic:
LRConsistencyCheck with LOR = 0 (stereoMatching.cpp:2296-2326) and RV_combine_BG (cpp:7146-7216) with
cal_histogram_for_HV (cpp:6830-6862) and backgroundInterpolateCore (cpp:6964-7043).  It is the yardstick of
tests/test_outlier_host.py and tests/test_gpu_outlier.py; refine_outlier() composes it with the C oracle's
lr_check / region_vote / proper_ipol / median3 and with pyref_refine_ext / pyref_da in refine()'s order.

Not restated: the DT-based counters, their cout lines, the imwrite of the mask, RV_combine_BG's DT side channel.
One defined deviation: a value >= D in the map counts in validNum and in no bin (the reference indexes past its
histogram with it).
"""
import numpy as np

import pyref_da as DA
import pyref_refine_ext as RX

f32 = np.float32
DISP_OCC, DISP_MIS, DISP_PKR = -32, -48, -64
BG_IPL_DEPTH = 1000


# ---- the classifying LR check --------------------------------------------------------------------------

def lr_fails(d0, d1, max_diff):
    """The test LRConsistencyCheck shares with LRConsistencyCheck_normal; the int difference is compared as a float."""
    H, W = d0.shape
    bad = np.zeros((H, W), bool)
    md = f32(max_diff)
    for v in range(H):
        for u in range(W):
            d = int(d0[v, u])
            bad[v, u] = d < 0 or u - d < 0 or f32(abs(d - int(d1[v, u - d]))) > md
    return bad


def mismatch_loop(row1, u, D):
    """The reference's scan: some d' in [0, min(D, u + 1)) has DP1(u - d') == d'."""
    for dd in range(min(D, u + 1)):
        if int(row1[u - dd]) == dd:
            return True
    return False


def mismatch_scatter(row1, D):
    """The O(W) form for a whole row: u is a mismatch exactly when some x has 0 <= DP1(x) < D and x + DP1(x) == u
    (substitute x = u - d': d' = DP1(x) in [0, D) and x >= 0 is d' <= u)."""
    W = len(row1)
    flag = np.zeros(W, bool)
    for x in range(W):
        e = int(row1[x])
        if 0 <= e < D and x + e < W:
            flag[x + e] = True
    return flag


def lr_classify(d0, d1, D, max_diff=0.0, disp_occ=DISP_OCC, disp_mis=DISP_MIS, scatter=False):
    """Returns (labelled map, mask 0 / 255).  The scan reads DP1 only, so the order of the pixels does not matter."""
    d0 = np.asarray(d0, np.int16)
    d1 = np.asarray(d1, np.int16)
    H, W = d0.shape
    bad = lr_fails(d0, d1, max_diff)
    out = d0.copy()
    mask = np.zeros((H, W), np.uint8)
    for v in range(H):
        flags = mismatch_scatter(d1[v], D) if scatter else None
        for u in range(W):
            if bad[v, u]:
                mask[v, u] = 255
                mis = flags[u] if scatter else mismatch_loop(d1[v], u, D)
                out[v, u] = disp_mis if mis else disp_occ
    return out, mask


# ---- RV_combine_BG -------------------------------------------------------------------------------------------

def _above(count, valid, rv_ratio):
    """(float)hist[most] / validNum > rv_ratio: a float division and a strict compare; 0 / 0 compares false."""
    with np.errstate(invalid="ignore"):
        return bool(f32(count) / f32(valid) > f32(rv_ratio))


def vote_hv(dp, arms, v, u, D, rv_s, rv_ratio):
    """cal_histogram_for_HV: arms is H x W x 4 (L, R, U, D) of the left image."""
    hist = [0] * D
    valid = 0
    for vn in range(v - int(arms[v, u, 2]), v + int(arms[v, u, 3]) + 1):
        for un in range(u - int(arms[vn, u, 0]), u + int(arms[vn, u, 1]) + 1):
            q = int(dp[vn, un])
            if q >= 0:
                valid += 1
                if q < D:   # the deviation: the reference writes past its histogram here
                    hist[q] += 1
    if valid <= rv_s:
        return -1
    most = 0
    for d in range(1, D):
        if hist[d] > hist[most]:   # strict: the first most frequent value stays
            most = d
    return most if _above(hist[most], valid, rv_ratio) else -1


def vote_hv_rows(dp, arms, v, u, D, rv_s, rv_ratio):
    """vote_hv with each region row taken as a slice (the same counts; np.argmax returns the first maximum)."""
    hist = np.zeros(D, np.int64)
    valid = 0
    for vn in range(v - int(arms[v, u, 2]), v + int(arms[v, u, 3]) + 1):
        seg = dp[vn, u - int(arms[vn, u, 0]):u + int(arms[vn, u, 1]) + 1]
        seg = seg[seg >= 0]
        valid += len(seg)
        hist += np.bincount(seg[seg < D], minlength=D)
    if valid <= rv_s:
        return -1
    most = int(np.argmax(hist))
    return most if _above(hist[most], valid, rv_ratio) else -1


def fill_bg(dp, v, u, depth=BG_IPL_DEPTH):
    """backgroundInterpolateCore (both overloads reduce to this): the nearest value >= 0 to the right, then to the
    left, within `depth` columns; the smaller of those found, or -1."""
    W = dp.shape[1]
    found = []
    for step in (1, -1):
        for k in range(1, depth + 1):
            x = u + k * step
            if x < 0 or x >= W:
                break
            if dp[v, x] >= 0:
                found.append(int(dp[v, x]))
                break
    return min(found) if found else -1


def rv_combine(dp, arms, D, rv_s=20, rv_ratio=0.4, itype=0, depth=BG_IPL_DEPTH, disp_occ=DISP_OCC, disp_mis=DISP_MIS,
               stats=None, vote=None):
    """One call of RV_combine_BG: reads dp, returns the filled copy.  `vote` is vote_hv or vote_hv_rows.  `last` is
    the reference's dp_, declared outside both loops and left alone, under types 2 and 3, by a hole that is neither
    disp_occ nor disp_mis: such a hole takes the result of the nearest earlier classified hole in raster order (-1
    before the first).  stats (a dict) receives `carried`, the holes filled that way, and `last`, dp_ at the end."""
    dp = np.asarray(dp, np.int16)
    H, W = dp.shape
    out = dp.copy()
    vote_hv = vote or globals()["vote_hv"]
    last = -1
    carried = 0
    for v in range(H):
        for u in range(W):
            cur = int(dp[v, u])
            if cur >= 0:
                continue
            own = True
            if itype == 0:
                last = vote_hv(dp, arms, v, u, D, rv_s, rv_ratio)
            elif itype == 1:
                last = fill_bg(dp, v, u, depth)
            elif cur == disp_occ:
                bg = fill_bg(dp, v, u, depth)
                if itype == 2:
                    last = bg
                else:
                    rv = vote_hv(dp, arms, v, u, D, rv_s, rv_ratio)
                    if bg >= 0 and rv >= 0:
                        last = min(rv, bg)
                    elif bg >= 0:
                        last = bg
                    elif rv >= 0:
                        last = rv
                    else:
                        last = -1
            elif cur == disp_mis:
                last = vote_hv(dp, arms, v, u, D, rv_s, rv_ratio)
            else:
                own = False
            if last >= 0:
                out[v, u] = last
                carried += 0 if own else 1
    if stats is not None:
        stats["carried"] = carried
        stats["last"] = last
    return out


# ---- refine() --------------------------------------------------------------------------------------------------

def refine_outlier(O, cfg, d0, d1, arms_l, bgr, vm=None, classify=False, rv=False, itype=0, disp_mis=DISP_MIS,
                   do_pkr=False, do_bg=False, do_da=False, do_se=False, depth=BG_IPL_DEPTH, stats=None, vote=None,
                   pkr_ratio=RX.RATIO_PKR):
    """refine() (cpp:1364-1506) with the two source switches, the oracle module O's stages and the other
    restatements, in the reference's order.  Returns dict(disp, mask, pkr_mask, edges, se, labelled): `labelled` is
    the map right after the LR check; stats (a dict) receives what the non-vacuity checks need."""
    D = cfg.D
    mask = pkr = edges = se = None
    if classify:
        d, mask = lr_classify(d0, d1, D, cfg.lr_max_diff, cfg.disp_occ, disp_mis)
    else:
        d = O.lr_check(d0, d1, cfg)
    labelled = d.copy()
    if do_pkr:
        pkr = RX.cal_pkr(vm, f32(pkr_ratio))
        d = RX.sign_dp(d, pkr)
    if cfg.do_region_vote:
        for _ in range(cfg.region_vote_nums):
            d = (rv_combine(d, arms_l, D, cfg.rv_s, cfg.rv_ratio, itype, depth, cfg.disp_occ, disp_mis, vote=vote) if rv
                 else O.region_vote(d, arms_l, cfg))
    if cfg.do_proper_ipol:
        for i in range(cfg.region_vote_nums):
            nd = O.proper_ipol(d, bgr, cfg)
            if stats is not None and i == 0:
                # what the closest-colour rule gives where the smallest-disparity rule (DISP_OCC holes) ran
                other = d.copy()
                other[other == cfg.disp_occ] = -1 if cfg.disp_occ != -1 else -2
                alt = O.proper_ipol(other, bgr, cfg)
                occ = d == cfg.disp_occ
                stats["occ_rule_differs"] = int(((nd != alt) & occ & (nd >= 0)).sum())
            d = nd
    if do_bg:
        d = RX.bg_ipol(d, depth)
    if do_da:
        d, edges = DA.discontinuity_adjust(d, vm)
    if do_se:
        se = RX.median3_f32(RX.subpixel(d, vm, RX.SE_REFERENCE))
    if cfg.do_last_median:
        d = O.median3(d)
    return {"disp": d, "mask": mask, "pkr_mask": pkr, "edges": edges, "se": se, "labelled": labelled}
