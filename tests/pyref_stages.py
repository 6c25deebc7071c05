"""The reference's err txt on the CPU: the (name, map) list of every place where dispOptimize and refine() call
saveFromDisp<short, 0> (stereoMatching.cpp:1102, 1131, 1373-1501), and calErr's sums for one map (h:1748-1825).

TEST INFRASTRUCTURE ONLY.  The maps come from the oracle module's stage functions and the restatements
pyref_refine_ext, pyref_da and pyref_outlier, composed in refine()'s order like pyref_outlier.refine_outlier; the
sums are exact: integer counts and math.fsum over the float64 terms."""
import math

import numpy as np

import pyref_da as DA
import pyref_outlier as OC
import pyref_refine_ext as RX

f32 = np.float32
REGIONS = ("nonocc", "all", "disc")


def stage0_name(optimization="sgm", vmtop=False):
    """dispOptimize's name (cpp:1102, 1129-1131): "so"; "vmTop" with Do_vmTop after "sgm" or ""; else "wta"."""
    return "so" if optimization == "so" else ("vmTop" if vmtop else "wta")


def stage_names(cfg, optimization="sgm", vmtop=False, refine=True, do_pkr=False, do_bg=False, do_da=False):
    names = [stage0_name(optimization, vmtop)]
    if refine:
        names.append("od")
        names += ["PKR"] if do_pkr else []
        names += [f"RV{i}" for i in range(cfg.region_vote_nums)] if cfg.do_region_vote else []
        names += ["pi"] if cfg.do_proper_ipol else []
        names += ["BG"] if do_bg else []
        names += ["da"] if do_da else []
        names += ["mb"] if cfg.do_last_median else []
    return names


def chain(O, cfg, d0, d1, arms_l, bgr, vm=None, name0="wta", refine=True, classify=False, rv=False, itype=0,
          disp_mis=OC.DISP_MIS, do_pkr=False, do_bg=False, do_da=False, depth=RX.BG_IPL_DEPTH, vote=None,
          pkr_ratio=RX.RATIO_PKR):
    """[(name, map)] from DP[0] = d0 and DP[1] = d1 as dispOptimize left them; vm is vm[0] as it left it."""
    out = [(name0, np.ascontiguousarray(d0, np.int16).copy())]
    if not refine:
        return out
    D = cfg.D
    d = OC.lr_classify(d0, d1, D, cfg.lr_max_diff, cfg.disp_occ, disp_mis)[0] if classify else O.lr_check(d0, d1, cfg)
    out.append(("od", d.copy()))
    if do_pkr:
        d = RX.sign_dp(d, RX.cal_pkr(vm, f32(pkr_ratio)))
        out.append(("PKR", d.copy()))
    if cfg.do_region_vote:
        for i in range(cfg.region_vote_nums):
            d = (OC.rv_combine(d, arms_l, D, cfg.rv_s, cfg.rv_ratio, itype, depth, cfg.disp_occ, disp_mis, vote=vote) if rv
                 else O.region_vote(d, arms_l, cfg))
            out.append((f"RV{i}", d.copy()))
    if cfg.do_proper_ipol:
        for _ in range(cfg.region_vote_nums):
            d = O.proper_ipol(d, bgr, cfg)
        out.append(("pi", d.copy()))
    if do_bg:
        d = RX.bg_ipol(d, depth)
        out.append(("BG", d.copy()))
    if do_da:
        d = DA.discontinuity_adjust(d, vm)[0]
        out.append(("da", d.copy()))
    if cfg.do_last_median:
        d = O.median3(d)
        out.append(("mb", d.copy()))
    return out


def changed(ch):
    """Pixels each stage after the first changed against the stage before it."""
    return {ch[i][0]: int((ch[i][1] != ch[i - 1][1]).sum()) for i in range(1, len(ch))}


def pack(shape, masks):
    """bit r = (masks[r] == 255); None is an absent region."""
    out = np.zeros(shape, np.uint8)
    for r, m in enumerate(masks):
        if m is not None:
            out |= ((np.asarray(m) == 255).astype(np.uint8) << r).astype(np.uint8)
    return out


def stage_err(dp, gt, masks, thres):
    """calErr's sums per region: dict(count, invalid, bad[len(thres)], sum_sq) for each of the three masks (None:
    absent, all zero).  dif = |DT - (float)DP| in float32; the terms dif^2 in float64 (exact: 48 bits), 2.0 where
    DP < 0; sum_sq = math.fsum of them."""
    dp = np.asarray(dp, np.int16)
    gt = np.asarray(gt, f32)
    dif = np.abs(gt - dp.astype(f32)).astype(f32)
    term = np.where(dp >= 0, dif.astype(np.float64) ** 2, 2.0)
    out = []
    for m in masks:
        inr = np.zeros(dp.shape, bool) if m is None else (np.asarray(m) == 255)
        neg = inr & (dp < 0)
        out.append({"count": int(inr.sum()), "invalid": int(neg.sum()),
                    "bad": [int((neg | (inr & (dp >= 0) & (dif > f32(t)))).sum()) for t in thres],
                    "sum_sq": math.fsum(term[inr].tolist())})
    return out
