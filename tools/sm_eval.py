#!/usr/bin/env python3
"""Evaluate the GPU pipeline on a Middlebury-layout dataset, the way main_.cpp does (main:26-178).

usage: tools/sm_eval.py ROOT [--objects teddy cones ...] [--refine] [--pyr L] [--device N] [--stages]
                        [--so-variant so|so_R2L|so_T2D]

For each object: load (mystereomatching_amd.dataset), Parameters(maxdisp, ...), costCalculate per
pyramid level, SolveAll(PY_LEV, 0.3), dispOptimize [, refine], then calErr over nonocc / all /
disc at t = 1 (errorThreshold, h:225) and t = 2 (BASELINE's bad-2.0).  Prints one JSON line per
object.  --stages also prints the reference's err-txt lines (calErr after dispOptimize and after every stage of
refine(), h:1756-1817), one per stage, from the table the GPU builds while the pipeline runs (sm_eval_config).
--so-variant runs the scan-line optimiser instead of SGM: "so", or one of the calls dispOptimize keeps commented out
(cpp:1096-1100), "so_R2L" or "so_T2D" (sm_so_config).
No dataset ships with this repository; point ROOT at a local Middlebury copy.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from mystereomatching_amd import SolveAll, StereoMatching, dataset, pyrDown  # noqa: E402
from mystereomatching_amd.evaluate import cal_err_regions, format_err_lines  # noqa: E402


def run(sample, refine, levels, device):
    return run_stages(sample, refine, levels, device, False)[:2]


def run_stages(sample, refine, levels, device, stages=True, so_variant=None):
    """run() plus, with `stages`, calErr's err-txt lines of level 0 (one per stage).  so_variant: the scan-line
    optimiser of that name instead of SGM."""
    saved = (StereoMatching.optimization, StereoMatching.SO_VARIANT)
    StereoMatching.costcalculation, StereoMatching.aggregation = "censusGrad", "CBCA"
    StereoMatching.optimization = "so" if so_variant else "sgm"
    StereoMatching.SO_VARIANT = so_variant or "so"
    try:
        return _run_stages(sample, refine, levels, device, stages)
    finally:   # the selectors are process-wide statics: a later caller does not inherit the variant
        StereoMatching.optimization, StereoMatching.SO_VARIANT = saved


def _run_stages(sample, refine, levels, device, stages):
    StereoMatching.Do_refine = refine
    StereoMatching.Do_stageErrors = bool(stages) and sample.gt is not None
    masks = sample.masks if stages else {}
    imgs = sample.pair()
    sms, md, sc = [], sample.max_disp, 1
    t0 = time.perf_counter()
    for _ in range(levels):
        H, W = imgs["lgray"].shape
        prm = StereoMatching.Parameters(md, H, W, 13, 1, 2, 109, 10, "", sc)
        sm = StereoMatching(imgs["lbgr"], imgs["rbgr"], imgs["lgray"], imgs["rgray"], sample.gt if not (stages and sms) else None,
                            masks.get("all") if not sms else None, masks.get("nonocc") if not sms else None,
                            masks.get("disc") if not sms else None, prm, device=device)
        sm.costCalculate()
        sms.append(sm)
        md, sc = md // 2 + 1, sc * 2
        imgs = {k: pyrDown(v, device) for k, v in imgs.items()}
    SolveAll(sms, levels, 0.3)
    dp = sms[0].dispOptimize()
    if refine:
        dp = sms[0].refine()
    t = time.perf_counter() - t0
    lines = format_err_lines(sms[0].stageErrors()) if StereoMatching.Do_stageErrors else []
    return dp, t, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--objects", nargs="*", default=["teddy", "cones"])
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--pyr", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dataset", default="MD")
    ap.add_argument("--stages", action="store_true", help="print calErr's err-txt line of every stage")
    ap.add_argument("--so-variant", choices=["so", "so_R2L", "so_T2D"], default=None,
                    help="the scan-line optimiser of that name instead of SGM (sm_so_config)")
    a = ap.parse_args()
    for obj in a.objects:
        s = dataset.load(a.root, obj, a.dataset)
        dp, t, lines = run_stages(s, a.refine, a.pyr, a.device, a.stages, a.so_variant)
        out = {"object": obj, "H": s.lgray.shape[0], "W": s.lgray.shape[1], "D": s.max_disp + 1,
               "refine": a.refine, "py_lev": a.pyr, "seconds": round(t, 4)}
        if a.so_variant:
            out["so_variant"] = a.so_variant
        if s.gt is not None:
            for t_ in (1.0, 2.0):
                for r, (pbm, rms) in cal_err_regions(dp, s.gt, s.masks, t_).items():
                    out[f"bad{t_:.1f}_{r}"] = round(100 * pbm, 3)
                    if t_ == 1.0:
                        out[f"rms_{r}"] = round(rms, 4)
        print(json.dumps(out))
        for line in lines:
            print(line)


if __name__ == "__main__":
    main()
