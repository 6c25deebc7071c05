#!/usr/bin/env python3
"""The cost-volume kernel of every cost measure at the Teddy shape: ms, elements/s, share of the copy ceiling.

The workload is bench.py's Teddy leg (Middlebury Teddy 450 x 375, D = 64, 16 synthetic pairs, cost +
CBCA + SolveAll + SGM 4-path + WTA) through StereoBatch, one context per costcalculation string, all in
one job and from one build: the six measures of k_cost_ext (SD, BT, grad, TruncAD, adGrad,
ADCensusGrad) and, as the yardstick, k_cost's four (censusGrad, Census, ADCensus, AD).  Per measure:
warm-up, --steps timed sm_run calls ending in one synchronise (ms per step), then the same steps with
per-kernel HIP-event timing (sm_profile_read) for the `cost_volume` kernel.  The cost kernel's first
CBCA sweep fusion is switched off (fuse_cost_scan = 0) so that censusGrad has a cost_volume launch of
its own to compare with.  The kernel writes 4 B per element; that store rate is stated as a share of
sm_copy_ceiling (a dwordx4 copy, read + write counted) measured in the same job.  Teddy's volume fits
the 256 MB cache, so this is no HBM-roofline fraction.  Prints one JSON line.

  python tools/bench_cost.py [--steps 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW = ("SD", "BT", "grad", "TruncAD", "adGrad", "ADCensusGrad")
OLD = ("censusGrad", "Census", "ADCensus", "AD")


def timed_steps(sb, steps, warmup):
    for _ in range(warmup):
        sb.run(0.3, download=False)
    sb.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def cost_kernel(sb, steps):
    sb.profile(True)
    sb.profile_reset()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    kernels = sb.profile_read()
    sb.profile(False)
    k = kernels["cost_volume"]
    return k["total_ms"] / max(1, k["launches"]), k["launches"] / steps, k["bytes_per_launch"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B = args.rows, args.cols, args.max_disp, args.batch
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    imgs = [batch[k] for k in ("lbgr", "rbgr", "lgray", "rgray")]
    nelem = float(B) * H * W * D
    rows, best, median = {}, 0.0, 0.0
    for cost in NEW + OLD:
        # one stream and one pair group: a single cost_volume launch per step covers all B pairs
        sb = StereoBatch(md, H, W, B, device=args.device, cost_method=cost, num_streams=1, sub_batch=B, fuse_cost_scan=0)
        try:
            sb.upload(*imgs)
            step_ms = timed_steps(sb, args.steps, args.warmup)
            valid = float((sb.download() >= 0).mean())
            ms, launches, nbytes = cost_kernel(sb, args.steps)
            if best == 0.0:
                best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
        finally:
            sb.close()
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        rows[cost] = {"cost_volume_ms": round(ms, 4), "launches_per_step": launches,
                      "elements_per_launch": nbytes / 4.0,
                      "gelem_per_s": round(nbytes / 4.0 / (ms * 1e-3) / 1e9, 2) if ms > 0 else None,
                      "store_gbs": round(gbs, 1), "ms_per_step": round(step_ms, 4), "valid_pixels": valid}
    for r in rows.values():
        r["store_frac_of_copy_ceiling"] = round(r["store_gbs"] / best, 4) if best > 0 else None
    ref = rows["censusGrad"]["cost_volume_ms"]
    out = {"workload": f"{W}x{H} D={D} x{B}, cost + CBCA + SolveAll + sgm (4 paths), fuse_cost_scan = 0",
           "steps": args.steps, "warmup": args.warmup, "elements": nelem, "volume_mb_per_pair": round(nelem * 4 / 1e6 / B, 1),
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "yardstick_censusGrad_cost_volume_ms": ref,
           "vs_censusGrad": {c: round(rows[c]["cost_volume_ms"] / ref, 3) for c in rows} if ref > 0 else None,
           "new": {c: rows[c] for c in NEW}, "existing": {c: rows[c] for c in OLD}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
