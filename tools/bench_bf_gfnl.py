#!/usr/bin/env python3
"""Aggregations "BF" and "GFNL" at the Teddy shape: step times, per-kernel times, shares of the copy ceiling.

bench.py's --agg cannot select them, so this tool times the same workload (Middlebury Teddy
450 x 375, D = 64, 16 synthetic pairs, censusGrad + aggregation + SolveAll + SGM 4-path + WTA)
through StereoBatch, for each of BF, GFNL, GF, NL and CBCA in one job: warm-up, then --steps timed
sm_run calls ending in one synchronise; for BF and GFNL then the same steps with per-kernel
HIP-event timing (sm_profile_read).  BF's two sweeps move 4 + 8 + 8 + 4 = 24 B per element (read
p, write and read the double row sums, write q); their bytes over their time are stated as a share
of sm_copy_ceiling (a dwordx4 copy, read + write counted).  GFNL's step is quoted next to GF's
and NL's: the two together hold the cost and optimiser stages twice, so GFNL should stay below
their sum.  Prints one JSON line.

  python tools/bench_bf_gfnl.py [--steps 20] [--warmup 3] [--batch 16] [--opt sgm|wta]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_steps(sb, steps, warmup):
    for _ in range(warmup):
        sb.run(0.3, download=False)
    sb.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def profiled(sb, steps):
    sb.profile(True)
    sb.profile_reset()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    kernels = sb.profile_read()
    sb.profile(False)
    kern = {}
    for name, k in sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"]):
        per = k["total_ms"] / max(1, k["launches"])
        gbs = k["bytes_per_launch"] / (per * 1e-3) / 1e9 if per > 0 else 0.0
        kern[name] = {"ms_per_launch": round(per, 4), "launches_per_step": k["launches"] / steps,
                      "bytes_per_launch": k["bytes_per_launch"], "gbs": round(gbs, 1)}
    return kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--opt", default="sgm", choices=["sgm", "wta"])
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
    steps_ms, kern, valid = {}, {}, {}
    best = median = 0.0
    for agg in ("BF", "GFNL", "GF", "NL", "CBCA"):
        sb = StereoBatch(md, H, W, B, device=args.device, aggregation=agg, optimization=args.opt, num_streams=1)
        try:
            sb.upload(*imgs)
            steps_ms[agg] = round(timed_steps(sb, args.steps, args.warmup), 4)
            if agg in ("BF", "GFNL"):
                valid[agg] = float((sb.download() >= 0).mean())
                kern[agg] = profiled(sb, args.steps)
            if agg == "BF":
                best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
        finally:
            sb.close()

    nelem = float(B) * H * W * D
    bf = {n: v for n, v in kern["BF"].items() if n.startswith("bf_")}
    for v in bf.values():
        v["frac_of_copy_ceiling"] = round(v["gbs"] / best, 4)
    bf_ms = sum(v["ms_per_launch"] * v["launches_per_step"] for v in bf.values())
    bf_bytes = sum(v["bytes_per_launch"] * v["launches_per_step"] for v in bf.values())
    bf_gbs = bf_bytes / (bf_ms * 1e-3) / 1e9 if bf_ms > 0 else 0.0
    gfnl_own = sum(v["ms_per_launch"] * v["launches_per_step"] for n, v in kern["GFNL"].items() if n.startswith("gfnl_"))
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + aggregation + SolveAll + {args.opt}",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": steps_ms,
           "bf_ms_per_step": round(bf_ms, 4), "bf_bytes_per_element": round(bf_bytes / nelem, 2),
           "bf_gbs": round(bf_gbs, 1), "bf_frac_of_copy_ceiling": round(bf_gbs / best, 4) if best > 0 else None,
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(nelem * 4 / 1e6 / B, 1),
           "gfnl_mask_blend_ms_per_step": round(gfnl_own, 4),
           "gfnl_vs_gf_plus_nl": round(steps_ms["GFNL"] / (steps_ms["GF"] + steps_ms["NL"]), 4),
           "valid_pixels": valid, "kernels": kern}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
