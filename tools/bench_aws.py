#!/usr/bin/env python3
"""Aggregation "AWS" at the Teddy shape: step time, the aws_* kernels' times, taps per second.

bench.py's --agg cannot select AWS, so this tool times the same workload (Middlebury Teddy
450 x 375, D = 64, 16 synthetic pairs, censusGrad + AWS + SolveAll + SGM 4-path + WTA) through
StereoBatch: warm-up, then --steps timed sm_run calls ending in one synchronise; then the same
steps with per-kernel HIP-event timing (sm_profile_read).  AWS is bound by the vector ALU, not by
HBM: a tap is four separately rounded f32 operations (two products, two sums), so packed mul / add
at the issue rate of the 157.3 TFLOPS f32 peak (v_pk_fma_f32 counts two per lane) give
157.3 / 2 / 4 = 19.7 T taps/s.  The taps counted are those of the elements that aggregate
(u - d >= 0), S = (2 rv + 1)(2 ru + 1) each.  GF, NL and FIF run the same workload in the same
job for context.  Prints one JSON line.

  python tools/bench_aws.py [--steps 5] [--warmup 1] [--batch 16] [--radius 17] [--opt sgm|wta|so]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CEILING_TAPS = 157.3e12 / 2 / 4   # packed mul / add issue rate over four operations per tap


def timed_steps(sb, steps, warmup):
    for _ in range(warmup):
        sb.run(0.3, download=False)
    sb.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--radius", type=int, default=17)
    ap.add_argument("--opt", default="sgm", choices=["sgm", "wta", "so"])
    ap.add_argument("--no-context", action="store_true", help="skip the GF / NL / FIF runs")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B, R = args.rows, args.cols, args.max_disp, args.batch, args.radius
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    imgs = [batch[k] for k in ("lbgr", "rbgr", "lgray", "rgray")]
    sb = StereoBatch(md, H, W, B, device=args.device, aggregation="AWS", optimization=args.opt, num_streams=1,
                     aws_radius_v=R, aws_radius_u=R)
    try:
        sb.upload(*imgs)
        ms = timed_steps(sb, args.steps, args.warmup)
        disp = sb.download()
        sb.profile(True)
        sb.profile_reset()
        for _ in range(args.steps):
            sb.run(0.3, download=False)
        sb.synchronize()
        kernels = sb.profile_read()
        sb.profile(False)
    finally:
        sb.close()

    kern = {}
    for name, k in sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"]):
        kern[name] = {"ms_per_step": round(k["total_ms"] / args.steps, 4), "launches_per_step": k["launches"] / args.steps}
    aws_ms = sum(v["ms_per_step"] for n, v in kern.items() if n.startswith("aws_"))
    agg_ms = sum(v["ms_per_step"] for n, v in kern.items() if n.startswith("aws_agg"))
    in_range = sum(max(0, W - d) for d in range(D))   # (u, d) with u - d >= 0
    taps = float(B) * H * in_range * (2 * R + 1) ** 2
    rate = taps / (agg_ms * 1e-3) if agg_ms > 0 else 0.0
    context = {}
    if not args.no_context:
        for agg in ("GF", "NL", "FIF"):
            cb = StereoBatch(md, H, W, B, device=args.device, aggregation=agg, optimization=args.opt, num_streams=1)
            try:
                cb.upload(*imgs)
                context[agg + "_ms_per_step"] = round(timed_steps(cb, max(args.steps, 10), 2), 4)
            finally:
                cb.close()
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + AWS (radius {R}) + SolveAll + {args.opt}",
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 4),
           "pairs_per_s": round(B / (ms * 1e-3), 2),
           "aws_ms_per_step": round(aws_ms, 4), "aws_agg_ms_per_step": round(agg_ms, 4),
           "taps_per_step": taps, "taps_per_s": round(rate / 1e12, 4), "taps_per_s_unit": "T taps/s",
           "ceiling_taps_per_s": round(CEILING_TAPS / 1e12, 2),
           "share_of_ceiling": round(rate / CEILING_TAPS, 4),
           "valid_pixels": float((disp >= 0).mean()),
           "context": context, "kernels": kern}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
