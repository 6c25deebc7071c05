#!/usr/bin/env python3
"""Aggregation "FIF" at the Teddy shape: step time, per-kernel times, share of the copy ceiling.

bench.py's --agg cannot select FIF, so this tool times the same workload (Middlebury Teddy
450 x 375, D = 64, 16 synthetic pairs, censusGrad + FIF + SolveAll + SGM 4-path + WTA) through
StereoBatch: warm-up, then --steps timed sm_run calls ending in one synchronise; then the same
steps with per-kernel HIP-event timing (sm_profile_read), and each FIF kernel's algorithmic bytes
over its time as a share of sm_copy_ceiling (a dwordx4 copy, read + write counted).  Prints one
JSON line.

  python tools/bench_fif.py [--steps 20] [--warmup 3] [--batch 16] [--mode 0|1] [--opt sgm|wta|so]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--mode", type=int, default=0, choices=[0, 1], help="0 = FIF_Improve, 1 = FIF (plain)")
    ap.add_argument("--opt", default="sgm", choices=["sgm", "wta", "so"])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B = args.rows, args.cols, args.max_disp, args.batch
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    sb = StereoBatch(md, H, W, B, device=args.device, aggregation="FIF", fif_mode=args.mode, optimization=args.opt,
                     num_streams=1)
    try:
        sb.upload(*(batch[k] for k in ("lbgr", "rbgr", "lgray", "rgray")))
        for _ in range(args.warmup):
            sb.run(0.3, download=False)
        sb.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sb.run(0.3, download=False)
        sb.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        disp = sb.download()

        sb.profile(True)
        sb.profile_reset()
        for _ in range(args.steps):
            sb.run(0.3, download=False)
        sb.synchronize()
        kernels = sb.profile_read()
        sb.profile(False)
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    kern = {}
    for name, k in sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"]):
        per = k["total_ms"] / max(1, k["launches"])
        gbs = k["bytes_per_launch"] / (per * 1e-3) / 1e9 if per > 0 else 0.0
        kern[name] = {"ms_per_launch": round(per, 4), "launches_per_step": k["launches"] / args.steps,
                      "bytes_per_launch": k["bytes_per_launch"], "gbs": round(gbs, 1)}
        if name.startswith("fif_"):
            kern[name]["frac_of_copy_ceiling"] = round(gbs / best, 4)
    fif_ms = sum(v["ms_per_launch"] * v["launches_per_step"] for n, v in kern.items() if n.startswith("fif_"))
    fif_bytes = sum(v["bytes_per_launch"] * v["launches_per_step"] for n, v in kern.items() if n.startswith("fif_"))
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + FIF (fif_mode {args.mode}) + SolveAll + {args.opt}",
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 4),
           "pairs_per_s": round(B / (ms * 1e-3), 1),
           "fif_ms_per_step": round(fif_ms, 4),
           "fif_bytes_per_element": round(fif_bytes / (B * H * W * D), 2),
           "fif_gbs": round(fif_bytes / (fif_ms * 1e-3) / 1e9, 1) if fif_ms > 0 else None,
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "valid_pixels": float((disp >= 0).mean()),
           "kernels": kern}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
