#!/usr/bin/env python3
"""The three scan-line optimisers (sm_so_config: so, so_R2L, so_T2D) at the Teddy shape in one process: ms per step,
each optimiser kernel's time, and its algorithmic bytes per second against the copy ceiling of the same job.

The workload is bench.py's Teddy one with optimization "so" (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA
+ SolveAll + so on both views) through StereoBatch, one stream.  Per variant, in the order so, so_R2L, so_T2D, so
again: warm-up, then --steps timed sm_run calls ending in one synchronise, then the same steps with per-kernel
HIP-event timing (sm_profile_read).  The kernels' bytes are the library's own (so and so_R2L: 4 B read and a 1 B trace
code per volume element; so_T2D: 4 B read, no write); bytes over time are stated as a share of sm_copy_ceiling (a
dwordx4 copy, read + write counted) measured in the same job.  Teddy's volumes fit the 256 MB cache, so this is no
HBM-roofline fraction.  Prints one JSON line (and writes it to --out).

  python tools/bench_so.py [--steps 20] [--warmup 3] [--batch 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VARIANTS = ("so", "so_R2L", "so_T2D")
KERNEL_OF = {"so": "so", "so_R2L": "so_r2l", "so_T2D": "so_t2d"}   # profile names; the right view's end in _r


def is_so_kernel(name, variant):
    base = KERNEL_OF[variant]
    return name in (base, base + "_r")


def per_step(v):
    return v["ms_per_launch"] * v["launches_per_step"]


def summarise(kern, variant, ceiling_gbs):
    """The variant's optimiser kernels (left and right view): ms per launch, launches per step, bytes per launch, GB/s
    and share of the copy ceiling; and their sum per step."""
    rows = {}
    for name, v in kern.items():
        if not is_so_kernel(name, variant):
            continue
        row = dict(v)
        if v["ms_per_launch"] > 0:
            gbs = v["bytes_per_launch"] / (v["ms_per_launch"] * 1e-3) / 1e9
            row["gbs"] = round(gbs, 1)
            row["frac_of_copy_ceiling"] = round(gbs / ceiling_gbs, 4) if ceiling_gbs > 0 else None
        rows[name] = row
    return {"kernels": rows, "ms_per_step": round(sum(per_step(v) for v in rows.values()), 4)}


def ratios(summary):
    """Each variant's optimiser ms per step over so's (None when so took no measurable time)."""
    base = summary["so"]["ms_per_step"]
    return {v: (round(summary[v]["ms_per_step"] / base, 4) if base > 0 else None) for v in VARIANTS if v != "so"}


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
        kern[name] = {"ms_per_launch": round(per, 4), "launches_per_step": k["launches"] / steps,
                      "bytes_per_launch": k["bytes_per_launch"]}
    return kern


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    return args


def main():
    args = parse()

    import numpy as np

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B = args.rows, args.cols, args.max_disp, args.batch
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    imgs = [np.ascontiguousarray(batch[k]) for k in ("lbgr", "rbgr", "lgray", "rgray")]

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1, optimization="so")
    ms, kern, maps = {}, {}, {}
    try:
        sb.upload(*imgs)
        for v in VARIANTS:
            sb.so_config(v)
            ms[v] = timed_steps(sb, args.steps, args.warmup)
            maps[v] = sb.download()
            kern[v] = profiled(sb, args.steps)
        sb.so_config("so")
        ms["so_again"] = timed_steps(sb, args.steps, args.warmup)
        if not np.array_equal(sb.download(), maps["so"]):
            raise SystemExit("so's maps changed after switching to the variants and back")
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    summary = {v: summarise(kern[v], v, best) for v in VARIANTS}
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + so (both views), one stream",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": {k: round(x, 4) for k, x in ms.items()},
           "optimiser": summary,
           "optimiser_ms_over_so": ratios(summary),
           "pixels_differing_from_so": {v: float((maps[v] != maps["so"]).mean()) for v in VARIANTS if v != "so"},
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(float(H) * W * D * 4 / 1e6, 1),
           "kernels": kern}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
