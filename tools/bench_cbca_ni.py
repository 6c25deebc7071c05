#!/usr/bin/env python3
"""Cross-based aggregation without arm intersection (sm_cbca_intersect_config(ctx, 0)) at the Teddy shape: step
times with intersection on and off, the times of the `_ni` kernels, their algorithmic bytes against the copy
ceiling, and CBCA's share of the step in both modes.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll + SGM
4-path) through StereoBatch, one stream, in one process.  Warm-up, then --steps timed sm_run calls ending in one
synchronise, first with intersection on (the default path), then off, then on again; each mode's steps are then
repeated with per-kernel HIP-event timing (sm_profile_read).  Every `_ni` kernel moves 8 B per volume element
(the prefix reads and writes the volume in place; the window reads every prefix position once from memory and
writes the other volume); those bytes over its time are stated as a share of sm_copy_ceiling (a dwordx4 copy,
read + write counted) measured in the same job.  Teddy's volumes fit the 256 MB cache, so this is no HBM-roofline
fraction.  Prints one JSON line.

  python tools/bench_cbca_ni.py [--steps 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NI_BYTES_PER_ELEMENT = 8.0   # every `_ni` kernel: 4 B read + 4 B written per volume element


def is_cbca(name):
    """Kernels of the aggregation itself: the sweeps of the intersecting form or the `_ni` kernels.  The cost
    volume belongs to it too: the intersecting form computes the costs inside its first sweep."""
    return name.startswith("cbca_") or name.startswith("cost_volume")


def per_step(v):
    return v["ms_per_launch"] * v["launches_per_step"]


def cbca_share(kern):
    """(CBCA + cost ms per step, all kernels' ms per step, the share)."""
    total = sum(per_step(v) for v in kern.values())
    agg = sum(per_step(v) for n, v in kern.items() if is_cbca(n))
    return round(agg, 4), round(total, 4), (round(agg / total, 4) if total > 0 else None)


def summarise_ni(kern, elements, ceiling_gbs):
    """Per `_ni` kernel: ms per launch, launches per step, bytes per element, GB/s and share of the copy ceiling."""
    out = {}
    for name, v in kern.items():
        if not name.endswith("_ni"):
            continue
        bpe = v["bytes_per_launch"] / elements if elements else None
        row = {"ms_per_launch": v["ms_per_launch"], "launches_per_step": v["launches_per_step"], "bytes_per_element": bpe}
        if v["ms_per_launch"] > 0:
            gbs = v["bytes_per_launch"] / (v["ms_per_launch"] * 1e-3) / 1e9
            row["gbs"] = round(gbs, 1)
            row["frac_of_copy_ceiling"] = round(gbs / ceiling_gbs, 4) if ceiling_gbs > 0 else None
        out[name] = row
    return out


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
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
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

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1)
    try:
        sb.upload(*imgs)
        on_ms = timed_steps(sb, args.steps, args.warmup)
        isect = sb.download()
        kern_on = profiled(sb, args.steps)
        sb.cbca_intersect_config(False)
        off_ms = timed_steps(sb, args.steps, args.warmup)
        maps = sb.download()
        area = sb.get_cbca_area(0)
        kern_off = profiled(sb, args.steps)
        sb.cbca_intersect_config(True)
        on2_ms = timed_steps(sb, args.steps, args.warmup)
        if not np.array_equal(sb.download(), isect):
            raise SystemExit("the intersect maps changed after switching intersection off and on again")
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    elements = float(B) * H * W * D
    a_on, t_on, s_on = cbca_share(kern_on)
    a_off, t_off, s_off = cbca_share(kern_off)
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm, one stream",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": {"intersect_on": round(on_ms, 4), "intersect_off": round(off_ms, 4),
                           "intersect_on_again": round(on2_ms, 4)},
           "off_minus_on_ms": round(off_ms - on_ms, 4),
           "cbca_and_cost_ms": {"intersect_on": a_on, "intersect_off": a_off},
           "kernel_sum_ms": {"intersect_on": t_on, "intersect_off": t_off},
           "cbca_share_of_step": {"intersect_on": s_on, "intersect_off": s_off},
           "pixels_changed_without_intersection": float((maps != isect).mean()),
           "mean_area_pair0": float(area.mean()), "max_area_pair0": int(area.max()),
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(float(H) * W * D * 4 / 1e6, 1),
           "ni_kernels": summarise_ni(kern_off, elements, best),
           "kernels_intersect_on": kern_on, "kernels_intersect_off": kern_off}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
