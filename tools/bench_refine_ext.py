#!/usr/bin/env python3
"""refine()'s peak-ratio check, background fill and sub-pixel map (sm_refine_ext_config) at the Teddy shape: step
times with the stages off, each alone and all on, and the new kernels' times and bytes against the copy ceiling.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) with do_refine, through StereoBatch, one stream, in one process.  For every configuration: warm-up,
then --steps timed sm_run calls ending in one synchronise, then the same steps with per-kernel HIP-event timing
(sm_profile_read).  A last configuration switches vmTop on beside the stages, so that vmtop_select -- which reads
the same volume in the same pattern as refine_pkr -- is timed in the same job.  Every kernel's algorithmic bytes
over its time are stated as a share of sm_copy_ceiling (a dwordx4 copy, read + write counted) measured in the same
job.  Teddy's volumes fit the 256 MB cache in part, so this is no HBM-roofline fraction.  With PKR or SE on, SGM's
last pass also writes its path sum (4 B per element more): sgm_last_wta's time is listed for every configuration.
Prints one JSON line.

  python tools/bench_refine_ext.py [--steps 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_KERNELS = ("refine_pkr", "refine_bg_ipol", "refine_subpixel", "refine_median3_f32")
# name -> sm_refine_ext_config's switches; "all_on_vmtop" adds sm_vmtop_config (method 0, 2 candidates)
CONFIGS = [("all_off", {}), ("pkr", {"do_pkr": True}), ("bg_ipol", {"do_bg_ipol": True}), ("subpixel", {"do_subpixel": True}),
           ("all_on", {"do_pkr": True, "do_bg_ipol": True, "do_subpixel": True}),
           ("all_on_vmtop", {"do_pkr": True, "do_bg_ipol": True, "do_subpixel": True})]


def kernel_shares(kern, ceiling_gbs, names=NEW_KERNELS + ("vmtop_select", "sgm_last_wta")):
    """Per kernel of `names` present in the profile: ms per launch, bytes per launch, GB/s and the share of the
    copy ceiling."""
    out = {}
    for n in names:
        k = kern.get(n)
        if not k:
            continue
        ms, by = k["ms_per_launch"], k["bytes_per_launch"]
        gbs = by / (ms * 1e-3) / 1e9 if ms > 0 else None
        out[n] = {"ms": ms, "bytes": by, "gbs": round(gbs, 1) if gbs is not None else None,
                  "frac_of_copy_ceiling": round(gbs / ceiling_gbs, 4) if gbs is not None and ceiling_gbs > 0 else None}
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
        if k["launches"] == 0:   # a name an earlier configuration registered: not launched in this one
            continue
        per = k["total_ms"] / k["launches"]
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

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1, do_refine=1)
    ms, kerns, stats = {}, {}, {}
    try:
        sb.upload(*imgs)
        for name, cfg in CONFIGS:
            sb.vmtop_config(name == "all_on_vmtop", 0, 2, float(np.float32(1.09)), 10, True, False)
            sb.refine_ext_config(**cfg)
            ms[name] = round(timed_steps(sb, args.steps, args.warmup), 4)
            maps = sb.download()
            st = {"holes_left": float((maps < 0).mean())}
            if cfg.get("do_pkr"):
                st["pkr_marked_pair0"] = float(sb.get_pkr_mask().mean())
            if cfg.get("do_subpixel"):
                se = sb.download_subpixel()
                st["se_differs_from_map"] = float((se != maps).mean())
            stats[name] = st
            kerns[name] = profiled(sb, args.steps)
        sb.vmtop_config(False, 0, 2, float(np.float32(1.09)), 10, True, False)
        sb.refine_ext_config()
        ms["all_off_again"] = round(timed_steps(sb, args.steps, args.warmup), 4)
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm + refine, one stream",
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
           "minus_all_off_ms": {k: round(v - ms["all_off"], 4) for k, v in ms.items() if k != "all_off"},
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(float(H) * W * D * 4 / 1e6, 1), "maps": stats,
           "new_kernels": {name: kernel_shares(k, best) for name, k in kerns.items()},
           "kernels_all_on": kerns["all_on"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
