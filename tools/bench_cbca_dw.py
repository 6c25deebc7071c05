#!/usr/bin/env python3
"""CBCA's double window (sm_cbca_double_config) at the Teddy shape: step times with and without it, the times of
its kernels and of the second aggregation run, and the selection kernel's bytes against the copy ceiling.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) through StereoBatch, one stream, in one process -- with the left two thirds of every image's columns
replaced by their 5 x 5 box mean, as in the test fixtures: the raw synthetic texture has only short arms and
would select every pixel.  Warm-up, then --steps timed sm_run calls ending in one synchronise, first with the
double window off, then on (window 1 = 23 / 23 / 30 / 0, threshold 5), then the same steps with per-kernel
HIP-event timing (sm_profile_read), then off again.  dw_select moves 8 B per selected volume element (4 read,
4 written) plus 1 B of mask per pixel; those bytes over its time are stated as a share of sm_copy_ceiling (a
dwordx4 copy, read + write counted) measured in the same job.  The selected share comes from every pair's mask,
recomputed on the host from the CPU oracle's window-0 arms (pair 0's is checked against sm_get_cbca_dw_mask).
Teddy's volumes fit the 256 MB cache, so this is no HBM-roofline fraction.  Prints one JSON line.

  python tools/bench_cbca_dw.py [--steps 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW1 = (23, 23, 30, 0, 5.0)


def soften(img):
    """The left two thirds of the columns replaced by their 5 x 5 integer box mean (edge padding, floor division)."""
    import numpy as np
    a = img.astype(np.int32)
    H, W = a.shape[:2]
    p = np.pad(a, ((2, 2), (2, 2), (0, 0)), mode="edge")
    s = np.zeros_like(a)
    for dy in range(5):
        for dx in range(5):
            s += p[dy:dy + H, dx:dx + W]
    out = img.copy()
    out[:, :W * 2 // 3] = (s // 25).astype(np.uint8)[:, :W * 2 // 3]
    return out


def mask_from_arms(arms, isum=45):
    """arm_Mask from an H x W x 4 arm array: the 3 x 3 BORDER_REFLECT_101 sum of the four arms' maximum < isum
    (45: the integer form of `boxFilter < 5`)."""
    import numpy as np
    m = np.asarray(arms).astype(np.int64).max(axis=2)
    H, W = m.shape
    ri = [1] + list(range(H)) + [H - 2]
    ci = [1] + list(range(W)) + [W - 2]
    p = m[ri][:, ci]
    s = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3))
    return (s < isum).astype(np.uint8)


def select_bytes(selected_pixels, pixels, D, views=1):
    """dw_select's traffic: 8 B per selected volume element (read + write) and the mask's 1 B per pixel, per view."""
    return views * (8 * selected_pixels * D + pixels)


def summarise(kern, sel_bytes, ceiling_gbs):
    """From the per-kernel profile: the mask, the selection (time, GB/s over its true bytes, share of the copy
    ceiling) and the second aggregation run (window 1's arms, the raw-cost copy if any, the *_dw sweeps)."""
    per_step = lambda v: v["ms_per_launch"] * v["launches_per_step"]
    second = {n: v for n, v in kern.items() if n.endswith("_dw") or n.startswith("dw_copy_raw")}
    sel = kern.get("dw_select")
    out = {"dw_mask_ms": kern["dw_mask"]["ms_per_launch"] if "dw_mask" in kern else None,
           "dw_select_ms": sel["ms_per_launch"] if sel else None,
           "second_run_ms": round(sum(per_step(v) for v in second.values()), 4),
           "second_run_kernels": {n: v["ms_per_launch"] for n, v in second.items()},
           "first_run_ms": round(sum(per_step(v) for n, v in kern.items() if n.startswith("cbca_") and n not in second), 4),
           "dw_select_bytes": sel_bytes}
    if sel and sel["ms_per_launch"] > 0:
        gbs = sel_bytes / (sel["ms_per_launch"] * 1e-3) / 1e9
        out["dw_select_gbs"] = round(gbs, 1)
        out["dw_select_frac_of_copy_ceiling"] = round(gbs / ceiling_gbs, 4) if ceiling_gbs > 0 else None
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
    from oracle import oracle as O

    H, W, md, B = args.rows, args.cols, args.max_disp, args.batch
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    for k in ("lbgr", "rbgr"):
        batch[k] = np.ascontiguousarray(np.stack([soften(im) for im in batch[k]]))
    batch["lgray"], batch["rgray"] = S.bgr_to_gray(batch["lbgr"]), S.bgr_to_gray(batch["rbgr"])
    imgs = [np.ascontiguousarray(batch[k]) for k in ("lbgr", "rbgr", "lgray", "rgray")]
    cfg = O.config(H, W, md)
    masks = np.stack([mask_from_arms(O.arms(im, cfg)) for im in batch["lbgr"]])

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1)
    try:
        sb.upload(*imgs)
        off_ms = timed_steps(sb, args.steps, args.warmup)
        plain = sb.download()
        sb.cbca_double_config(True, *WINDOW1)
        on_ms = timed_steps(sb, args.steps, args.warmup)
        maps = sb.download()
        if not np.array_equal(sb.get_cbca_dw_mask(), masks[0]):
            raise SystemExit("pair 0's device mask differs from the host's")
        kern = profiled(sb, args.steps)
        sb.cbca_double_config(False, *WINDOW1)
        off2_ms = timed_steps(sb, args.steps, args.warmup)
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    selected = int(masks.sum())
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm, left 2/3 of the columns softened; "
                       "double window 23/23/30/0, threshold 5",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": {"double_off": round(off_ms, 4), "double_on": round(on_ms, 4), "double_off_again": round(off2_ms, 4)},
           "double_on_minus_off_ms": round(on_ms - off_ms, 4),
           "selected_share": round(selected / masks.size, 4),
           "selected_share_per_pair": [round(float(m.mean()), 4) for m in masks],
           "pixels_changed_by_double_window": float((maps != plain).mean()),
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(float(H) * W * D * 4 / 1e6, 1)}
    out.update(summarise(kern, select_bytes(selected, masks.size, D), best))
    out["kernels"] = kern
    print(json.dumps(out))


if __name__ == "__main__":
    main()
