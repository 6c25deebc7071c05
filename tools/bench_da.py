#!/usr/bin/env python3
"""refine()'s discontinuity adjustment (sm_refine_da_config) at the Teddy shape: step times with the stage off and
on in one process, every refine_da_* kernel's time, and what SGM's kept path sum costs.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) with do_refine, through StereoBatch, one stream.  The two configurations alternate --rounds times (off,
on, off, on, ...), each round: warm-up, then --steps timed sm_run calls ending in one synchronise; the medians and
the spread of the rounds are reported, so that "on minus off" can be read against the run-to-run spread of the
same job.  Then each configuration runs the same steps with per-kernel HIP-event timing (sm_profile_read): the
refine_da_* kernels, the two refine_proper_ipol launches they are compared with, and sgm_last_wta, which with the
stage on also writes its path sum (4 B per element more) for the ordered pass to read.
Prints one JSON line and writes it to --out.

  python tools/bench_da.py [--steps 20] [--warmup 3] [--rounds 3] [--batch 16] [--out profiles/da/bench_da_teddy_b16.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_refine_ext import profiled, timed_steps  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "da", "bench_da_teddy_b16.json"))
    args = ap.parse_args(argv)
    if args.steps < 1 or args.rounds < 1:
        ap.error("--steps and --rounds must be >= 1")
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
    ms = {"off": [], "on": []}
    kerns, maps = {}, {}
    try:
        sb.upload(*imgs)
        for _ in range(args.rounds):
            for name in ("off", "on"):
                sb.refine_da_config(name == "on")
                ms[name].append(round(timed_steps(sb, args.steps, args.warmup), 4))
        for name in ("off", "on"):
            sb.refine_da_config(name == "on")
            kerns[name] = profiled(sb, args.steps)
            maps[name] = sb.download()
        edges = sb.get_da_edges()
    finally:
        sb.close()

    da = {k: v for k, v in kerns["on"].items() if k.startswith("refine_da_")}
    da_ms = sum(v["ms_per_launch"] * v["launches_per_step"] for v in da.values())
    ipol = kerns["on"].get("refine_proper_ipol", {})
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm + refine, one stream",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "ms_per_step": ms, "median_ms_per_step": med,
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
           "on_minus_off_ms": round(med["on"] - med["off"], 4),
           "refine_da_kernels": da, "refine_da_kernels_ms_per_step": round(da_ms, 4),
           "refine_proper_ipol_ms_per_step": round(ipol.get("ms_per_launch", 0) * ipol.get("launches_per_step", 0), 4),
           "sgm_last_wta_ms": {k: kerns[k].get("sgm_last_wta", {}).get("ms_per_launch") for k in ("off", "on")},
           "maps": {"pixels_changed_by_da": float((maps["on"] != maps["off"]).mean()),
                    "edge_pixels_pair0": float((edges > 0).mean())},
           "kernels_on": kerns["on"]}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
