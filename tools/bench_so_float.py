#!/usr/bin/env python3
"""The float-minima scan-line optimiser (sm_create_ex, so_float_minima = 1) at the Teddy shape in one process: ms per
step, the so kernel's ms per launch, and its algorithmic bytes per second against the copy ceiling of the same job.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, SolveAll, both views) through StereoBatch,
one stream.  Jobs:
  cbca_so        censusGrad + CBCA + so on a default context (the bit-pattern kernel)
  cbca_so_fm     the same with so_float_minima = 1 (the float-minima kernel); its maps must equal cbca_so's
  gf_so, gf_wta  censusGrad + GF + so, and GF + "" for the step without the optimiser
  bf_grad_so     grad + BF + so (inexact box sums)
  cbca_so_pkr    censusGrad + CBCA + so + Do_refine + calPKR, keep_final_volume = 1 (the accumulated volume is stored)
cbca_so and cbca_so_fm are timed in alternating rounds (--rounds) on two live contexts, so that a drift of the clocks
falls on both; `so_kernel_ratio` is the float-minima kernel's ms per launch over the bit-pattern kernel's, per round and
as the median.  The kernels' bytes are the library's own (4 B read and a 1 B trace code per volume element, + 4 B where
the accumulated volume is kept); bytes over time are stated as a share of sm_copy_ceiling (a dwordx4 copy, read +
write counted) measured in the same job.  Teddy's volumes fit the 256 MB cache, so this is no HBM-roofline fraction.
Prints one JSON line (and writes it to --out).

  python tools/bench_so_float.py [--steps 20] [--warmup 3] [--rounds 3] [--batch 16] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "tools")):
    if q not in sys.path:
        sys.path.insert(0, q)

from bench_so import profiled, summarise, timed_steps  # noqa: E402

# name -> StereoBatch's overrides
JOBS = {
    "cbca_so": dict(optimization="so"),
    "cbca_so_fm": dict(optimization="so", so_float_minima=True),
    "gf_so": dict(optimization="so", aggregation="GF"),
    "gf_wta": dict(optimization="", aggregation="GF"),
    "bf_grad_so": dict(optimization="so", aggregation="BF", cost_method="grad"),
    "cbca_so_pkr": dict(optimization="so", do_refine=1, refine_ext=dict(do_pkr=True)),
}
PAIR = ("cbca_so", "cbca_so_fm")   # timed in alternating rounds


def so_ms_per_launch(summary):
    """The left view's so kernel of a job's summary (bench_so.summarise), ms per launch; None without one."""
    k = summary["kernels"].get("so")
    return k["ms_per_launch"] if k else None


def kernel_ratio(rounds):
    """rounds: [(ms of the bit-pattern kernel, ms of the float-minima kernel)] -> per round and the median."""
    per = [round(b / a, 4) for a, b in rounds if a and b and a > 0]
    return {"per_round": per, "median": round(statistics.median(per), 4) if per else None}


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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    if args.rounds < 1:
        ap.error("--rounds must be >= 1")
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

    def make(name):
        sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1, **JOBS[name])
        sb.upload(*imgs)
        return sb

    ms, kern, rounds, ms_rounds = {}, {}, [], []
    a, b = make(PAIR[0]), make(PAIR[1])
    try:
        for _ in range(args.rounds):
            t = (timed_steps(a, args.steps, args.warmup), timed_steps(b, args.steps, args.warmup))
            k = (profiled(a, args.steps), profiled(b, args.steps))
            ms_rounds.append([round(x, 4) for x in t])
            rounds.append(tuple(so_ms_per_launch(summarise(q, "so", 0.0)) for q in k))
            ms[PAIR[0]], ms[PAIR[1]] = t
            kern[PAIR[0]], kern[PAIR[1]] = k
        if not np.array_equal(a.download(), b.download()):
            raise SystemExit("so_float_minima = 1 changed the maps on a CBCA volume")
        best, median = a.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        a.close()
        b.close()
    for name in JOBS:
        if name in PAIR:
            continue
        sb = make(name)
        try:
            ms[name] = timed_steps(sb, args.steps, args.warmup)
            kern[name] = profiled(sb, args.steps)
        finally:
            sb.close()

    summary = {name: summarise(kern[name], "so", best) for name in JOBS}
    out = {"workload": f"{W}x{H} D={D} x{B}, SolveAll, both views, one stream", "jobs": {k: {**v} for k, v in JOBS.items()},
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "ms_per_step": {k: round(x, 4) for k, x in ms.items()},
           "ms_per_step_rounds": {"order": list(PAIR), "rounds": ms_rounds},
           "so_kernel_ms_per_launch": {name: so_ms_per_launch(summary[name]) for name in JOBS},
           "so_kernel_ratio": kernel_ratio(rounds),
           "so_kernel_rounds": {"order": list(PAIR), "rounds": [list(r) for r in rounds]},
           "optimiser": summary,
           "gf_so_minus_gf_wta_ms": round(ms["gf_so"] - ms["gf_wta"], 4),
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
