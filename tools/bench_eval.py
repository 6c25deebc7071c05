#!/usr/bin/env python3
"""The per-stage error table (sm_eval_config) at the Teddy shape: step times with evaluation off, on (one threshold)
and on with keep_maps in one process, the eval_stage / eval_final kernel times, eval_stage's GB/s against the copy
ceiling of the same job, and the table's overhead as a share of the refine() launches.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) with do_refine, through StereoBatch, one stream.  The three configurations alternate --rounds times
(off, on, keep, off, ...), each round: warm-up, then --steps timed sm_run calls ending in one synchronise; the
medians and the spread of the rounds are reported, so that "on minus off" can be read against the run-to-run spread
of the same job.  Then each configuration runs the same steps with per-kernel HIP-event timing (sm_profile_read).
The final maps of the three configurations are compared (they must be equal), and the table of two runs bit for bit.
Prints one JSON line and writes it to --out.

  python tools/bench_eval.py [--steps 20] [--warmup 3] [--rounds 3] [--batch 16] [--out profiles/eval/bench_eval_teddy_b16.json]
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

CONFIGS = ("off", "on", "keep")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "bench_eval_teddy_b16.json"))
    args = ap.parse_args(argv)
    if args.steps < 1 or args.rounds < 1:
        ap.error("--steps and --rounds must be >= 1")
    return args


def eval_bytes(pixels, keep):
    """eval_stage's algorithmic bytes: the int16 map, the float truth and the region byte, plus the snapshot."""
    return pixels * (2 + 4 + 1 + (2 if keep else 0))


def main():
    args = parse()

    import numpy as np

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B = args.rows, args.cols, args.max_disp, args.batch
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    imgs = [np.ascontiguousarray(batch[k]) for k in ("lbgr", "rbgr", "lgray", "rgray")]
    gt = np.ascontiguousarray(batch["gt"], np.float32)
    nonocc = np.ascontiguousarray(batch["nonocc"])
    rng = np.random.default_rng(0)
    disc = np.where(rng.random(nonocc.shape) < 0.2, 255, 0).astype(np.uint8)

    def configure(sb, name):
        sb.eval_config(name != "off", keep_maps=name == "keep", thresholds=(1.0,))

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1, do_refine=1)
    ms = {k: [] for k in CONFIGS}
    kerns, maps, tables = {}, {}, {}
    try:
        sb.upload(*imgs)
        sb.eval_config(True, keep_maps=True)    # the buffers exist before anything is timed
        sb.upload_truth(gt, nonocc, np.full_like(nonocc, 255), disc)
        for _ in range(args.rounds):
            for name in CONFIGS:
                configure(sb, name)
                ms[name].append(round(timed_steps(sb, args.steps, args.warmup), 4))
        for name in CONFIGS:
            configure(sb, name)
            kerns[name] = profiled(sb, args.steps)
            maps[name] = sb.download()
            if name != "off":
                tables[name] = np.asarray(sb.stage_errors()).tobytes()
        names = sb.stage_names()
        table = sb.stage_errors()
        # the copy ceiling of the same job: a copy that moves eval_stage's bytes (half read, half written)
        ceiling = sb.copy_ceiling(eval_bytes(B * H * W, False), 20)
    finally:
        sb.close()

    med = {k: statistics.median(v) for k, v in ms.items()}

    def per_step(k, prefix):
        return round(sum(v["ms_per_launch"] * v["launches_per_step"] for n, v in k.items() if n.startswith(prefix)), 4)

    ev = {}
    for name in ("on", "keep"):
        st = kerns[name]["eval_stage"]
        ev[name] = {"eval_stage": st, "eval_final": kerns[name]["eval_final"],
                    "eval_ms_per_step": per_step(kerns[name], "eval_"),
                    "refine_ms_per_step": per_step(kerns[name], "refine_"),
                    "eval_stage_gbs": round(st["bytes_per_launch"] / (st["ms_per_launch"] * 1e-3) / 1e9, 1)}
        ev[name]["eval_share_of_refine"] = round(ev[name]["eval_ms_per_step"] / ev[name]["refine_ms_per_step"], 4)
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm + refine, one stream",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "stages": names,
           "ms_per_step": ms, "median_ms_per_step": med,
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
           "on_minus_off_ms": round(med["on"] - med["off"], 4), "keep_minus_off_ms": round(med["keep"] - med["off"], 4),
           "eval": ev, "copy_ceiling_gbs": {"best": round(ceiling[0], 1), "median": round(ceiling[1], 1)},
           "maps_equal": bool((maps["on"] == maps["off"]).all() and (maps["keep"] == maps["off"]).all()),
           "tables_equal": tables["on"] == tables["keep"],
           "pbm_all_pair0": [round(float(x), 5) for x in table.pbm()[0, :, 1]],
           "rms_all_pair0": [round(float(x), 4) for x in table.rms()[0, :, 1]],
           "kernels_on": kerns["on"]}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
