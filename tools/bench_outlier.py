#!/usr/bin/env python3
"""refine()'s outlier classification (sm_refine_outlier_config) at the Teddy shape: step times with the classifying
LR check off and on and RV_combine_BG off and on for every interpolate_type, in one process; every new launch's time;
the fraction of pixels in each class; holes per second of the votes.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) with do_refine, through StereoBatch, one stream.  The configurations alternate --rounds times, each
round: warm-up, then --steps timed sm_run calls ending in one synchronise; the medians and the spread of the rounds
are reported, so that a difference can be read against the run-to-run spread of the same job.  Then each
configuration runs the same steps with per-kernel HIP-event timing (sm_profile_read).  The holes a vote launch meets
are counted on maps of contexts that stop after 0 and 1 vote rounds (no interpolation, no median): holes per second
is their sum over the two launches' time.  refine_proper_ipol is given with the holes its first launch meets over
its mean launch time (its second launch meets fewer: an upper estimate).
Prints one JSON line and writes it to --out.

  python tools/bench_outlier.py [--steps 20] [--warmup 3] [--rounds 3] [--batch 16] [--out profiles/outlier/bench_outlier_teddy_b16.json]
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

NEW = ("refine_lr_classify", "refine_rv_combine", "refine_rv_carry")
CONFIGS = [("off", dict()), ("classify", dict(classify=True))] + \
          [(f"classify_rv{t}", dict(classify=True, rv_combine=True, interpolate_type=t)) for t in range(4)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier", "bench_outlier_teddy_b16.json"))
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

    def maps_after(vote_rounds, **outlier):
        """The maps after the LR check and `vote_rounds` vote rounds, nothing else."""
        kw = dict(do_region_vote=int(vote_rounds > 0), region_vote_nums=max(vote_rounds, 1), do_proper_ipol=0,
                  do_last_median_blur=0)
        b = StereoBatch(md, H, W, B, device=args.device, num_streams=1, do_refine=1, refine_outlier=outlier or None, **kw)
        try:
            b.upload(*imgs)
            return b.run(0.3).copy()
        finally:
            b.close()

    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1, do_refine=1)
    ms = {name: [] for name, _ in CONFIGS}
    kerns = {}
    try:
        sb.upload(*imgs)
        for _ in range(args.rounds):
            for name, cfg in CONFIGS:
                sb.refine_outlier_config(**cfg)
                ms[name].append(round(timed_steps(sb, args.steps, args.warmup), 4))
        for name, cfg in CONFIGS:
            sb.refine_outlier_config(**cfg)
            kerns[name] = profiled(sb, args.steps)
    finally:
        sb.close()

    labelled = maps_after(0, classify=True)
    npx = float(labelled.size)
    classes = {"disp_occ": float((labelled == -32).sum() / npx), "disp_mis": float((labelled == -48).sum() / npx),
               "valid": float((labelled >= 0).sum() / npx)}

    def per_step(k, name):
        e = k.get(name)
        return round(e["ms_per_launch"] * e["launches_per_step"], 4) if e else 0.0

    def holes_per_s(holes, k, name):
        e = k.get(name)
        if not e or e["ms_per_launch"] <= 0:
            return None
        return round(sum(holes) / (len(holes) * e["ms_per_launch"] * 1e-3), 0)

    votes = {}
    plain = [int((maps_after(r) < 0).sum()) for r in (0, 1)]
    votes["refine_region_vote"] = {"holes_in": plain, "holes_per_s": holes_per_s(plain, kerns["off"], "refine_region_vote")}
    for t in range(4):
        cfg = dict(classify=True, rv_combine=True, interpolate_type=t)
        h = [int((labelled < 0).sum()), int((maps_after(1, **cfg) < 0).sum())]
        k = kerns[f"classify_rv{t}"]
        votes[f"refine_rv_combine_type{t}"] = {"holes_in": h, "holes_per_s": holes_per_s(h, k, "refine_rv_combine"),
                                               "refine_rv_carry_ms_per_launch": k.get("refine_rv_carry", {}).get("ms_per_launch")}
    ipol_in = [int((maps_after(2) < 0).sum())]
    votes["refine_proper_ipol"] = {"holes_in_first_launch": ipol_in,
                                   "holes_per_s": holes_per_s(ipol_in, kerns["off"], "refine_proper_ipol")}

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm + refine, one stream",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "ms_per_step": ms, "median_ms_per_step": med,
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
           "minus_off_ms": {k: round(med[k] - med["off"], 4) for k in med if k != "off"},
           "new_launches": {name: {n: kerns[name][n] for n in NEW if n in kerns[name]} for name, _ in CONFIGS},
           "replaced_launches_ms_per_step": {"refine_lr_check": per_step(kerns["off"], "refine_lr_check"),
                                             "refine_region_vote": per_step(kerns["off"], "refine_region_vote"),
                                             "refine_proper_ipol": per_step(kerns["off"], "refine_proper_ipol")},
           "class_fractions": classes, "votes": votes}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
