#!/usr/bin/env python3
"""The cross-scale pyramid inside the batch path (sm_pyramid_config) at the Teddy shape: ms per step with
PY_LVL = 1, 2 and 3, the per-kernel lines, the share of the coarse levels, of pyr_down@* and of solve_all_pyr,
and two same-process A/Bs -- the batch SolveAll kernel against the staged API's k_solve_all_pyr on the same
volumes, and the batched pyrDown launch against one launch per image -- with the copy ceiling of the same job.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll + SGM
4-path) through StereoBatch with the default schedule, one context per configuration, all in one process.  Step
times: warm-up, then --steps sm_run calls ending in one synchronise, --rounds interleaved rounds over the
configurations (the median is reported, the rounds are listed).  Kernel times: the same steps again with HIP-event
timing (sm_profile_read).  SolveAll moves 8 B per level-0 element (the coarse reads are 1/8 + 1/64 of that and
mostly hit in cache); its GB/s is stated at those bytes and as a share of sm_copy_ceiling (a dwordx4 copy, read
+ write counted).  The A/B variants are chosen by SM_PYR_AB (read by sm_pyramid_config).  Prints one JSON line.

  python tools/bench_pyramid.py [--steps 20] [--warmup 3] [--rounds 3] [--batch 16] [--num-streams 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, MAXDISP = 375, 450, 63


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
    """{kernel: ms per step, launches per step, bytes per launch}"""
    sb.profile(True)
    sb.profile_reset()
    for _ in range(steps):
        sb.run(0.3, download=False)
    sb.synchronize()
    kern = sb.profile_read()
    sb.profile(False)
    return {k: {"ms_per_step": round(v["total_ms"] / steps, 5), "launches_per_step": v["launches"] / steps,
                "bytes_per_launch": v["bytes_per_launch"]} for k, v in sorted(kern.items()) if v["launches"]}


def shares(kern):
    total = sum(v["ms_per_step"] for v in kern.values())
    pick = lambda f: round(sum(v["ms_per_step"] for k, v in kern.items() if f(k)), 4)
    out = {"kernels_ms": round(total, 4), "coarse_levels_ms": pick(lambda k: "@" in k),
           "pyr_down_ms": pick(lambda k: k.startswith("pyr_down@")), "solve_all_pyr_ms": pick(lambda k: k.startswith("solve_all_pyr"))}
    for k in ("coarse_levels", "pyr_down", "solve_all_pyr"):
        out[k + "_share"] = round(out[k + "_ms"] / total, 4) if total > 0 else None
    return out


def solve_line(kern, ceiling):
    v = kern.get("solve_all_pyr")
    if not v or v["ms_per_step"] <= 0:
        return None
    ms = v["ms_per_step"] / v["launches_per_step"]
    gbs = v["bytes_per_launch"] / (ms * 1e-3) / 1e9
    return {"ms_per_launch": round(ms, 5), "launches_per_step": v["launches_per_step"], "gbs_at_8B_per_element": round(gbs, 1),
            "frac_of_copy_ceiling": round(gbs / ceiling, 4) if ceiling > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--num-streams", type=int, default=0, help="sm_params.num_streams (0: the default schedule, two pipelined groups)")
    a = ap.parse_args()
    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    batch = S.make_batch(a.batch, H, W, MAXDISP + 1, first_index=0)
    keys = ("lbgr", "rbgr", "lgray", "rgray")

    def make(L, ab=""):
        os.environ["SM_PYR_AB"] = ab
        sb = StereoBatch(MAXDISP, H, W, a.batch, py_lvl=L, num_streams=a.num_streams)
        os.environ["SM_PYR_AB"] = ""
        sb.upload(*(batch[k] for k in keys))
        return sb

    cfgs = {"L1": make(1), "L2": make(2), "L3": make(3), "L3_old_solve": make(3, "old_solve"), "L3_loop_down": make(3, "loop_down")}
    try:
        ms = {k: [] for k in cfgs}
        for _ in range(a.rounds):
            for k, sb in cfgs.items():
                ms[k].append(round(timed_steps(sb, a.steps, a.warmup), 4))
        kern = {k: profiled(sb, a.steps) for k, sb in cfgs.items()}
        # the A/B kernels three interleaved rounds each, under the profiler
        ab = {"solve_new": [], "solve_old": [], "pyr_down_batch": [], "pyr_down_loop": []}
        for _ in range(a.rounds):
            for name, cfg, f in (("solve_new", "L3", lambda k: k == "solve_all_pyr"), ("solve_old", "L3_old_solve", lambda k: k == "solve_all_pyr"),
                                 ("pyr_down_batch", "L3", lambda k: k.startswith("pyr_down@")),
                                 ("pyr_down_loop", "L3_loop_down", lambda k: k.startswith("pyr_down@"))):
                p = profiled(cfgs[cfg], a.steps)
                ab[name].append(round(sum(v["ms_per_step"] for k, v in p.items() if f(k)), 5))
        elements = a.batch * H * W * (MAXDISP + 1)
        best, med = cfgs["L1"].copy_ceiling(elements * 4, 5)
        res = {
            "tool": "bench_pyramid", "shape": [H, W, MAXDISP + 1], "batch": a.batch, "num_streams": a.num_streams, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": {k: {"median": statistics.median(v), "rounds": v} for k, v in ms.items()},
            "copy_ceiling_gbs": {"best": round(best, 1), "median": round(med, 1)},
            "shares": {k: shares(kern[k]) for k in ("L1", "L2", "L3")},
            "solve_all_pyr": {k: solve_line(kern[k], med) for k in ("L2", "L3", "L3_old_solve")},
            "ab_ms_per_step": {k: {"median": statistics.median(v), "rounds": v} for k, v in ab.items()},
            "pyr_down_launches_saved_per_step": 4 * a.batch * 2 - 2 * 2,
            "kernels": {k: kern[k] for k in ("L1", "L2", "L3")},
        }
        print(json.dumps(res))
    finally:
        for sb in cfgs.values():
            sb.close()


if __name__ == "__main__":
    main()
