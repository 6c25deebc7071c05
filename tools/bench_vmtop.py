#!/usr/bin/env python3
"""dispOptimize's Do_vmTop branch at the Teddy shape: step times with and without it, the selection kernel's share
of the copy ceiling, the decision kernels' times and the worst case of the ordered pass.

The workload is bench.py's Teddy one (450 x 375, D = 64, 16 synthetic pairs, censusGrad + CBCA + SolveAll +
SGM 4-path) through StereoBatch, one stream, in one process: warm-up, then --steps timed sm_run calls ending in
one synchronise, first with vmTop off, then with vmTop on (M = 2, thres 1.09f, ts 10, method 0), then the same
steps with per-kernel HIP-event timing (sm_profile_read).  vmtop_select reads 4 B per volume element and writes
at most 8 M + 4 B per pixel; its bytes over its time are stated as a share of sm_copy_ceiling (a dwordx4 copy,
read + write counted) measured in the same job.  Teddy's volumes fit the 256 MB cache, so this is no
HBM-roofline fraction.  The worst case of method 0's ordered pass is the all-case-2 33 x 41 fixture
(tests/golden/vmtop/vmtop_case2.npz) through sm_set_volume and optimization "".  Prints one JSON line.

  python tools/bench_vmtop.py [--steps 20] [--warmup 3] [--batch 16]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
        gbs = k["bytes_per_launch"] / (per * 1e-3) / 1e9 if per > 0 else 0.0
        kern[name] = {"ms_per_launch": round(per, 4), "launches_per_step": k["launches"] / steps,
                      "bytes_per_launch": k["bytes_per_launch"], "gbs": round(gbs, 1)}
    return kern


def worst_case_decide(device, reps=20):
    """The all-case-2 fixture: every pixel off row 0 and column 0 waits for its four neighbours."""
    import numpy as np

    from mystereomatching_amd import _capi

    fx = np.load(os.path.join(ROOT, "tests", "golden", "vmtop", "vmtop_case2.npz"))
    vol, bgr = np.ascontiguousarray(fx["vol"]), np.ascontiguousarray(fx["bgr"])
    H, W, D = vol.shape
    lib = _capi.load()
    p = _capi.default_params(D - 1, H, W, cost_method="AD", aggregation=0, optimization=0)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), device))
    try:
        gray = np.ascontiguousarray(bgr[:, :, 1])
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(bgr), _capi.ptr(bgr), W * 3, _capi.ptr(gray), _capi.ptr(gray), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        _capi.check(lib, ctx, lib.sm_vmtop_config(ctx, 1, 0, int(fx["num"]), float(fx["thres"]), int(fx["ts"]), 1, 0))
        _capi.check(lib, ctx, lib.sm_profile_enable(ctx, 1))
        for _ in range(reps + 1):
            _capi.check(lib, ctx, lib.sm_set_volume(ctx, 0, _capi.ptr(vol)))
            _capi.check(lib, ctx, lib.sm_disp_optimize(ctx, None))
        names = C.create_string_buffer(64 * 48)
        launches, ms, by = (C.c_int64 * 64)(), (C.c_double * 64)(), (C.c_double * 64)()
        cnt = C.c_int32()
        _capi.check(lib, ctx, lib.sm_profile_read(ctx, 64, names, launches, ms, by, C.byref(cnt)))
        out = {}
        for i in range(min(cnt.value, 64)):
            name = names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode()
            if name.startswith("vmtop_"):
                out[name] = round(ms[i] / max(1, launches[i]), 4)
        return {"shape": [H, W, D], "pending_pixels": (H - 1) * (W - 1), "steps_t": W + 2 * H - 3, "ms_per_launch": out}
    finally:
        lib.sm_destroy(ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=375)
    ap.add_argument("--cols", type=int, default=450)
    ap.add_argument("--max-disp", type=int, default=63)
    ap.add_argument("--num", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    import numpy as np

    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S

    H, W, md, B, M = args.rows, args.cols, args.max_disp, args.batch, args.num
    D = md + 1
    batch = S.make_batch(B, H, W, D, first_index=0)
    imgs = [batch[k] for k in ("lbgr", "rbgr", "lgray", "rgray")]
    sb = StereoBatch(md, H, W, B, device=args.device, num_streams=1)
    try:
        sb.upload(*imgs)
        off_ms = timed_steps(sb, args.steps, args.warmup)
        plain = sb.download()
        sb.vmtop_config(True, 0, M, float(np.float32(1.09)), 10, True, False)
        on_ms = timed_steps(sb, args.steps, args.warmup)
        maps = sb.download()
        kern = profiled(sb, args.steps)
        sb.vmtop_config(False, 0, M, float(np.float32(1.09)), 10, True, False)
        off2_ms = timed_steps(sb, args.steps, args.warmup)
        best, median = sb.copy_ceiling(max(H * W * D * 4, 2 << 30), reps=5)
    finally:
        sb.close()

    vt = {n: v for n, v in kern.items() if n.startswith("vmtop_")}
    for v in vt.values():
        v["frac_of_copy_ceiling"] = round(v["gbs"] / best, 4) if best > 0 else None
    decide_ms = sum(v["ms_per_launch"] * v["launches_per_step"] for n, v in vt.items() if n.startswith("vmtop_decide"))
    sel = vt.get("vmtop_select", {})
    out = {"workload": f"{W}x{H} D={D} x{B}, censusGrad + CBCA + SolveAll + sgm, vmTop M={M} thres=1.09f ts=10 method 0",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": {"vmtop_off": round(off_ms, 4), "vmtop_on": round(on_ms, 4), "vmtop_off_again": round(off2_ms, 4)},
           "vmtop_on_over_off": round(on_ms / off_ms, 4),
           "select_ms": sel.get("ms_per_launch"), "select_gbs": sel.get("gbs"),
           "select_frac_of_copy_ceiling": sel.get("frac_of_copy_ceiling"),
           "decide_ms_per_step": round(decide_ms, 4),
           "copy_ceiling_gbs": round(best, 1), "copy_ceiling_median_gbs": round(median, 1),
           "volume_mb": round(float(H) * W * D * 4 / 1e6, 1),
           "pixels_changed_by_vmtop": float((maps != plain).mean()),
           "worst_case_decide": worst_case_decide(args.device),
           "kernels": kern}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
