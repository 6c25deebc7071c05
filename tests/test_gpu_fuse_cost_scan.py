"""sm_params.fuse_cost_scan: the first CBCA H scan computes its censusGrad costs itself (k_cbca_hsc),
so the cost volume is never written.  Every comparison is bit-exact against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _volumes(pair, H, W, md, views=(0,), maps=None, **over):
    """sm_cost_calculate through the C-ABI: the volumes of `views` after aggregation and, with
    maps = (reg_lambda, refine), the disparity map of the reference-ordered calls."""
    lib = _capi.load()
    p = _capi.default_params(md, H, W, keep_final_volume=1, **over)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3,
                                                _capi.ptr(a["lgray"]), _capi.ptr(a["rgray"]), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        vols = []
        for view in views:
            got = np.empty((H, W, md + 1), np.float32)
            _capi.check(lib, ctx, lib.sm_get_volume(ctx, view, _capi.ptr(got)))
            vols.append(got)
        dp = None
        if maps is not None:
            _capi.check(lib, ctx, lib.sm_solve_all(ctx, 1, maps[0]))
            dp = np.empty((H, W), np.int16)
            _capi.check(lib, ctx, lib.sm_disp_optimize(ctx, _capi.ptr(dp)))
            if maps[1]:
                _capi.check(lib, ctx, lib.sm_refine(ctx, _capi.ptr(dp)))
        return vols, dp
    finally:
        lib.sm_destroy(ctx)


CASES = [
    (2, 20, 63, 1, 0),     # all rows are border rows (no FAST elements); line shorter than T and than the lag
    (5, 40, 255, 2, 1),    # W < 64: chunks 1-3 see only out-of-range candidates
    (9, 87, 127, 2, 1),    # W = 63 + T exactly
    (7, 100, 255, 2, 1),   # W not a multiple of T
    (6, 130, 69, 2, 0),    # D % 64 != 0: masked lanes
    (37, 61, 39, 1, 0),    # D < 64
    (12, 300, 191, 3, 1),  # three chunks, steady tiles
]


@pytest.mark.parametrize("H,W,md,iters,refine", CASES)
def test_fused_volume_and_map(oracle, H, W, md, iters, refine):
    """Aggregated volume(s) (both views with Do_refine) and the map of the reference-ordered calls,
    then the batched path (SolveAll fused into the last sweep), with fuse_cost_scan = 1."""
    pair = S.make_pair(H, W, md + 1, 1300 + H + md)
    cfg = oracle.config(H, W, md, cbca_iters=iters, do_refine=refine)
    ref = oracle.run_ex(pair, cfg, dumps=("agg", "agg_right") if refine else ("agg",))
    views = (0, 1) if refine else (0,)
    vols, dp = _volumes(pair, H, W, md, views, maps=(0.3, refine), cbca_iterations=iters, do_refine=refine,
                        fuse_cost_scan=1)
    for view, got in zip(views, vols):
        np.testing.assert_array_equal(bits(got), bits(ref["agg" if view == 0 else "agg_right"]), err_msg=f"view {view}")
    np.testing.assert_array_equal(dp, ref["disp"])
    sb = StereoBatch(md, H, W, 2, cbca_iterations=iters, do_refine=refine, fuse_cost_scan=1)
    try:
        b = S.make_batch(2, H, W, md + 1, first_index=1400 + H)
        sb.upload(*(b[k] for k in KEYS))
        got = sb.run(0.3)
        for i in range(2):
            pr = {k: b[k][i] for k in KEYS}
            np.testing.assert_array_equal(got[i], oracle.run_ex(pr, cfg)["disp"], err_msg=f"pair {i}")
    finally:
        sb.close()


@pytest.mark.parametrize("H,W,md", [(9, 87, 127), (6, 130, 69)])
def test_switch_off_same_volume(H, W, md):
    """fuse_cost_scan = 0 (cost volume + H scan) and = 1 give identical aggregated volumes."""
    pair = S.make_pair(H, W, md + 1, 1500 + md)
    (off,), _ = _volumes(pair, H, W, md, fuse_cost_scan=0)
    (on,), _ = _volumes(pair, H, W, md, fuse_cost_scan=1)
    np.testing.assert_array_equal(bits(on), bits(off))


FALLBACKS = [
    ("Census", {}, {}),
    ("ADCensus", {}, {}),
    ("AD", {}, {}),
    ("censusGrad", {"lam_g": 20.0}, {"lam_g": 20.0}),
    ("censusGrad", {"grad_trunc": 10.0}, {"grad_trunc": 10.0}),
    ("censusGrad", {"grad_adaptive": 0}, {"grad_adaptive": 0}),
    ("censusGrad", {"census_rv": 2, "census_ru": 2, "census_ring": 0}, {"census_rv": 2, "census_ru": 2, "census_ring": 0}),
]


@pytest.mark.parametrize("cost,over,cfg_over", FALLBACKS, ids=["census", "adcensus", "ad", "lam_g20", "trunc10",
                                                                "no_adaptive", "census5x5"])
def test_fallbacks_match_oracle(oracle, cost, over, cfg_over):
    """Configurations outside the fused sweep's conditions (or at their edge) with the switch on:
    the aggregated volume equals the oracle's whichever kernels ran."""
    H, W, md = 19, 88, 23
    pair = S.make_pair(H, W, md + 1, 1600)
    cfg = oracle.config(H, W, md, cost=cost, **cfg_over)
    ref = oracle.run_ex(pair, cfg, dumps=("agg",))
    (got,), _ = _volumes(pair, H, W, md, cost_method=cost, fuse_cost_scan=1, **over)
    np.testing.assert_array_equal(bits(got), bits(ref["agg"]))


def test_right_view_only_built(oracle):
    """compute_right_view without refinement: CBCA runs on the left view only (fused), and the
    right view's raw cost volume still comes from the cost kernel."""
    H, W, md = 19, 88, 23
    pair = S.make_pair(H, W, md + 1, 1601)
    cfg = oracle.config(H, W, md)
    ref = oracle.run_ex(pair, cfg, dumps=("agg",))
    (left, right), _ = _volumes(pair, H, W, md, views=(0, 1), compute_right_view=1, fuse_cost_scan=1)
    np.testing.assert_array_equal(bits(left), bits(ref["agg"]))
    np.testing.assert_array_equal(bits(right), bits(oracle.cost_volume(pair, cfg, view=1)))


def test_pipelined_async_uploads(oracle):
    """The pipelined schedule (two groups across calls) with the next batch's upload issued right
    behind run + download_async, no host wait in between: the fused sweep reads the gray images,
    so the group's "inputs read" event follows its first CBCA sweep.  Three different batches;
    every map equals the oracle's."""
    import torch
    md, H, W, n = 63, 30, 52, 8
    cfg = oracle.config(H, W, md)
    sets = [S.make_batch(n, H, W, md + 1, first_index=1700 + 16 * s) for s in range(3)]
    want = [np.stack([oracle.run_ex({k: b[k][i] for k in KEYS}, cfg)["disp"] for i in range(n)]) for b in sets]
    dev = [{k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in KEYS} for b in sets]
    torch.cuda.synchronize()
    sb = StereoBatch(md, H, W, n, device=0, fuse_cost_scan=1)
    try:
        outs = [torch.full((n, H, W), -5, dtype=torch.int16, pin_memory=True).numpy() for _ in range(3)]
        sb.upload_async(*(dev[0][k] for k in KEYS))
        for i in range(3):
            sb.run(0.3, download=False)
            sb.download_async(outs[i])
            if i + 1 < 3:
                sb.upload_async(*(dev[i + 1][k] for k in KEYS))
        sb.download_wait(0)
        sb.upload_wait()
        for i in range(3):
            np.testing.assert_array_equal(outs[i], want[i], err_msg=f"batch {i}")
    finally:
        sb.close()


def _launched(H, W, md, **over):
    """Profile names with launches of one profiled sm_run of two pairs."""
    sb = StereoBatch(md, H, W, 2, **over)
    try:
        b = S.make_batch(2, H, W, md + 1, first_index=1800)
        sb.upload(*(b[k] for k in KEYS))
        sb.profile(True)
        sb.run(0.3)
        return {k for k, v in sb.profile_read().items() if v["launches"] > 0}
    finally:
        sb.close()


def test_eligibility_by_profile_names():
    """Which kernels ran: an eligible configuration launches cbca_h_scan_cost (both views with
    Do_refine) and neither the cost volume nor the plain first H scan; the default (auto) does the
    same; the switch off, lam_g != 1 and a 5 x 5 census keep the two kernels."""
    H, W, md = 19, 88, 23
    for over in ({"fuse_cost_scan": 1}, {}):
        names = _launched(H, W, md, do_refine=1, **over)
        assert {"cbca_h_scan_cost", "cbca_h_scan_cost_r"} <= names, (over, names)
        assert not names & {"cost_volume", "cost_volume_right", "cbca_h_scan", "cbca_h_scan_r"}, (over, names)
    # a right view that is only built keeps its cost kernel
    names = _launched(H, W, md, compute_right_view=1, fuse_cost_scan=1)
    assert "cbca_h_scan_cost" in names and "cost_volume_right" in names and "cost_volume" not in names, names
    for over in ({"fuse_cost_scan": 0}, {"fuse_cost_scan": 1, "lam_g": 20.0},
                 {"fuse_cost_scan": 1, "census_rv": 2, "census_ru": 2, "census_ring": 0},
                 {"fuse_cost_scan": 1, "grad_trunc": 10.0}):
        names = _launched(H, W, md, **over)
        assert {"cost_volume", "cbca_h_scan"} <= names and "cbca_h_scan_cost" not in names, (over, names)
