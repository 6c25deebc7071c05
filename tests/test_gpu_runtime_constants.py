"""GPU parity with the runtime constants of the C ABI away from their defaults.

sm_params exposes sgm_p1, sgm_p2, sgm_cor_dif_thres, sgm_redu_coeff, lr_max_diff, rv_s, rv_ratio,
region_vote_nums and disp_occ, and sm_solve_all / sm_run take SolveAll's lambda; the other GPU tests
leave them at the defaults, so a kernel with 1.0f / 3.0f, `>> 2` or -32 baked in would pass them.
Every case here sets one of them (tests/rc_cases.py) on the GPU and in the oracle and compares the
volumes' bit patterns and the int16 maps.  That every case changes the oracle's output on its input
is asserted in tests/test_degenerate_host.py, without a GPU.  sm_set_images's row strides are
covered at the end: it is the only entry point that takes them.
"""
import numpy as np
import pytest

import pyref_refine_ext as X
import rc_cases as R
from capi_run import KEYS, Ctx, assert_bits_equal, run_ctx
from mystereomatching_amd import StereoBatch, _capi

pytestmark = pytest.mark.gpu

SGM_INPUTS = {"d24": (R.pair, R.H, R.W, R.MD), "d200": (R.pair_d200, R.H2, R.W2, R.MD2)}


def _sgm_case(oracle, pair, H, W, md, paths, refine=0, **kw):
    """kw: sm_params fields.  The final (summed) volume, DP[0], and with refine DP[1] and the refined map."""
    dumps = ("final",) + (("disp_raw", "disp_right") if refine else ())
    want = oracle.run_ex(pair, oracle.config(H, W, md, sgm_paths=paths, do_refine=refine, **R.oracle_kw(kw)), dumps=dumps)
    if not refine:
        want["disp_raw"] = want["disp"]   # (the oracle dumps DP[0] before refine() only when refine() runs)
    got = run_ctx(pair, md, sgm_paths=paths, do_refine=refine, **kw)
    assert_bits_equal(got["final"], want["final"], err_msg=f"final volume {kw}")
    np.testing.assert_array_equal(got["disp_raw"], want["disp_raw"], err_msg=f"DP[0] {kw}")
    if refine:
        np.testing.assert_array_equal(got["disp_right"], want["disp_right"], err_msg=f"DP[1] {kw}")
        np.testing.assert_array_equal(got["disp"], want["disp"], err_msg=f"refined map {kw}")


@pytest.mark.parametrize("p1,p2", R.P1P2)
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("inp", sorted(SGM_INPUTS))
def test_sgm_penalties(oracle, inp, paths, p1, p2):
    """P1 < P2, both 0, P1 > P2 and a large P2.  (The kernels leave out-of-range neighbours at
    FLT_MAX + (P1 - m), which rounds to FLT_MAX and so stays above any finite P2.)"""
    mk, H, W, md = SGM_INPUTS[inp]
    _sgm_case(oracle, mk(), H, W, md, paths, sgm_p1=p1, sgm_p2=p2)


@pytest.mark.parametrize("redu", R.REDU)
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("inp", sorted(SGM_INPUTS))
def test_sgm_redu_coeff(oracle, inp, paths, redu):
    """P / redu is a float division: 3 and 7 round, 1 leaves the penalties alone."""
    mk, H, W, md = SGM_INPUTS[inp]
    _sgm_case(oracle, mk(), H, W, md, paths, sgm_redu_coeff=redu)


def test_sgm_penalties_batch(oracle):
    """The same fields as StereoBatch keyword overrides, through sm_run."""
    pair = R.pair()
    kw = dict(sgm_p1=7.25, sgm_p2=100.0, sgm_redu_coeff=3, sgm_cor_dif_thres=1)
    sb = StereoBatch(R.MD, R.H, R.W, 1, device=0, sgm_paths=8, **kw)
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        got = sb.run(0.3)[0]
    finally:
        sb.close()
    want = oracle.run_ex(pair, oracle.config(R.H, R.W, R.MD, sgm_paths=8, **R.oracle_kw(kw)))["disp"]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("thres", R.COR_THRES)
@pytest.mark.parametrize("l_out", [34, 80], ids=["split_prep", "whole_prep"])
@pytest.mark.parametrize("inp", ["small", "tiles"])
def test_sgm_cor_dif_thres(oracle, inp, l_out, thres):
    """The colour-difference threshold of the penalty flags at and beyond the ends of [0, 255], both
    views (do_refine), 4 and 8 paths.  The flags come from one of two prep paths, chosen by the arm
    length: arm_l_out <= 64 runs the split prep (k_prep_h, which clamps the threshold to [-1, 255]
    for its guard-bit test), a longer arm the whole-image prep (k_pack_arms, which compares raw)."""
    pair, (H, W, md) = (R.pair(), (R.H, R.W, R.MD)) if inp == "small" else (R.pair_tiles(), (R.HT, R.WT, R.MDT))
    for paths in (4, 8):
        _sgm_case(oracle, pair, H, W, md, paths, refine=1, sgm_cor_dif_thres=thres, arm_l_out=l_out)


# ---- refine()'s constants on given maps -------------------------------------------------------------

REFINE_CASES = [(f, v) for f, vals in (("lr_max_diff", R.LR_MAX_DIFF), ("rv_s", R.RV_S), ("rv_ratio", R.RV_RATIO),
                                       ("region_vote_nums", R.REGION_VOTE_NUMS)) for v in vals]


@pytest.mark.parametrize("field,value", REFINE_CASES, ids=lambda x: str(x))
def test_refine_constants_on_given_maps(oracle, field, value):
    """DP[0] / DP[1] overwritten (sm_set_disp) with maps on which the constant decides something
    (rc_cases.given_maps), then refine().  rv_ratio > 1 is the can_fill = 0 branch."""
    pair = R.vote_pair()
    d0, d1 = R.given_maps()
    cfg = oracle.config(R.H, R.W, R.MD, do_refine=1, **{field: value})
    want = oracle.refine(d0, d1, oracle.arms(pair["lbgr"], cfg), pair["lbgr"], cfg)
    with Ctx(R.MD, R.H, R.W, do_refine=1, **{field: value}) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        c.call("sm_solve_all", 1, 0.3)
        c.optimize()
        c.set_disp(0, d0)
        c.set_disp(1, d1)
        np.testing.assert_array_equal(c.refine(), want)


@pytest.mark.parametrize("field,value", [("lr_max_diff", 1.0), ("lr_max_diff", 2.5), ("rv_s", 0), ("rv_s", 5),
                                         ("rv_ratio", 1.5), ("region_vote_nums", 1), ("region_vote_nums", 5),
                                         ("disp_occ", -1)], ids=lambda x: str(x))
def test_refine_constants_pipeline_batch(oracle, field, value):
    """The same fields as StereoBatch keyword overrides through sm_run, on the pipeline's own maps."""
    pair = R.pair()
    sb = StereoBatch(R.MD, R.H, R.W, 1, device=0, do_refine=1, **{field: value})
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        got = sb.run(0.3)[0]
    finally:
        sb.close()
    np.testing.assert_array_equal(got, oracle.run_ex(pair, oracle.config(R.H, R.W, R.MD, do_refine=1, **{field: value}))["disp"])


@pytest.mark.parametrize("occ", R.DISP_OCC)
def test_disp_occ(oracle, occ):
    """properIpol's occlusion branch (the smallest disparity found) at DISP_OCC = -2 and -100.
    refine()'s LR check turns every negative disparity of DP[0] into -1, so a mark that the caller
    sets never reaches properIpol; the peak-ratio stage runs after the check, and with DISP_PKR =
    DISP_OCC its marks do.  Also the caller's marks through sm_set_disp, which must change nothing."""
    pair = R.pair()
    cfg = oracle.config(R.H, R.W, R.MD, do_refine=1, disp_occ=occ)
    aL = oracle.arms(pair["lbgr"], cfg)
    ref = oracle.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
    want = X.refine_ext(oracle, cfg, ref["disp_raw"], ref["disp_right"], aL, pair["lbgr"], ref["final"], do_pkr=True, disp_pkr=occ)
    marked = np.where(np.random.default_rng(3).random((R.H, R.W)) < 0.3, occ, ref["disp_raw"]).astype(np.int16)
    with Ctx(R.MD, R.H, R.W, do_refine=1, disp_occ=occ, keep_final_volume=1) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        # (before sm_disp_optimize, so that SGM keeps its path sum for the stage)
        c.call("sm_refine_ext_config", 1, _capi.REFINE_EXT_DEFAULTS[0], occ, 0, _capi.REFINE_EXT_DEFAULTS[2], 0, 0)
        c.call("sm_solve_all", 1, 0.3)
        np.testing.assert_array_equal(c.optimize(), ref["disp_raw"])
        np.testing.assert_array_equal(c.refine(), want["disp"])
        c.call("sm_refine_ext_config", 0, _capi.REFINE_EXT_DEFAULTS[0], occ, 0, _capi.REFINE_EXT_DEFAULTS[2], 0, 0)
        c.set_disp(0, marked)
        c.set_disp(1, ref["disp_right"])
        np.testing.assert_array_equal(c.refine(), oracle.refine(marked, ref["disp_right"], aL, pair["lbgr"], cfg))


# ---- SolveAll's lambda --------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", R.REG_LAMBDA)
def test_reg_lambda(oracle, lam):
    """sm_solve_all (the standalone scale) and sm_run (fused into the last aggregation sweep)."""
    pair = R.pair()
    for opt, agg in ((1, 1), (0, 1), (0, 0)):
        cfg = oracle.config(R.H, R.W, R.MD, optimization=opt, aggregation=agg, reg_lambda=lam)
        want = oracle.run_ex(pair, cfg, dumps=("final",))
        got = run_ctx(pair, R.MD, reg_lambda=lam, optimization=opt, aggregation=agg)
        assert_bits_equal(got["final"], want["final"], err_msg=f"opt {opt} agg {agg}")
        np.testing.assert_array_equal(got["disp_raw"], want["disp"])
        sb = StereoBatch(R.MD, R.H, R.W, 1, device=0, optimization=opt, aggregation=agg, keep_final_volume=1)
        try:
            sb.upload(*(pair[k][None] for k in KEYS))
            np.testing.assert_array_equal(sb.run(lam)[0], want["disp"])
            vol = np.empty((R.H, R.W, R.MD + 1), np.float32)
            _capi.check(sb._lib, sb._ctx, sb._lib.sm_get_volume(sb._ctx, 0, _capi.ptr(vol)))
            assert_bits_equal(vol, want["final"], err_msg=f"sm_run, opt {opt} agg {agg}")
        finally:
            sb.close()


# ---- row strides ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,md", [(24, 30, 7), (33, 61, 23)])
def test_set_images_row_strides(oracle, H, W, md):
    """sm_set_images with cstride = 3 W + 5 and gstride = W + 3 on padded host buffers whose pad bytes
    are 0xFF: the raw cost volume of both views and the map equal those of the tight upload (and
    the oracle's)."""
    from mystereomatching_amd import synthetic as S
    p = S.make_pair(H, W, md + 1, 710)
    pair = {k: p[k] for k in KEYS}
    cs, gs = 3 * W + 5, W + 3
    padded = {}
    for k in KEYS:
        stride, row = (cs, 3 * W) if "bgr" in k else (gs, W)
        buf = np.full((H, stride), 0xFF, np.uint8)
        buf[:, :row] = pair[k].reshape(H, row)
        padded[k] = buf
    cfg = oracle.config(H, W, md)
    outs = []
    for tight in (True, False):
        for kw in (dict(aggregation=0, optimization=0, compute_right_view=1), dict()):
            with Ctx(md, H, W, **kw) as c:
                if tight:
                    c.set_images(pair)
                else:
                    c.call("sm_set_images", _capi.ptr(padded["lbgr"]), _capi.ptr(padded["rbgr"]), cs,
                           _capi.ptr(padded["lgray"]), _capi.ptr(padded["rgray"]), gs)
                c.call("sm_cost_calculate")
                vols = [c.volume(v) for v in ((0, 1) if kw else (0,))]
                c.call("sm_solve_all", 1, 0.3)
                outs.append((vols, c.optimize()))
    (raw_t, _), (agg_t, map_t), (raw_p, _), (agg_p, map_p) = outs
    for view in (0, 1):
        assert_bits_equal(raw_p[view], raw_t[view], err_msg=f"raw cost, view {view}")
        assert_bits_equal(raw_p[view], oracle.cost_volume(pair, cfg, view=view), err_msg=f"raw cost vs oracle, view {view}")
    assert_bits_equal(agg_p[0], agg_t[0], err_msg="aggregated volume")
    np.testing.assert_array_equal(map_p, map_t)
    np.testing.assert_array_equal(map_p, oracle.run_ex(pair, cfg)["disp"])
