"""Conditions of the degenerate-input and runtime-constant GPU tests, asserted on the CPU oracle alone.

tests/test_gpu_degenerate.py and tests/test_gpu_runtime_constants.py compare the GPU with the oracle on
inputs chosen to make a special case decide the result: equal minima, negative costs, NaN volumes, a
constant away from its default.  Such a test passes vacuously if the input does not do what it was
chosen for, so each property is pinned here, without a GPU:

  ties       constant / striped pairs leave most pixels with two or more equal minima;
  signed     signed_blocks drives the guided filter's minimum below zero on >= 5 % of the pixels;
  NaN        grey_contrast makes the guided filter's volume NaN at every element, the map -1;
  oracle     the oracle's own tie-breaking equals the independent numpy restatement's (pyref);
  constants  every runtime-constant case changes the oracle's output on its input (or is listed as
             inert with the reason, and then provably changes nothing).
"""
import numpy as np
import pytest

import degenerate as G
import pyref
import pyref_refine_ext as X
import rc_cases as R

f32 = np.float32
H, W, MD = 40, 61, 23
SIGNED_SEED = 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tie_share(vol):
    """Share of pixels whose minimum cost is taken by two or more disparities."""
    mn = vol.min(axis=2, keepdims=True)
    return float(((vol == mn).sum(axis=2) >= 2).mean())


# ---- ties ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["constant", "vstripes"])
@pytest.mark.parametrize("agg", [0, 1])
def test_tie_share(oracle, name, agg):
    pair = getattr(G, name)(H, W)
    ref = oracle.run(pair, oracle.config(H, W, MD, aggregation=agg, optimization=0), dumps=True)
    share = tie_share(ref["final"])
    print(f"{name} aggregation {agg}: {share:.3f} of the pixels have >= 2 equal minima")
    assert share >= 0.5


# ---- signed costs --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_signed_blocks_goes_negative(oracle, mode):
    pair = G.signed_blocks(H, W, SIGNED_SEED)
    ref = oracle.run(pair, oracle.config(H, W, MD, aggregation=2, gf_mode=mode, optimization=1), dumps=True)
    assert not np.isnan(ref["agg"]).any()
    share = float((ref["agg"].min(axis=2) < 0).mean())
    print(f"gf_mode {mode}: negative minimum on {share:.3f} of the pixels, "
          f"{int((ref['final'] < 0).sum())} negative elements after SGM")
    assert share >= 0.05
    assert (ref["final"] < 0).any()


# ---- NaN volumes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", G.GREY_KINDS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W,md", [(24, 30, 7), (40, 61, 23), (33, 80, 69)])
def test_grey_contrast_is_all_nan(oracle, kind, mode, H, W, md):
    """B = G = R at 0 / 255: the three variances and three covariances of a window are one float v of
    a few thousand, and fl(v + eps) = v (eps = 1e-4 is below half an ulp of v), so the 3 x 3 matrix
    has nine equal entries: every cofactor is 0 and so is the determinant -- as floats in
    ximgproc's form, as doubles of those floats in MY_GUIDE's (cpp:5048-5078, `double a11 =
    vData[0][u] + eps` adds in float) -- and 0 / 0 or inf * 0 is NaN.  gen_dispFromVm's `minC >
    vmP[d]` (cpp:3940-3964) is false on NaN: -1."""
    pair = G.grey_contrast(H, W, 5, kind)
    for opt, paths in ((0, 4), (1, 4), (1, 8)):
        cfg = oracle.config(H, W, md, aggregation=2, gf_mode=mode, optimization=opt, sgm_paths=paths)
        ref = oracle.run(pair, cfg, dumps=True)
        assert np.isnan(ref["agg"]).all()
        assert (ref["disp"] == -1).all()
    ref = oracle.run_ex(pair, oracle.config(H, W, md, aggregation=2, gf_mode=mode, do_refine=1), dumps=("agg_right",))
    assert np.isnan(ref["agg_right"]).all() and (ref["disp"] == -1).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_gf_nan_is_per_pixel(oracle, mode):
    """What the signed SGM kernels guarantee is parity on volumes whose pixels are finite or NaN at
    every disparity (NaN enters through the guide's inverse covariance, which does not depend on d;
    sm_sgm.hip, keep_nan).  Every input that the GPU tests send through GF is of that kind, and has
    no infinity; the 0 / 255 grey tie inputs are NaN too, step_edge around its edge only."""
    partial = 0
    for H, W, md in G.SHAPES:
        pairs = [mk(H, W) for mk in G.TIE_INPUTS.values()] + [G.signed_blocks(H, W, SIGNED_SEED)]
        pairs += [G.grey_contrast(H, W, 5, kind) for kind in G.GREY_KINDS]
        for pair in pairs:
            cfg = oracle.config(H, W, md, gf_mode=mode)
            for view, img in ((0, "lbgr"), (1, "rbgr")):
                vol = oracle.guided_filter(oracle.cost_volume(pair, cfg, view=view), pair[img], cfg)
                nan = np.isnan(vol)
                assert not np.isinf(vol).any()
                assert (nan.all(axis=2) | ~nan.any(axis=2)).all()
                partial += int(nan.any() and not nan.all())
    assert partial > 0   # a path that runs from NaN pixels into finite ones is among the cases


# ---- the oracle's own tie-breaking ---------------------------------------------------------------

TH, TW, TMD = 9, 20, 7
TINY = {"constant": lambda: G.constant(TH, TW), "vstripes": lambda: G.vstripes(TH, TW, period=4, shift=1), "checker": lambda: G.checker(TH, TW)}


@pytest.mark.parametrize("name", sorted(TINY))
@pytest.mark.parametrize("paths", [4, 8])
def test_oracle_ties_pipeline_wta_sgm(oracle, name, paths):
    pair = TINY[name]()
    ref = pyref.pipeline(pair, TMD, paths=paths)
    got = oracle.run(pair, oracle.config(TH, TW, TMD, sgm_paths=paths), dumps=True)
    for k in ("cost", "agg", "final"):
        np.testing.assert_array_equal(bits(got[k]), bits(ref[k]), err_msg=k)
    np.testing.assert_array_equal(got["disp"], ref["disp"])
    if paths == 4:   # WTA alone, without and with CBCA
        for agg in (0, 1):
            w = oracle.run(pair, oracle.config(TH, TW, TMD, aggregation=agg, optimization=0), dumps=True)
            vol = pyref.solve_all(ref["agg"] if agg else ref["cost"])
            assert tie_share(vol) > 0   # the comparison below is about pixels with equal minima: some exist
            np.testing.assert_array_equal(bits(w["final"]), bits(vol))
            np.testing.assert_array_equal(w["disp"], pyref.wta(vol))


@pytest.mark.parametrize("name", sorted(TINY))
def test_oracle_ties_so(oracle, name):
    pair = TINY[name]()
    got = oracle.run(pair, oracle.config(TH, TW, TMD, optimization=2), dumps=True)
    vm, dp = pyref.so(pyref.solve_all(pyref.pipeline(pair, TMD)["agg"]), pair["lbgr"])
    np.testing.assert_array_equal(bits(got["final"]), bits(vm))
    np.testing.assert_array_equal(got["disp"], dp)


@pytest.mark.parametrize("name", sorted(TINY))
def test_oracle_ties_refine_stages(oracle, name):
    """LR check, region vote (equal histogram maxima: the first wins), properIpol (equal colour
    differences: the first direction wins) and the median on maps over a degenerate image."""
    pair = TINY[name]()
    cfg = oracle.config(TH, TW, TMD, do_refine=1)
    aL = oracle.arms(pair["lbgr"], cfg)
    np.testing.assert_array_equal(aL, pyref.arms(pair["lbgr"]))
    rng = np.random.default_rng(11)
    d0 = rng.integers(0, 3, (TH, TW)).astype(np.int16)       # few values: equal vote counts are common
    d1 = rng.integers(0, 3, (TH, TW)).astype(np.int16)
    holes = np.where(rng.random((TH, TW)) < 0.4, -1, d0).astype(np.int16)
    np.testing.assert_array_equal(oracle.lr_check(d0, d1, cfg), pyref.lr_check(d0, d1))
    for s, ratio in ((0, 0.4), (20, 0.4), (3, 1.5)):
        c = oracle.config(TH, TW, TMD, do_refine=1, rv_s=s, rv_ratio=ratio)
        np.testing.assert_array_equal(oracle.region_vote(holes, aL, c), pyref.region_vote(holes, aL, TMD + 1, f32(ratio), s))
    for occ in (-32, -1):
        c = oracle.config(TH, TW, TMD, do_refine=1, disp_occ=occ)
        np.testing.assert_array_equal(oracle.proper_ipol(holes, pair["lbgr"], c), pyref.proper_ipol(holes, pair["lbgr"], occ))
    np.testing.assert_array_equal(oracle.median3(holes), pyref.median3(holes))
    np.testing.assert_array_equal(oracle.refine(d0, d1, aL, pair["lbgr"], cfg), pyref.refine(d0, d1, aL, pair["lbgr"], TMD + 1))


# ---- runtime constants: every case moves the oracle ----------------------------------------------

def _differs(a, b, keys):
    return any(not np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k],
                                  bits(b[k]) if b[k].dtype == np.float32 else b[k]) for k in keys)


SGM_INPUTS = {"d24": (R.pair, R.H, R.W, R.MD), "d200": (R.pair_d200, R.H2, R.W2, R.MD2)}


@pytest.mark.parametrize("inp", sorted(SGM_INPUTS))
@pytest.mark.parametrize("paths", [4, 8])
def test_sgm_constants_move_the_oracle(oracle, inp, paths):
    mk, h, w, md = SGM_INPUTS[inp]
    pair = mk()
    base = oracle.run_ex(pair, oracle.config(h, w, md, sgm_paths=paths), dumps=("final",))
    cases = [dict(sgm_p1=p1, sgm_p2=p2) for p1, p2 in R.P1P2] + [dict(sgm_redu=r) for r in R.REDU]
    for kw in cases:
        got = oracle.run_ex(pair, oracle.config(h, w, md, sgm_paths=paths, **kw), dumps=("final",))
        assert _differs(got, base, ("final",)) and _differs(got, base, ("disp",)), kw


@pytest.mark.parametrize("inp", ["small", "tiles"])
@pytest.mark.parametrize("paths", [4, 8])
def test_cor_dif_thres_moves_the_oracle(oracle, inp, paths):
    pair, (h, w, md) = (R.pair(), (R.H, R.W, R.MD)) if inp == "small" else (R.pair_tiles(), (R.HT, R.WT, R.MDT))
    dumps = ("final", "disp_right")
    base = oracle.run_ex(pair, oracle.config(h, w, md, sgm_paths=paths, do_refine=1), dumps=dumps)
    for t in R.COR_THRES:
        got = oracle.run_ex(pair, oracle.config(h, w, md, sgm_paths=paths, do_refine=1, sgm_cor_thres=t), dumps=dumps)
        assert _differs(got, base, ("final",)) and _differs(got, base, ("disp_right",)), t


def test_refine_constants_move_the_oracle(oracle):
    pair = R.vote_pair()
    d0, d1 = R.given_maps()
    cfg = oracle.config(R.H, R.W, R.MD, do_refine=1)
    aL = oracle.arms(pair["lbgr"], cfg)
    base = oracle.refine(d0, d1, aL, pair["lbgr"], cfg)
    seen = {}
    for field, vals in (("lr_max_diff", R.LR_MAX_DIFF), ("rv_s", R.RV_S), ("rv_ratio", R.RV_RATIO),
                        ("region_vote_nums", R.REGION_VOTE_NUMS)):
        for v in vals:
            got = oracle.refine(d0, d1, aL, pair["lbgr"], oracle.config(R.H, R.W, R.MD, do_refine=1, **{field: v}))
            moved = int((got != base).sum())
            print(f"{field} = {v}: {moved} pixels differ from the default's map")
            assert (moved == 0) == ((field, v) in R.INERT), (field, v, moved)
            seen[(field, v)] = got
    # and the values differ from each other where the reference tells them apart
    assert (seen[("lr_max_diff", 1.0)] != seen[("lr_max_diff", 2.0)]).any()
    assert (seen[("lr_max_diff", 2.0)] != seen[("lr_max_diff", 3.0)]).any()
    assert (seen[("rv_s", 0)] != seen[("rv_s", 5)]).any()
    assert (seen[("region_vote_nums", 1)] != seen[("region_vote_nums", 5)]).any()


@pytest.mark.parametrize("occ", R.DISP_OCC)
def test_disp_occ_moves_the_oracle(oracle, occ):
    """refine()'s LR check turns every negative disparity into -1 (cpp:2262-2282), so a DISP_OCC
    mark that the caller puts into DP[0] never reaches properIpol.  The marks that do are the
    peak-ratio stage's (signDp_UsingPKR runs after the LR check): with DISP_PKR = DISP_OCC its
    pixels take properIpol's occlusion branch, the smallest disparity found."""
    pair = R.pair()
    cfg = oracle.config(R.H, R.W, R.MD, do_refine=1)
    aL = oracle.arms(pair["lbgr"], cfg)
    ref = oracle.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
    args = (ref["disp_raw"], ref["disp_right"], aL, pair["lbgr"], ref["final"])
    base = X.refine_ext(oracle, cfg, *args, do_pkr=True, disp_pkr=occ)
    got = X.refine_ext(oracle, oracle.config(R.H, R.W, R.MD, do_refine=1, disp_occ=occ), *args, do_pkr=True, disp_pkr=occ)
    assert 0.05 < float(base["mask"].mean()) < 0.95
    assert (got["disp"] != base["disp"]).any()
    # a caller's mark, by contrast, is inert
    marked = np.where(np.random.default_rng(3).random((R.H, R.W)) < 0.3, occ, ref["disp_raw"]).astype(np.int16)
    np.testing.assert_array_equal(
        oracle.refine(marked, ref["disp_right"], aL, pair["lbgr"], oracle.config(R.H, R.W, R.MD, do_refine=1, disp_occ=occ)),
        oracle.refine(marked, ref["disp_right"], aL, pair["lbgr"], cfg))


@pytest.mark.parametrize("lam", R.REG_LAMBDA)
def test_reg_lambda_moves_the_oracle(oracle, lam):
    pair = R.pair()
    for opt in (0, 1):
        base = oracle.run_ex(pair, oracle.config(R.H, R.W, R.MD, optimization=opt), dumps=("final",))
        got = oracle.run_ex(pair, oracle.config(R.H, R.W, R.MD, optimization=opt, reg_lambda=lam), dumps=("final",))
        assert _differs(got, base, ("final",))
        if opt == 1:   # the penalties are not scaled with the costs, so the SGM map moves too
            assert _differs(got, base, ("disp",))
