"""GPU parity on degenerate inputs: equal minima, negative costs and NaN volumes, bit for bit.

Every other GPU test feeds the kernels synthetic.make_pair texture, on which costs are positive,
distinct and finite.  Here the special cases decide the result (tests/degenerate.py; that the inputs do
what they are chosen for is asserted on the oracle alone in tests/test_degenerate_host.py):

  ties    every arg-min is a wave reduction, a ballot and a count of trailing zeros (k_wta, SGM's fused
          last pass, so's row and end-of-row minima): the lowest disparity among equal minima must win;
  signed  the guided filter's costs go negative, SGM then runs its float-minimum variants
          (launch_kf_signed and the signed checkpointed kernels);
  NaN     on high-contrast grey images stored as colour the guided filter's volume is NaN everywhere
          (a singular 3 x 3 covariance); the map is -1 everywhere, as gen_dispFromVm gives.

All comparisons are exact: uint32 patterns of volumes, int16 maps.  Where the reference volume is NaN
the comparison is NaN-aware (capi_run.assert_bits_equal_nan): the NaN masks are equal and the patterns
equal elsewhere; x86 and the GPU differ in the sign of the default NaN.
"""
import numpy as np
import pytest

import degenerate as G
import pyref
import pyref_box as B
import pyref_fif as F
import pyref_refine_ext as X
import pyref_vmtop as V
from capi_run import KEYS, Ctx, assert_bits_equal, assert_bits_equal_nan, run_ctx
from mystereomatching_amd import StereoBatch

pytestmark = pytest.mark.gpu

SHAPES, INPUTS, NAMES = G.SHAPES, G.TIE_INPUTS, sorted(G.TIE_INPUTS)
COSTS = ["censusGrad", "Census", "ADCensus", "AD"]
OPTS = [(0, 4), (1, 4), (1, 8), (2, 4)]   # WTA, sgm 4, sgm 8, so
SIGNED_SEED = 2


def _eq(got, want, err_msg):
    """Bit equality; NaN-aware only where the reference volume has a NaN."""
    (assert_bits_equal_nan if np.isnan(want).any() else assert_bits_equal)(got, want, err_msg=err_msg)


def _check_against_oracle(oracle, pair, H, W, md, cost, agg, opt, paths, refine=0, **kw):
    """One pair through the C ABI against oracle.run_ex: aggregated volume(s), final volume, DP[0],
    DP[1] where it exists, the refined map.  Returns the oracle's outputs."""
    okw = {k: v for k, v in kw.items() if k == "gf_mode"}
    cfg = oracle.config(H, W, md, cost=cost, aggregation=agg, optimization=opt, sgm_paths=paths, do_refine=refine, **okw)
    views2 = bool(refine) or opt == 2
    dumps = ("agg", "final") + (("disp_right",) if views2 else ()) + (("agg_right", "disp_raw") if refine else ())
    want = oracle.run_ex(pair, cfg, dumps=dumps)
    if not refine:
        want["disp_raw"] = want["disp"]   # (the oracle dumps DP[0] before refine() only when refine() runs)
    got = run_ctx(pair, md, cost_method=cost, aggregation=agg, optimization=opt, sgm_paths=paths, do_refine=refine,
                  right_volume=bool(refine), **kw)
    what = f"{cost} agg {agg} opt {opt} paths {paths} {H}x{W} D {md + 1}"
    _eq(got["agg"], want["agg"], f"aggregated volume, {what}")
    _eq(got["final"], want["final"], f"final volume, {what}")
    np.testing.assert_array_equal(got["disp_raw"], want["disp_raw"], err_msg=f"DP[0], {what}")
    if views2:
        np.testing.assert_array_equal(got["disp_right"], want["disp_right"], err_msg=f"DP[1], {what}")
    if refine:
        _eq(got["agg_right"], want["agg_right"], f"right aggregated volume, {what}")
        np.testing.assert_array_equal(got["disp"], want["disp"], err_msg=f"refined map, {what}")
    return want


# ---- ties ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("name", NAMES)
def test_ties_core_costs(oracle, name, cost):
    """The four core costs x {no aggregation, CBCA} x {WTA, sgm 4, sgm 8, so}; the eight
    combinations of an (input, cost) pair walk through the shape set, so that every input meets
    every kernel layout under some cost."""
    first = NAMES.index(name) + 2 * COSTS.index(cost)
    raw_seen = set()
    for i, (agg, (opt, paths)) in enumerate((a, o) for a in (0, 1) for o in OPTS):
        H, W, md = SHAPES[(first + i) % len(SHAPES)]
        pair = INPUTS[name](H, W)
        _check_against_oracle(oracle, pair, H, W, md, cost, agg, opt, paths)
        if agg == 1 and (H, W, md) not in raw_seen:   # the raw cost volume under the CBCA runs
            raw_seen.add((H, W, md))
            cfg = oracle.config(H, W, md, cost=cost)
            with Ctx(md, H, W, cost_method=cost, aggregation=0, optimization=0, compute_right_view=1) as c:
                c.set_images(pair)
                c.call("sm_cost_calculate")
                for view in (0, 1):
                    assert_bits_equal(c.volume(view), oracle.cost_volume(pair, cfg, view=view), err_msg=f"raw cost, view {view}")


@pytest.mark.parametrize("opt,paths", [(1, 4), (1, 8), (2, 4)])
@pytest.mark.parametrize("name", NAMES)
def test_ties_with_refine(oracle, name, opt, paths):
    """Do_refine on: both views through CBCA and SGM / so, then the LR check, votes, interpolation
    and median on maps full of equal values."""
    H, W, md = SHAPES[(NAMES.index(name) + paths) % 3]
    _check_against_oracle(oracle, INPUTS[name](H, W), H, W, md, "censusGrad", 1, opt, paths, refine=1)


@pytest.mark.parametrize("agg,mode", [(3, 0), (2, 0), (2, 1)], ids=["NL", "GF-ximgproc", "GF-my_guide"])
@pytest.mark.parametrize("name", NAMES)
def test_ties_nl_gf(oracle, name, agg, mode):
    for i, (opt, paths) in enumerate(((0, 4), (1, 4))):
        H, W, md = SHAPES[(NAMES.index(name) + agg + mode + 2 * i) % len(SHAPES)]
        pair = INPUTS[name](H, W)
        kw = dict(gf_mode=mode) if agg == 2 else {}
        _check_against_oracle(oracle, pair, H, W, md, "censusGrad", agg, opt, paths, **kw)


@pytest.mark.parametrize("agg", ["BF", "FIF"])
@pytest.mark.parametrize("name", NAMES)
def test_ties_bf_fif(oracle, name, agg):
    """BF and FIF against the project's restatements (pyref_box, pyref_fif), as their own tests do."""
    for i, (opt, paths) in enumerate(((0, 4), (1, 4))):
        H, W, md = SHAPES[(NAMES.index(name) + i) % 2] if opt else SHAPES[(NAMES.index(name) + i) % len(SHAPES)]
        pair = INPUTS[name](H, W)
        raw = oracle.cost_volume(pair, oracle.config(H, W, md))
        vol = B.box_filter(raw) if agg == "BF" else F.fif(raw, pair["lbgr"])
        final = pyref.solve_all(vol)
        if opt:
            final = pyref.sgm(final, pair["lbgr"], paths=paths)
        got = run_ctx(pair, md, aggregation=agg, optimization=opt, sgm_paths=paths)
        assert_bits_equal(got["agg"], vol, err_msg=f"{agg} volume")
        assert_bits_equal(got["final"], final, err_msg=f"{agg} final volume")
        np.testing.assert_array_equal(got["disp_raw"], pyref.wta(final))


def test_ties_batch_of_three(oracle):
    """Three different degenerate pairs in one StereoBatch.run, 8 paths and refine()."""
    H, W, md = 40, 61, 23
    pairs = [G.vstripes(H, W), G.constant(H, W), G.step_edge(H, W)]
    b = G.batch(pairs)
    for kw in (dict(sgm_paths=8), dict(do_refine=1), dict(optimization=2), dict(aggregation=0, optimization=0)):
        sb = StereoBatch(md, H, W, 3, device=0, **kw)
        try:
            sb.upload(*(b[k] for k in KEYS))
            got = sb.run(0.3)
        finally:
            sb.close()
        cfg = oracle.config(H, W, md, **kw)
        for i, p in enumerate(pairs):
            np.testing.assert_array_equal(got[i], oracle.run_ex(p, cfg)["disp"], err_msg=f"{kw} pair {i}")


# ---- signed costs ----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,md", SHAPES)
@pytest.mark.parametrize("cost", ["censusGrad", "Census"])
@pytest.mark.parametrize("mode", [0, 1])
def test_signed_gf(oracle, mode, cost, H, W, md):
    """GF in both forms on signed_blocks: WTA, sgm 4 and sgm 8 at every shape of the set -- every
    launch_kf_signed instantiation and the signed checkpointed pairs (D = 200)."""
    pair = G.signed_blocks(H, W, SIGNED_SEED)
    neg = 0
    for opt, paths in ((0, 4), (1, 4), (1, 8)):
        want = _check_against_oracle(oracle, pair, H, W, md, cost, 2, opt, paths, gf_mode=mode)
        neg += int((want["final"] < 0).sum())
    assert neg > 0   # (the share at 40 x 61 is pinned in test_degenerate_host.py)


@pytest.mark.parametrize("cost", ["censusGrad", "Census"])
@pytest.mark.parametrize("H,W,md", SHAPES)
def test_signed_gfnl(oracle, cost, H, W, md):
    """GFNL (NL where the local variance is low, the NL / GF blend elsewhere) keeps GF's negative
    costs; its reference is the restatement (pyref_box.gfnl on the oracle's NL and GF volumes,
    pyref.sgm).  WTA, sgm 4 and sgm 8 at every shape, the GF form alternating with the shape."""
    mode = SHAPES.index((H, W, md)) % 2
    pair = G.signed_blocks(H, W, SIGNED_SEED)
    cfg = oracle.config(H, W, md, cost=cost, gf_mode=mode)
    raw = oracle.cost_volume(pair, cfg)
    # signed_blocks is high-contrast everywhere; the median of the variance plane as the threshold
    # sends half of the pixels to each branch
    thresh = float(np.float32(np.median(B.variance_plane(pair["lgray"]))))
    vol, mask = B.gfnl(oracle.nl_aggregate(raw, pair["lbgr"], cfg), oracle.guided_filter(raw, pair["lbgr"], cfg), pair["lgray"],
                       thresh)
    assert (vol < 0).any() and 0.25 < mask.mean() < 0.75
    scaled = pyref.solve_all(vol)
    for opt, paths in ((0, 4), (1, 4), (1, 8)):
        final = pyref.sgm(scaled, pair["lbgr"], paths=paths) if opt else scaled
        assert (final < 0).any()
        with Ctx(md, H, W, cost_method=cost, aggregation="GFNL", gf_mode=mode, optimization=opt, sgm_paths=paths,
                 keep_final_volume=1) as c:
            c.call("sm_gfnl_config", thresh)
            c.set_images(pair)
            c.call("sm_cost_calculate")
            assert_bits_equal(c.volume(0), vol, err_msg="GFNL volume")
            c.call("sm_solve_all", 1, 0.3)
            np.testing.assert_array_equal(c.optimize(), pyref.wta(final), err_msg=f"opt {opt} paths {paths}")
            assert_bits_equal(c.volume(0), final, err_msg=f"final volume, opt {opt} paths {paths}")


@pytest.mark.parametrize("mode", [0, 1])
def test_signed_with_refine(oracle, mode):
    H, W, md = 40, 61, 23
    _check_against_oracle(oracle, G.signed_blocks(H, W, SIGNED_SEED), H, W, md, "censusGrad", 2, 1, 4, refine=1, gf_mode=mode)


def test_signed_vmtop(oracle):
    """Candidate selection (Do_vmTop) on a final volume with negative elements."""
    H, W, md = 40, 61, 23
    vt = dict(method=0, num=3, thres=float(np.float32(1.09)), ts=10, has_cir2=True, cir3_color_limit=False)
    pair = G.signed_blocks(H, W, SIGNED_SEED)
    ref = oracle.run_ex(pair, oracle.config(H, W, md, aggregation=2, gf_mode=0), dumps=("final",))
    assert (ref["final"] < 0).any()
    want = V.vmtop(ref["final"], pair["lbgr"], vt["num"], np.float32(vt["thres"]), vt["method"], vt["ts"], vt["has_cir2"],
                   vt["cir3_color_limit"])
    sb = StereoBatch(md, H, W, 1, device=0, aggregation=2, gf_mode=0)
    try:
        sb.vmtop_config(True, **vt)
        sb.upload(*(pair[k][None] for k in KEYS))
        got = sb.run(0.3)[0]
    finally:
        sb.close()
    np.testing.assert_array_equal(got, want)


def test_signed_pkr(oracle):
    """refine()'s peak-ratio stage on a final volume with negative elements: (c1 - c0) / c1 with
    c1 < 0 or c0 < 0 <= c1."""
    H, W, md = 40, 61, 23
    pair = G.signed_blocks(H, W, SIGNED_SEED)
    cfg = oracle.config(H, W, md, aggregation=2, gf_mode=0, do_refine=1)
    ref = oracle.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
    assert (ref["final"] < 0).any()
    want = X.refine_ext(oracle, cfg, ref["disp_raw"], ref["disp_right"], oracle.arms(pair["lbgr"], cfg), pair["lbgr"],
                        ref["final"], do_pkr=True)
    sb = StereoBatch(md, H, W, 1, device=0, aggregation=2, gf_mode=0, do_refine=1, refine_ext=dict(do_pkr=True))
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        got = sb.run(0.3)[0]
        mask = sb.get_pkr_mask()
    finally:
        sb.close()
    np.testing.assert_array_equal(mask, want["mask"])
    np.testing.assert_array_equal(got, want["disp"])


# ---- NaN volumes -----------------------------------------------------------------------------------

NAN_CASES = [(kind, mode, shape) for kind in G.GREY_KINDS for mode in (0, 1) for shape in SHAPES]


def _nan_ids(c):
    return f"{c[0]}-mode{c[1]}-{c[2][0]}x{c[2][1]}-D{c[2][2] + 1}"


@pytest.mark.parametrize("case", NAN_CASES, ids=_nan_ids)
def test_nan_volume_wta(oracle, case):
    """WTA alone: k_wta keeps FLT_MAX on a false `>` and answers -1."""
    kind, mode, (H, W, md) = case
    want = _check_against_oracle(oracle, G.grey_contrast(H, W, 5, kind), H, W, md, "censusGrad", 2, 0, 4, gf_mode=mode)
    assert np.isnan(want["agg"]).all() and (want["disp"] == -1).all()


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("case", NAN_CASES, ids=_nan_ids)
def test_nan_volume_sgm(oracle, case, paths):
    """The signed SGM kernels on an all-NaN volume: every path cost is NaN, no lane matches the
    minimum, the map is -1."""
    kind, mode, (H, W, md) = case
    want = _check_against_oracle(oracle, G.grey_contrast(H, W, 5, kind), H, W, md, "censusGrad", 2, 1, paths, gf_mode=mode)
    assert np.isnan(want["final"]).all() and (want["disp"] == -1).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_volume_with_refine(oracle, mode):
    H, W, md = 40, 61, 23
    want = _check_against_oracle(oracle, G.grey_contrast(H, W, 5, "blocks"), H, W, md, "censusGrad", 2, 1, 4, refine=1, gf_mode=mode)
    assert (want["disp"] == -1).all()


# images wide enough for the NaN of step_edge (18 columns to either side of the edge: two box
# filters of radius 9) to leave finite pixels at both ends of a row, one per SGM kernel layout
PARTIAL_SHAPES = [(40, 61, 23), (33, 80, 69), (23, 64, 130), (21, 64, 199)]


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W,md", PARTIAL_SHAPES)
def test_nan_partial_volume_sgm(oracle, H, W, md, mode, paths):
    """step_edge under GF: NaN pixels around the edge, finite ones beside them.  The reference's
    std::min chain keeps the NaN of an all-NaN previous column, so a path that has crossed a NaN
    pixel stays NaN to its end and the summed volume is NaN on more pixels than the aggregated one;
    v_min_f32 would drop the NaN and go on with P2 (sm_sgm.hip, keep_nan)."""
    want = _check_against_oracle(oracle, G.step_edge(H, W), H, W, md, "censusGrad", 2, 1, paths, gf_mode=mode)
    agg_nan, final_nan = np.isnan(want["agg"]).all(axis=2), np.isnan(want["final"]).all(axis=2)
    assert agg_nan.any() and not agg_nan.all()
    assert (final_nan & ~agg_nan).any() and ((want["disp"] == -1) == final_nan).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_partial_volume_with_refine(oracle, mode):
    H, W, md = 33, 80, 69
    want = _check_against_oracle(oracle, G.step_edge(H, W), H, W, md, "censusGrad", 2, 1, 4, refine=1, gf_mode=mode)
    assert not np.isnan(want["agg"]).all() and (want["disp_raw"] == -1).all()   # the two horizontal paths poison every row
