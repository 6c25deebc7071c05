"""GPU parity of the float-minima scan-line optimisers (sm_create_ex, so_float_minima = 1): so, so_R2L and so_T2D on
volumes with costs of either sign, both zeros and NaN, and refine()'s volume-reading stages after "so".

The yardstick is tests/pyref_so_float.py, the reference's loops restated with its C++ first minimum and pinned to the C
oracle's smo_so on the same crafted volumes in tests/test_so_float_host.py.  Volumes are injected with sm_set_volume
into contexts made by sm_create_ex; the crafted ones (tests/so_float_cases.py) start from the context's own CBCA volume.
On every sizeable shape the restatement alone shows that the comparison is not vacuous: the right map differs from what
minima on unsigned bit patterns (the kernels for costs >= +0), NaN-dropping minima (v_min_f32) and an ordering with
-0 < +0 would give (so_float_cases.assert_not_vacuous).
"""
import numpy as np
import pytest

import degenerate
import pyref_da as DA
import pyref_refine_ext as RX
import pyref_so_float as PF
import so_float_cases as SC
from mystereomatching_amd import StereoBatch, StereoMatching, SolveAll, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
VARIANTS = ("so", "so_R2L", "so_T2D")
# (H, W, D) for so and so_R2L; so_T2D takes them with H and W exchanged
SHAPES = [(5, 3, 10), (2, 2, 1), (31, 57, 16), (9, 70, 100), (17, 150, 128), (13, 300, 256),
          (6, 1100, 256), (7, 2100, 64),                            # the trace in global memory
          (4, 63, 16), (4, 64, 16), (4, 65, 16), (4, 129, 16),      # the map's 64-wide flush groups
          (13, 40, 600)]                                            # K = 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def shape_for(variant, H, W, D):
    return (W, H, D) if variant == "so_T2D" else (H, W, D)


def steps_lines(variant, H, W):
    return (H, W) if variant == "so_T2D" else (W, H)


class Ctx:
    """A context made by sm_create_ex (so_float_minima = fm) with the pair's images loaded and costCalculate run:
    run(vols) injects vm[0], vm[1], runs dispOptimize and returns (maps, volumes after)."""

    def __init__(self, H, W, D, pair, fm, variant="so", keep=False, aggregation="CBCA", pn=None, **kw):
        self.lib = _capi.load()
        self.shape = (H, W, D)
        p = _capi.default_params(D - 1, H, W, optimization="so", aggregation=aggregation, keep_final_volume=int(keep), **kw)
        self.ctx, st, entry = _capi.create(self.lib, p, 0, fm)
        assert entry == ("sm_create_ex" if fm else "sm_create")
        self.ok(st, entry)
        pn = pn or (_capi.SO_PN_DEFAULT, _capi.SO_PN_DEFAULT)
        self.ok(self.lib.sm_so_config(self.ctx, _capi.SO_VARIANTS[variant], float(pn[0]), float(pn[1])), "sm_so_config")
        im = [np.ascontiguousarray(pair[k]) for k in KEYS]
        self.ok(self.lib.sm_set_images(self.ctx, _capi.ptr(im[0]), _capi.ptr(im[1]), W * 3, _capi.ptr(im[2]), _capi.ptr(im[3]), W),
                "sm_set_images")
        self.ok(self.lib.sm_cost_calculate(self.ctx), "sm_cost_calculate")

    def ok(self, st, what):
        _capi.check(self.lib, self.ctx, st, what)

    def volume(self, view):
        a = np.empty(self.shape, np.float32)
        self.ok(self.lib.sm_get_volume(self.ctx, view, _capi.ptr(a)), "sm_get_volume")
        return a

    def run(self, vols):
        H, W, D = self.shape
        for view, v in enumerate(vols):
            v = np.ascontiguousarray(v, np.float32)
            self.ok(self.lib.sm_set_volume(self.ctx, view, _capi.ptr(v)), "sm_set_volume")
        self.ok(self.lib.sm_disp_optimize(self.ctx, None), "sm_disp_optimize")
        maps = []
        for view in (0, 1):
            d = np.empty((H, W), np.int16)
            self.ok(self.lib.sm_get_disp(self.ctx, view, _capi.ptr(d)), "sm_get_disp")
            maps.append(d)
        return maps, [self.volume(0), self.volume(1)]

    def close(self):
        if self.ctx is not None and self.ctx.value:
            self.lib.sm_destroy(self.ctx)
            self.ctx = None


def crafted_for(c, variant, seed):
    lines = "cols" if variant == "so_T2D" else "rows"
    return [SC.craft(c.volume(view), seed + view, lines=lines) for view in (0, 1)]


# ---- every kernel path on the crafted volumes ----------------------------------------------------------------

@pytest.mark.parametrize("H,W,D", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_paths(variant, H, W, D):
    H, W, D = shape_for(variant, H, W, D)
    pair = S.make_pair(H, W, D, 700 + min(H, W))
    c = Ctx(H, W, D, pair, True, variant, keep=True)
    try:
        base = c.volume(0)
        assert (base >= 0).all()
        vols = crafted_for(c, variant, 1000 + max(H, W))
        maps, after = c.run(vols)
    finally:
        c.close()
    img = pair["lbgr"]
    for view in (0, 1):
        dp, acc = SC.FUNCS[variant](vols[view], img)
        np.testing.assert_array_equal(maps[view], dp, err_msg=f"view {view}")
        if variant == "so_T2D":   # the reference runs on a clone: vm[view] keeps its bits, NaN payloads included
            assert bits(after[view]).tobytes() == bits(vols[view]).tobytes(), f"view {view}: vm changed"
        else:
            assert PF.same_floats(after[view], acc), f"view {view}: accumulated volume"
    if SC.sizeable(*steps_lines(variant, H, W), D):
        print(variant, H, W, D, SC.assert_not_vacuous(variant, vols[0], img))


# ---- the float-minima kernels against the bit-pattern kernels on costs >= +0 -------------------------------

@pytest.mark.parametrize("H,W,D", [(31, 57, 16), (13, 300, 256), (6, 1100, 256)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_old_against_new(variant, H, W, D):
    H, W, D = shape_for(variant, H, W, D)
    pair = S.make_pair(H, W, D, 640 + min(H, W))
    got = []
    for fm in (False, True):
        c = Ctx(H, W, D, pair, fm, variant, keep=True)
        try:
            vols = [c.volume(0), c.volume(1)]
            assert all((v >= 0).all() and not np.signbit(v).any() for v in vols)
            got.append(c.run(vols))
        finally:
            c.close()
    for view in (0, 1):
        np.testing.assert_array_equal(got[0][0][view], got[1][0][view], err_msg=f"view {view}: maps")
        assert bits(got[0][1][view]).tobytes() == bits(got[1][1][view]).tobytes(), f"view {view}: kept volumes"
        np.testing.assert_array_equal(got[1][0][view], SC.FUNCS[variant](vols[view], pair["lbgr"])[0])


# ---- the +inf boundary -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_inf_boundary(variant):
    """+inf at d = 0 and d = D - 1 along one interior line: the reference's backtrack would leave its trace there.
    Every other line equals the restatement, the affected line stays inside [0, D), and the next run is clean."""
    H, W, D = shape_for(variant, 21, 70, 20)
    pair = S.make_pair(H, W, D, 733)
    img = pair["lbgr"]
    c = Ctx(H, W, D, pair, True, variant, keep=True)
    try:
        clean = [c.volume(view) for view in (0, 1)]
        clean = [v - np.float32(np.median(v)) for v in clean]          # finite, about half of the costs negative
        assert all(np.isfinite(v).all() and (v < 0).mean() > 0.3 for v in clean)
        bad = [v.copy() for v in clean]
        line = 9
        for v in bad:
            sel = v[:, line] if variant == "so_T2D" else v[line]     # [steps][D]
            sel[:, 0] = np.inf
            sel[:, D - 1] = np.inf
        maps, _ = c.run(bad)
        keep = np.ones((H, W), bool)
        if variant == "so_T2D":
            keep[:, line] = False
        else:
            keep[line] = False
        for view in (0, 1):
            dp = SC.FUNCS[variant](bad[view], img)[0]
            np.testing.assert_array_equal(maps[view][keep], dp[keep], err_msg=f"view {view}: another line changed")
            assert (maps[view] >= 0).all() and (maps[view] < D).all()
        maps, _ = c.run(clean)
        for view in (0, 1):
            np.testing.assert_array_equal(maps[view], SC.FUNCS[variant](clean[view], img)[0], err_msg=f"view {view}: the next run")
    finally:
        c.close()


# ---- end to end: the aggregations whose costs are signed or NaN ---------------------------------------------

class Statics:
    """StereoMatching's class-level selectors for one block, restored afterwards."""

    NAMES = ("costcalculation", "aggregation", "optimization", "Do_refine", "SO_VARIANT", "SO_PN", "MY_GUIDE", "Do_calPKR",
             "Do_subpixelEnhancement", "Do_discontinuityAdjust")

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: getattr(StereoMatching, k) for k in self.NAMES}
        for k, v in self.kw.items():
            setattr(StereoMatching, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(StereoMatching, k, v)


def staged(pair, H, W, D, variant, aggregation, cost="censusGrad", my_guide=False, refine=False, stages=()):
    """costCalculate + SolveAll, the volumes read back, dispOptimize [+ refine]; the facade chooses sm_create_ex and
    keep_final_volume by itself."""
    with Statics(costcalculation=cost, aggregation=aggregation, optimization="so", Do_refine=refine, SO_VARIANT=variant,
                 MY_GUIDE=my_guide, **{s: True for s in stages}):
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None,
                            StereoMatching.Parameters(D - 1, H, W))
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        vol = sm.vm
        sm.dispOptimize()
        out = dict(vol=vol, dp=[sm.DP[0].copy(), sm.DP[1].copy()], after=sm.vm, arms=sm.HVL[0])
        if refine:
            out["refined"] = sm.refine().copy()
            out.update(mask=sm.PKR_Err_Mask, se=sm.SE, edges=sm.DA_Edge)
    return out


GF_SEED = 5   # degenerate.signed_blocks: GF's minimum is negative at 13 % / 23 % of the pixels (test_so_float_host.py)


def e2e_pair(aggregation, H, W, D, seed=GF_SEED):
    """GF and GFNL on make_pair's texture stay >= 0 (measured: no negative cost at all), which would show nothing:
    they take degenerate.signed_blocks, whose isolated bright blocks drive the guided filter below zero."""
    return degenerate.signed_blocks(H, W, seed) if aggregation in ("GF", "GFNL") else S.make_pair(H, W, D, 600)


E2E = [("GF", "censusGrad", False, (26, 71, 32)), ("GF", "censusGrad", False, (12, 40, 16)), ("GF", "censusGrad", True, (26, 71, 32)),
       ("GFNL", "censusGrad", False, (26, 71, 32)), ("GFNL", "censusGrad", False, (12, 40, 16)),
       ("BF", "grad", False, (26, 71, 32)), ("BF", "grad", False, (12, 40, 16))]


@pytest.mark.parametrize("aggregation,cost,my_guide,shape", E2E)
@pytest.mark.parametrize("variant", VARIANTS)
def test_end_to_end(variant, aggregation, cost, my_guide, shape):
    H, W, D = shape
    pair = e2e_pair(aggregation, H, W, D)
    r = staged(pair, H, W, D, variant, aggregation, cost, my_guide)
    for view in (0, 1):
        dp, acc = SC.FUNCS[variant](r["vol"][view], pair["lbgr"])
        np.testing.assert_array_equal(r["dp"][view], dp, err_msg=f"view {view}")
    if aggregation == "GF":
        neg = (np.nan_to_num(r["vol"][0], nan=0.0).min(axis=2) < 0).mean()
        print(f"GF {H}x{W}x{D} my_guide={my_guide}: a negative cost at {100 * neg:.1f} % of the pixels")
        assert neg > 0.10   # without it the case shows nothing about signed costs
        # What minima on unsigned bit patterns would give on this volume, from the restatement alone.  Measured: so and
        # so_R2L add a cost_min of about 1 per step, so their running minima are positive after the first steps and the
        # two maps agree; so_T2D's normalised costs stay signed and the maps differ.  test_kernel_paths is where every
        # kernel path meets signed running minima.
        wrong = SC.FUNCS[variant](r["vol"][0], pair["lbgr"], first_min=PF.first_min_unsigned)[0]
        print(f"  {variant}: unsigned minima would change {100 * (wrong != r['dp'][0]).mean():.2f} % of the map")


@pytest.mark.parametrize("kind", degenerate.GREY_KINDS)
def test_all_nan_volume(kind):
    """GF on the image tests/degenerate.py describes for it (grey_contrast: B = G = R at 0 / 255): the guided filter's
    determinant cancels to 0, every cost is NaN and every first minimum is the sticky NaN at index 0, so the map is 0
    everywhere.  (A constant image does not give NaN: its GF volume is finite and full of ties, next test.)"""
    H, W, D = 24, 30, 8
    pair = degenerate.grey_contrast(H, W, 3, kind)
    for variant in VARIANTS:
        r = staged(pair, H, W, D, variant, "GF")
        assert np.isnan(r["vol"][0]).all(), variant
        assert not r["dp"][0].any(), variant
        # (without Do_refine vm[1] is the raw right cost volume, finite)
        np.testing.assert_array_equal(r["dp"][1], SC.FUNCS[variant](r["vol"][1], pair["lbgr"])[0], err_msg=variant)
        rr = staged(pair, H, W, D, variant, "GF", refine=True)      # Do_refine: GF on both views, both all NaN
        assert np.isnan(rr["vol"][1]).all() and not rr["dp"][1].any(), variant


def test_constant_image_through_gf():
    """GF on a constant image: finite costs, equal along every row, and the first index wins every tie."""
    H, W, D = 24, 30, 8
    pair = degenerate.constant(H, W)
    for variant in VARIANTS:
        r = staged(pair, H, W, D, variant, "GF")
        assert np.isfinite(r["vol"][0]).all()
        for view in (0, 1):
            np.testing.assert_array_equal(r["dp"][view], SC.FUNCS[variant](r["vol"][view], pair["lbgr"])[0], err_msg=f"{variant} view {view}")


@pytest.fixture(scope="module")
def batch3():
    H, W, D, n = 26, 71, 32, 3
    pairs = [degenerate.signed_blocks(H, W, GF_SEED + i) for i in range(n)]
    return H, W, D, pairs, degenerate.batch(pairs)


@pytest.mark.parametrize("aggregation,cost", [("GF", "censusGrad"), ("GFNL", "censusGrad"), ("BF", "grad")])
def test_batch_schedules(batch3, aggregation, cost):
    """A batch of 3 under sub_batch 1 and 2 with 1 and 2 streams: the same maps (the right view's of pair 0 too)."""
    H, W, D, pairs, st = batch3
    vols = [staged(p, H, W, D, "so", aggregation, cost)["vol"] for p in pairs]
    want = [[PF.so(vols[i][view], pairs[i]["lbgr"])[0] for view in (0, 1)] for i in range(3)]
    b = StereoBatch(D - 1, H, W, 3, optimization="so", aggregation=aggregation, cost_method=cost)
    try:
        b.upload(*(st[k] for k in KEYS))
        for streams, sub in ((0, 0), (1, 1), (1, 2), (2, 1), (2, 2)):
            b.set_schedule(streams, sub)
            out = b.run()
            for i in range(3):
                np.testing.assert_array_equal(out[i], want[i][0], err_msg=f"pair {i} streams {streams} sub_batch {sub}")
            np.testing.assert_array_equal(b.get_disp(1), want[0][1])
    finally:
        b.close()


# ---- refine()'s volume-reading stages after "so" ------------------------------------------------------------

STAGES = {"pkr": ("Do_calPKR",), "se": ("Do_subpixelEnhancement",), "da": ("Do_discontinuityAdjust",),
          "all": ("Do_calPKR", "Do_subpixelEnhancement", "Do_discontinuityAdjust")}
RH, RW, RD = 40, 66, 24


def expected_refine(oracle, pair, r, variant, stages):
    """refine() restated on the restatement's maps and on vm[0] as the reference's refine() finds it: the accumulated
    volume after so / so_R2L, the aggregated one after so_T2D (which runs on a clone, cpp:1096)."""
    img = pair["lbgr"]
    d0, acc = SC.FUNCS[variant](r["vol"][0], img)
    d1 = SC.FUNCS[variant](r["vol"][1], img)[0]
    vm = r["vol"][0] if variant == "so_T2D" else acc
    cfg = oracle.config(RH, RW, RD - 1, optimization=2, do_refine=1)
    want = DA.refine_da(oracle, cfg, d0, d1, r["arms"], img, vm, do_da="Do_discontinuityAdjust" in stages,
                        do_pkr="Do_calPKR" in stages, do_se="Do_subpixelEnhancement" in stages)
    return d0, d1, vm, want


@pytest.mark.parametrize("which", sorted(STAGES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_refine_after_so(oracle, variant, which):
    stages = STAGES[which]
    pair = S.make_pair(RH, RW, RD, 77)
    r = staged(pair, RH, RW, RD, variant, "CBCA", refine=True, stages=stages)
    d0, d1, vm, want = expected_refine(oracle, pair, r, variant, stages)
    np.testing.assert_array_equal(r["dp"][0], d0)
    np.testing.assert_array_equal(r["dp"][1], d1)
    assert bits(r["after"][0]).tobytes() == bits(vm).tobytes()         # the facade kept the volume by itself
    np.testing.assert_array_equal(r["refined"], want["disp"])
    if "Do_calPKR" in stages:
        np.testing.assert_array_equal(r["mask"], want["mask"])
        assert want["mask"].any()
        if variant != "so_T2D":   # an implementation that forgot the in-place store would read this volume
            assert (want["mask"] != RX.cal_pkr(r["vol"][0])).any()
    if "Do_subpixelEnhancement" in stages:
        assert bits(r["se"]).tobytes() == bits(want["se"]).tobytes()
    if "Do_discontinuityAdjust" in stages:
        np.testing.assert_array_equal(r["edges"], want["edges"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_refine_after_so_in_a_batch(oracle, variant):
    """sm_run with every stage on, and the eval table's stage names: PKR and da follow stage 0, "so"."""
    stages = STAGES["all"]
    pair = S.make_pair(RH, RW, RD, 77)
    r = staged(pair, RH, RW, RD, variant, "CBCA", refine=True, stages=stages)
    want = expected_refine(oracle, pair, r, variant, stages)[3]
    b = StereoBatch(RD - 1, RH, RW, 1, optimization="so", do_refine=1, so_variant=variant,
                    refine_ext=dict(do_pkr=True, do_subpixel=True), refine_da=dict(on=True),
                    eval=dict(keep_maps=True, thresholds=(1.0,)))
    try:
        assert b.params.keep_final_volume == 1
        b.upload(*(pair[k][None] for k in KEYS))
        b.upload_truth(pair["gt"][None].astype(np.float32), pair["nonocc"][None])
        for streams, sub in ((0, 0), (2, 1)):
            b.set_schedule(streams, sub)
            out = b.run()
            np.testing.assert_array_equal(out[0], want["disp"])
            np.testing.assert_array_equal(b.get_pkr_mask(), want["mask"])
            np.testing.assert_array_equal(b.get_da_edges(), want["edges"])
            assert bits(b.download_subpixel()[0]).tobytes() == bits(want["se"]).tobytes()
        assert b.stage_names() == ["so", "od", "PKR", "RV0", "RV1", "pi", "da", "mb"]
        np.testing.assert_array_equal(b.stage_maps(0)[0], r["dp"][0])
    finally:
        b.close()


def test_refine_after_gf_and_so(oracle):
    """GF + so + PKR: the float-minima kernel's accumulated volume (signed, kept in place) is what calPKR reads."""
    pair = degenerate.signed_blocks(RH, RW, 600)
    r = staged(pair, RH, RW, RD, "so", "GF", refine=True, stages=STAGES["pkr"])
    d0, d1, vm, want = expected_refine(oracle, pair, r, "so", STAGES["pkr"])
    assert (r["vol"][0] < 0).any()          # GF's costs are signed here; so's running sums then turn positive
    np.testing.assert_array_equal(r["dp"][0], d0)
    assert PF.same_floats(r["after"][0], vm)
    np.testing.assert_array_equal(r["mask"], want["mask"])
    np.testing.assert_array_equal(r["refined"], want["disp"])
    assert want["mask"].any() and (want["mask"] != RX.cal_pkr(r["vol"][0])).any()
