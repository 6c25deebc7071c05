"""GPU: the default pipeline's kernels against the reference's OWN functions, bit for bit, the oracle out of the loop.

The expected census codes, arms, volumes and maps are outputs of oracle/_ref/ref_core_driver -- the reference's
genCensusCode_NC_Sur, calArms, censusGrad / censusCal, cbca_core, sgm, gen_dispFromVm, so, so_R2L and so_T2D,
compiled by oracle/ref_core.mk behind our driver -- on the same images, every stage fed the reference build's
own output of the stage before (tests/ref_core_cases.py).  The kernels are driven through the C ABI and read
back with sm_get_census, sm_get_arms, sm_get_volume after each stage, and the maps.

Where the binary is present (build() makes it beside a reference checkout) it is run on the host, and its output
must also equal the recording.  A GPU machine may have neither the checkout nor oracle/_ref/: there the
expectation is the binary's RECORDED output, tests/golden/ref_core_gpu.npz (written by
tests/golden/make_ref_core.py, kept current by tests/test_ref_core.py): the sha256 of every expected array's bits,
the array itself where it is small, and the sha256 of its inputs, which must match the inputs regenerated here.
The comparison is the same either way: every bit.  With a checkout and no binary the tests fail.  No test skips.

Shapes: the smallest that reach each kernel layout -- census words, cost and prep tiles (23 x 97 with D 24 / 100,
67 x 257 x 16); the CBCA fast sweeps of both views (2 and 68 x 96 x 256, 40 x 80 x 128 on long arms, 200 x 90 x 64
for steady tiles); the SGM row, dwordx4 and scalar layouts and the checkpointed pairs (9 x 17 x 64, 17 x 33 x 256,
23 x 7 x 200, 8 paths at 12 x 19 x 256); the scan-line optimisers on default and so_float_minima contexts
(33 x 71 x 32); gen_dispFromVm's tie and NaN rule on crafted volumes at one, two and four disparities per lane.
so_T2D's expectation is recorded with fill byte 0 only: DESIGN section 25, finding 1."""
import functools
import os

import numpy as np
import pytest

import ref_core_cases as K
from capi_run import Ctx
from mystereomatching_amd import _capi
from oracle import ref_core as R

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_core_gpu.npz")


@functools.lru_cache(maxsize=None)
def _recorded():
    return dict(np.load(RECORDED))


@functools.lru_cache(maxsize=None)
def expected(key):
    """{name: array, or the sha256 of its bits} of case `key` from the reference build: run now where the binary
    is, else recorded."""
    spec, rec = K.gpu_keys()[key], _recorded()
    assert K.gpu_input_digest(spec) == str(rec[f"in_{key}"]), f"{key}: the inputs differ from the recorded ones"
    names = str(rec[f"names_{key}"]).split(",")
    if R.available():
        arrays = K.gpu_expected(spec)
        assert list(arrays) == names
        for n, a in arrays.items():
            assert K.sha256(a) == str(rec[f"sha_{key}_{n}"]), f"{key}.{n}: the recording is stale (make_ref_core.py)"
        return arrays
    if R.checkout_present():
        pytest.fail(f"a reference checkout is at {R.reference_dir()} but {R.BINARY} is not built: "
                    "build() (make -C oracle -f ref_core.mk) must produce it")
    return {n: rec[f"arr_{key}_{n}"] if f"arr_{key}_{n}" in rec else str(rec[f"sha_{key}_{n}"]) for n in names}


def assert_is_expected(got, want, what):
    got = np.ascontiguousarray(got)
    if isinstance(want, str):
        assert K.sha256(got) == want, f"{what}: the bits differ from the reference build's (by sha256)"
        return
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        got, want = K.bits(got), K.bits(want)
    np.testing.assert_array_equal(got, want, err_msg=what)


def census(c, view):
    H, W, _ = c.shape
    out = np.empty((H, W, R.CENSUS_WORDS), np.uint64)
    c.call("sm_get_census", view, _capi.ptr(out))
    return out


def arms(c, view):
    H, W, _ = c.shape
    out = np.empty((H, W, 4), np.uint16)
    c.call("sm_get_arms", view, _capi.ptr(out))
    return out


def assert_arms(c, view, want, what):
    """HVL[view] is H x W x 5 in the reference (L, R, U, D and their sum, cpp:3031-3043); sm_get_arms gives the four."""
    got = arms(c, view)
    if isinstance(want, str):
        full = np.concatenate([got, got.sum(axis=2, dtype=np.uint16)[..., None]], axis=2)
        assert K.sha256(full) == want, f"{what}: the arms differ from the reference build's (by sha256)"
    else:
        np.testing.assert_array_equal(got, want[..., :4], err_msg=what)


@pytest.mark.parametrize("cost", ["censusGrad", "Census"])
@pytest.mark.parametrize("H,W,D", K.GPU_COST)
def test_census_arms_cost_vs_reference_build(H, W, D, cost):
    want = expected(f"cost_{cost}_{H}x{W}x{D}")
    pair = K.pair(K.gpu_kind(H, W, D), H, W, D)
    with Ctx(D - 1, H, W, cost_method=cost, aggregation=0, optimization=0, compute_right_view=1) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        for view in (0, 1):
            assert_is_expected(census(c, view), want[f"census{view}"], f"census codes, view {view}")
            if cost == "censusGrad":      # the arms weigh the two gradient terms (cpp:403-424)
                assert_arms(c, view, want[f"arms{view}"], f"arms, view {view}")
            assert_is_expected(c.volume(view), want[f"cost{view}"], f"raw costs, view {view}")


@pytest.mark.parametrize("H,W,D", K.GPU_CBCA)
def test_cbca_vs_reference_build(H, W, D):
    """Both views (cbca_core's LOR loop with Do_refine, cpp:5592-5599), two iterations, from the kernels' own costs."""
    want = expected(f"cbca_{H}x{W}x{D}")
    pair = K.pair(K.gpu_kind(H, W, D), H, W, D)
    with Ctx(D - 1, H, W, do_refine=1) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        for view in (0, 1):
            assert_arms(c, view, want[f"arms{view}"], f"arms, view {view}")     # 40 x 80: arms at the cap 34
            assert_is_expected(c.volume(view), want[f"agg{view}"], f"aggregated volume, view {view}")


@pytest.mark.parametrize("H,W,D,paths", K.GPU_SGM)
def test_sgm_wta_vs_reference_build(H, W, D, paths):
    """SolveAll's scale, sgm(vm[0], true), sgm(vm[1], false) and gen_dispFromVm of both.  8 paths: DESIGN section 2, row a15-a16
    (sm_params.sgm_paths; the recipe hands sgm() the count, the direction table is the reference's)."""
    want = expected(f"sgm{paths}_{H}x{W}x{D}")
    pair = K.pair(K.gpu_kind(H, W, D), H, W, D)
    with Ctx(D - 1, H, W, do_refine=1, sgm_paths=paths, keep_final_volume=1) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        c.call("sm_solve_all", 1, K.REG_LAMBDA)
        assert_is_expected(c.volume(0), want["scaled0"], "after SolveAll")
        assert_is_expected(c.optimize(), want["disp0"], "DP[0]")
        assert_is_expected(c.disp(1), want["disp1"], "DP[1]")
        for view in (0, 1):
            assert_is_expected(c.volume(view), want[f"sgm{view}"], f"path sum, view {view}")


@pytest.mark.parametrize("H,W,D", K.GPU_WTA)
def test_wta_rule_vs_reference_build(H, W, D):
    """gen_dispFromVm's rule by itself: a volume of tied minima (-0 against +0 too), NaN at d = 0 and elsewhere, pixels
    of NaN or FLT_MAX only (ref_core_cases.wta_volume) is put into vm[0] and k_wta's map compared with the build's."""
    want = expected(f"wta_{H}x{W}x{D}")
    vol = K.wta_volume(H, W, D)
    with Ctx(D - 1, H, W, aggregation=0, optimization=0) as c:
        c.set_images(K.pair("make_pair", H, W, D))
        c.call("sm_cost_calculate")
        c.call("sm_set_volume", 0, _capi.ptr(vol))
        assert_is_expected(c.optimize(), want["disp0"], "DP[0]")


@pytest.mark.parametrize("float_minima", [False, True], ids=["default", "so_float_minima"])
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_scanline_vs_reference_build(variant, float_minima):
    """so / so_R2L / so_T2D on both views after CBCA and SolveAll (cpp:1093-1104: I[0] is the left image for both).
    so and so_R2L leave their accumulated costs in vm[view]; so_T2D runs on a clone (cpp:1096-1097)."""
    H, W, D = K.GPU_SO
    want = expected(f"{variant}_{H}x{W}x{D}")
    pair = K.pair(K.gpu_kind(H, W, D), H, W, D)
    lib = _capi.load()
    # do_refine: vm[1] goes through CBCA and SolveAll too, as in the recorded chain (without it so() runs on the raw
    # right-view costs, cpp:5592, 2178)
    p = _capi.default_params(D - 1, H, W, optimization="so", keep_final_volume=1, do_refine=1)
    ctx, st, entry = _capi.create(lib, p, 0, float_minima)
    assert entry == ("sm_create_ex" if float_minima else "sm_create")
    _capi.check(lib, ctx, st, entry)
    try:
        def call(name, *args):
            _capi.check(lib, ctx, getattr(lib, name)(ctx, *args), name)
        im = [np.ascontiguousarray(pair[k]) for k in R.KEYS]
        call("sm_so_config", _capi.SO_VARIANTS[variant], _capi.SO_PN_DEFAULT, _capi.SO_PN_DEFAULT)
        call("sm_set_images", _capi.ptr(im[0]), _capi.ptr(im[1]), W * 3, _capi.ptr(im[2]), _capi.ptr(im[3]), W)
        call("sm_cost_calculate")
        call("sm_solve_all", 1, K.REG_LAMBDA)
        scaled = []
        for view in (0, 1):
            scaled.append(np.empty((H, W, D), np.float32))
            call("sm_get_volume", view, _capi.ptr(scaled[view]))
        call("sm_disp_optimize", None)
        for view in (0, 1):
            dp, vol = np.empty((H, W), np.int16), np.empty((H, W, D), np.float32)
            call("sm_get_disp", view, _capi.ptr(dp))
            call("sm_get_volume", view, _capi.ptr(vol))
            assert_is_expected(dp, want[f"disp{view}"], f"DP[{view}]")
            if variant == "so_T2D":
                np.testing.assert_array_equal(K.bits(vol), K.bits(scaled[view]), err_msg=f"vm[{view}] is left alone")
            else:
                assert_is_expected(vol, want[f"acc{view}"], f"accumulated costs, view {view}")
    finally:
        lib.sm_destroy(ctx)
