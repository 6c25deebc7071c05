"""GPU: aggregation "NL" against the reference's OWN tree-filter code, bit for bit.

The expected volumes are outputs of oracle/_ref/ref_nl_driver -- the reference's
qx_mst_kruskals_image, qx_tree_filter and ctmf, compiled by oracle/ref_nl.mk -- on the raw cost
volume, with the division as NL() has it (stereoMatching.cpp:4892-4917; oracle/ref_nl.py).  Nothing
between the raw costs and the compared volume is a restatement: the GPU's median, edge weights,
Boruvka spanning trees, tree walk and filter rounds answer to the reference's Kruskal and its own
filter.  The raw costs are the oracle's (censusGrad needs no NL code), pinned on the GPU by
tests/test_gpu_parity.py.

Where the binary is present (build() makes it beside a reference checkout) it is run on the host,
and its output must also equal the recording.  A GPU machine may have neither the checkout nor
oracle/_ref/: there the expectation is the binary's RECORDED output, tests/golden/ref_nl_gpu.npz
(written by tests/golden/make_ref_nl.py and kept current by tests/test_ref_nl.py): the sha256 of
every expected volume's bits, the volume itself where it is small, and the sha256 of its inputs,
which must match the inputs regenerated here.  The comparison is the same either way: every bit.
With a checkout and no binary the tests fail.  No test skips.

Every shape lies outside 363..543 px, where the reference's ctmf call cannot work."""
import functools
import os

import numpy as np
import pytest

import pyref
import ref_nl_cases as K
from capi_run import KEYS, Ctx, assert_bits_equal
from mystereomatching_amd import StereoBatch, _capi
from oracle import ref_nl as R

pytestmark = pytest.mark.gpu

NL, GFNL = 3, 10
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nl_gpu.npz")


@functools.lru_cache(maxsize=None)
def _cases():
    return K.gpu_cases()


@functools.lru_cache(maxsize=None)
def _recorded():
    return dict(np.load(RECORDED))


@functools.lru_cache(maxsize=None)
def expected(key):
    """The reference build's NL() volume of case `key`: run now where the binary is, else recorded.
    Returns the float32 volume, or -- for a large volume without the binary -- the sha256 of its bits."""
    raw, bgr, sigma = _cases()[key]
    rec = _recorded()
    assert K.input_digest(raw, bgr, sigma) == str(rec[f"in_{key}"]), f"{key}: the inputs differ from the recorded ones"
    if R.available():
        vol = R.nl(raw, bgr, sigma)
        assert K.sha256(K.bits(vol)) == str(rec[f"sha_{key}"]), f"{key}: the recording is stale (make_ref_nl.py)"
        vol.setflags(write=False)
        return vol
    if R.checkout_present():
        pytest.fail(f"a reference checkout is at {R.reference_dir()} but {R.BINARY} is not built: "
                    "build() (make -C oracle -f ref_nl.mk) must produce it")
    return rec[f"vol_{key}"] if f"vol_{key}" in rec else str(rec[f"sha_{key}"])


def assert_is_expected(got, want, err_msg=""):
    if isinstance(want, str):
        assert K.sha256(K.bits(got)) == want, f"{err_msg}: the volume's bits differ from the reference build's (by sha256)"
    else:
        assert_bits_equal(got, want, err_msg=err_msg)


def _gpu_volumes(pair, D, views=(0,), **params):
    H, W = pair["lgray"].shape
    params.setdefault("aggregation", NL)
    with Ctx(D - 1, H, W, optimization=0, **params) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        return [c.volume(v) for v in views]


@pytest.mark.parametrize("kind", K.GPU_KINDS)
@pytest.mark.parametrize("H,W,D", K.GPU_SHAPES)
def test_nl_volume_vs_reference_build(kind, H, W, D):
    assert not R.in_window(H, W)
    got, = _gpu_volumes(K.gpu_pair(kind, H, W, D, 600), D)
    assert_is_expected(got, expected(f"left_{kind}_{H}x{W}x{D}"))


def test_nl_both_views_vs_reference_build():
    """Do_refine builds vm[1] too, but NL() (cpp:4892-4917) hands aggreCV vm[0] alone, with I_c[0] as the
    guide: vm[0] is the reference build's NL of the left costs under the left image, vm[1] stays the
    raw right-view costs -- no tree is ever built from the right image."""
    H, W, D, idx = K.GPU_BOTH
    pair = K.gpu_pair("make_pair", H, W, D, idx)
    got0, got1 = _gpu_volumes(pair, D, views=(0, 1), do_refine=1)
    assert_is_expected(got0, expected("both_view0"), err_msg="view 0")
    raw1 = _cases()["both_view1_if_filtered"][0]
    assert_bits_equal(got1, raw1, err_msg="view 1")
    # a filtered vm[1] would show: the reference build's filter changes nearly all of it
    filtered = expected("both_view1_if_filtered")
    frac = float(_recorded()["frac_both_view1_changed"]) if isinstance(filtered, str) else \
        float((K.bits(filtered) != K.bits(raw1)).mean())
    assert frac > 0.9


@pytest.mark.parametrize("sigma", [0.5, 0.005])
def test_nl_sigma_vs_reference_build(sigma):
    """sm_params.nl_sigma, above the default and below update_table's 0.01 clamp."""
    H, W, D, idx = K.GPU_SIGMA
    got, = _gpu_volumes(K.gpu_pair("make_pair", H, W, D, idx), D, nl_sigma=sigma)
    want, default = expected(f"sigma_{sigma}"), expected("sigma_0.1")
    assert_is_expected(got, want)
    assert (K.bits(want) != K.bits(default)).mean() > 0.9   # sigma reaches the result (volumes recorded in full)


def test_gfnl_nl_half_vs_reference_build():
    """GFNL: where sm_get_gfnl_mask selects NL alone, the volume is the reference build's NL volume."""
    H, W, D, _ = K.GPU_GFNL
    pair = K.gfnl_pair()
    with Ctx(D - 1, H, W, aggregation=GFNL, optimization=0) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        got = c.volume(0)
        mask = np.empty((H, W), np.uint8)
        c.call("sm_get_gfnl_mask", _capi.ptr(mask))
    share = float((mask != 0).mean())
    print(f"NL alone at {100 * share:.1f} % of the pixels")
    assert 0.10 <= share <= 0.90, "a bad input: both classes must hold >= 10 % of the pixels"
    want = expected("gfnl")                                          # recorded in full
    sel = mask != 0
    np.testing.assert_array_equal(K.bits(got)[sel], K.bits(want)[sel])
    assert (K.bits(got)[~sel] != K.bits(want)[~sel]).mean() > 0.5    # the other class is blended with GF


@pytest.mark.parametrize("opt", [0, 1], ids=["wta", "sgm"])
def test_batched_nl_vs_reference_build(opt):
    """Three different pairs on two streams through sm_run.  The C ABI reaches the volume of slot 0
    only (sm_get_volume): with WTA it is SolveAll of NL's volume and is compared bit for bit; the
    other pairs, and "sgm" (whose NL front runs on a stream of its own), are held to the reference
    build through their maps: WTA (and pyref's SGM) of the reference-built volumes (recorded in full)."""
    H, W, D, members = K.GPU_BATCH
    n = len(members)
    pairs = [K.gpu_pair(kind, H, W, D, idx) for kind, idx in members]
    vols = [pyref.solve_all(np.array(expected(f"batch_{i}"))) for i in range(n)]
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation=NL, optimization=opt, sgm_paths=4, sub_batch=1,
                     num_streams=2, keep_final_volume=int(opt == 0))
    try:
        sb.upload(*(np.stack([p[k] for p in pairs]) for k in KEYS))
        got = sb.run(0.3)
        if opt == 0:
            vol = np.empty((H, W, D), np.float32)
            _capi.check(sb._lib, sb._ctx, sb._lib.sm_get_volume(sb._ctx, 0, _capi.ptr(vol)))
            assert_bits_equal(vol, vols[0], err_msg="slot 0 after SolveAll")
    finally:
        sb.close()
    for i in range(n):
        want = pyref.wta(vols[i] if opt == 0 else pyref.sgm(vols[i], pairs[i]["lbgr"], paths=4))
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")
