"""GPU parity of the cost measures "SD", "BT", "grad", "TruncAD", "adGrad" and "ADCensusGrad"
(k_cost_ext, sm_cost_ext.hip) against the numpy twin tests/pyref_cost.py: uint32 equality of both
views' volumes and int16 equality of the maps that tests/pyref.py's stages make of them.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref
import pyref_box
import pyref_cost as PC
import pyref_fif
from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
METHODS = ["SD", "BT", "grad", "TruncAD", "adGrad", "ADCensusGrad"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _freeze(pair):
    pair = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
    for a in pair.values():
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def _noise_pair(H, W, seed):
    """Blocks of colour with noise on top (arms of every length, differences of every size up to
    255); the right image is the left one moved by two columns, with its own noise."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, ((H + 3) // 4, (W + 6) // 5 + 1, 3))
    base = np.kron(coarse, np.ones((4, 5, 1), np.int64))[:H, :W + 2]
    spike = (rng.random((H, W + 2, 1)) < 0.1) * rng.integers(-255, 256, (H, W + 2, 3))
    img = np.clip(base + rng.integers(-12, 13, base.shape) + spike, 0, 255).astype(np.uint8)
    left, right = img[:, :W], np.clip(img[:, 2:].astype(np.int64) + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    return _freeze({"lbgr": left, "rbgr": right, "lgray": S.bgr_to_gray(left), "rgray": S.bgr_to_gray(right)})


@functools.lru_cache(maxsize=None)
def _synthetic_pair(H, W, D, idx):
    return _freeze(S.make_pair(H, W, D, idx))


@functools.lru_cache(maxsize=None)
def _flat_pair(H, W):
    bgr = np.empty((H, W, 3), np.uint8)
    bgr[:] = (90, 140, 33)
    return _freeze({"lbgr": bgr, "rbgr": bgr.copy(), "lgray": S.bgr_to_gray(bgr), "rgray": S.bgr_to_gray(bgr)})


_PRE = {}


def _pre(pair):
    """The twin's per-pair inputs (arms, census bits), computed once per pair and left unchanged."""
    key = id(pair["lbgr"])
    if key not in _PRE:
        _PRE[key] = (pair, PC.prepare(pair, census=True))   # (the pair is kept alive with its id)
    return _PRE[key][1]


def _want_volume(pair, D, method, view):
    pre = _pre(pair)
    return PC.cost_volume(pair, D, method, view, pre["arms"][view], pre["census"])


def _gpu_volumes(pair, D, **over):
    """vm[0], vm[1] after sm_cost_calculate (do_refine = 1: both views exist)."""
    H, W = pair["lgray"].shape
    lib = _capi.load()
    over.setdefault("aggregation", 0)
    p = _capi.default_params(D - 1, H, W, optimization=0, do_refine=1, **over)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(pair["lbgr"]), _capi.ptr(pair["rbgr"]), W * 3,
                                                _capi.ptr(pair["lgray"]), _capi.ptr(pair["rgray"]), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        out = []
        for view in (0, 1):
            got = np.empty((H, W, D), np.float32)
            _capi.check(lib, ctx, lib.sm_get_volume(ctx, view, _capi.ptr(got)))
            out.append(got)
        return out
    finally:
        lib.sm_destroy(ctx)


def _check_raw(pair, D, method):
    got = _gpu_volumes(pair, D, cost_method=method)
    for view in (0, 1):
        want = _want_volume(pair, D, method, view)
        assert (want >= 0).all() and not np.signbit(want).any()
        np.testing.assert_array_equal(bits(got[view]), bits(want), err_msg=f"{method} view {view}")


# the smallest image and D = 1; W < D (whole columns out of range); one short segment; a row in two
# segments at both segment sizes with a ragged last 64-lane chunk; D = 256; a tall image
SHAPES = [(2, 2, 1), (5, 9, 16), (9, 40, 8), (6, 250, 70), (3, 300, 256), (130, 9, 64)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_raw_volume_bits(H, W, D, method):
    _check_raw(_noise_pair(H, W, 9000 + H * 1000 + W), D, method)


@pytest.mark.parametrize("method", METHODS)
def test_raw_volume_bits_synthetic_pair(method):
    H, W, D = 20, 37, 24
    _check_raw(_synthetic_pair(H, W, D, 940 + METHODS.index(method)), D, method)


@pytest.mark.parametrize("method", METHODS)
def test_flat_pair(method):
    """All pixels equal: BT and the gradients are 0, the arms are at their maximum."""
    H, W, D = 8, 40, 8
    pair = _flat_pair(H, W)
    _check_raw(pair, D, method)
    if method in ("BT", "grad", "SD", "TruncAD"):
        v = _want_volume(pair, D, method, 0)
        assert (v[:, D:, :] == 0).all()


def test_grad_without_adaptive_weights():
    H, W, D = 9, 40, 8
    pair = _noise_pair(H, W, 9000 + H * 1000 + W)
    got = _gpu_volumes(pair, D, cost_method="grad", grad_adaptive=0)
    for view in (0, 1):
        want = PC.grad_cost(pair["lgray"], pair["rgray"], None, D, 500, view, adaptive=False)
        np.testing.assert_array_equal(bits(got[view]), bits(want))


def test_sd_reads_ad_trunc_ad():
    H, W, D = 9, 40, 8
    pair = _noise_pair(H, W, 9000 + H * 1000 + W)
    got = _gpu_volumes(pair, D, cost_method="SD", ad_trunc_ad=1e9)
    for view in (0, 1):
        want = PC.sd_cost(pair["lbgr"], pair["rbgr"], D, 1e9, view)
        assert want.max() > 20000
        np.testing.assert_array_equal(bits(got[view]), bits(want))


@pytest.mark.parametrize("cost", ["censusGrad", "Census", "ADCensus", "AD"])
def test_existing_methods_still_equal_the_oracle(oracle, cost):
    """The dispatch change did not reroute k_cost's four methods."""
    H, W, D = 9, 40, 8
    pair = _noise_pair(H, W, 9000 + H * 1000 + W)
    got = _gpu_volumes(pair, D, cost_method=cost)
    for view in (0, 1):
        want = oracle.cost_volume(pair, oracle.config(H, W, D - 1, cost=cost), view=view)
        np.testing.assert_array_equal(bits(got[view]), bits(want), err_msg=f"view {view}")


# ---- maps ------------------------------------------------------------------------------------------

MH, MW, MD = 24, 30, 16


def _map_pair(i=0):
    return _synthetic_pair(MH, MW, MD, 960 + i)


def _run_maps(pairs, **over):
    sb = StereoBatch(MD - 1, MH, MW, len(pairs), device=0, **over)
    try:
        sb.upload(*(np.stack([p[k] for p in pairs]) for k in KEYS))
        return sb.run(0.3)
    finally:
        sb.close()


@pytest.mark.parametrize("method", METHODS)
def test_maps_cbca_sgm4(method):
    pair = _map_pair()
    got = _run_maps([pair], cost_method=method, cbca_iterations=2, optimization=1, sgm_paths=4)[0]
    np.testing.assert_array_equal(got, PC.pipeline(pair, MD, method, pre=_pre(pair)))


@pytest.mark.parametrize("method", ["adGrad", "BT"])
def test_maps_with_refine(method):
    pair = _map_pair()
    got = _run_maps([pair], cost_method=method, cbca_iterations=2, optimization=1, sgm_paths=4, do_refine=1)[0]
    np.testing.assert_array_equal(got, PC.pipeline(pair, MD, method, refine=True, pre=_pre(pair)))


@pytest.mark.parametrize("method", ["SD", "TruncAD"])
def test_maps_so(method):
    pair = _map_pair()
    got = _run_maps([pair], cost_method=method, cbca_iterations=2, optimization=2)[0]
    np.testing.assert_array_equal(got, PC.pipeline(pair, MD, method, opt="so", pre=_pre(pair)))


def test_maps_adcensusgrad_8_paths():
    pair = _map_pair()
    got = _run_maps([pair], cost_method="ADCensusGrad", cbca_iterations=2, optimization=1, sgm_paths=8)[0]
    np.testing.assert_array_equal(got, PC.pipeline(pair, MD, "ADCensusGrad", paths=8, pre=_pre(pair)))


def test_maps_wta_only():
    pair = _map_pair()
    got = _run_maps([pair], cost_method="grad", cbca_iterations=2, optimization=0)[0]
    np.testing.assert_array_equal(got, PC.pipeline(pair, MD, "grad", opt="wta", pre=_pre(pair)))


def test_fif_on_truncad():
    pair = _map_pair()
    got = _gpu_volumes(pair, MD, cost_method="TruncAD", aggregation="FIF")
    for view, img in ((0, "lbgr"), (1, "rbgr")):
        want = pyref_fif.fif(_want_volume(pair, MD, "TruncAD", view), pair[img])
        np.testing.assert_array_equal(bits(got[view]), bits(want), err_msg=f"view {view}")


def test_bf_on_adgrad():
    """BF after a gradient-bearing measure (no exactness proof: SGM / WTA take the float minima)."""
    pair = _map_pair()
    got = _gpu_volumes(pair, MD, cost_method="adGrad", aggregation="BF")
    vols = [pyref_box.box_filter(_want_volume(pair, MD, "adGrad", view)) for view in (0, 1)]
    for view in (0, 1):
        np.testing.assert_array_equal(bits(got[view]), bits(vols[view]), err_msg=f"view {view}")
    gotmap = _run_maps([pair], cost_method="adGrad", aggregation="BF", optimization=1, sgm_paths=4)[0]
    want = pyref.wta(pyref.sgm(pyref.solve_all(vols[0]), pair["lbgr"], paths=4))
    np.testing.assert_array_equal(gotmap, want)


def test_gf_on_bt(oracle):
    pair = _map_pair()
    mode = _capi.default_params(15, 32, 32).gf_mode
    cfg = oracle.config(MH, MW, MD - 1, gf_mode=mode)
    got = _gpu_volumes(pair, MD, cost_method="BT", aggregation="GF")
    for view, img in ((0, "lbgr"), (1, "rbgr")):
        want = oracle.guided_filter(_want_volume(pair, MD, "BT", view), pair[img], cfg)
        np.testing.assert_array_equal(bits(got[view]), bits(want), err_msg=f"view {view}")


@pytest.mark.parametrize("method", ["BT", "ADCensusGrad"])
def test_sm_run_sub_batches_and_streams(method):
    pairs = [_map_pair(i) for i in range(3)]
    got = _run_maps(pairs, cost_method=method, cbca_iterations=2, optimization=1, sgm_paths=4, sub_batch=2, num_streams=2)
    for i, pair in enumerate(pairs):
        np.testing.assert_array_equal(got[i], PC.pipeline(pair, MD, method, pre=_pre(pair)), err_msg=f"pair {i}")


# ---- the device expf below its proven range ----------------------------------------------------------

def test_device_expf_is_zero_below_the_underflow_bound(oracle):
    """ADCensusGrad reaches expf(-m) with m <= 163 and expf(-G / 2) with G <= 707.1: every float from the
    first one below -0x1.9fe368p6 (glibc's underflow bound, -103.97) down to -354 gives +0, as libm does."""
    lib = _capi.load()
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(_capi.default_params(15, 8, 8)), 0))
    try:
        first = int(np.float32(float.fromhex("-0x1.9fe368p6")).view(np.uint32)) + 1
        last = int(np.float32(-354.0).view(np.uint32))
        assert 14_000_000 < last - first < 16_000_000
        chunk = 1 << 23
        out = np.empty(chunk, np.float32)
        b = first
        while b <= last:
            n = min(chunk, last - b + 1)
            out[:] = 1
            _capi.check(lib, ctx, lib.sm_expf_device_range(ctx, b, n, _capi.ptr(out)))
            assert not out[:n].view(np.uint32).any(), hex(b)
            assert not oracle.expf_range(b, n).view(np.uint32).any()
            b += n
    finally:
        lib.sm_destroy(ctx)
