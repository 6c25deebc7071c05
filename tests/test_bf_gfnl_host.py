"""Aggregations "BF" and "GFNL" without a GPU: the numpy twin of cv::boxFilter (tests/pyref_box.py)
and the C ABI's validation, setters and facades.

The twin is OpenCV's normalised box filter with BORDER_REFLECT_101 and the default anchor k / 2
(RowSum<float, double> + ColumnSum<double, float>, literal running sums).  Its inputs here are
integers or multiples of 2^-10, so every double sum is exact and the running sums must equal a
direct, explicitly padded sum.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyref_box as B
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the twin --------------------------------------------------------------------------------

@pytest.mark.parametrize("kv,ku", [(12, 12), (19, 19), (1, 1), (2, 3), (32, 32)])
def test_constant_plane_stays_constant(kv, ku):
    a = np.full((17, 20), 37.0, np.float32)   # 37 k / k = 37 needs k 37 exact and the scale's rounding to cancel
    out = B.box_filter(a, kv, ku)
    want = (np.float64(37.0 * kv * ku) * (1.0 / (kv * ku))).astype(np.float32)
    assert (out == want).all() and abs(float(want) - 37.0) < 1e-5


def test_unit_impulse_shows_the_asymmetric_window():
    """A 12 x 12 window covers the offsets -6 .. +5 of the output pixel, so the impulse at (y, x)
    reaches the outputs y - 5 .. y + 6, x - 5 .. x + 6 (and no others), each 1 / 144 exactly."""
    H, W, y, x = 30, 33, 14, 16
    a = np.zeros((H, W), np.float32)
    a[y, x] = 1.0
    out = B.box_filter(a)
    want = np.zeros((H, W), np.float32)
    want[y - 5:y + 7, x - 5:x + 7] = np.float32(1.0 / 144)
    np.testing.assert_array_equal(bits(out), bits(want))
    assert out[y + 6, x + 6] != 0 and out[y - 6, x] == 0 and out[y, x - 6] == 0


@pytest.mark.parametrize("H,W,kv,ku", [(7, 7, 12, 12), (10, 12, 19, 19), (24, 30, 12, 12), (24, 30, 11, 12),
                                       (24, 30, 12, 11), (24, 30, 2, 3), (24, 30, 32, 32), (17, 40, 32, 5)])
def test_borders_agree_with_a_padded_direct_sum(H, W, kv, ku):
    rng = np.random.default_rng(H * 1000 + W + kv * 7 + ku)
    a = (rng.integers(0, 2048, (H, W, 3)) / 1024.0).astype(np.float32)   # multiples of 2^-10: exact sums
    np.testing.assert_array_equal(bits(B.box_filter(a, kv, ku)), bits(B.box_filter_direct(a, kv, ku)))


def test_padding_is_reflect_101():
    """Row 0 of a 3 x 1 window on a column ramp reads rows 1, 0, 1 (not 0, 0, 1)."""
    a = np.arange(5, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)
    out = B.box_filter(a, 3, 1)
    assert out[0, 0] == np.float32((1 + 0 + 1) * (1.0 / 3)) and out[4, 0] == np.float32((3 + 4 + 3) * (1.0 / 3))
    assert [B.reflect101(p, 7) for p in (-6, -1, 0, 6, 7, 11)] == [6, 1, 0, 6, 5, 1]


def test_one_by_one_window_is_the_identity():
    rng = np.random.default_rng(5)
    a = rng.random((9, 11, 4)).astype(np.float32)
    np.testing.assert_array_equal(bits(B.box_filter(a, 1, 1)), bits(a))


def test_gfnl_blend_twin():
    gray = np.zeros((24, 30), np.uint8)
    gray[:, 15:] = (np.arange(24)[:, None] * 37 + np.arange(15)[None] * 91) % 256   # flat left, busy right
    nl = np.full((24, 30, 2), 0.75, np.float32)
    gf = np.full((24, 30, 2), -0.25, np.float32)
    vol, mask = B.gfnl(nl, gf, gray)
    assert mask[:, :5].all() and not mask[:, 25:].any()
    assert (vol[mask == 1] == np.float32(0.75)).all() and (vol[mask == 0] == np.float32(0.25)).all()
    assert B.gfnl(nl, gf, gray, 1e30)[1].all() and not B.gfnl(nl, gf, gray, -1e30)[1].any()


# ---- the C ABI (no device needed: validation and the setters are host code) --------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("name,value", [("BF", 9), ("GFNL", 10)])
def test_enumerators_9_and_10_pass_validation(name, value):
    assert _capi.AGGREGATIONS[name] == value
    for opt in ((0, 1, 2) if name == "BF" else (0, 1)):
        lib, ctx, st = _create(_capi.default_params(15, 32, 32, aggregation=value, optimization=opt))
        try:
            assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("value", [4, 6, 8, -1, 1000])
def test_reserved_and_unknown_enumerators_are_rejected(value):
    assert value not in _capi.AGGREGATIONS.values()
    lib, ctx, st = _create(_capi.default_params(15, 32, 32, aggregation=value))
    try:
        assert st == _capi.SM_EINVAL and b"aggregation" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


@pytest.mark.parametrize("over,msg", [
    (dict(aggregation=9, rows=6, cols=40), b"BF"),
    (dict(aggregation=9, rows=40, cols=6), b"BF"),
    (dict(aggregation=10, rows=9, cols=40), b"GFNL"),
    (dict(aggregation=10, rows=40, cols=9), b"GFNL"),
    (dict(aggregation=10, optimization=2), b"GFNL"),
    (dict(aggregation=10, gf_eps=0.0), b"GFNL"),
    (dict(aggregation=10, nl_sigma=0.0), b"GFNL"),
    (dict(aggregation=10, gf_mode=2), b"GFNL"),
    (dict(aggregation=10, gf_mode=1, rows=18, cols=40), b"GFNL"),
    # BF's costs stay >= +0 only while its sums are exact: "so" with an AD truncation off the 2^-25 grid
    (dict(aggregation=9, optimization=2, cost_method=3, ad_trunc_ad=1e-30), b"BF"),
])
def test_create_rejections_name_the_aggregation(over, msg):
    over = dict(over)
    rows, cols = over.pop("rows", 32), over.pop("cols", 32)
    lib, ctx, st = _create(_capi.default_params(15, rows, cols, **over))
    try:
        assert st == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_minimum_sizes_pass_validation():
    for over in (dict(aggregation=9, rows=7, cols=7), dict(aggregation=10, rows=10, cols=10),
                 dict(aggregation=9, optimization=2, cost_method=3)):
        over = dict(over)
        rows, cols = over.pop("rows", 32), over.pop("cols", 32)
        lib, ctx, st = _create(_capi.default_params(3, rows, cols, **over))
        try:
            assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("args,msg", [((0, 12), b"ksize_v"), ((33, 12), b"ksize_v"), ((12, 0), b"ksize_u"),
                                      ((12, 33), b"ksize_u"), ((-3, 12), b"ksize_v")])
def test_bf_config_messages(args, msg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="BF"))
    try:
        assert lib.sm_bf_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
        for good in ((12, 12), (1, 1), (32, 32), (2, 3)):
            assert lib.sm_bf_config(ctx, *good) == _capi.SM_OK
    finally:
        lib.sm_destroy(ctx)


def test_bf_config_rejects_a_window_the_image_cannot_reflect():
    lib, ctx, _ = _create(_capi.default_params(3, 7, 9, aggregation="BF"))
    try:
        assert lib.sm_bf_config(ctx, 12, 16) == _capi.SM_OK          # 7 >= 6 + 1, 9 >= 8 + 1
        assert lib.sm_bf_config(ctx, 14, 12) == _capi.SM_EINVAL and b"ksize_v" in lib.sm_last_error(ctx)
        assert lib.sm_bf_config(ctx, 12, 18) == _capi.SM_EINVAL and b"ksize_u" in lib.sm_last_error(ctx)
        assert lib.sm_bf_config(ctx, 32, 32) == _capi.SM_EINVAL
    finally:
        lib.sm_destroy(ctx)


def test_gfnl_config_messages():
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="GFNL"))
    try:
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert lib.sm_gfnl_config(ctx, bad) == _capi.SM_EINVAL
            assert b"var_thresh" in lib.sm_last_error(ctx)
        for good in (400.0, 0.0, -1e30, 1e30):
            assert lib.sm_gfnl_config(ctx, good) == _capi.SM_OK
    finally:
        lib.sm_destroy(ctx)


def test_setters_need_their_own_aggregation():
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="GF"))
    try:
        assert lib.sm_bf_config(ctx, 12, 12) == _capi.SM_EINVAL and b"aggregation" in lib.sm_last_error(ctx)
        assert lib.sm_gfnl_config(ctx, 400.0) == _capi.SM_EINVAL and b"aggregation" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="BF"))
    try:
        assert lib.sm_gfnl_config(ctx, 400.0) == _capi.SM_EINVAL
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_bf_config(None, 12, 12) == _capi.SM_EINVAL
    assert lib.sm_gfnl_config(None, 400.0) == _capi.SM_EINVAL


def test_sm_params_unchanged():
    """Neither aggregation adds a field: the struct ends as before and keeps its size."""
    names = [n for n, _ in _capi.sm_params._fields_]
    assert names[-4:] == ["fuse_cost_scan", "fif_mode", "fif_eps", "fif_pn"]
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


def test_python_facade_accepts_both():
    prm = StereoMatching.Parameters(15, 32, 32)
    assert prm.to_c("censusGrad", "BF", "sgm").aggregation == 9
    assert prm.to_c("censusGrad", "BF", "so").aggregation == 9
    assert prm.to_c("censusGrad", "GFNL", "sgm").aggregation == 10
    assert prm.to_c("censusGrad", "GFNL", "sgm", my_guide=True).gf_mode == 1
    assert (StereoMatching.BF_KSIZE_V, StereoMatching.BF_KSIZE_U, StereoMatching.GFNL_VAR_THRESH) == (12, 12, 400.0)
    assert callable(StereoBatch.bf_config) and callable(StereoBatch.gfnl_config)


def test_cpp_facade_and_header_accept_both():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    assert re.search(r'aggregation == "BF" \? SM_AGG_BF', src) and "sm_bf_config(ctx_" in src
    assert re.search(r'aggregation == "GFNL" \? SM_AGG_GFNL', src) and "sm_gfnl_config(ctx_" in src
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    assert re.search(r"SM_AGG_BF = 9\b", hdr) and re.search(r"SM_AGG_GFNL = 10\b", hdr)
    for fn in ("sm_bf_config", "sm_gfnl_config", "sm_get_gfnl_mask"):
        assert re.search(r"SM_API sm_status " + fn + r"\(", hdr)
