"""Host-side checks of refine()'s peak-ratio check, background fill and sub-pixel map (no GPU): known answers
of the restatement tests/pyref_refine_ext.py, the BGIpol recurrence against the literal walk,
sm_refine_ext_config's argument validation, and the facades' new fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyref_refine_ext as R
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
OK_ARGS = (1, 0.1, -64, 1, 1000, 1, 0)


# ---- calPKR ------------------------------------------------------------------------------------------

def test_two_minima_known_answers():
    assert R.two_minima([5, 3]) == (3, 5)                       # two elements
    assert R.two_minima([3, 5]) == (3, 5)
    assert R.two_minima([4, 2, 7, 2, 9]) == (2, 2)              # a duplicated minimum counts twice
    assert R.two_minima([2, 2]) == (2, 2)
    assert R.two_minima([7, 1, 3, 1, 1]) == (1, 1)
    assert R.two_minima([-1, 6, -3, 0]) == (-3, -1)
    assert R.two_minima([9, 8, 7, 6]) == (6, 7)
    # the masked slot is the FIRST strict minimum: the second search still sees the later duplicate
    assert R.two_minima([3, 1, 1]) == (1, 1) and R.two_minima([1, 3, 1]) == (1, 1)
    with pytest.raises(ValueError):
        R.two_minima([4])                                       # D == 1: slot -1 in the reference


def test_pkr_predicate():
    assert R.pkr_bad(f32(9.5), f32(10))          # 0.05 < 0.1
    assert not R.pkr_bad(f32(8), f32(10))        # 0.2
    assert R.pkr_bad(f32(2), f32(2))             # 0 / 2
    assert not R.pkr_bad(f32(0), f32(0))         # 0 / 0 = NaN compares false: not marked
    assert not R.pkr_bad(f32(-1), f32(0))        # 1 / 0 = +inf
    assert not R.pkr_bad(f32(0), f32(3))         # 1
    # float throughout: 0.9 and 1 give fl(fl(1 - 0.9f) / 1) = 0.100000024 > 0.1f, where exact arithmetic gives 0.1 = the bound
    assert not R.pkr_bad(f32(0.9), f32(1))
    assert R.pkr_bad(f32(-10), f32(-9.5))        # negative costs (GF): (0.5) / (-9.5) < 0.1
    vm = np.array([[[5, 3], [2, 2], [0, 0], [0, 7]]], f32)
    assert R.cal_pkr(vm).tolist() == [[0, 1, 0, 0]]
    assert R.cal_pkr(vm, f32(0.5)).tolist() == [[1, 1, 0, 0]]
    dp = np.array([[3, -1, 4, 0]], np.int16)
    assert R.sign_dp(dp, np.array([[1, 1, 0, 1]], np.uint8)).tolist() == [[-64, -1, 4, -64]]


# ---- BGIpol ------------------------------------------------------------------------------------------

def _brute(row, depth):
    """The double search written out: the left candidate is found in the row as filled so far."""
    row = list(row)
    for u in range(len(row)):
        if row[u] >= 0:
            continue
        right = next((row[u + d] for d in range(1, depth + 1) if u + d < len(row) and row[u + d] >= 0), None)
        left = next((row[u - d] for d in range(1, depth + 1) if u - d >= 0 and row[u - d] >= 0), None)
        found = [x for x in (right, left) if x is not None]
        if found:
            row[u] = min(found)
    return row


def test_bg_ipol_known_answers():
    m = lambda *r: np.array([r], np.int16)
    assert R.bg_ipol(m(-1, -1, -32, -64)).tolist() == [[-1, -1, -32, -64]]          # a row of holes keeps its values
    assert R.bg_ipol(m(-1, -1, 5, 7, -1, -1)).tolist() == [[5, 5, 5, 7, 7, 7]]      # holes at both borders
    assert R.bg_ipol(m(9, -1, -1, 4)).tolist() == [[9, 4, 4, 4]]                    # the smaller of the two
    assert R.bg_ipol(m(2, -1, -1, 8)).tolist() == [[2, 2, 2, 8]]                    # ... carried on by the in-place walk
    assert R.bg_ipol(m(-1, -1, -1, -1, 6), 2).tolist() == [[-1, -1, 6, 6, 6]]       # depth 2 from the right
    assert R.bg_ipol(m(6, -1, -1, -1, -1), 1).tolist() == [[6, 6, 6, 6, 6]]         # depth 1 from the left reaches on
    assert R.bg_ipol(m(3, -1, -1), 0).tolist() == [[3, -1, -1]]                     # depth 0 fills nothing
    assert R.bg_ipol(m(-1), 5).tolist() == [[-1]] and R.bg_ipol(m(4), 5).tolist() == [[4]]
    # -1 in the reference's vec means "none": found values are >= 0, 0 among them
    assert R.bg_ipol(m(-5, 0, -5)).tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_bg_ipol_against_brute_force(depth):
    rng = np.random.default_rng(depth)
    for W in (1, 2, 5, 17, 40):
        for rate in (0.1, 0.6, 0.9, 1.0):
            dp = rng.integers(0, 30, (6, W)).astype(np.int16)
            dp[rng.random((6, W)) < rate] = -1
            dp[rng.random((6, W)) < 0.1] = -64
            want = np.array([_brute(r, depth) for r in dp.tolist()], np.int16)
            np.testing.assert_array_equal(R.bg_ipol(dp, depth), want)


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 7, 64, 1000])
def test_bg_ipol_recurrence_equals_the_walk(depth):
    """The scan form the kernel uses against the literal in-place walk."""
    rng = np.random.default_rng(100 + depth)
    for W in (1, 2, 3, 63, 64, 65, 130, 200):
        for rate in (0.1, 0.6, 0.95, 1.0):
            dp = rng.integers(0, 90, (5, W)).astype(np.int16)
            holes = rng.random((5, W)) < rate
            dp[holes] = rng.choice(np.array([-1, -32, -64], np.int16), size=int(holes.sum()))
            np.testing.assert_array_equal(R.bg_ipol_scan(dp, depth), R.bg_ipol(dp, depth), err_msg=f"W={W} rate={rate}")


def _wave_bg_r(src, depth):
    """k_bg_r lane by lane: 64-column chunks right to left, a ballot of the valid lanes, each lane's nearest set bit
    above it, and the carried (position, value) of the nearest valid pixel right of the chunk."""
    W = len(src)
    r = [None] * W
    cpos, cval = -1, 0
    for c0 in range((W - 1) // 64 * 64, -1, -64):
        v = [int(src[c0 + l]) if c0 + l < W else -1 for l in range(64)]
        m = sum(1 << l for l in range(64) if v[l] >= 0)
        for lane in range(64):
            above = 0 if lane == 63 else m & ((~0 << (lane + 1)) & (2 ** 64 - 1))
            j = (above & -above).bit_length() - 1 if above else 0
            pos, val = (c0 + j, v[j]) if above else (cpos, cval)
            if c0 + lane < W:
                r[c0 + lane] = val if (pos >= 0 and pos - (c0 + lane) <= depth) else -1
        if m:
            j0 = (m & -m).bit_length() - 1
            cpos, cval = c0 + j0, v[j0]
    return r


def _wave_bg_scan(src, r):
    """k_bg_scan lane by lane: per chunk a 6-step inclusive scan of (constant flag, k) maps, then the carry."""
    NONE = 0x7fffffff
    W = len(src)
    out = list(r)
    carry = NONE
    for c0 in range(0, W, 64):
        old = [int(src[c0 + l]) if c0 + l < W else -1 for l in range(64)]
        ru = [int(r[c0 + l]) if c0 + l < W else -1 for l in range(64)]
        cf = [1 if o >= 0 else 0 for o in old]
        k = [o if o >= 0 else (x if x >= 0 else NONE) for o, x in zip(old, ru)]
        s = 1
        while s < 64:
            pc, pk = list(cf), list(k)   # the values before this step (the shuffles read them)
            for l in range(s, 64):
                k[l] = k[l] if cf[l] else min(k[l], pk[l - s])
                cf[l] |= pc[l - s]
            s <<= 1
        y = [k[l] if cf[l] else min(k[l], carry) for l in range(64)]
        for l in range(64):
            if c0 + l < W:
                out[c0 + l] = old[l] if y[l] == NONE else y[l]
        carry = y[63]
    return out


@pytest.mark.parametrize("depth", [1, 3, 70, 1000])
def test_bg_ipol_wave_form_equals_the_walk(depth):
    """The chunked form of sm_refine_ext.hip's two BGIpol kernels, restated lane by lane."""
    rng = np.random.default_rng(200 + depth)
    for W in (2, 63, 64, 65, 130, 200, 450):
        for rate in (0.1, 0.6, 0.97, 1.0):
            d = rng.integers(0, 90, W).astype(np.int16)
            h = rng.random(W) < rate
            d[h] = rng.choice(np.array([-1, -32, -64], np.int16), size=int(h.sum()))
            want = R.bg_ipol(d[None], depth)[0].tolist()
            assert _wave_bg_scan(d, _wave_bg_r(d, depth)) == want, (W, rate)


# ---- subpixelEnhancement ---------------------------------------------------------------------------------

def test_subpixel_known_answers():
    c = [f32(x) for x in (9, 4, 2, 5, 9)]                 # D = 5
    for mode in (R.SE_REFERENCE, R.SE_FLOAT):
        assert R.subpixel_px(0, c, mode) == 0             # d = 0
        assert R.subpixel_px(4, c, mode) == 4             # d = D - 1
        assert R.subpixel_px(-1, c, mode) == -1 and R.subpixel_px(-64, c, mode) == -64   # holes keep their value
        assert R.subpixel_px(2, [1, 3, 3, 3, 1], mode) == 2     # denom == 0
        assert R.subpixel_px(2, [0, 4, 2, 0, 0], mode) == 2     # cp + cm - 2 c == 0 with unequal neighbours
    # d = 2: cp = 5, cm = 4, c = 2: denom = 2 * (9 - 4) = 10, diff = 0.1
    assert R.subpixel_px(2, c, R.SE_FLOAT) == f32(2) - f32(f32(1) / f32(10))
    assert R.subpixel_px(2, c, R.SE_REFERENCE) == 1       # diff > 0: (short)1.9 = 1 = d - 1
    # d = 1: cp = 2, cm = 9, c = 4: denom = 2 * (11 - 8) = 6, diff = -7 / 6 <= -1: not applied
    assert R.subpixel_px(1, c, R.SE_FLOAT) == 1
    # diff < 0: d - diff in (d, d + 1) truncates to d
    neg =[f32(x) for x in (0, 6, 2, 4, 0)]               # d = 2: cp = 4, cm = 6: denom = 2 * (10 - 4) = 12, diff = -1 / 6
    assert R.subpixel_px(2, neg, R.SE_FLOAT) == f32(2) - f32(f32(-2) / f32(12))
    assert R.subpixel_px(2, neg, R.SE_REFERENCE) == 2
    # diff just inside +-1: neighbours (0, 4) around c = 1 - 2^-23 give denom = 2 * (4 - (2 - 2^-22)) = 4 + 2^-21 and
    # |diff| = fl(4 / (4 + 2^-21)), a few ulp below 1
    cc = f32(1 - 2.0 ** -23)
    for cm, cp in ((0, 4), (4, 0)):
        diff = f32(f32(f32(cp) - f32(cm)) / f32(4 + 2.0 ** -21))
        assert -1 < diff < 1 and abs(diff) > 0.999999
        want = f32(f32(7) - diff)
        costs = [0] * 6 + [cm, cc, cp, 0]
        # (fl(7 - diff) rounds to the integer 6 resp. 8 here: the float subtraction is part of the reference's value)
        assert R.subpixel_px(7, costs, R.SE_FLOAT) == want and want == (6 if diff > 0 else 8)
        assert R.subpixel_px(7, costs, R.SE_REFERENCE) == f32(int(want))
    # exactly +-1 is outside: c = 0, (cm, cp) = (1, -3) gives denom = -4 = cp - cm, and mirrored
    for cm, cp in ((1, -3), (-3, 1)):
        for mode in (R.SE_REFERENCE, R.SE_FLOAT):
            assert R.subpixel_px(1, [f32(cm), f32(0), f32(cp)], mode) == 1


def test_subpixel_reference_round_trip_is_truncation():
    """`disp -= diff` on a short: the value is trunc(fl(d - diff)), which is d - 1 for most diff > 0, d for
    diff <= 0 and for a diff so small that fl(d - diff) == d."""
    rng = np.random.default_rng(5)
    D = 40
    vm = rng.random((8, 12, D)).astype(f32)
    dp = rng.integers(-1, D, (8, 12)).astype(np.int16)
    ref, flt = R.subpixel(dp, vm, R.SE_REFERENCE), R.subpixel(dp, vm, R.SE_FLOAT)
    np.testing.assert_array_equal(ref, np.trunc(flt))
    moved = flt != dp
    assert moved.any() and (ref[flt < dp] == dp[flt < dp] - 1).all() and (ref[flt > dp] == dp[flt > dp]).all()
    # d = 4 (ulp 2^-22 below it) and a diff near 2^-26: fl(4 - diff) = 4, so the reference form stays d
    c = f32(0)
    cp, cm = f32(0.5), f32(0.5 - 2.0 ** -25)
    diff = f32(f32(cp - cm) / f32(2 * f32(f32(cp + cm) - 2 * c)))
    assert 0 < diff < 2.0 ** -25 and f32(f32(4) - diff) == 4
    assert R.subpixel_px(4, [0, 0, 0, cm, c, cp, 0], R.SE_REFERENCE) == 4
    assert R.subpixel_px(4, [0, 0, 0, cm, c, cp, 0], R.SE_FLOAT) == 4


def test_median3_f32():
    a = np.arange(12, dtype=f32).reshape(3, 4)
    m = R.median3_f32(a)
    assert m[1, 1] == 5 and m[0, 0] == 1 and m[2, 3] == 10 and m[0, 3] == 3 and m[2, 0] == 8
    one = np.array([[2.5]], f32)
    assert R.median3_f32(one)[0, 0] == f32(2.5)
    spike = np.zeros((5, 5), f32)
    spike[2, 2] = 9
    assert not R.median3_f32(spike).any()


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("args,msg", [
    ((1, float("nan"), -64, 1, 1000, 1, 0), b"pkr_ratio"), ((0, float("inf"), -64, 0, 1000, 0, 0), b"pkr_ratio"),
    ((1, 0.1, 0, 1, 1000, 1, 0), b"disp_pkr"), ((1, 0.1, -32769, 1, 1000, 1, 0), b"disp_pkr"), ((0, 0.1, 5, 0, 1000, 0, 0), b"disp_pkr"),
    ((1, 0.1, -64, 1, -1, 1, 0), b"bg_ipl_depth"), ((1, 0.1, -64, 1, 32768, 1, 0), b"bg_ipl_depth"),
    ((1, 0.1, -64, 1, 1000, 1, 2), b"se_mode"), ((1, 0.1, -64, 1, 1000, 1, -1), b"se_mode"),
])
def test_refine_ext_config_messages(args, msg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, do_refine=1))
    try:
        assert lib.sm_refine_ext_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_refine_ext_config(None, *OK_ARGS) == _capi.SM_EINVAL


def test_refine_ext_config_needs_do_refine():
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32))
    try:
        for args in (OK_ARGS, (0, 0.1, -64, 0, 1000, 0, 0)):
            assert lib.sm_refine_ext_config(ctx, *args) == _capi.SM_EINVAL
            assert b"do_refine" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_refine_ext_config_refuses_one_disparity_and_so():
    lib, ctx, _ = _create(_capi.default_params(0, 32, 32, do_refine=1, aggregation="", optimization=""))
    try:
        assert lib.sm_refine_ext_config(ctx, 1, 0.1, -64, 0, 1000, 0, 0) == _capi.SM_EINVAL
        assert b"do_pkr" in lib.sm_last_error(ctx) and b"num_disparities" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, do_refine=1, optimization="so"))
    try:
        assert lib.sm_refine_ext_config(ctx, 1, 0.1, -64, 0, 1000, 0, 0) == _capi.SM_EINVAL
        assert b"do_pkr" in lib.sm_last_error(ctx) and b"so" in lib.sm_last_error(ctx)
        assert lib.sm_refine_ext_config(ctx, 0, 0.1, -64, 1, 1000, 1, 1) == _capi.SM_EINVAL
        assert b"do_subpixel" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_null_arguments():
    lib = _capi.load()
    assert lib.sm_get_pkr_mask(None, None) == _capi.SM_EINVAL
    assert lib.sm_get_subpixel(None, None) == _capi.SM_EINVAL
    assert lib.sm_download_subpixel(None, 1, None) == _capi.SM_EINVAL


def test_sm_params_unchanged():
    names = [n for n, _ in _capi.sm_params._fields_]
    assert not any(k in n.lower() for n in names for k in ("pkr", "bg_ip", "subpixel", "se_mode"))
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


def test_header_and_ctypes_symbol_tables_agree():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in ("sm_refine_ext_config", "sm_get_pkr_mask", "sm_get_subpixel", "sm_download_subpixel"):
        assert fn in declared and hasattr(lib, fn)
    args = dict((n, a) for n, _, a in _capi.SIGNATURES)["sm_refine_ext_config"]
    assert args[1:] == [C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    assert "SM_SE_REFERENCE = 0" in hdr and "SM_SE_FLOAT = 1" in hdr
    assert (_capi.SE_REFERENCE, _capi.SE_FLOAT) == (0, 1) and _capi.REFINE_EXT_DEFAULTS == (0.1, -64, 1000, 0)
    assert (float(R.RATIO_PKR), R.DISP_PKR, R.BG_IPL_DEPTH) == (float(f32(0.1)), -64, 1000)


# ---- the facades -------------------------------------------------------------------------------------

def test_python_facade_defaults():
    assert (StereoMatching.Do_calPKR, StereoMatching.Do_bgIpol, StereoMatching.Do_subpixelEnhancement,
            StereoMatching.SE_FLOAT) == (False, False, False, False)
    prm = StereoMatching.Parameters(59, 30, 40)
    assert prm.DISP_PKR == -64 and prm.bgIplDepth == 1000
    for fn in ("refine_ext_config", "get_pkr_mask", "download_subpixel"):
        assert callable(getattr(StereoBatch, fn))


def test_switches_leave_sm_params_alone():
    a = StereoMatching.Parameters(59, 30, 40)
    b = StereoMatching.Parameters(59, 30, 40)
    b.DISP_PKR, b.bgIplDepth = -80, 7
    assert bytes(a.to_c("censusGrad", "CBCA", "sgm", do_refine=True)) == bytes(b.to_c("censusGrad", "CBCA", "sgm", do_refine=True))


def test_cpp_facade_source():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("inline static bool Do_calPKR = false;", "inline static bool Do_bgIpol = false;",
                 "inline static bool Do_subpixelEnhancement = false;", "inline static bool SE_FLOAT = false;",
                 "int DISP_PKR = -4 * 16;", "int bgIplDepth = 1000;", "Mat SE;", "Mat PKR_Err_Mask;"):
        assert decl in src, decl
    assert "sm_refine_ext_config(ctx_, Do_calPKR ? 1 : 0, pkr_ratio, param.DISP_PKR, Do_bgIpol ? 1 : 0, param.bgIplDepth," in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("Do_calPKR", "Do_bgIpol", "Do_subpixelEnhancement"):
        assert name in doc, name


def test_refine_ext_facade_check_compiles(tmp_path):
    """tests/cpp/refine_ext_facade_check.cpp builds against the facade and the library (its maps are compared on the
    GPU in tests/test_refine_ext_facade.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "refine_ext_facade_check.cpp"), str(tmp_path / "refine_ext_facade_check"))
