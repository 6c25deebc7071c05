"""The cost measures "SD", "BT", "grad", "TruncAD", "adGrad" and "ADCensusGrad" without a GPU: the
numpy twin (tests/pyref_cost.py) against the parts that already have a second implementation and
against hand cases, then the C ABI's validation and the facades' string tables.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import pyref
import pyref_cost as PC
from mystereomatching_amd import StereoMatching, _capi
from mystereomatching_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lbgr", "rbgr", "lgray", "rgray")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _pair(H=9, W=14, D=6, idx=930):
    pair = S.make_pair(H, W, D, idx)
    pair = {k: pair[k] for k in KEYS}
    for a in pair.values():
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def _arms(view):
    return pyref.arms(_pair()["rbgr" if view else "lbgr"])


# ---- the twin against second implementations -------------------------------------------------

@pytest.mark.parametrize("view", [0, 1])
def test_grad_equals_pyref_grad_cost(view):
    p, D = _pair(), 6
    gx0, gy0 = pyref.grads(p["lgray"])
    gx1, gy1 = pyref.grads(p["rgray"])
    want = pyref.grad_cost(gx0, gx1, gy0, gy1, _arms(view), D, view=view)
    np.testing.assert_array_equal(bits(PC.cost_volume(p, D, "grad", view, _arms(view))), bits(want))


@pytest.mark.parametrize("view", [0, 1])
def test_adgrad_parts(view):
    p, D = _pair(), 6
    A, G = PC.ad_grad_parts(p, D, view, _arms(view))
    np.testing.assert_array_equal(bits(A), bits(pyref.ad_cost(p["lbgr"], p["rbgr"], D, 7, view=view)))
    assert A.max() == 7 and G.max() == f32(np.sqrt(8.0))
    v = PC.ad_grad_cost(p, D, view, _arms(view))
    assert (v >= 0).all() and not np.signbit(v).any()


@pytest.mark.parametrize("view", [0, 1])
def test_adcensusgrad_parts_equal_the_oracle(view):
    """A and C are the oracle's AD (truncation 255) and Census volumes bit for bit.  The oracle has no
    gradient-only volume: G is pinned through its censusGrad volume with lamG = 512, where
    expf(-G / 512) moves with G over all of [0, 707.1], and equals pyref.grad_cost besides."""
    from oracle import oracle as O
    p, D = _pair(), 6
    H, W = p["lgray"].shape
    A, Cn, G = PC.ad_census_grad_parts(p, D, view, _arms(view))
    np.testing.assert_array_equal(bits(A), bits(O.cost_volume(p, O.config(H, W, D - 1, cost="AD", ad_trunc_ad=255.0), view=view)))
    np.testing.assert_array_equal(bits(Cn), bits(O.cost_volume(p, O.config(H, W, D - 1, cost="Census"), view=view)))
    fused = O.cost_volume(p, O.config(H, W, D - 1, cost="censusGrad", lam_g=512.0), view=view)
    np.testing.assert_array_equal(bits(pyref.fuse(Cn, G, 13, 512)), bits(fused))
    gx0, gy0 = pyref.grads(p["lgray"])
    gx1, gy1 = pyref.grads(p["rgray"])
    np.testing.assert_array_equal(bits(G), bits(pyref.grad_cost(gx0, gx1, gy0, gy1, _arms(view), D, view=view)))


@pytest.mark.parametrize("view", [0, 1])
def test_census_twin_equals_pyref_census_cost(view):
    p, D = _pair(), 6
    got = PC.census_cost(PC.census_bits(p["lgray"]), PC.census_bits(p["rgray"]), D, view)
    want = pyref.census_cost(pyref.census(p["lgray"]), pyref.census(p["rgray"]), D, view=view)
    np.testing.assert_array_equal(bits(got), bits(want))


# ---- hand cases --------------------------------------------------------------------------------

def test_bt_hand_case():
    L = np.array([[10, 20, 90]], np.uint8)
    R = np.array([[12, 30, 40]], np.uint8)
    lo, hi = PC.nei_min_max(L)
    assert list(zip(lo[0], hi[0])) == [(10, 15), (15, 55), (55, 90)]
    lo, hi = PC.nei_min_max(R)
    assert list(zip(lo[0], hi[0])) == [(12, 21), (21, 35), (35, 40)]
    V = PC.bt_cost(L, R, 2, view=0)
    # u = 2, d = 0: L 90 against R(2)'s range (35, 40) is 50, R 40 against L(2)'s (55, 90) is 15
    assert V[0, 2, 0] == 15
    # u = 2, d = 1: L 90 against (21, 35) is 55, R 30 against (55, 90) is 25: truncated at 20
    assert V[0, 2, 1] == 20
    assert V[0, 0, 1] == 20          # u - d < 0
    assert V[0, 0, 0] == 0           # L 10 lies below (12, 21) by 2, but R 12 lies inside (10, 15)
    assert V[0, 1, 1] == 0           # L 20 inside (12, 21); R 12 lies below (15, 55) by 3: min(0, 3)
    # the right view pairs left u + d with right u: the same pairs, indexed by the right pixel
    V1 = PC.bt_cost(L, R, 2, view=1)
    assert V1[0, 2, 1] == 20 and V1[0, 1, 1] == V[0, 2, 1] and V1[0, 0, 1] == V[0, 1, 1]


def test_bt_two_columns():
    """W = 2: both columns are image edges, (lo, hi) = (min, max) of I and the one half-way value."""
    L = np.array([[10, 31]], np.uint8)
    R = np.array([[40, 4]], np.uint8)
    lo, hi = PC.nei_min_max(L)
    assert list(zip(lo[0], hi[0])) == [(10, 20.5), (20.5, 31)]
    lo, hi = PC.nei_min_max(R)
    assert list(zip(lo[0], hi[0])) == [(22, 40), (4, 22)]
    V = PC.bt_cost(L, R, 2)
    assert V[0, 0, 0] == 12          # min(22 - 10, 40 - 20.5)
    assert V[0, 1, 0] == 9           # min(31 - 22, 20.5 - 4)
    assert V[0, 1, 1] == 0           # L 31 inside (22, 40)
    assert V[0, 0, 1] == 20


def _px(*rows):
    return np.array(rows, np.uint8)[None]      # one row of BGR pixels


def test_sd_truncad_hand_cases():
    L, R = _px((10, 20, 30), (0, 0, 0)), _px((12, 19, 30), (255, 255, 255))
    sd = PC.sd_cost(L, R, 2, 20)
    assert sd[0, 0, 0] == f32(5) / f32(3)                 # (4 + 1 + 0) / 3
    assert sd[0, 1, 0] == 20 and sd[0, 0, 1] == 20        # 195075 / 3 truncated; out of range
    assert sd[0, 1, 1] == 20                              # L(1) = 0 against R(0): (144 + 361 + 900) / 3
    assert PC.sd_cost(L, R, 2, 1e9)[0, 1, 0] == f32(65025)
    ta = PC.trunc_ad_cost(L, R, 2)
    assert ta[0, 0, 0] == 3 and ta[0, 1, 0] == 60 and ta[0, 0, 1] == 60 and ta[0, 1, 1] == 60
    assert PC.trunc_ad_cost(L, _px((12, 19, 30), (20, 20, 19)), 2)[0, 1, 0] == 59


def _flat_gray(H, W, fill):
    return np.full((H, W), fill, np.uint8)


def test_grad_hand_case():
    """One bright column in the left image: gx = 0.5 (I(u + 1) - I(u - 1)); first without the arm weights."""
    L, R = _flat_gray(3, 5, 10), _flat_gray(3, 5, 10)
    L[:, 2] = 50
    arm = np.zeros((3, 5, 4), np.uint16)
    G = PC.grad_cost(L, R, arm, 2, trunc=500, adaptive=False)
    assert G[1, 1, 0] == 20 and G[1, 3, 0] == 20 and G[1, 2, 0] == 0 and G[1, 0, 0] == 0
    assert G[1, 0, 1] == f32(np.sqrt(500000.0)) == f32(707.1068)
    assert PC.grad_cost(L, R, arm, 2, trunc=2, adaptive=False)[1, 1, 0] == 2
    # arms 0 count as 1 (cpp:421-424): a = 1 / 2, so the adaptive value is half the sum
    assert PC.grad_cost(L, R, arm, 2, trunc=500)[1, 1, 0] == 10


def test_adgrad_hand_case():
    A, G = np.array([[[7.0, 3.0]]], f32), np.array([[[f32(np.sqrt(8.0)), 1.5]]], f32)
    want0 = f32(f32(f32(7) * f32(0.11)) + f32(f32(np.sqrt(8.0)) * f32(1 - 0.11)))
    want1 = f32(f32(f32(3) * f32(0.11)) + f32(f32(1.5) * f32(1 - 0.11)))
    got = ((A * PC.W_AD).astype(f32) + (G * PC.W_GRAD).astype(f32)).astype(f32)
    assert got[0, 0, 0] == want0 and got[0, 0, 1] == want1


def test_adcensusgrad_hand_case():
    A, Cn, G = (np.array([[[x]]], f32) for x in (0.0, 0.0, 0.0))
    assert bits(PC.ad_census_grad_blend(A, Cn, G))[0, 0, 0] == 0          # +0, not -0
    A, Cn, G = (np.array([[[x]]], f32) for x in (255.0, 71.0, np.sqrt(500000.0)))
    assert PC.ad_census_grad_blend(A, Cn, G)[0, 0, 0] == f32(0.7 * 1.0 + 0.3 * 1.0)   # both exponentials underflow
    A, Cn, G = (np.array([[[x]]], f32) for x in (1.0, 2.0, 3.0))
    e0 = f32(1) - f32(pyref.expf(f32(-1.5)))
    e1 = f32(1) - f32(pyref.expf(f32(-1.5)))
    assert PC.ad_census_grad_blend(A, Cn, G)[0, 0, 0] == f32(0.7 * float(e0) + 0.3 * float(e1))


def test_every_measure_is_nonnegative_and_never_minus_zero():
    p, D = _pair(), 6
    for m in PC.METHODS:
        for view in (0, 1):
            v = PC.cost_volume(p, D, m, view, _arms(view))
            assert (v >= 0).all() and not np.signbit(v).any() and np.isfinite(v).all(), m


# ---- the C ABI (no device needed: validation is host code) ---------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("name,value", sorted(PC.METHODS.items(), key=lambda kv: kv[1]))
def test_new_cost_methods_pass_validation(name, value):
    assert value in (4, 5, 6, 8, 9, 10)
    for agg in (0, 1):
        lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method=value, aggregation=agg))
        try:
            assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("value", [7, 11, -1])
def test_reserved_and_unknown_cost_methods_are_rejected(value):
    lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method=value))
    try:
        assert st == _capi.SM_EINVAL and b"cost_method" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


@pytest.mark.parametrize("name", ["grad", "adGrad", "ADCensusGrad"])
def test_bf_with_so_names_the_gradient_bearing_method(name):
    lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method=name, aggregation="BF", optimization="so"))
    try:
        msg = lib.sm_last_error(ctx)
        assert st == _capi.SM_EINVAL and b"cost_method" in msg and name.encode() in msg, msg
    finally:
        lib.sm_destroy(ctx)
    # sgm and WTA run (through the float minima)
    for opt in (1, 0):   # sgm, WTA
        lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method=name, aggregation="BF", optimization=opt))
        try:
            assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("name", ["BT", "TruncAD", "SD"])
def test_bf_with_so_accepts_the_exact_methods(name):
    lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method=name, aggregation="BF", optimization="so"))
    try:
        assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_bf_with_so_and_sd_follows_ads_truncation_rule():
    lib, ctx, st = _create(_capi.default_params(15, 32, 32, cost_method="SD", aggregation="BF", optimization="so",
                                                ad_trunc_ad=1e-30))
    try:
        assert st == _capi.SM_EINVAL and b"BF" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_sm_params_unchanged():
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


# ---- facades -------------------------------------------------------------------------------------

def test_string_tables():
    want = {"censusGrad": 0, "Census": 1, "ADCensus": 2, "AD": 3, "SD": 4, "BT": 5, "grad": 6, "TruncAD": 8, "adGrad": 9,
            "ADCensusGrad": 10}
    assert _capi.COST_METHODS == want
    prm = StereoMatching.Parameters(15, 32, 32)
    for name, value in want.items():
        assert prm.to_c(name, "CBCA", "sgm").cost_method == value
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for name, enum, value in [("SD", "SM_COST_SD", 4), ("BT", "SM_COST_BT", 5), ("grad", "SM_COST_GRAD", 6),
                              ("TruncAD", "SM_COST_TRUNC_AD", 8), ("adGrad", "SM_COST_AD_GRAD", 9),
                              ("ADCensusGrad", "SM_COST_AD_CENSUS_GRAD", 10)]:
        assert re.search(enum + r" = %d\b" % value, hdr), enum
        assert re.search(r'costcalculation == "%s"\s*\? %s\b' % (name, enum), src), name


def test_zncc_is_refused():
    with pytest.raises((KeyError, ValueError), match="ZNCC"):
        StereoMatching.Parameters(15, 32, 32).to_c("ZNCC", "CBCA", "sgm")
    with pytest.raises((KeyError, ValueError), match="ZNCC"):
        _capi.default_params(15, 32, 32, cost_method="ZNCC")
    assert "ZNCC" not in _capi.COST_METHODS and 7 not in _capi.COST_METHODS.values()
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    assert '"ZNCC"' not in src.split("p.cost_method = costcalculation")[1].split("unsupported costcalculation")[0]
