"""Aggregation "FIF" without a GPU: the numpy twin (tests/pyref_fif.py) on hand-checkable cases, the
C ABI's new fields, their defaults and validation, and the Python facade's selector.

FIF_Improve: stereoMatching.cpp:4707-4890 (what costCalculate calls, cpp:1010-1012); FIF, the
plain form: cpp:4541-4705.  PARITY UNPINNED (the guide comes from OpenCV's convertTo).
"""
import ctypes as C

import numpy as np
import pytest

import pyref_fif as F
from mystereomatching_amd import StereoMatching, _capi

f32 = np.float32
BIG = np.finfo(f32).max


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _loops(vm, wh, wv, plain, pn=f32(2)):
    """The reference loops, element by element (cpp:4754-4886), on given weight planes."""
    H, W, D = vm.shape

    def st(prev, add, w):
        out = np.empty(D, f32)
        for d in range(D):
            if plain:
                m = prev[d]
            else:
                lo = f32(prev[d - 1] + pn) if d > 0 else BIG
                up = f32(prev[d + 1] + pn) if d < D - 1 else BIG
                m = min(min(lo, up), prev[d])
            out[d] = f32(add[d] + f32(m * w))
        return out

    c1, c2 = np.zeros_like(vm), np.zeros_like(vm)
    for v in range(H):
        c1[v, 0] = vm[v, 0]
        for u in range(1, W):
            c1[v, u] = st(c1[v, u - 1], vm[v, u], wh[v, u - 1])
        c2[v, W - 1] = vm[v, W - 1]
        for u in range(W - 2, -1, -1):
            c2[v, u] = st(c2[v, u + 1], vm[v, u], wh[v, u])
    A = ((c1 + c2).astype(f32) - vm).astype(f32)
    T, B = np.zeros_like(vm), np.zeros_like(vm)
    for u in range(W):
        T[0, u] = A[0, u]
        for v in range(1, H):
            T[v, u] = st(T[v - 1, u], A[v, u], wv[v - 1, u])
        B[H - 1, u] = A[H - 1, u]
        for v in range(H - 2, -1, -1):
            B[v, u] = st(B[v + 1, u], A[v, u], wv[v, u])
    return ((T + B).astype(f32) - A).astype(f32)


def test_weights_by_hand():
    """Equal neighbours weigh exactly 1; one step of 255 in one channel gives s = 1 and
    expf(-1 / (0.08f * 0.08f)), which underflows to 0."""
    bgr = np.zeros((2, 3, 3), np.uint8)
    bgr[0, 1] = (255, 0, 0)
    bgr[1, 2] = (10, 10, 10)
    wh, wv = F.weights(bgr)
    assert wh[0, 0] == 0 and wh[0, 1] == 0 and wh[1, 0] == 1
    assert wv[0, 0] == 1 and wv[0, 1] == 0
    # (10 / 255)^2 * 3 / 0.0064: the three squares in double, one rounding to float
    d = np.float64(f32(10) * f32(1 / 255.0))
    s = f32((d * d + d * d) + d * d)
    want = F.expf(f32(-s) / f32(f32(0.08) * f32(0.08)))
    assert wh[1, 1] == want and wv[0, 2] == want and 0 < want < 1
    assert wh[0, 2] == 0 and wh[1, 2] == 0 and (wv[1] == 0).all()   # never read: left 0


def test_d1_has_no_neighbours():
    """D = 1: both d +/- 1 neighbours are absent (FLT_MAX), so FIF_Improve equals the plain form."""
    rng = np.random.default_rng(1)
    vm = rng.random((4, 5, 1), dtype=f32)
    bgr = (rng.integers(0, 3, (4, 5, 3)) * 4).astype(np.uint8)
    a, b = F.fif(vm, bgr), F.fif(vm, bgr, plain=True)
    np.testing.assert_array_equal(bits(a), bits(b))
    wh, wv = F.weights(bgr)
    np.testing.assert_array_equal(bits(a), bits(_loops(vm, wh, wv, False)))


@pytest.mark.parametrize("plain", [False, True])
def test_2x2_by_hand(plain):
    """2 x 2, D = 3, constant guide (weights 1): every sweep has one step, written out."""
    vm = np.array([[[1, 5, 2], [4, 0.5, 3]], [[2, 2, 9], [0.25, 7, 1]]], f32)
    bgr = np.full((2, 2, 3), 77, np.uint8)
    wh, wv = F.weights(bgr)
    assert wh[0, 0] == 1 and wh[1, 0] == 1 and wv[0, 0] == 1 and wv[0, 1] == 1
    pn = f32(2)

    def m(p):   # min over d - 1, d, d + 1 of the previous pixel
        if plain:
            return p
        return np.array([min(p[1] + pn, p[0]), min(min(p[0] + pn, p[2] + pn), p[1]), min(p[1] + pn, p[2])], f32)

    A = np.empty_like(vm)
    for v in range(2):
        c1 = [vm[v, 0], vm[v, 1] + m(vm[v, 0])]
        c2 = [vm[v, 0] + m(vm[v, 1]), vm[v, 1]]
        for u in range(2):
            A[v, u] = (c1[u] + c2[u]) - vm[v, u]
    want = np.empty_like(vm)
    for u in range(2):
        T = [A[0, u], A[1, u] + m(A[0, u])]
        B = [A[0, u] + m(A[1, u]), A[1, u]]
        for v in range(2):
            want[v, u] = (T[v] + B[v]) - A[v, u]
    np.testing.assert_array_equal(bits(F.fif(vm, bgr, plain=plain)), bits(want))


@pytest.mark.parametrize("plain", [False, True])
def test_constant_guide_and_random_guide_match_the_loops(plain):
    rng = np.random.default_rng(2)
    vm = (rng.random((5, 6, 7), dtype=f32) * f32(2)).astype(f32)
    for bgr in (np.full((5, 6, 3), 200, np.uint8), (rng.integers(0, 4, (5, 6, 3)) * 3).astype(np.uint8)):
        wh, wv = F.weights(bgr)
        if bgr.min() == bgr.max():
            assert (wh[:, :-1] == 1).all() and (wv[:-1] == 1).all()
        got = F.fif(vm, bgr, plain=plain)
        np.testing.assert_array_equal(bits(got), bits(_loops(vm, wh, wv, plain)))
        assert (got >= vm).all() and not np.signbit(got).any()   # outputs >= +0 for inputs >= +0


def test_forms_differ_where_expected():
    """A cheap neighbour disparity (cost 0 next to cost 10, Pn = 2) is taken by FIF_Improve only."""
    vm = np.zeros((1, 2, 3), f32)
    vm[0, 0] = (0, 10, 10)
    vm[0, 1] = (1, 1, 1)
    bgr = np.zeros((1, 2, 3), np.uint8)
    imp, pl = F.fif(vm, bgr), F.fif(vm, bgr, plain=True)
    # c1[1] = vm[1] + min(...): improve (0, 2, 10) vs plain (0, 10, 10); c2[1] = vm[1]; H = 1: T = Bt = A
    np.testing.assert_array_equal(imp[0, 1], np.array([1, 3, 11], f32))
    np.testing.assert_array_equal(pl[0, 1], np.array([1, 11, 11], f32))
    np.testing.assert_array_equal(imp[0, 0, 0], pl[0, 0, 0])


def test_defaults_and_struct_tail():
    p = _capi.default_params(63, 32, 32)
    assert p.fif_mode == _capi.FIF_IMPROVE == 0 and _capi.FIF_PLAIN == 1
    assert f32(p.fif_eps) == f32(0.08) and p.fif_pn == 2.0
    assert _capi.AGGREGATIONS["FIF"] == 5 and 4 not in _capi.AGGREGATIONS.values()
    # the struct holds a double: its size is a multiple of 8, and the new fields are the tail
    assert p.struct_size == C.sizeof(_capi.sm_params) and C.sizeof(_capi.sm_params) % 8 == 0
    names = [n for n, _ in _capi.sm_params._fields_]
    assert names[-4:] == ["fuse_cost_scan", "fif_mode", "fif_eps", "fif_pn"]
    assert _capi.sm_params.fif_pn.offset + 4 <= C.sizeof(_capi.sm_params)


def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    try:
        return st, lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


@pytest.mark.parametrize("over,msg", [(dict(fif_mode=2), b"fif_mode"), (dict(fif_mode=-1), b"fif_mode"),
                                      (dict(fif_eps=0.0), b"fif_eps"), (dict(fif_eps=-0.08), b"fif_eps"),
                                      (dict(fif_eps=float("nan")), b"fif_eps"),
                                      (dict(fif_pn=-1.0), b"fif_pn"), (dict(fif_pn=-0.0), b"fif_pn"),
                                      (dict(fif_pn=float("nan")), b"fif_pn")])
def test_fif_validation_messages(over, msg):
    st, err = _create(_capi.default_params(15, 32, 32, aggregation=5, **over))
    assert st == _capi.SM_EINVAL and msg in err, err


@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_aggregation_5_passes_validation(mode, opt):
    """Without a GPU sm_create then fails at the device, not with SM_EINVAL; D = 1 and 2 x 2 pass."""
    st, err = _create(_capi.default_params(0, 2, 2, aggregation="FIF", fif_mode=mode, optimization=opt))
    assert st != _capi.SM_EINVAL, err
    st, err = _create(_capi.default_params(1023, 32, 32, aggregation=5, fif_mode=mode, optimization=opt, fif_pn=0.0))
    assert st != _capi.SM_EINVAL, err


@pytest.mark.parametrize("value", [4, 6])
def test_reserved_and_unknown_aggregations_rejected(value):
    st, err = _create(_capi.default_params(15, 32, 32, aggregation=value))
    assert st == _capi.SM_EINVAL and b"aggregation" in err


def test_fif_constants_zeroed_under_cbca_pass():
    st, err = _create(_capi.default_params(15, 32, 32, fif_mode=9, fif_eps=0.0, fif_pn=-1.0))
    assert st != _capi.SM_EINVAL, err


def test_python_facade_accepts_fif():
    """to_c maps "FIF" and the FIF_PLAIN class switch (like MY_GUIDE) into sm_params."""
    assert StereoMatching.FIF_PLAIN is False
    prm = StereoMatching.Parameters(15, 32, 32)
    p = prm.to_c("censusGrad", "FIF", "sgm")
    assert (p.aggregation, p.fif_mode) == (5, 0)
    assert prm.to_c("censusGrad", "FIF", "so", fif_plain=True).fif_mode == 1
    with pytest.raises(KeyError):
        prm.to_c("censusGrad", "FIFX", "sgm")
