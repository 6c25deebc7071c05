"""Aggregation "AWS" without a GPU: the numpy twin (tests/pyref_aws.py) on hand-checkable cases,
the host Lab conversion over every colour, the C ABI's enumerator and sm_aws_config, and the
Python facade's selector.

AWS(): stereoMatching.cpp:5692-5801, the branch without JBF_STANDARD; genWeight_AWS / calW4_AWS /
calvm_AWS: stereoMatching.h:1305-1350, 1472-1493, 1533-1548.  PARITY UNPINNED (the Lab planes
restate OpenCV's 8-bit BGR2Lab).
"""
import ctypes as C
import math

import numpy as np
import pytest

import pyref_aws as A
from pyref import expf
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


ANCHORS = [((255, 255, 255), (255, 128, 128)), ((0, 0, 0), (0, 128, 128)), ((255, 0, 0), (82, 207, 20)),
           ((0, 255, 0), (224, 42, 211)), ((0, 0, 255), (136, 208, 195)), ((0, 255, 255), (248, 106, 223)),
           ((255, 0, 255), (154, 226, 67)), ((128, 128, 128), (137, 128, 128))]


def _host_lab(bgr):
    lib = _capi.load()
    bgr = np.ascontiguousarray(bgr, np.uint8)
    out = np.empty_like(bgr)
    lib.sm_bgr2lab_host(_capi.ptr(bgr), bgr.size // 3, _capi.ptr(out))
    return out


@pytest.mark.parametrize("bgr,lab", ANCHORS)
def test_lab_anchors(bgr, lab):
    px = np.array([bgr], np.uint8)
    assert tuple(A.bgr2lab(px)[0]) == lab
    assert tuple(_host_lab(px)[0]) == lab


def test_host_lab_every_colour():
    """sm_bgr2lab_host against the twin on all 2^24 colours, a blue plane (65536 colours) at a time."""
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    px = np.empty((65536, 3), np.uint8)
    px[:, 1], px[:, 2] = g.ravel(), r.ravel()
    for b in range(256):
        px[:, 0] = b
        np.testing.assert_array_equal(_host_lab(px), A.bgr2lab(px), err_msg=f"blue {b}")


def _refl1(i, n):
    """The border rule, one index at a time."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def test_reflection_rule():
    assert [_refl1(i, 3) for i in range(-1, 4)] == [1, 0, 1, 2, 1]
    assert _refl1(-3, 2) == 1 and _refl1(4, 2) == 0 and _refl1(-17, 2) == 1   # reflected more than once
    assert _refl1(-17, 1) == 0 and _refl1(5, 1) == 0
    for n in (1, 2, 3, 5):
        idx = np.arange(-40, 40)
        assert A.refl(idx, n).tolist() == [_refl1(int(i), n) for i in idx]


def _loops(vm, lab, lor, rv, ru, gamma_c=f32(5)):
    """The reference loops element by element, on python scalars rounded with numpy float32."""
    H, W, D = vm.shape

    def wgt(i, v, u, dv, du):
        p = lab[i][v, u].astype(f32)
        q = lab[i][_refl1(v + dv, H), _refl1(u + du, W)].astype(f32)
        d = [f32(p[c] - q[c]) for c in range(3)]
        s = f32((float(f32(d[0] * d[0])) * 0.153787 + float(f32(d[1] * d[1]))) + float(f32(d[2] * d[2])))
        dif = f32(math.sqrt(float(s)))
        return expf(np.array([f32(-dif) / f32(gamma_c)], f32))[0]

    out = vm.copy()
    for v in range(H):
        for u in range(W):
            for d in range(D):
                u1, u2 = u + d * lor, u - d * (1 - lor)
                if u1 >= W or u2 < 0:
                    continue
                numer = denom = f32(0)
                for dv in range(-rv, rv + 1):
                    for du in range(-ru, ru + 1):
                        ele = f32(wgt(0, v, u1, dv, du) * wgt(1, v, u2, dv, du))
                        denom = f32(denom + ele)
                        numer = f32(numer + f32(ele * vm[_refl1(v + dv, H), _refl1(u + du, W), d]))
                out[v, u, d] = f32(numer / denom)
    return out


def test_3x3_constant_colour_by_hand():
    """3 x 3, D = 2, radius 1, one colour: every weight is 1, so an element is the f32 sum of its
    reflected 3 x 3 window over 9; view 0 leaves (u = 0, d = 1) untouched, view 1 (u = 2, d = 1)."""
    vm = np.arange(18, dtype=f32).reshape(3, 3, 2) * f32(0.5) + f32(1)
    img = np.full((3, 3, 3), 90, np.uint8)
    vols, oks, wt = A.aws([vm, vm], img, img, 1, 1)
    assert (wt[0] == 1).all() and (wt[1] == 1).all()
    idx = [1, 0, 1, 2, 1]   # reflect-101 of -1 .. 3 into [0, 3)
    for lor in (0, 1):
        for v in range(3):
            for u in range(3):
                for d in range(2):
                    if (u - d < 0) if lor == 0 else (u + d >= 3):
                        assert not oks[lor][u, d]
                        assert vols[lor][v, u, d] == vm[v, u, d]
                        continue
                    acc = f32(0)
                    for dv in (-1, 0, 1):
                        for du in (-1, 0, 1):
                            acc = f32(acc + vm[idx[v + dv + 1], idx[u + du + 1], d])
                    assert vols[lor][v, u, d] == f32(acc / f32(9)), (lor, v, u, d)
    # the centre pixel of view 0 at d = 0 by hand: the plain mean of all nine d = 0 costs
    assert vols[0][1, 1, 0] == f32(vm[:, :, 0].sum(dtype=np.float64)) / f32(9)   # (the sum is exact)


@pytest.mark.parametrize("H,W,D,rv,ru", [(3, 3, 2, 1, 1),     # the hand case's shape with real colours
                                         (1, 2, 2, 3, 3),     # indices reflected more than once
                                         (2, 4, 3, 0, 2)])
def test_twin_matches_the_scalar_loops(H, W, D, rv, ru):
    rng = np.random.default_rng(H * 100 + W)
    vm = [(rng.random((H, W, D), dtype=f32) * f32(3)).astype(f32) for _ in range(2)]
    imgs = [(120 + rng.integers(0, 12, (H, W, 3))).astype(np.uint8) for _ in range(2)]
    lab = [A.bgr2lab(i) for i in imgs]
    vols, oks, wt = A.aws(vm, imgs[0], imgs[1], rv, ru)
    centre = rv * (2 * ru + 1) + ru
    assert (wt[0][..., centre] == 1).all() and 0 < wt[0].min() < 1
    for lor in (0, 1):
        np.testing.assert_array_equal(bits(vols[lor]), bits(_loops(vm[lor], lab, lor, rv, ru)))
        assert not np.signbit(vols[lor]).any()
        np.testing.assert_array_equal(bits(vols[lor])[:, ~oks[lor]], bits(vm[lor])[:, ~oks[lor]])


def test_weight_by_hand():
    """One step of 10 in a (grey -> L only changes): s = (float)(dL^2 * 0.153787), w = expf(-sqrt(s) / 5)."""
    lab = np.zeros((1, 2, 3), np.uint8)
    lab[0, 1] = (10, 0, 0)
    w = A.weights(lab, 0, 1)
    s = f32(100.0 * 0.153787)
    want = expf(np.array([f32(-f32(math.sqrt(float(s)))) / f32(5)], f32))[0]
    # pixel 0: taps u - 1 -> refl = 1, u, u + 1 = 1; pixel 1: taps 0, 1, refl(2) = 0
    assert w[0, 0].tolist() == [want, 1, want] and w[0, 1].tolist() == [want, 1, want]


def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


def test_enumerator_7_passes_validation_4_and_6_do_not():
    assert _capi.AGGREGATIONS["AWS"] == 7
    assert 4 not in _capi.AGGREGATIONS.values() and 6 not in _capi.AGGREGATIONS.values()
    for opt in (0, 1, 2):
        lib, ctx, st = _create(_capi.default_params(15, 32, 32, aggregation="AWS", optimization=opt))
        try:
            assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)
    for value in (4, 6, 8):
        lib, ctx, st = _create(_capi.default_params(15, 32, 32, aggregation=value))
        try:
            assert st == _capi.SM_EINVAL and b"aggregation" in lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("args,msg", [((-1, 17, 5.0), b"radius_v"), ((18, 17, 5.0), b"radius_v"),
                                      ((17, -1, 5.0), b"radius_u"), ((17, 18, 5.0), b"radius_u"),
                                      ((17, 17, 0.0), b"gamma_c"), ((17, 17, -5.0), b"gamma_c"),
                                      ((17, 17, float("nan")), b"gamma_c"), ((17, 17, float("inf")), b"gamma_c")])
def test_aws_config_messages(args, msg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="AWS"))
    try:
        assert lib.sm_aws_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
        for good in ((17, 17, 5.0), (0, 0, 0.5), (5, 3, 50.0)):
            assert lib.sm_aws_config(ctx, *good) == _capi.SM_OK
    finally:
        lib.sm_destroy(ctx)


def test_aws_config_needs_an_aws_context():
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation="CBCA"))
    try:
        assert lib.sm_aws_config(ctx, 17, 17, 5.0) == _capi.SM_EINVAL
        assert b"aggregation" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_aws_config(None, 17, 17, 5.0) == _capi.SM_EINVAL


def test_sm_params_unchanged():
    """AWS adds no field: the struct ends as before and keeps its size."""
    names = [n for n, _ in _capi.sm_params._fields_]
    assert names[-4:] == ["fuse_cost_scan", "fif_mode", "fif_eps", "fif_pn"]
    p = _capi.default_params(15, 32, 32)
    assert p.struct_size == C.sizeof(_capi.sm_params) == 216   # as before this aggregation was added


def test_python_facade_accepts_aws():
    assert (StereoMatching.AWS_RADIUS_V, StereoMatching.AWS_RADIUS_U, StereoMatching.AWS_GAMMA_C) == (17, 17, 5.0)
    prm = StereoMatching.Parameters(15, 32, 32)
    assert prm.to_c("censusGrad", "AWS", "sgm").aggregation == 7
    assert prm.to_c("censusGrad", "AWS", "so").aggregation == 7
    assert callable(StereoBatch.aws_config)


def test_cpp_facade_accepts_aws():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "stereo_matching.hpp")).read()
    assert re.search(r'aggregation == "AWS" \? SM_AGG_AWS', src) and "sm_aws_config(ctx_" in src
    hdr = open(os.path.join(root, "include", "sm_capi.h")).read()
    assert re.search(r"SM_AGG_AWS = 7\b", hdr)
