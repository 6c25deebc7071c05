"""refine()'s outlier classification without a GPU: the restatement's (tests/pyref_outlier.py) own properties on
hand-computed cases, a recorded fixture of its outputs, sm_refine_outlier_config's and sm_get_lrc_mask's argument
checks on a device-less context, the symbol tables, and the facades' plumbing through a recording stand-in for the
library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyref_outlier as P
from mystereomatching_amd import StereoBatch, StereoMatching, _capi
from test_da_host import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "outlier", "outlier_small.npz")
f32 = np.float32
OCC, MIS, PKR = P.DISP_OCC, P.DISP_MIS, P.DISP_PKR


# ---- the restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,W", [(1, 5), (2, 9), (16, 40), (70, 65), (256, 130)])
def test_scatter_form_equals_the_loop(D, W):
    rng = np.random.default_rng(D + W)
    for _ in range(20):
        row = rng.choice([rng.integers(-3, D + 4), -1, 0, D - 1, D], W).astype(np.int16)
        row = np.where(rng.random(W) < 0.5, rng.integers(-2, D + 3, W), row).astype(np.int16)
        np.testing.assert_array_equal(P.mismatch_scatter(row, D), [P.mismatch_loop(row, u, D) for u in range(W)])
    d0 = rng.integers(-2, D + 3, (4, W)).astype(np.int16)
    d1 = rng.integers(-2, D + 3, (4, W)).astype(np.int16)
    for md in (0.0, 1.0, 1e9):
        a, ma = P.lr_classify(d0, d1, D, md)
        b, mb = P.lr_classify(d0, d1, D, md, scatter=True)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ma, mb)


def test_classify_by_hand():
    #            u:  0   1   2   3   4   5
    d0 = np.array([[0, 2, 1, -1, 3, 9]], np.int16)
    d1 = np.array([[0, 1, 5, 3, 9, 0]], np.int16)
    # u=0: d=0, DP1(0)=0: passes.  u=1: u-d<0: fails; DP1(1-0)=1? no (d'=0 needs 0), DP1(0)=0 with d'=1? no: occlusion
    # u=2: d=1, DP1(1)=1: passes.  u=3: d<0: fails; d'=0: DP1(3)=3 no, d'=1: DP1(2)=5 no, d'=2: DP1(1)=1 no,
    # d'=3: DP1(0)=0 no: occlusion.  u=4: d=3, DP1(1)=1, |3-1|=2 > 0: fails; d'=0: DP1(4)=9, ..., d'=3: DP1(1)=1 no: occlusion
    # u=5: d=9 > u: fails; d'=0: DP1(5)=0: mismatch
    out, mask = P.lr_classify(d0, d1, 16)
    np.testing.assert_array_equal(out, [[0, OCC, 1, OCC, OCC, MIS]])
    np.testing.assert_array_equal(mask, [[0, 255, 0, 255, 255, 0 + 255]])
    # LRmaxDiff 2 lets u=4 pass; the float compare: |d - DP1| = 2 > 2.0f is false
    out, mask = P.lr_classify(d0, d1, 16, 2.0)
    assert out[0, 4] == 3 and mask[0, 4] == 0
    # the scan stops at D: with D = 1 only d' = 0 is tried; u=5 stays a mismatch, and DP1(u - 1) == 1 is not seen
    d1b = np.array([[0, 1, 5, 3, 1, 7]], np.int16)
    assert P.lr_classify(d0, d1b, 2)[0][0, 5] == MIS and P.lr_classify(d0, d1b, 1)[0][0, 5] == OCC


def _region(vals, H=5, W=5):
    """A H x W map whose centre is a hole, arms spanning the whole map from the centre column, the other pixels
    taken row-major from vals (the rest holes)."""
    dp = np.full((H, W), -1, np.int16)
    cells = [(a, b) for a in range(H) for b in range(W) if (a, b) != (H // 2, W // 2)]
    for (a, b), x in zip(cells, vals):
        dp[a, b] = x
    arms = np.zeros((H, W, 4), np.uint16)
    arms[:, W // 2, 0] = arms[:, W // 2, 1] = W // 2
    arms[H // 2, W // 2, 2] = arms[H // 2, W // 2, 3] = H // 2
    return dp, arms


@pytest.mark.parametrize("vote", [P.vote_hv, P.vote_hv_rows])
def test_vote_boundaries(vote):
    def run(vals, rv_s, D=16):
        dp, arms = _region(vals)
        return vote(dp, arms, 2, 2, D, rv_s, 0.4)
    assert not (f32(2) / f32(5) > f32(0.4)) and f32(3) / f32(7) > f32(0.4)
    assert run([7, 7, 1, 2, 3], 0) == -1                # 2 of 5: (float)2 / 5 > 0.4f is false
    assert run([7, 7, 7, 1, 2, 3, 4], 0) == 7           # 3 of 7
    assert run([7] * 5, 5) == -1                        # validNum == rv_s
    assert run([7] * 6, 5) == 7                         # rv_s + 1
    assert run([9, 4, 9, 4], 0) == 4                    # the lowest disparity wins a tie
    assert run([12, 3, 12, 3, 3, 12], 0) == 3
    assert run([], 0) == -1 and run([], -1) == -1       # no valid value: 0 / 0 compares false
    # the deviation: a value >= D counts in validNum and in no bin
    assert run([7, 7, 20, 20, 20], 0, D=16) == -1       # 2 of 5
    assert run([7, 7, 7, 20, 20], 0, D=16) == 7         # 3 of 5
    assert run([20, 20, 20], 0, D=16) == -1             # every bin empty: 0 / 3


def test_vote_region_follows_each_rows_arms():
    dp = np.full((5, 7), -1, np.int16)
    dp[1, 3], dp[2, 0], dp[2, 6], dp[3, 2], dp[0, 3] = 4, 9, 9, 4, 9
    arms = np.zeros((5, 7, 4), np.uint16)
    arms[2, 3] = (1, 1, 1, 1)          # rows 1..3; row 2 spans columns 2..4
    arms[1, 3, :2] = (0, 0)            # row 1: column 3 only
    arms[3, 3, :2] = (1, 0)            # row 3: columns 2..3
    assert P.vote_hv(dp, arms, 2, 3, 16, 0, 0.4) == 4   # (1, 3) and (3, 2): the 9s lie outside the region
    assert P.vote_hv_rows(dp, arms, 2, 3, 16, 0, 0.4) == 4


def test_background_value():
    row = np.array([[5, -1, -1, -1, 2, -1, 7]], np.int16)
    assert P.fill_bg(row, 0, 2) == 2 and P.fill_bg(row, 0, 2, 1) == -1 and P.fill_bg(row, 0, 2, 0) == -1
    assert P.fill_bg(row, 0, 1, 1) == 5 and P.fill_bg(row, 0, 1, 3) == 2 and P.fill_bg(row, 0, 5) == 2
    assert P.fill_bg(np.array([[-1, -1, 3]], np.int16), 0, 0) == 3 and P.fill_bg(np.array([[-1, -1]], np.int16), 0, 0) == -1


def test_types_by_hand():
    dp = np.array([[6, OCC, 2, MIS, 2, 2, PKR, -1]], np.int16)
    arms = np.zeros((1, 8, 4), np.uint16)
    arms[0, :, 0] = arms[0, :, 1] = 1
    arms[0, 0, 0] = arms[0, 7, 1] = 0
    kw = dict(rv_s=0, rv_ratio=0.4)
    # rv: (0,1): {6, 2} a tie of 1 of 2 -> the lowest, 2; (0,3): {2, 2} -> 2; (0,6): {2} -> 2; (0,7): {} -> -1
    np.testing.assert_array_equal(P.rv_combine(dp, arms, 16, itype=0, **kw), [[6, 2, 2, 2, 2, 2, 2, -1]])
    # bg: min of the neighbours found: (0,1): min(2, 6) = 2; (0,7): left only
    np.testing.assert_array_equal(P.rv_combine(dp, arms, 16, itype=1, **kw), [[6, 2, 2, 2, 2, 2, 2, 2]])
    # type 2: occ -> bg, mis -> rv, the others carry the last result (2)
    st = {}
    np.testing.assert_array_equal(P.rv_combine(dp, arms, 16, itype=2, stats=st, **kw), [[6, 2, 2, 2, 2, 2, 2, 2]])
    assert st == {"carried": 2, "last": 2}
    # type 3 on an occlusion: rv when bg is missing, the smaller when both exist
    d3 = np.array([[9, OCC, 9, -1, -1, OCC, 4, 4]], np.int16)
    a3 = arms.copy()
    np.testing.assert_array_equal(P.rv_combine(d3, a3, 16, itype=3, depth=0, **kw)[0, [1, 5]], [9, 4])   # bg none
    np.testing.assert_array_equal(P.rv_combine(d3, a3, 16, itype=3, **kw)[0, [1, 5]], [9, 4])
    d3[0, 2] = 3
    assert P.rv_combine(d3, a3, 16, itype=3, **kw)[0, 1] == 3                         # rv: tie {9, 3} -> 3; bg: 3
    assert P.rv_combine(d3, a3, 16, itype=3, rv_s=2, rv_ratio=0.4)[0, 1] == 3         # rv fails (validNum 2): bg


def test_carry():
    # the first hole of the image is of neither class: -1 carried, it stays; a value crosses a row end
    dp = np.array([[PKR, 4, OCC, 4, PKR], [PKR, -1, MIS, 1, PKR], [PKR, 5, 5, 5, 5]], np.int16)
    arms = np.zeros((3, 5, 4), np.uint16)
    st = {}
    out = P.rv_combine(dp, arms, 16, rv_s=0, itype=2, stats=st)
    # (0,2) occ: bg = 4.  (0,4), (1,0), (1,1): carry 4.  (1,2) mis: its region is itself, no valid value: -1, so
    # (1,4) and (2,0) get nothing
    np.testing.assert_array_equal(out, [[PKR, 4, 4, 4, 4], [4, 4, MIS, 1, PKR], [PKR, 5, 5, 5, 5]])
    assert st == {"carried": 3, "last": -1}
    # Jacobi: the carried fills are not seen by later holes of the same call
    assert P.fill_bg(out, 1, 2) == 1 and out[1, 2] == MIS
    # types 0 and 1 assign every hole: nothing is carried
    for t in (0, 1):
        st = {}
        P.rv_combine(dp, arms, 16, rv_s=0, itype=t, stats=st)
        assert st["carried"] == 0
    # without classification every hole is of neither class under types 2 and 3: nothing is ever filled
    plain = np.where(dp < 0, -1, dp).astype(np.int16)
    for t in (2, 3):
        np.testing.assert_array_equal(P.rv_combine(plain, arms, 16, rv_s=0, itype=t), plain)


def _golden_inputs():
    rng = np.random.default_rng(20261020)
    H, W, D = 12, 40, 16
    uu = np.arange(W)[None, :]
    d0 = np.minimum(rng.integers(0, D, (H, W)), uu).astype(np.int16)
    d0[rng.random((H, W)) < 0.3] = -1
    d1 = np.where(rng.random((H, W)) < 0.6, np.minimum(d0, D - 1), rng.integers(-1, D + 2, (H, W))).astype(np.int16)
    vv = np.arange(H)[:, None]
    arms = np.stack([np.minimum(rng.integers(0, 6, (H, W)), uu), np.minimum(rng.integers(0, 6, (H, W)), W - 1 - uu),
                     np.minimum(rng.integers(0, 4, (H, W)), vv), np.minimum(rng.integers(0, 4, (H, W)), H - 1 - vv)],
                    axis=2).astype(np.uint16)
    pkr = rng.random((H, W)) < 0.15
    return d0, d1, arms, pkr, D


def golden_outputs():
    d0, d1, arms, pkr, D = _golden_inputs()
    out = {}
    lab, mask = P.lr_classify(d0, d1, D, 1.0)
    out["labelled"], out["mask"] = lab, mask
    d = lab.copy()
    d[pkr & (d >= 0)] = PKR
    for t in range(4):
        out[f"type{t}_depth1000_s3"] = P.rv_combine(d, arms, D, 3, 0.4, t)
        out[f"type{t}_depth2_s0"] = P.rv_combine(P.rv_combine(d, arms, D, 0, 0.4, t, 2), arms, D, 0, 0.4, t, 2)
    return out


def test_recorded_fixture():
    """tests/golden/outlier/outlier_small.npz holds the restatement's outputs as first written: a later edit that changes
    what it computes shows here."""
    rec = np.load(GOLDEN)
    out = golden_outputs()
    assert sorted(rec.files) == sorted(out)
    for k, v in out.items():
        assert rec[k].dtype == v.dtype
        np.testing.assert_array_equal(rec[k], v, err_msg=k)
    assert (out["labelled"] == OCC).sum() > 10 and (out["labelled"] == MIS).sum() > 10
    assert any((out[f"type{t}_depth1000_s3"] != out["type0_depth1000_s3"]).any() for t in (1, 2, 3))


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx


OK_ARGS = (1, -48, 1, 0)


@pytest.mark.parametrize("args,msg", [
    ((2, -48, 0, 0), b"classify"), ((-1, -48, 0, 0), b"classify"),
    ((0, -48, 2, 0), b"rv_combine"), ((1, -48, -1, 3), b"rv_combine"),
    ((1, 0, 0, 0), b"disp_mis"), ((0, -32768, 0, 0), b"disp_mis"), ((1, 5, 1, 0), b"disp_mis"),
    ((1, -32, 1, 0), b"disp_occ"), ((0, -32, 0, 0), b"disp_occ"),
    ((1, -48, 1, 4), b"interpolate_type"), ((0, -48, 0, -1), b"interpolate_type"),
])
def test_refine_outlier_config_messages(args, msg):
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1))
    try:
        assert lib.sm_refine_outlier_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_refine_outlier_config(None, *OK_ARGS) == _capi.SM_EINVAL


def test_refine_outlier_config_needs_do_refine_and_takes_every_optimiser():
    lib, ctx = _create(_capi.default_params(15, 32, 32))
    try:
        assert lib.sm_refine_outlier_config(ctx, *OK_ARGS) == _capi.SM_EINVAL
        assert b"do_refine" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    for opt in ("so", "sgm", ""):
        lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1, optimization=opt))
        try:
            for args in (OK_ARGS, (0, -48, 0, 0), (1, -32767, 1, 3), (1, -1, 0, 2)):
                assert lib.sm_refine_outlier_config(ctx, *args) == _capi.SM_OK, lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)
    # disp_occ is the context's: another value frees -32 and takes its own
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1, disp_occ=-7))
    try:
        assert lib.sm_refine_outlier_config(ctx, 1, -32, 0, 0) == _capi.SM_OK
        assert lib.sm_refine_outlier_config(ctx, 1, -7, 0, 0) == _capi.SM_EINVAL
    finally:
        lib.sm_destroy(ctx)


def test_null_arguments():
    lib = _capi.load()
    assert lib.sm_get_lrc_mask(None, None) == _capi.SM_EINVAL
    assert lib.sm_refine_outlier_config(None, 0, -48, 0, 0) == _capi.SM_EINVAL


def test_get_lrc_mask_checks_on_a_context():
    """sm_get_lrc_mask on a context that exists: a null destination is SM_EINVAL with the argument named; before
    a classifying refine the answer is SM_ESTATE, whether or not the switch was set -- both decided without a device."""
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1))
    buf = np.full((32, 32), 7, np.uint8)
    try:
        assert lib.sm_get_lrc_mask(ctx, None) == _capi.SM_EINVAL
        assert b"null dst" in lib.sm_last_error(ctx)
        assert lib.sm_get_lrc_mask(ctx, _capi.ptr(buf)) == _capi.SM_ESTATE
        assert b"no mask yet" in lib.sm_last_error(ctx)
        assert lib.sm_refine_outlier_config(ctx, *OK_ARGS) == _capi.SM_OK
        assert lib.sm_get_lrc_mask(ctx, _capi.ptr(buf)) == _capi.SM_ESTATE
        assert (buf == 7).all()
    finally:
        lib.sm_destroy(ctx)


def test_symbol_tables_and_sm_params():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in ("sm_refine_outlier_config", "sm_get_lrc_mask"):
        assert fn in declared and hasattr(lib, fn)
    sig = dict((n, a) for n, _, a in _capi.SIGNATURES)
    assert sig["sm_refine_outlier_config"][1:] == [C.c_int32] * 4
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216
    assert not any("mis" in n or "interpolate" in n or "classify" in n for n, _ in _capi.sm_params._fields_)
    assert _capi.REFINE_OUTLIER_DEFAULTS == (P.DISP_MIS, 0)
    for cite in ("cpp:2284-2335", "cpp:7146-7216", "cpp:6830-6862", "cpp:6964-7043", "cpp:1367", "cpp:1408"):
        assert cite in hdr, cite


# ---- the facades -------------------------------------------------------------------------------------

@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    real = _capi.load()
    r.sm_params_default = real.sm_params_default          # host-only: fills the struct
    monkeypatch.setattr(_capi, "load", lambda: r)
    return r


def test_python_facade_defaults():
    assert StereoMatching.LRC_CLASSIFY is False and StereoMatching.RV_COMBINE_BG is False
    prm = StereoMatching.Parameters(15, 32, 40)
    assert prm.interpolateType == 0 and prm.DISP_MIS == -48 and prm.DISP_OCC == -32
    for fn in ("refine_outlier_config", "get_lrc_mask"):
        assert callable(getattr(StereoBatch, fn))


def test_stereo_batch_plumbing(rec):
    sb = StereoBatch(15, 32, 40, 2, do_refine=1, refine_outlier=dict(classify=True, interpolate_type=3))
    assert [a[1:] for a in rec.named("sm_refine_outlier_config")] == [(1, -48, 0, 3)]
    sb.refine_outlier_config(rv_combine=True, disp_mis=-9)
    assert rec.named("sm_refine_outlier_config")[-1][1:] == (0, -9, 1, 0)
    m = sb.get_lrc_mask()
    assert m.shape == (32, 40) and m.dtype == np.uint8 and len(rec.named("sm_get_lrc_mask")) == 1
    sb._ctx = None
    rec.calls.clear()
    sb = StereoBatch(15, 32, 40, 2, do_refine=1)          # without the override the entry point is not called
    assert not rec.named("sm_refine_outlier_config")
    sb._ctx = None


def test_compute_function_hands_the_override_on(rec):
    batch = pytest.importorskip("mystereomatching_amd.batch")
    fn = batch.hip_compute_fn(15, 32, 40, 2, 0, do_refine=1, refine_outlier=dict(classify=True, rv_combine=True))
    assert [a[1:] for a in rec.named("sm_refine_outlier_config")] == [(1, -48, 1, 0)]
    assert fn.get_lrc_mask().shape == (32, 40)


def test_stereo_matching_plumbing(rec):
    cls = StereoMatching
    saved = (cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG)
    z3, z1 = np.zeros((32, 40, 3), np.uint8), np.zeros((32, 40), np.uint8)
    try:
        for refine, lrc, rv, want in ((True, True, True, [(1, -40, 1, 2)]), (True, True, False, [(1, -40, 0, 2)]),
                                      (True, False, True, [(0, -40, 1, 2)]), (True, False, False, []), (False, True, True, [])):
            rec.calls.clear()
            cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG = refine, lrc, rv
            prm = cls.Parameters(15, 32, 40)
            prm.DISP_MIS, prm.interpolateType = -40, 2
            sm = cls(z3, z3, z1, z1, param=prm)
            assert [a[1:] for a in rec.named("sm_refine_outlier_config")] == want
            if refine:
                sm.refine()
                assert (sm.LRC_Err_Mask is not None) == lrc and len(rec.named("sm_get_lrc_mask")) == int(lrc)
            sm._ctx = None
    finally:
        cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG = saved


def test_cpp_facade_source_and_docs():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("inline static bool LRC_CLASSIFY = false;", "inline static bool RV_COMBINE_BG = false;", "Mat LRC_Err_Mask;",
                 "int DISP_MIS = -3 * 16;", "int interpolateType = 0;",
                 "sm_refine_outlier_config(ctx_, LRC_CLASSIFY ? 1 : 0, param.DISP_MIS, RV_COMBINE_BG ? 1 : 0, param.interpolateType)",
                 "sm_get_lrc_mask(ctx_, LRC_Err_Mask.ptr<uint8_t>())"):
        assert decl in src, decl
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "RV_combine_BG" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "sm_refine_oc.hip" in design and "## 21." in design


def test_outlier_facade_check_compiles(tmp_path):
    """tests/cpp/outlier_facade_check.cpp builds against the facade and the library (its maps are compared on the GPU
    in tests/test_gpu_outlier.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "outlier_facade_check.cpp"), str(tmp_path / "outlier_facade_check"))
