"""CBCA()'s double-window branch without a GPU: the restatement (tests/pyref_cbca_dw.py) against the fixtures
tests/golden/cbca_dw/*.npz, the conditions those fixtures must meet, and the C ABI's validation, symbol tables
and facades.
"""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

import pyref_box
import pyref_cbca_dw as P
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cbca_dw")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"cbca_dw_{name}.npz")))


@pytest.fixture(scope="module")
def main():
    fx = load("main")
    pair = {k: fx[k] for k in ("lbgr", "rbgr", "lgray", "rgray")}
    return fx, pair, P.compose(pair, 16, refine=True)


# ---- the restatement and the fixtures ------------------------------------------------------------

def test_fixture_set_is_complete_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
    assert [os.path.basename(f) for f in files] == ["cbca_dw_main.npz", "cbca_dw_odd.npz"]
    assert all(os.path.getsize(f) < 512 * 1024 for f in files)


def test_fixture_input_is_the_documented_one(main):
    fx, pair, _ = main
    want = P.make_input(40, 56, 16, int(fx["index"]))
    for k in ("lbgr", "rbgr", "lgray", "rgray"):
        np.testing.assert_array_equal(pair[k], want[k])
    assert int(fx["index"]) == 0


def test_pyref_reproduces_the_fixture(main):
    fx, _, r = main
    np.testing.assert_array_equal(r["mask"], fx["mask"])
    np.testing.assert_array_equal(r["arms"], fx["arms"])
    for v in ("vm0", "vm1"):
        np.testing.assert_array_equal(r[v].view(np.uint32), fx[v].view(np.uint32))
    odd = load("odd")
    pair = {k: odd[k] for k in ("lbgr", "rbgr", "lgray", "rgray")}
    assert odd["vm0"].shape == (23, 37, 13) and 13 % 4 and (37 * 13) % 4
    ro = P.compose(pair, 13, refine=False)
    np.testing.assert_array_equal(ro["mask"], odd["mask"])
    np.testing.assert_array_equal(ro["vm0"].view(np.uint32), odd["vm0"].view(np.uint32))


def test_mask_equals_the_integer_predicate(main):
    """boxFilter's float result < 5 is "sum of the nine reflected maxima < 45" on the fixture (and a sum of 45,
    which gives exactly 5.0f, is not selected)."""
    fx, _, _ = main
    np.testing.assert_array_equal(P.mask_from_arms(fx["arms"]), P.mask_int(fx["arms"]))
    np.testing.assert_array_equal(fx["mask"], P.mask_int(fx["arms"]))
    s = P.nine_sum(P.arm_max(fx["arms"]))
    assert (fx["mask"][s == 44] == 1).all() and (fx["mask"][s == 45] == 0).all()
    # the rolling sums of cv::boxFilter and the direct nine-term sum agree: the sums are exact
    lst = P.arm_max(fx["arms"]).astype(np.float32)
    np.testing.assert_array_equal(pyref_box.box_filter(lst, 3, 3), pyref_box.box_filter_direct(lst, 3, 3))


def test_integer_predicate_for_every_sum():
    """(float)(s * (1.0 / 9)) < 5.0f <=> s < 45 for every sum of nine arm lengths <= 84."""
    s = np.arange(0, 9 * 84 + 1, dtype=np.float64)
    f = (s * (1.0 / 9)).astype(np.float32)
    np.testing.assert_array_equal(f < np.float32(5), s < 45)
    assert f[45] == np.float32(5)


def test_fixture_conditions(main):
    """The conditions the generator asserts (tests/golden/make_cbca_dw.py)."""
    import make_cbca_dw as M
    fx, _, r = main
    assert M.conditions(r) == []
    share = float(fx["mask"].mean())
    assert 0.2 <= share <= 0.8
    s = P.nine_sum(P.arm_max(fx["arms"]))
    assert (s == 44).sum() >= 1 and (s == 45).sum() >= 1
    for v in ("0", "1"):
        assert (r["vm" + v] != r["small" + v]).any() and (r["vm" + v] != r["large" + v]).any()
    assert (P.wta(r["vm0"]) != P.wta(r["small0"])).any()
    # selected and unselected pixels on every border row and column
    m = fx["mask"]
    for edge in (m[0], m[-1], m[:, 0]):
        assert 0 < edge.sum() < edge.size
    assert P.arm_max(fx["arms"]).max() == 22
    ro = P.compose({k: load("odd")[k] for k in ("lbgr", "rbgr", "lgray", "rgray")}, 13, refine=False)
    assert M.conditions(ro, need_edge_sums=False) == []


def test_both_windows_start_from_window0_costs(main):
    """`vm2 = clone(vm)`: the large-window run aggregates the costs costCalculate made, whose gradient weights
    came from window 0's arms.  The restatement's small-window volume is a whole oracle run's; its large-window
    volume is NOT a whole oracle run with window 1's settings (that one weights the gradients by window 1's arms)."""
    from oracle import oracle as O
    _, pair, r = main
    w0 = O.run_ex(pair, O.config(40, 56, 15, cbca_iters=2, do_refine=1, **P.WIN0), dumps=("agg", "agg_right"))
    np.testing.assert_array_equal(w0["agg"].view(np.uint32), r["small0"].view(np.uint32))
    np.testing.assert_array_equal(w0["agg_right"].view(np.uint32), r["small1"].view(np.uint32))
    w1 = O.run_ex(pair, O.config(40, 56, 15, cbca_iters=2, **P.WIN1), dumps=("agg",))
    assert (w1["agg"] != r["large0"]).any()


def test_view1_is_composed_with_the_left_mask(main):
    fx, pair, r = main
    sel = fx["mask"].astype(bool)
    assert (fx["vm1"][sel] == r["large1"][sel]).all() and (fx["vm1"][~sel] == r["small1"][~sel]).all()
    # the right image's own arms would give another mask
    from oracle import oracle as O
    right = P.mask_from_arms(O.arms(pair["rbgr"], O.config(40, 56, 15, **P.WIN0)))
    assert (right != fx["mask"]).any()


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("args,msg", [
    ((1, -1, 23, 30, 0, 5.0), b"arm_l2"), ((1, 23, -1, 30, 0, 5.0), b"arm_l_out2"), ((1, 23, 85, 30, 0, 5.0), b"arm_l_out2"),
    ((1, 23, 23, -1, 0, 5.0), b"arm_c_thresh2"), ((1, 23, 23, 30, -1, 5.0), b"arm_c_thresh_out2"),
    ((1, 23, 23, 30, 0, float("nan")), b"arm_len_thres"), ((1, 23, 23, 30, 0, float("inf")), b"arm_len_thres"),
    ((0, 23, 23, 30, 0, float("-inf")), b"arm_len_thres"),
])
def test_cbca_double_config_messages(args, msg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32))
    try:
        assert lib.sm_cbca_double_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_cbca_double_config(None, 1, 23, 23, 30, 0, 5.0) == _capi.SM_EINVAL


@pytest.mark.parametrize("agg", ["", "GF", "NL", "FIF", "AWS", "BF", "GFNL"])
def test_cbca_double_config_needs_cbca(agg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation=agg))
    try:
        assert lib.sm_cbca_double_config(ctx, 1, 23, 23, 30, 0, 5.0) == _capi.SM_EINVAL
        assert b"aggregation" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_sm_params_unchanged():
    names = [n for n, _ in _capi.sm_params._fields_]
    assert not any("double" in n.lower() or "dw" in n.lower() for n in names)
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


def test_header_and_ctypes_symbol_tables_agree():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in ("sm_cbca_double_config", "sm_get_cbca_dw_mask"):
        assert fn in declared and hasattr(lib, fn)
    args = dict((n, a) for n, _, a in _capi.SIGNATURES)["sm_cbca_double_config"]
    assert args[1:] == [C.c_int32] * 5 + [C.c_float]
    assert _capi.CBCA_DW_DEFAULTS == (23, 23, 30, 0, 5.0)


# ---- the facades -------------------------------------------------------------------------------------

def test_python_facade_defaults():
    prm = StereoMatching.Parameters(59, 30, 40)
    assert prm.cbca_double_win is False and prm.GF_double_win is False
    assert (prm.cbca_crossL, prm.cbca_crossL_out, prm.cbca_cTresh, prm.cbca_cTresh_out) == (
        [17, 23, 34], [34, 23, 34], [20, 30, 30], [6, 0, 0])
    assert prm.cbca_double_args() == (23, 23, 30, 0, 5.0)
    assert StereoMatching.Parameters(59, 30, 40, disSc=2).cbca_double_args() == (11, 11, 30, 0, 5.0)
    assert callable(StereoBatch.cbca_double_config) and callable(StereoBatch.get_cbca_dw_mask)


def test_double_win_fields_leave_sm_params_alone():
    """Neither switch is an sm_params field: GF_double_win changes nothing at all (both arms of the reference's
    branch run guideFilter(0, vm)), cbca_double_win goes through sm_cbca_double_config."""
    for agg in ("GF", "CBCA"):
        a = StereoMatching.Parameters(59, 30, 40)
        b = StereoMatching.Parameters(59, 30, 40)
        b.GF_double_win = True
        b.cbca_double_win = True
        pa, pb = a.to_c("censusGrad", agg, "sgm"), b.to_c("censusGrad", agg, "sgm")
        assert bytes(pa) == bytes(pb)
    src = open(os.path.join(ROOT, "mystereomatching_amd", "stereo_matching.py")).read()
    assert src.count("GF_double_win") == 1   # the field's default and nothing that reads it


def test_cpp_facade_source():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("bool cbca_double_win = false;", "bool GF_double_win = false;", "unsigned char cbca_crossL[3] = {17, 23, 34};",
                 "unsigned char cbca_crossL_out[3] = {34, 23, 34};", "unsigned char cbca_cTresh[3] = {20, 30, 30};",
                 "unsigned char cbca_cTresh_out[3] = {6, 0, 0};"):
        assert decl in src, decl
    assert "p.arm_l = param.cbca_crossL[0] / sc;" in src and "p.arm_l_out = param.cbca_crossL_out[0] / sc;" in src
    assert "sm_cbca_double_config(ctx_, 1, param.cbca_crossL[1] / sc, param.cbca_crossL_out[1] / sc" in src
    assert src.count("GF_double_win") == 1


def test_cbca_dw_facade_check_compiles(tmp_path):
    """tests/cpp/cbca_dw_facade_check.cpp builds against the facade and the library (its maps are compared on the
    GPU in tests/test_cbca_dw_facade.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "cbca_dw_facade_check.cpp"), str(tmp_path / "cbca_dw_facade_check"))
