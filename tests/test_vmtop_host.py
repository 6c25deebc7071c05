"""dispOptimize's Do_vmTop branch without a GPU: the restatement (tests/pyref_vmtop.py) against the fixtures
tests/golden/vmtop/vmtop_*.npz, the branch coverage those fixtures must have, and the C ABI's validation, symbol
tables and facades.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import pyref_vmtop as V
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vmtop")
NAMES = ("mix", "mix_m8", "case2", "rows", "signed")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"vmtop_{name}.npz")))


def settings(fx):
    return sorted(k[4:] for k in fx if k.startswith("map_"))


# ---- the restatement ---------------------------------------------------------------------------

def test_fixture_set_is_complete_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "vmtop_*.npz")))
    assert [os.path.basename(f) for f in files] == sorted(f"vmtop_{n}.npz" for n in NAMES)
    assert sum(os.path.getsize(f) for f in files) < 200 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_pyref_reproduces_the_fixture(name):
    fx = load(name)
    num, thres, ts = int(fx["num"]), f32(fx["thres"]), int(fx["ts"])
    table, counts = V.select(fx["vol"], num, thres)
    np.testing.assert_array_equal(counts, fx["counts"])
    np.testing.assert_array_equal(bits(table), bits(fx["table"]))
    # entries past the count are never written; the count sits in [num][0]
    k = np.arange(num)[None, None, :]
    assert (table[:, :, :num][k >= counts[:, :, None]] == 0).all()
    np.testing.assert_array_equal(table[:, :, num, 0], counts.astype(f32))
    # the sorted top-M prefix gives the same table
    tf, cf = V.select_fast(fx["vol"], num, thres)
    np.testing.assert_array_equal(cf, counts)
    np.testing.assert_array_equal(bits(tf), bits(table))
    for s in settings(fx):
        m, cir2, col = int(s[0]), int(s[1]), int(s[2])
        disp, cnt = V.decide(table, counts, fx["bgr"], m, ts, cir2, col)
        assert disp.dtype == np.int16
        np.testing.assert_array_equal(disp, fx[f"map_{s}"], err_msg=s)
        np.testing.assert_array_equal([cnt[c] for c in V.COUNTERS], fx[f"cnt_{s}"], err_msg=s)


def test_branch_coverage_of_the_fixture_set():
    """A condition on the fixtures: every branch of genDispFromTopCostVm2 is taken at least 20 times."""
    total = {c: 0 for c in V.COUNTERS}
    for name in NAMES:
        fx = load(name)
        for s in settings(fx):
            for c, n in zip(V.COUNTERS, fx[f"cnt_{s}"]):
                total[c] += int(n)
    for c in ("case1", "case2", "case3", "case3_tie_by_cost", "dedup", "m1_fallback", "m2_pre", "m2_aft", "m2_none",
              "m2_both"):
        assert total[c] >= 20, (c, total)


def test_case2_fixture_is_one_dependency_chain():
    fx = load("case2")
    H, W = fx["counts"].shape
    assert (H, W) == (33, 41)
    assert int(fx["cnt_010"][V.COUNTERS.index("case2")]) == (H - 1) * (W - 1)   # every pixel off row 0 / column 0


def test_select_rules():
    # the lowest d wins a tie; the winner is masked; candidate k >= 1 needs cost < firstV * thres
    vol = np.array([[[5, 3, 3, 4, 9]]], f32)
    t, c = V.select(vol, 3, f32(1.5))
    assert c[0, 0] == 3 and t[0, 0, :3].tolist() == [[1, 3], [2, 3], [3, 4]] and t[0, 0, 3, 0] == 3
    t, c = V.select(vol, 3, f32(1.0))   # 3 < 3 * 1 fails: the loop breaks
    assert c[0, 0] == 1 and t[0, 0, 1:3].tolist() == [[0, 0], [0, 0]]
    # firstV <= 0 with thres > 1: only candidate 0 survives
    for first in (0.0, -2.0):
        t, c = V.select(np.array([[[first, first, 7]]], f32), 3, f32(1.09))
        assert c[0, 0] == 1 and t[0, 0, 0].tolist() == [0, first]
    # more candidates asked for than disparities: the rescan meets the masked FLT_MAX entries and stops
    t, c = V.select(np.array([[[2, 2]]], f32), 8, f32(1.5))
    assert c[0, 0] == 2


def test_dedup_keeps_the_first_insert():
    """Candidates (d, c): (0, 5), (20, 6), (3, 6) with ts = 10: the pair (0, 2) is close, (0, 1) and (1, 2) are
    not, so the container holds 5 -> 0 and 6 -> 3; without hasCir2 every candidate is inserted in order and
    6 -> 20 stays.  Both are alone at their disparity: the cheaper one wins."""
    table = np.zeros((2, 2, 4, 2), f32)
    counts = np.ones((2, 2), np.int32)
    table[:, :, 3, 0] = 1
    table[1, 1, :3] = [[0, 5], [20, 6], [3, 6]]
    table[1, 1, 3, 0] = 3
    counts[1, 1] = 3
    table[0, 1, 0] = table[1, 0, 0] = table[0, 0, 0] = [3, 1]   # three neighbours vote for d = 3
    bgr = np.zeros((2, 2, 3), np.uint8)
    disp, cnt = V.decide(table, counts, bgr, 0, 10, True, False)
    assert disp[1, 1] == 3 and cnt["case3"] == 1
    disp, cnt = V.decide(table, counts, bgr, 0, 10, False, False)
    assert disp[1, 1] == 0 and cnt["dedup"] == 1   # 6 -> 20 stayed, d = 3 was dropped: d = 0 and d = 20 tie at num 1


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("args,msg", [
    ((1, 3, 2, 1.09, 10, 1, 0), b"method"), ((1, -1, 2, 1.09, 10, 1, 0), b"method"),
    ((1, 0, 0, 1.09, 10, 1, 0), b"num"), ((1, 0, 9, 1.09, 10, 1, 0), b"num"), ((0, 0, -2, 1.09, 10, 1, 0), b"num"),
    ((1, 0, 2, float("nan"), 10, 1, 0), b"thres"), ((1, 0, 2, float("inf"), 10, 1, 0), b"thres"),
    ((0, 0, 2, float("-inf"), 10, 1, 0), b"thres"),
])
@pytest.mark.parametrize("opt", [0, 1, 2])
def test_vmtop_config_messages(args, msg, opt):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, optimization=opt))
    try:
        assert lib.sm_vmtop_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_vmtop_config(None, 1, 0, 2, 1.09, 10, 1, 0) == _capi.SM_EINVAL


def test_sm_params_unchanged():
    names = [n for n, _ in _capi.sm_params._fields_]
    assert names[-4:] == ["fuse_cost_scan", "fif_mode", "fif_eps", "fif_pn"]
    assert not any("vmtop" in n.lower() for n in names)
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


def test_header_and_ctypes_symbol_tables_agree():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    bound = {n for n, _, _ in _capi.SIGNATURES}
    assert declared == bound
    for fn in ("sm_vmtop_config", "sm_set_volume", "sm_get_top_disp"):
        assert fn in declared and re.search(r"SM_API sm_status " + fn + r"\(", hdr)
    lib = _capi.load()
    for n in bound:
        assert hasattr(lib, n), n
    args = dict((n, a) for n, _, a in _capi.SIGNATURES)["sm_vmtop_config"]
    assert args[1:] == [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32]


def test_python_facade_defaults():
    prm = StereoMatching.Parameters(59, 30, 40)
    assert (prm.Do_vmTop, prm.vmTop_method, prm.vmTop_thres_dirNum, prm.vmTop_hasCir2,
            prm.vmTop_cir3_doColorLimit) == (False, 0, 8, True, False)
    assert (prm.vmTop_Num, prm.ts) == (2, 10)
    prm = StereoMatching.Parameters(59, 30, 40, 13, 1, 6, 108, 7)
    assert (prm.vmTop_Num, prm.ts) == (6, 7)
    assert callable(StereoBatch.vmtop_config) and callable(StereoBatch.get_top_disp)


@pytest.mark.parametrize("lamc", range(100, 121))
def test_vmtop_thres_bits(lamc):
    """vmTop_thres = lamc_ * 0.01 (h:323): the product in double, one rounding to float."""
    want = np.float32(np.float64(lamc) * np.float64(0.01))
    got = np.float32(StereoMatching.Parameters(59, 30, 40, lamc=lamc).vmTop_thres)
    assert bits(got) == bits(want)
    assert C.c_float(StereoMatching.Parameters(59, 30, 40, lamc=lamc).vmTop_thres).value == float(want)


def test_cpp_facade_source():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("bool Do_vmTop = false;", "int vmTop_method = 0;", "int vmTop_thres_dirNum = 8;",
                 "bool vmTop_hasCir2 = true;", "bool vmTop_cir3_doColorLimit = false;"):
        assert decl in src, decl
    assert "vmTop_thres((float)(lamc * 0.01))" in src and "lamc * 0.01f" not in src
    assert "sm_vmtop_config(ctx_, 1, param.vmTop_method, param.vmTop_Num, param.vmTop_thres, param.ts" in src


def test_vmtop_facade_check_compiles(tmp_path):
    """tests/cpp/vmtop_facade_check.cpp builds against the facade and the library (its maps are compared on the
    GPU in tests/test_gpu_vmtop.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "vmtop_facade_check.cpp"), str(tmp_path / "vmtop_facade_check"))


def test_float_product_would_differ():
    """Why the C++ facade multiplies in double: in float the threshold differs for some lamc in 100 .. 120."""
    dif = [l for l in range(100, 121) if bits(np.float32(np.float32(l) * np.float32(0.01))) != bits(np.float32(l * 0.01))]
    assert dif
