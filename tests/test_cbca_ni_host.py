"""Cross-based aggregation without arm intersection (cbca_intersect == false) without a GPU: the restatement
(tests/pyref_cbca_ni.py) against the fixtures tests/golden/cbca_ni/*.npz and against a literal loop
transliteration of gen1DCumu / cal1DCost / genfinalVm_cbca, the conditions those fixtures must meet, and the C
ABI's validation, symbol tables and facades.
"""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

import pyref
import pyref_cbca_ni as P
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cbca_ni")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"cbca_ni_{name}.npz")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def main():
    fx = load("main")
    pair = {k: fx[k] for k in KEYS}
    return fx, pair, P.aggregate(pair, 16, 2)


# ---- the restatement and the fixtures ------------------------------------------------------------

def test_fixture_set_is_complete_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
    assert [os.path.basename(f) for f in files] == ["cbca_ni_main.npz", "cbca_ni_odd.npz"]
    assert all(os.path.getsize(f) < 512 * 1024 for f in files)
    assert set(load("main")) == set(KEYS) | {"vm0", "vm1", "area0", "area1", "vm0_n1", "vm0_n3", "index"}
    assert set(load("odd")) == set(KEYS) | {"vm0", "vm1", "area0", "area1", "index"}


def test_fixture_inputs_are_the_documented_ones(main):
    fx, pair, _ = main
    assert int(fx["index"]) == 0
    want = P.make_input(40, 56, 16, 0)
    for k in KEYS:
        np.testing.assert_array_equal(pair[k], want[k])
    odd = load("odd")
    want = P.make_input(23, 37, 13, 0)
    for k in KEYS:
        np.testing.assert_array_equal(odd[k], want[k])
    assert odd["vm0"].shape == (23, 37, 13) and 13 % 4 and (37 * 13) % 4


def test_pyref_reproduces_the_fixtures(main):
    fx, pair, r = main
    for v in ("0", "1"):
        np.testing.assert_array_equal(bits(r["vm" + v]), bits(fx["vm" + v]))
        np.testing.assert_array_equal(r["area" + v], fx["area" + v])
        assert fx["area" + v].dtype == np.int32
    for n in (1, 3):
        got = P.aggregate(pair, 16, n, refine=False)["vm0"]
        np.testing.assert_array_equal(bits(got), bits(fx[f"vm0_n{n}"]))
    odd = load("odd")
    ro = P.aggregate({k: odd[k] for k in KEYS}, 13, 2)
    for v in ("0", "1"):
        np.testing.assert_array_equal(bits(ro["vm" + v]), bits(odd["vm" + v]))
        np.testing.assert_array_equal(ro["area" + v], odd["area" + v])


def literal(vm, arms, iters):
    """gen1DCumu (cpp:3896-3926), cal1DCost (h:1643-1715) and genfinalVm_cbca (cpp:3969-3992) with
    cbca_intersect == false, loop by loop, every f32 operation rounded on its own."""
    f = np.float32
    H, W, D = vm.shape
    vm = vm.astype(f).copy()
    area = None
    for k in range(iters):
        area = np.ones((H, W), np.int32)
        for horiz in ((True, False) if k % 2 == 0 else (False, True)):
            n_line, n_pos = (H, W) if horiz else (W, H)
            at = (lambda l, x: (l, x)) if horiz else (lambda l, x: (x, l))
            for l in range(n_line):                      # gen1DCumu: in place, in scan order
                for x in range(1, n_pos):
                    for d in range(D):
                        vm[at(l, x) + (d,)] = f(vm[at(l, x - 1) + (d,)] + vm[at(l, x) + (d,)])
                    area[at(l, x)] = area[at(l, x - 1)] + area[at(l, x)]
            out, aout = np.empty_like(vm), np.empty_like(area)   # cal1DCost: into a temporary, copied back
            for l in range(n_line):
                for x in range(n_pos):
                    tail, head = (int(arms[at(l, x) + (j,)]) for j in ((0, 1) if horiz else (2, 3)))
                    pt = x - tail - 1
                    for d in range(D):
                        s = vm[at(l, x + head) + (d,)]
                        out[at(l, x) + (d,)] = f(s - vm[at(l, pt) + (d,)]) if pt >= 0 else s
                    a = area[at(l, x + head)]
                    aout[at(l, x)] = a - area[at(l, pt)] if pt >= 0 else a
            vm, area = out, aout
        for v in range(H):                               # genfinalVm_cbca: float / (float)int
            for u in range(W):
                for d in range(D):
                    vm[v, u, d] = f(vm[v, u, d] / f(area[v, u]))
    return vm, area


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_restatement_equals_the_literal_loops(main, iters):
    """On a 9 x 11 x 3 crop: the crop's own arms (recomputed on the cropped image, so they stay inside it)."""
    _, pair, _ = main
    img = np.ascontiguousarray(pair["lbgr"][20:29, 30:41])
    arms = pyref.arms(img)
    inner_h, inner_v = P.inner_masks(arms)
    assert inner_h.any() and not inner_h.all() and inner_v.any() and not inner_v.all()
    rng = np.random.default_rng(5)
    vm = (rng.random((9, 11, 3), dtype=np.float32) * np.float32(3)).astype(np.float32)
    want, want_area = literal(vm, arms, iters)
    got, got_area = P.cbca_ni(vm, arms, iters)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(got_area, want_area)


def test_fixture_conditions(main):
    """`inner` true and false in both directions for both images' arms; the views' areas differ; the result is
    not the intersecting form's, and one, two and three iterations differ."""
    import make_cbca_ni as M
    fx, pair, r = main
    assert M.conditions(r) == []
    for arms in (r["armsL"], r["armsR"]):
        for inner in P.inner_masks(arms):
            assert inner.any() and not inner.all()
    assert (fx["area0"] != fx["area1"]).any()
    assert fx["area0"].min() >= 1 and fx["area0"].max() <= (2 * 34 + 1) ** 2
    isect = pyref.cbca(r["raw0"], r["armsL"].astype(np.int32), r["armsR"].astype(np.int32), 2, 0)
    assert (bits(isect) != bits(fx["vm0"])).mean() > 0.5
    assert (P.wta(isect) != P.wta(fx["vm0"])).any()
    assert (bits(fx["vm0_n1"]) != bits(fx["vm0"])).any() and (bits(fx["vm0_n3"]) != bits(fx["vm0"])).any()
    # view 1 runs with the right image's arms: the left image's would give another volume
    other, _ = P.cbca_ni(r["raw1"], r["armsL"], 2)
    assert (bits(other) != bits(fx["vm1"])).any()


def test_first_iteration_area_is_the_cross_region(main):
    """After one iteration the area is the number of pixels in the cross region: the sum over the vertical arm
    span of the rows' horizontal spans."""
    _, pair, r = main
    _, area = P.cbca_ni(r["raw0"][:, :, :1], r["armsL"], 1)
    a = r["armsL"].astype(np.int64)
    span = a[..., 0] + a[..., 1] + 1
    for v, u in ((0, 0), (17, 20), (39, 55), (5, 50)):
        assert area[v, u] == span[v - a[v, u, 2]:v + a[v, u, 3] + 1, u].sum()


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx, st


@pytest.mark.parametrize("value", [2, -1, 7])
def test_cbca_intersect_config_value(value):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32))
    try:
        assert lib.sm_cbca_intersect_config(ctx, value) == _capi.SM_EINVAL
        assert b"intersect" in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_cbca_intersect_config(None, 0) == _capi.SM_EINVAL


@pytest.mark.parametrize("agg", ["", "GF", "NL", "FIF", "AWS", "BF", "GFNL"])
def test_cbca_intersect_config_needs_cbca(agg):
    lib, ctx, _ = _create(_capi.default_params(15, 32, 32, aggregation=agg))
    try:
        for value in (0, 1):
            assert lib.sm_cbca_intersect_config(ctx, value) == _capi.SM_EINVAL
            assert b"aggregation" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_sm_params_unchanged():
    names = [n for n, _ in _capi.sm_params._fields_]
    assert not any("intersect" in n.lower() for n in names)
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216


def test_header_and_ctypes_symbol_tables_agree():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in ("sm_cbca_intersect_config", "sm_get_cbca_area"):
        assert fn in declared and hasattr(lib, fn)
    sig = dict((n, a) for n, _, a in _capi.SIGNATURES)
    assert sig["sm_cbca_intersect_config"][1:] == [C.c_int32]
    assert sig["sm_get_cbca_area"][1] == C.c_int32


# ---- the facades -------------------------------------------------------------------------------------

def test_python_facade_carries_the_field():
    prm = StereoMatching.Parameters(59, 30, 40)
    assert prm.cbca_intersect is True
    assert callable(StereoBatch.cbca_intersect_config) and callable(StereoBatch.get_cbca_area)
    # not an sm_params field: the struct is the same either way
    off = StereoMatching.Parameters(59, 30, 40)
    off.cbca_intersect = False
    assert bytes(prm.to_c("censusGrad", "CBCA", "sgm")) == bytes(off.to_c("censusGrad", "CBCA", "sgm"))
    src = open(os.path.join(ROOT, "mystereomatching_amd", "stereo_matching.py")).read()
    assert "if not param.cbca_intersect and self.aggregation == \"CBCA\":" in src
    assert "sm_cbca_intersect_config(ctx, 0)" in src


def test_cpp_facade_source():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    assert "bool cbca_intersect = true;" in src
    assert "if (!param.cbca_intersect && aggregation == \"CBCA\") check(sm_cbca_intersect_config(ctx_, 0)" in src


def test_cbca_ni_facade_check_compiles(tmp_path):
    """tests/cpp/cbca_ni_facade_check.cpp builds against the facade and the library (its maps are compared on the
    GPU in tests/test_cbca_ni_facade.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "cbca_ni_facade_check.cpp"), str(tmp_path / "cbca_ni_facade_check"))
