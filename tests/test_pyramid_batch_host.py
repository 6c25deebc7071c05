"""The cross-scale pyramid inside the batch path, without a GPU: the three C ABI symbols, sm_pyramid_config's
argument checks (host code: they run before any device call, so also on a context whose sm_create found no
device), and the staged sm_solve_all's unchanged refusal.
"""
import ctypes as C
import os
import re

import pytest

from mystereomatching_amd import StereoBatch, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx


def test_symbols_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    assert declared == set(sig)
    lib = _capi.load()
    for fn in ("sm_pyramid_config", "sm_pyramid_level", "sm_pyramid_levels"):
        assert fn in declared and hasattr(lib, fn)
    assert sig["sm_pyramid_config"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert sig["sm_pyramid_level"] == (C.c_void_p, [C.c_void_p, C.c_int32])
    assert sig["sm_pyramid_levels"] == (C.c_int32, [C.c_void_p])
    assert re.search(r"SM_API sm_status sm_pyramid_config\(sm_ctx\* ctx, int32_t py_lvl\);", hdr)
    assert re.search(r"SM_API sm_ctx\* sm_pyramid_level\(sm_ctx\* ctx, int32_t level\);", hdr)
    assert re.search(r"SM_API int32_t sm_pyramid_levels\(const sm_ctx\* ctx\);", hdr)
    assert C.sizeof(_capi.sm_params) == 216   # the struct keeps its size
    for m in ("pyramid_config", "pyramid_level_volume", "pyramid_level_arms", "pyramid_level_census"):
        assert callable(getattr(StereoBatch, m))


@pytest.mark.parametrize("py_lvl", [0, 9, -1])
def test_py_lvl_out_of_range(py_lvl):
    lib, ctx = _create(_capi.default_params(63, 300, 260))
    try:
        assert lib.sm_pyramid_config(ctx, py_lvl) == _capi.SM_EINVAL
        assert b"PY_LVL" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_pyramid_config(None, 2) == _capi.SM_EINVAL
    assert lib.sm_pyramid_levels(None) == 0 and lib.sm_pyramid_level(None, 0) is None


@pytest.mark.parametrize("kw,rows,cols,L,level,why", [
    ({}, 3, 40, 3, 2, b"rows and cols must be >= 2"),              # 3 -> 2 -> 1 row
    ({"aggregation": "BF"}, 12, 12, 2, 1, b"BF needs rows, cols >= 7"),     # level 1 is 6 x 6
    ({"aggregation": "GF"}, 16, 16, 2, 1, b"GF (ximgproc) needs rows, cols >= 9"),   # level 1 is 8 x 8
    ({"aggregation": "GFNL"}, 18, 30, 2, 1, b"GFNL needs rows, cols >= 10"),
    ({"aggregation": "NL"}, 5, 9, 3, 2, b"NL needs rows, cols >= 3"),       # 5 -> 3 -> 2 rows
    ({"aggregation": "GF", "gf_mode": 1}, 36, 40, 2, 1, b"MY_GUIDE) needs rows, cols >= 19"),
])
def test_level_that_cannot_exist(kw, rows, cols, L, level, why):
    lib, ctx = _create(_capi.default_params(15, rows, cols, **kw))
    try:
        assert lib.sm_pyramid_config(ctx, L) == _capi.SM_EINVAL
        msg = lib.sm_last_error(ctx)
        assert b"level %d" % level in msg and why in msg, msg
        assert lib.sm_pyramid_config(ctx, L - 1 if L > 2 else 1) == _capi.SM_OK   # one level fewer fits
        assert lib.sm_pyramid_levels(ctx) == 1
    finally:
        lib.sm_destroy(ctx)


@pytest.mark.parametrize("py_lvl", [1, 8])
def test_py_lvl_accepted(py_lvl):
    lib, ctx = _create(_capi.default_params(63, 300, 260))
    try:
        assert lib.sm_pyramid_levels(ctx) == 1   # a fresh context
        assert lib.sm_pyramid_config(ctx, py_lvl) == _capi.SM_OK, lib.sm_last_error(ctx)
        assert lib.sm_pyramid_level(ctx, 0) == ctx.value
        assert lib.sm_pyramid_level(ctx, -1) is None and lib.sm_pyramid_level(ctx, 8) is None
    finally:
        lib.sm_destroy(ctx)


def test_staged_solve_all_still_refuses_a_pyramid():
    """sm_solve_all's contract is unchanged: the call order is checked first, and the message of the PY_LVL
    refusal is the one the library has always given."""
    lib, ctx = _create(_capi.default_params(15, 32, 32))
    try:
        st = lib.sm_solve_all(ctx, 2, 0.3)
        assert st in (_capi.SM_ESTATE, _capi.SM_EINVAL, _capi.SM_EHIP)
        assert st != _capi.SM_OK
    finally:
        lib.sm_destroy(ctx)
    src = open(os.path.join(ROOT, "mystereomatching_amd", "csrc", "sm_capi.cpp")).read()
    assert 'if (py_lev != 1) return fail(c, SM_EINVAL, "PY_LVL > 1 needs every level\'s context: use sm_solve_all_pyr");' in src
