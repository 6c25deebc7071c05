"""GPU parity of aggregation "GFNL" (GFNL(), stereoMatching.cpp:4421-4490), bit for bit.

vm[0] = NL of the raw costs where the left gray image's 19 x 19 variance (cv::boxFilter,
BORDER_REFLECT_101) is below 400, else (float)(0.5 NL + 0.5 GF) with the sum formed in double;
vm[1] (Do_refine) is GF's.  Expected: the oracle's guided_filter and nl_aggregate, the numpy twin
of the box filter for the variance plane, and the blend in float64 (tests/pyref_box.py).

The synthetic pairs have a variance of 165-385 everywhere, which reaches only the `var < 400`
branch, so the right half of both images (columns >= W / 2, gray and every BGR channel) is
stretched to clip(128 + 3 (v - 128)); every case asserts from the twin's mask that both classes
then hold >= 10 % of the pixels.  10 x 12 (the size minimum) is single-class and exempt.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pyref
import pyref_box as B
from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S
from test_cpp_facade import _compile, write_ppm

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
GF, NL, GFNL = 2, 3, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


def stretched(pair):
    """Columns >= W / 2 of every image become clip(128 + 3 (v - 128))."""
    out = {}
    for k in KEYS:
        a = pair[k].astype(np.int32)
        axis = a.ndim - (2 if k in ("lbgr", "rbgr") else 1)   # the column axis (images or batches of images)
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(a.shape[axis] // 2, None)
        a[tuple(sl)] = np.clip(128 + 3 * (a[tuple(sl)] - 128), 0, 255)
        out[k] = a.astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _case(H, W, md, idx, mode, stretch=True):
    """The pair, view 0's NL and GF volumes (oracle) and the twin's variance plane, computed once."""
    O = _oracle()
    pair = S.make_pair(H, W, md + 1, idx)
    pair = {k: pair[k] for k in KEYS}
    if stretch:
        pair = stretched(pair)
    cfg = O.config(H, W, md, gf_mode=mode)
    raw = O.cost_volume(pair, cfg, view=0)
    nl = O.nl_aggregate(raw, pair["lbgr"], cfg)
    gf = O.guided_filter(raw, pair["lbgr"], cfg)
    var = B.variance_plane(pair["lgray"])
    for a in (nl, gf, var):
        a.setflags(write=False)
    return pair, nl, gf, var


def _gpu(pair, H, W, md, agg=GFNL, mode=0, thresh=None, refine=0):
    """(vm[0], vm[1] or None, arm_Mask or None) after sm_cost_calculate."""
    lib = _capi.load()
    p = _capi.default_params(md, H, W, aggregation=agg, optimization=0, gf_mode=mode, do_refine=refine)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        if thresh is not None:
            _capi.check(lib, ctx, lib.sm_gfnl_config(ctx, thresh))
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3,
                                                _capi.ptr(a["lgray"]), _capi.ptr(a["rgray"]), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        vols = []
        for view in range(2 if refine else 1):
            got = np.empty((H, W, md + 1), np.float32)
            _capi.check(lib, ctx, lib.sm_get_volume(ctx, view, _capi.ptr(got)))
            vols.append(got)
        mask = None
        if agg == GFNL:
            mask = np.empty((H, W), np.uint8)
            _capi.check(lib, ctx, lib.sm_get_gfnl_mask(ctx, _capi.ptr(mask)))
        return vols[0], (vols[1] if refine else None), mask
    finally:
        lib.sm_destroy(ctx)


SHAPES = [(24, 30, 7, 900), (40, 61, 63, 901), (33, 47, 69, 902), (48, 64, 31, 903), (40, 56, 23, 904)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W,md,idx", SHAPES)
def test_gfnl_volume_bits_and_mask(H, W, md, idx, mode):
    pair, nl, gf, var = _case(H, W, md, idx, mode)
    want, wmask = B.gfnl(nl, gf, pair["lgray"])
    share = float(wmask.mean())
    print(f"{H}x{W}: {100 * share:.1f} % of the pixels below 400, variance {var.min():.0f} .. {var.max():.0f}")
    assert 0.10 <= share <= 0.90, "a bad input: both classes must hold >= 10 % of the pixels"
    got, _, mask = _gpu(pair, H, W, md, mode=mode)
    np.testing.assert_array_equal(mask, wmask)
    np.testing.assert_array_equal(bits(got), bits(want))


def test_gfnl_size_minimum():
    """10 x 12, D = 4: radius 9 with one reflection on every side (single-class; ximgproc form only,
    MY_GUIDE needs 19 x 19)."""
    H, W, md = 10, 12, 3
    pair, nl, gf, _ = _case(H, W, md, 905, 0, stretch=False)
    want, wmask = B.gfnl(nl, gf, pair["lgray"])
    got, _, mask = _gpu(pair, H, W, md)
    np.testing.assert_array_equal(mask, wmask)
    np.testing.assert_array_equal(bits(got), bits(want))


def test_gfnl_threshold_extremes():
    """var_thresh = 1e30: every pixel takes NL's value, the bits of a plain "NL" context;
    -1e30: every pixel is blended."""
    H, W, md = 24, 30, 7
    pair, nl, gf, _ = _case(H, W, md, 900, 0)
    got, _, mask = _gpu(pair, H, W, md, thresh=1e30)
    assert mask.all()
    plain, _, _ = _gpu(pair, H, W, md, agg=NL)
    np.testing.assert_array_equal(bits(got), bits(plain))
    np.testing.assert_array_equal(bits(got), bits(nl))
    got, _, mask = _gpu(pair, H, W, md, thresh=-1e30)
    assert not mask.any()
    want, _ = B.gfnl(nl, gf, pair["lgray"], -1e30)
    np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize("mode", [0, 1])
def test_gfnl_right_view_is_gf(mode):
    """With Do_refine view 1 is guideFilter's (cpp:4499) and never blended; view 0 is unchanged by it."""
    H, W, md = 24, 30, 7
    pair, nl, gf, _ = _case(H, W, md, 900, mode)
    got0, got1, _ = _gpu(pair, H, W, md, mode=mode, refine=1)
    _, plain1, _ = _gpu(pair, H, W, md, agg=GF, mode=mode, refine=1)
    np.testing.assert_array_equal(bits(got1), bits(plain1))
    np.testing.assert_array_equal(bits(got0), bits(B.gfnl(nl, gf, pair["lgray"])[0]))


@functools.lru_cache(maxsize=None)
def _batch(H, W, D, n, first):
    batch = S.make_batch(n, H, W, D, first_index=first)
    return stretched({k: batch[k] for k in KEYS})


@functools.lru_cache(maxsize=None)
def _want_volume(H, W, D, n, first, i, view):
    """Pair i's expected volume after SolveAll: GFNL's blend (view 0) or GF (view 1)."""
    O = _oracle()
    batch = _batch(H, W, D, n, first)
    pair = {k: batch[k][i] for k in KEYS}
    cfg = O.config(H, W, D - 1, gf_mode=0)
    raw = O.cost_volume(pair, cfg, view=view)
    if view == 0:
        vm, mask = B.gfnl(O.nl_aggregate(raw, pair["lbgr"], cfg), O.guided_filter(raw, pair["lbgr"], cfg), pair["lgray"])
        assert 0.10 <= float(mask.mean()) <= 0.90
    else:
        vm = O.guided_filter(raw, pair["rbgr"], cfg)
    vm = pyref.solve_all(vm)
    vm.setflags(write=False)
    return vm


MAPS = [dict(optimization=1, sgm_paths=4), dict(optimization=1, sgm_paths=8), dict(optimization=0),
        dict(optimization=1, sgm_paths=4, do_refine=1)]


@pytest.mark.parametrize("cfg", MAPS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_gfnl_maps(cfg):
    """sm_run (SolveAll fused into the blend's store, and into GF's for vm[1]) for n = 3 pairs."""
    H, W, D, n, first = 30, 44, 32, 3, 940
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation="GFNL", gf_mode=0, **cfg)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
    finally:
        sb.close()

    def view(i, v):
        vm = _want_volume(H, W, D, n, first, i, v)
        if cfg["optimization"] == 1:   # (costs may be negative: pyref.sgm takes plain float minima)
            return pyref.wta(pyref.sgm(vm, batch[("lbgr", "rbgr")[v]][i], paths=cfg["sgm_paths"]))
        return pyref.wta(vm)

    for i in range(n):
        want = view(i, 0)
        if cfg.get("do_refine"):
            want = pyref.refine(want, view(i, 1), pyref.arms(batch["lbgr"][i]), batch["lbgr"][i], D)
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")


def test_gfnl_cpp_facade_matches_python_path(tmp_path):
    """tests/cpp/bf_gfnl_facade_check.cpp with aggregation "GFNL", at the default threshold and
    with every pixel blended."""
    src = os.path.join(ROOT, "tests", "cpp", "bf_gfnl_facade_check.cpp")
    exe = str(tmp_path / "bf_gfnl_facade_check")
    _compile(src, exe)
    H, W, md = 24, 30, 15
    pair = S.make_pair(H, W, md + 1, 970)
    pair = {k: pair[k] for k in ("lbgr", "rbgr")}
    # the facade reads the gray images from the colour files (imread flags 0: libpng's weights)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    for k, thresh in enumerate([400.0, -1e30]):
        out = tmp_path / f"dp{k}.i16"
        r = subprocess.run([exe, "GFNL", str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(md), repr(thresh), "0",
                            str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(out, np.int16).reshape(H, W)
        sb = StereoBatch(md, H, W, 1, device=0, aggregation="GFNL", num_streams=1, gfnl_var_thresh=thresh)
        try:
            sb.upload(*(pair[k][None] for k in KEYS))
            want = sb.run(0.3)[0]
        finally:
            sb.close()
        np.testing.assert_array_equal(got, want)
