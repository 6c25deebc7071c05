"""GPU parity of aggregation "BF" against the numpy twin of cv::boxFilter (tests/pyref_box.py), bit for bit.

BF() (stereoMatching.cpp:1023-1043): boxFilter(vm[i], vm[i], -1, Size(12, 12)) on every view that
exists -- normalised, BORDER_REFLECT_101, anchor 6 (offsets -6 .. +5), running row and column sums
in double (sm_bf.hip).  The expected volume is the twin applied to the oracle's cost volume; the
expected maps are that volume through tests/pyref.py's SolveAll, optimisers and refine().
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pyref
import pyref_box as B
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import synthetic as S
from test_cpp_facade import _compile, write_ppm

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
BF = 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


@functools.lru_cache(maxsize=None)
def _case(H, W, md, idx, cost="censusGrad"):
    """The pair and both views' raw cost volumes (computed once, read-only)."""
    O = _oracle()
    pair = S.make_pair(H, W, md + 1, idx)
    pair = {k: pair[k] for k in KEYS}
    cfg = O.config(H, W, md, cost=cost)
    raw = [O.cost_volume(pair, cfg, view=v) for v in (0, 1)]
    for a in raw:
        a.setflags(write=False)
    return pair, raw


def _gpu_volumes(pair, H, W, md, cost="censusGrad", ksize=None, expect=_capi.SM_OK):
    """vm[0], vm[1] after sm_cost_calculate (do_refine = 1: both views exist and are filtered)."""
    lib = _capi.load()
    p = _capi.default_params(md, H, W, aggregation=BF, optimization=0, do_refine=1, cost_method=cost)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        if ksize is not None:
            st = lib.sm_bf_config(ctx, *ksize)
            if expect != _capi.SM_OK:
                assert st == expect, lib.sm_last_error(ctx)
                return None
            _capi.check(lib, ctx, st)
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3,
                                                _capi.ptr(a["lgray"]), _capi.ptr(a["rgray"]), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        out = []
        for view in (0, 1):
            got = np.empty((H, W, md + 1), np.float32)
            _capi.check(lib, ctx, lib.sm_get_volume(ctx, view, _capi.ptr(got)))
            out.append(got)
        return out
    finally:
        lib.sm_destroy(ctx)


# the minimum size and D = 1, ragged D across 64-lane chunks, tall and wide strips
SHAPES = [(7, 7, 0, 800, "censusGrad"), (7, 40, 7, 801, "censusGrad"), (24, 30, 7, 802, "censusGrad"),
          (40, 61, 63, 803, "censusGrad"), (33, 47, 69, 804, "censusGrad"), (21, 19, 255, 805, "censusGrad"),
          (130, 9, 64, 806, "censusGrad"), (24, 30, 15, 807, "AD"), (24, 30, 15, 808, "Census")]


@pytest.mark.parametrize("H,W,md,idx,cost", SHAPES)
def test_bf_volume_bits(H, W, md, idx, cost):
    """The default 12 x 12 window (the column sweep's ring form), both views: uint32 equality."""
    pair, raw = _case(H, W, md, idx, cost)
    got = _gpu_volumes(pair, H, W, md, cost)
    for v in (0, 1):
        want = B.box_filter(raw[v])
        assert (want >= 0).all() and not np.signbit(want).any()   # what the optimisers' minima assume
        np.testing.assert_array_equal(bits(got[v]), bits(want), err_msg=f"view {v}")


@pytest.mark.parametrize("kv,ku", [(1, 1), (2, 3), (11, 12), (12, 11), (32, 32)])
def test_bf_windows(kv, ku):
    """sm_bf_config: anchor parity, the identity and the largest window (the generic column sweep)."""
    H, W, md = 24, 30, 7
    pair, raw = _case(H, W, md, 802)
    got = _gpu_volumes(pair, H, W, md, ksize=(kv, ku))
    for v in (0, 1):
        np.testing.assert_array_equal(bits(got[v]), bits(B.box_filter(raw[v], kv, ku)), err_msg=f"view {v}")
        if (kv, ku) == (1, 1):
            np.testing.assert_array_equal(bits(got[v]), bits(raw[v]))


# the largest window on its minimum image (both reflections reach index 0 and n - 1, lines shorter than one
# tile pair, a ragged second chunk); the tiled column form alone; the row form alone on a one-lane second chunk
@pytest.mark.parametrize("H,W,D,kv,ku,idx", [(17, 17, 70, 32, 32, 810), (17, 40, 3, 32, 1, 811), (9, 17, 65, 1, 32, 812)])
def test_bf_windows_at_the_sweeps_limits(H, W, D, kv, ku, idx):
    """test_bf_windows' assertion at the smallest shapes where the shared line sweeps can still go wrong."""
    pair, raw = _case(H, W, D - 1, idx)
    got = _gpu_volumes(pair, H, W, D - 1, ksize=(kv, ku))
    for v in (0, 1):
        np.testing.assert_array_equal(bits(got[v]), bits(B.box_filter(raw[v], kv, ku)), err_msg=f"view {v}")


def test_bf_window_too_large_for_the_image():
    pair, _ = _case(7, 7, 0, 800)
    assert _gpu_volumes(pair, 7, 7, 0, ksize=(32, 32), expect=_capi.SM_EINVAL) is None


@functools.lru_cache(maxsize=None)
def _batch(H, W, D, n, first):
    batch = S.make_batch(n, H, W, D, first_index=first)
    return {k: batch[k] for k in KEYS}


@functools.lru_cache(maxsize=None)
def _want_volume(H, W, D, n, first, i, view, scaled=True):
    """Pair i's expected BF volume (after SolveAll when `scaled`), shared by the map tests."""
    O = _oracle()
    batch = _batch(H, W, D, n, first)
    pair = {k: batch[k][i] for k in KEYS}
    vm = B.box_filter(O.cost_volume(pair, O.config(H, W, D - 1), view=view))
    vm = pyref.solve_all(vm) if scaled else vm
    vm.setflags(write=False)
    return vm


def _want_map(H, W, D, n, first, i, opt, paths=4, refine=False):
    batch = _batch(H, W, D, n, first)
    pair = {k: batch[k][i] for k in KEYS}

    def view(v):
        vm = _want_volume(H, W, D, n, first, i, v)
        if opt == "sgm":
            return pyref.wta(pyref.sgm(vm, pair[("lbgr", "rbgr")[v]], paths=paths))
        return pyref.wta(vm)

    d0 = view(0)
    if refine:
        d0 = pyref.refine(d0, view(1), pyref.arms(pair["lbgr"]), pair["lbgr"], D)
    return d0


MAPS = [dict(optimization=1, sgm_paths=4), dict(optimization=1, sgm_paths=8), dict(optimization=0),
        dict(optimization=1, sgm_paths=4, do_refine=1)]


@pytest.mark.parametrize("H,W,D", [(30, 44, 32), (21, 30, 200)])
@pytest.mark.parametrize("cfg", MAPS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bf_maps(H, W, D, cfg):
    """sm_run (SolveAll fused into the column sweep's store) for n = 3 pairs: maps of the twin + pyref."""
    n, first = 3, 840
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation="BF", **cfg)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
    finally:
        sb.close()
    opt = {0: "wta", 1: "sgm"}[cfg["optimization"]]
    for i in range(n):
        want = _want_map(H, W, D, n, first, i, opt, paths=cfg.get("sgm_paths", 4), refine=bool(cfg.get("do_refine")))
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")


@pytest.mark.parametrize("H,W,D", [(30, 44, 32), (21, 30, 200)])
def test_bf_so_both_views(H, W, D):
    """"so" runs on both views (Do_LRConsis): DP[1] = so of the filtered vm[1], which SolveAll does
    not touch without Do_refine (cpp:2178); both read the left colours (cpp:1098)."""
    n, first = 3, 840
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation="BF", optimization=2)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
        got1 = sb.get_disp(1)
    finally:
        sb.close()
    for i in range(n):
        want = pyref.so(_want_volume(H, W, D, n, first, i, 0), batch["lbgr"][i])[1]
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")
    want1 = pyref.so(_want_volume(H, W, D, n, first, 0, 1, scaled=False), batch["lbgr"][0])[1]
    np.testing.assert_array_equal(got1, want1)


@pytest.mark.parametrize("sub_batch,num_streams", [(2, 2), (1, 3), (2, 1)])
def test_bf_schedules(sub_batch, num_streams):
    """Groups of pairs on alternating streams: the row sums are per group, so two runs give the
    same maps, the twin's."""
    H, W, D, n, first = 29, 41, 16, 5, 850
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation=BF, sub_batch=sub_batch, num_streams=num_streams)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        first_run = sb.run(0.3)
        second = sb.run(0.3)
    finally:
        sb.close()
    np.testing.assert_array_equal(second, first_run)
    for i in range(n):
        np.testing.assert_array_equal(first_run[i], _want_map(H, W, D, n, first, i, "sgm"), err_msg=f"pair {i}")


def test_bf_reference_ordered_api():
    """costCalculate -> SolveAll([sm], 1, 0.3) -> dispOptimize with the class selectors."""
    H, W, D, first = 30, 44, 32, 840
    batch = _batch(H, W, D, 3, first)
    pair = {k: batch[k][1] for k in KEYS}
    StereoMatching.aggregation = "BF"
    try:
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None,
                            StereoMatching.Parameters(D - 1, H, W), device=0)
        sm.costCalculate()
        vol = sm.vm[0]
        SolveAll([sm], 1, 0.3)
        got = sm.dispOptimize()
    finally:
        StereoMatching.aggregation = "CBCA"
    np.testing.assert_array_equal(bits(vol), bits(_want_volume(H, W, D, 3, first, 1, 0, scaled=False)))
    np.testing.assert_array_equal(got, _want_map(H, W, D, 3, first, 1, "sgm"))


def test_bf_cpp_facade_matches_python_path(tmp_path):
    """tests/cpp/bf_gfnl_facade_check.cpp: the C++ facade with aggregation "BF", at the default
    window and at 1 x 1 (the raw costs)."""
    src = os.path.join(ROOT, "tests", "cpp", "bf_gfnl_facade_check.cpp")
    exe = str(tmp_path / "bf_gfnl_facade_check")
    _compile(src, exe)
    H, W, md = 20, 26, 15
    pair = S.make_pair(H, W, md + 1, 870)
    pair = {k: pair[k] for k in ("lbgr", "rbgr")}
    # the facade reads the gray images from the colour files (imread flags 0: libpng's weights)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    maps = []
    for k, (kv, ku) in enumerate([(12, 12), (1, 1)]):
        out = tmp_path / f"dp{k}.i16"
        r = subprocess.run([exe, "BF", str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(md), str(kv), str(ku),
                            str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(out, np.int16).reshape(H, W)
        sb = StereoBatch(md, H, W, 1, device=0, aggregation="BF", num_streams=1, bf_ksize_v=kv, bf_ksize_u=ku)
        try:
            sb.upload(*(pair[k][None] for k in KEYS))
            want = sb.run(0.3)[0]
        finally:
            sb.close()
        np.testing.assert_array_equal(got, want)
        maps.append(got)
    assert (maps[0] != maps[1]).any()   # the window reached the kernels
