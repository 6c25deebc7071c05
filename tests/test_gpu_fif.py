"""GPU parity of aggregation "FIF" against the numpy twin (tests/pyref_fif.py), bit for bit.

FIF_Improve (stereoMatching.cpp:4707-4890, fif_mode 0, what costCalculate calls) and FIF
(cpp:4541-4705, fif_mode 1): four weighted sweeps over the whole volume (sm_fif.hip).  The
synthetic pairs are heavily textured, so most weights are ~ 0 and the sweeps hardly couple
pixels; every shape therefore also runs with all images quantised (x // q) * q, which flattens the
guide, and the test asserts that the twin's two forms then differ in more than 0.1 % of the
elements (the d +/- 1 path is really exercised).  Shares measured with the twin (view 0 / view 1):
  24x30x8 q 32: 31 % / 34 %     40x61x64 q 64: 7.0 % / 7.4 %    33x47x70 q 16: 1.8 % / 1.8 %
  21x19x256 q 128: 0.40 % / 0.39 %   70x3x63 q 32: 0.25 % / 0.36 %   3x130x129 q 32: 2.8 % / 3.3 %
  5x7x1024: q 64 gave 0.00 % / 0.03 % (7 columns: almost every disparity is out of range), so this
  shape runs with q 200 (a constant guide): 0.70 % / 0.72 %;  6x9x300 q 200: 3.3 % / 3.3 %;
  7x5x40 q 32 (seed 721): 0.57 % / 0.57 %.
PARITY UNPINNED: the guide is OpenCV's convertTo, restated as (float)u8 * (float)(1 / 255.0).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref
import pyref_fif as F
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
FIF = 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def quantised(pair, q):
    return {k: (pair[k] // q * q).astype(np.uint8) for k in KEYS}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


@functools.lru_cache(maxsize=None)
def _case(H, W, D, q, idx):
    """The pair, both views' cost volumes and the twin's volumes of both forms (computed once)."""
    O = _oracle()
    pair = quantised(S.make_pair(H, W, D, idx), q)
    cfg = O.config(H, W, D - 1)
    cost = [O.cost_volume(pair, cfg, view=v) for v in (0, 1)]
    want = {(mode, v): F.fif(cost[v], pair[("lbgr", "rbgr")[v]], plain=bool(mode)) for mode in (0, 1) for v in (0, 1)}
    for a in cost + list(want.values()):
        a.setflags(write=False)
    return pair, cost, want


def _gpu_volumes(pair, H, W, D, mode, **over):
    """vm[0], vm[1] after sm_cost_calculate (do_refine = 1: both views are aggregated)."""
    lib = _capi.load()
    p = _capi.default_params(D - 1, H, W, aggregation=FIF, optimization=0, fif_mode=mode, do_refine=1, **over)
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        _capi.check(lib, ctx, lib.sm_set_images(ctx, _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3,
                                                _capi.ptr(a["lgray"]), _capi.ptr(a["rgray"]), W))
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx))
        out = []
        for view in (0, 1):
            got = np.empty((H, W, D), np.float32)
            _capi.check(lib, ctx, lib.sm_get_volume(ctx, view, _capi.ptr(got)))
            out.append(got)
        return out
    finally:
        lib.sm_destroy(ctx)


# H, W, D, q, seed.  The kernel layouts: D <= 16 / 32 / 64 four lines per wave with 1 / 2 / 4
# disparities per lane, D <= 128 / 256 / 512 / 1024 one line per wave with 2 / 4 / 8 / 16; dwordx4
# accesses where D % 4 == 0 and a lane holds a multiple of 4.
SHAPES = [(2, 2, 1, 1, 700),        # smallest image and D = 1
          (3, 5, 2, 1, 701),        # D = 2
          (24, 30, 8, 32, 702),
          (40, 61, 64, 64, 703),
          (33, 47, 70, 16, 704),
          (9, 70, 65, 1, 706),      # one past a wave
          (21, 19, 256, 128, 705),
          (5, 7, 1024, 200, 707),   # the D limit (q 64 falls under the 0.1 % condition: see above)
          (70, 3, 63, 32, 708),     # tall, thin
          (3, 130, 129, 32, 709),   # long rows, ragged D
          (6, 9, 300, 200, 710),    # 8 disparities per lane (256 < D <= 512), dwordx4
          (7, 5, 40, 32, 721)]      # four lines per wave, dwordx4, lanes past D


@pytest.mark.parametrize("H,W,D,q,idx", SHAPES)
def test_fif_volume_bits(H, W, D, q, idx):
    """Both forms, both views, as generated and quantised: uint32 equality with the twin."""
    for qq in sorted({1, q}):
        pair, _, want = _case(H, W, D, qq, idx)
        if qq > 1:
            for v in (0, 1):
                share = float((bits(want[0, v]) != bits(want[1, v])).mean())
                print(f"{H}x{W}x{D} q {qq} view {v}: the forms differ in {100 * share:.3f} % of the elements")
                assert share > 0.001
        for mode in (0, 1):
            got = _gpu_volumes(pair, H, W, D, mode)
            for v in (0, 1):
                np.testing.assert_array_equal(bits(got[v]), bits(want[mode, v]), err_msg=f"q {qq} mode {mode} view {v}")


@pytest.mark.parametrize("mode", [0, 1])
def test_fif_constant_guide(mode):
    """Constant colours: every weight is exactly 1, the sums grow the most (no decay at all)."""
    H, W, D = 12, 14, 16
    O = _oracle()
    pair = S.make_pair(H, W, D, 730)
    pair = {k: pair[k] for k in KEYS}
    pair["lbgr"] = np.full_like(pair["lbgr"], 93)
    pair["rbgr"] = np.full_like(pair["rbgr"], 93)
    wh, wv = F.weights(pair["lbgr"])
    assert (wh[:, :-1] == 1).all() and (wv[:-1] == 1).all()
    cfg = O.config(H, W, D - 1)
    got = _gpu_volumes(pair, H, W, D, mode)
    for v, img in ((0, "lbgr"), (1, "rbgr")):
        want = F.fif(O.cost_volume(pair, cfg, view=v), pair[img], plain=bool(mode))
        np.testing.assert_array_equal(bits(got[v]), bits(want))


def test_fif_constants_are_read():
    """fif_eps and fif_pn reach the kernels (a wider eps, a Pn of 0.5)."""
    H, W, D = 10, 13, 12
    pair, cost, _ = _case(H, W, D, 16, 731)
    got = _gpu_volumes(pair, H, W, D, 0, fif_eps=0.5, fif_pn=0.5)
    for v, img in ((0, "lbgr"), (1, "rbgr")):
        want = F.fif(cost[v], pair[img], eps=np.float32(0.5), pn=np.float32(0.5))
        np.testing.assert_array_equal(bits(got[v]), bits(want))


def _want_map(pair, H, W, D, mode=0, opt="sgm", paths=4, refine=False, q=1):
    """The twin's volume through pyref's SolveAll and optimiser (and refine())."""
    O = _oracle()
    cfg = O.config(H, W, D - 1)

    def view(v):
        img = pair[("lbgr", "rbgr")[v]]
        vm = pyref.solve_all(F.fif(O.cost_volume(pair, cfg, view=v), img, plain=bool(mode)))
        if opt == "sgm":
            return pyref.wta(pyref.sgm(vm, img, paths=paths))
        if opt == "so":
            return pyref.so(vm, pair["lbgr"])[1]   # so reads I_c[0] for both views (cpp:1098)
        return pyref.wta(vm)

    d0 = view(0)
    if refine:
        d0 = pyref.refine(d0, view(1), pyref.arms(pair["lbgr"]), pair["lbgr"], D)
    return d0


MAPS = [dict(H=30, W=44, D=24, optimization=0),                          # WTA
        dict(H=30, W=44, D=32, optimization=1, sgm_paths=4),
        dict(H=26, W=37, D=16, optimization=1, sgm_paths=8),
        dict(H=24, W=30, D=16, optimization=2),                          # so
        dict(H=21, W=30, D=160, optimization=1, sgm_paths=4),            # checkpointed SGM pairs on FIF output
        dict(H=19, W=26, D=160, optimization=1, sgm_paths=8, fif_mode=1),  # + the diagonal pair, plain form
        dict(H=30, W=44, D=24, optimization=1, sgm_paths=4, do_refine=1)]


@pytest.mark.parametrize("cfg", MAPS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_fif_maps(cfg):
    """sm_run (SolveAll fused into the last sweep's store) for n = 3 pairs: maps of the twin + pyref."""
    cfg = dict(cfg)
    H, W, D = cfg.pop("H"), cfg.pop("W"), cfg.pop("D")
    n = 3
    batch = S.make_batch(n, H, W, D, first_index=740)
    batch = {k: batch[k] // 32 * 32 for k in KEYS}
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation="FIF", **cfg)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
    finally:
        sb.close()
    opt = {0: "wta", 1: "sgm", 2: "so"}[cfg["optimization"]]
    for i in range(n):
        want = _want_map({k: batch[k][i] for k in KEYS}, H, W, D, mode=cfg.get("fif_mode", 0), opt=opt,
                         paths=cfg.get("sgm_paths", 4), refine=bool(cfg.get("do_refine")))
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")


@functools.lru_cache(maxsize=None)
def _schedule_case():
    H, W, D, n = 29, 41, 16, 5
    batch = S.make_batch(n, H, W, D, first_index=750)
    batch = {k: batch[k] // 32 * 32 for k in KEYS}
    want = [_want_map({k: batch[k][i] for k in KEYS}, H, W, D) for i in range(n)]
    return H, W, D, n, batch, want


@pytest.mark.parametrize("sub_batch,num_streams", [(2, 2), (1, 3), (2, 1)])
def test_fif_schedules(sub_batch, num_streams):
    """Groups of pairs on alternating streams: the scratch volumes and weight planes are per
    group, so two runs give the same maps, the twin's."""
    H, W, D, n, batch, want = _schedule_case()
    sb = StereoBatch(D - 1, H, W, n, device=0, aggregation=FIF, sub_batch=sub_batch, num_streams=num_streams)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        first = sb.run(0.3)
        second = sb.run(0.3)
    finally:
        sb.close()
    np.testing.assert_array_equal(second, first)
    for i in range(n):
        np.testing.assert_array_equal(first[i], want[i], err_msg=f"pair {i}")


@pytest.mark.parametrize("plain", [False, True])
def test_fif_reference_ordered_api(plain):
    """costCalculate -> SolveAll([sm], 1, 0.3) -> dispOptimize with the class selectors."""
    H, W, D = 28, 36, 20
    pair = quantised(S.make_pair(H, W, D, 760), 32)
    StereoMatching.aggregation, StereoMatching.FIF_PLAIN = "FIF", plain
    try:
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None,
                            StereoMatching.Parameters(D - 1, H, W), device=0)
        sm.costCalculate()
        vol = sm.vm[0]
        SolveAll([sm], 1, 0.3)
        got = sm.dispOptimize()
    finally:
        StereoMatching.aggregation, StereoMatching.FIF_PLAIN = "CBCA", False
    O = _oracle()
    want_vol = F.fif(O.cost_volume(pair, O.config(H, W, D - 1)), pair["lbgr"], plain=plain)
    np.testing.assert_array_equal(bits(vol), bits(want_vol))
    np.testing.assert_array_equal(got, _want_map(pair, H, W, D, mode=int(plain)))
