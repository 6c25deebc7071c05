"""GPU parity of CBCA()'s double-window branch (sm_cbca_dw.hip and the second aggregation run) against the
restatement tests/pyref_cbca_dw.py and its fixtures tests/golden/cbca_dw/*.npz.

All comparisons are exact: masks as bytes, volumes as f32 bit patterns, maps as int16.  The end-to-end
expectations are built on the GPU from code that is already pinned: a plain single-window context takes the
composed volume(s) with sm_set_volume and runs sm_solve_all, sm_disp_optimize and sm_refine.
"""
import ctypes as C
import os

import numpy as np
import pytest

import pyref_cbca_dw as P
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi, pyrDown

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cbca_dw")
H, W, D = 40, 56, 16
DW = (23, 23, 30, 0, 5.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"cbca_dw_{name}.npz")))


class Ctx:
    """One pair through the reference-ordered C ABI."""

    def __init__(self, pair, D, dw=None, **params):
        self.lib = _capi.load()
        self.H, self.W = pair["lgray"].shape
        self.D = D
        p = _capi.default_params(D - 1, self.H, self.W, **params)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(p), 0))
        if dw is not None:
            self.config(1, *dw)
        im = [np.ascontiguousarray(pair[k]) for k in KEYS]
        self.ok(self.lib.sm_set_images(self.ctx, _capi.ptr(im[0]), _capi.ptr(im[1]), self.W * 3, _capi.ptr(im[2]),
                                       _capi.ptr(im[3]), self.W))

    def ok(self, st):
        _capi.check(self.lib, self.ctx, st)

    def config(self, *args):
        self.ok(self.lib.sm_cbca_double_config(self.ctx, *args))

    def cost(self):
        self.ok(self.lib.sm_cost_calculate(self.ctx))
        return self

    def volume(self, view=0):
        a = np.empty((self.H, self.W, self.D), np.float32)
        self.ok(self.lib.sm_get_volume(self.ctx, view, _capi.ptr(a)))
        return a

    def set_volume(self, view, vol):
        vol = np.ascontiguousarray(vol, np.float32)
        self.ok(self.lib.sm_set_volume(self.ctx, view, _capi.ptr(vol)))

    def mask(self):
        m = np.full((self.H, self.W), 255, np.uint8)
        self.ok(self.lib.sm_get_cbca_dw_mask(self.ctx, _capi.ptr(m)))
        return m

    def arms(self, view=0):
        a = np.empty((self.H, self.W, 4), np.uint16)
        self.ok(self.lib.sm_get_arms(self.ctx, view, _capi.ptr(a)))
        return a

    def finish(self, refine=False):
        """sm_solve_all -> sm_disp_optimize [-> sm_refine] on the volumes the context holds."""
        self.ok(self.lib.sm_solve_all(self.ctx, 1, 0.3))
        dp = np.empty((self.H, self.W), np.int16)
        self.ok(self.lib.sm_disp_optimize(self.ctx, _capi.ptr(dp)))
        if refine:
            self.ok(self.lib.sm_refine(self.ctx, _capi.ptr(dp)))
        return dp

    def close(self):
        self.lib.sm_destroy(self.ctx)


@pytest.fixture(scope="module")
def fx():
    f = load("main")
    f["pair"] = {k: f[k] for k in KEYS}
    return f


@pytest.fixture(scope="module")
def dw_volumes(fx):
    """The double-window context's mask and volumes of the fixture pair (do_refine: both views), computed once."""
    c = Ctx(fx["pair"], D, DW, do_refine=1).cost()
    try:
        return c.mask(), c.volume(0), c.volume(1), c.arms(0)
    finally:
        c.close()


# ---- mask and volumes ---------------------------------------------------------------------------------

def test_mask(fx, dw_volumes):
    mask = dw_volumes[0]
    s = P.nine_sum(P.arm_max(fx["arms"]))
    assert (s == 44).any() and (s == 45).any()
    np.testing.assert_array_equal(mask[s == 44], 1)
    np.testing.assert_array_equal(mask[s == 45], 0)
    for edge in (np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1]):
        np.testing.assert_array_equal(mask[edge], fx["mask"][edge])
    np.testing.assert_array_equal(mask, fx["mask"])


def test_arms_afterwards_are_window_0(fx, dw_volumes):
    np.testing.assert_array_equal(dw_volumes[3], fx["arms"])


def test_volumes_both_views(fx, dw_volumes):
    """View 1 is composed with the LEFT mask."""
    np.testing.assert_array_equal(bits(dw_volumes[1]), bits(fx["vm0"]))
    np.testing.assert_array_equal(bits(dw_volumes[2]), bits(fx["vm1"]))


def test_volume_view0_only(fx):
    c = Ctx(fx["pair"], D, DW).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        np.testing.assert_array_equal(c.mask(), fx["mask"])
    finally:
        c.close()


@pytest.mark.parametrize("params", [dict(fuse_cost_scan=0), dict(fuse_cost_scan=1), dict(fuse_norm_scan=0),
                                    dict(fuse_norm_scan=1), dict(fuse_cost_scan=0, fuse_norm_scan=1),
                                    dict(cbca_iterations=1), dict(cbca_iterations=0), dict(cbca_iterations=3)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_volume_settings(fx, params):
    """The kernels' two ways to the raw costs and the fused sweeps give the same volumes; cbca_iterations is not
    read in this branch (cbca_core(.., 2))."""
    c = Ctx(fx["pair"], D, DW, do_refine=1, **params).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        np.testing.assert_array_equal(bits(c.volume(1)), bits(fx["vm1"]))
    finally:
        c.close()


def test_window_and_threshold_arguments(fx):
    """Another window 1 (longer than window 0) and other thresholds go through the same restatement."""
    win1 = dict(arm_L=9, arm_L_out=40, arm_cT=25, arm_cT_out=3)
    for thres in (5.0, 7.3, float(np.nextafter(np.float32(5), np.float32(6)))):
        want = P.compose(fx["pair"], D, refine=False, thres=thres, win1=win1)
        c = Ctx(fx["pair"], D, (9, 40, 25, 3, thres)).cost()
        try:
            np.testing.assert_array_equal(c.mask(), want["mask"], err_msg=str(thres))
            np.testing.assert_array_equal(bits(c.volume(0)), bits(want["vm0"]), err_msg=str(thres))
        finally:
            c.close()


def test_scalar_tail_shape():
    """23 x 37 x 13: neither D nor W * D is a multiple of 4 (the selection's scalar head and tail pieces)."""
    f = load("odd")
    pair = {k: f[k] for k in KEYS}
    for refine in (0, 1):
        c = Ctx(pair, 13, DW, do_refine=refine).cost()
        try:
            np.testing.assert_array_equal(c.mask(), f["mask"])
            np.testing.assert_array_equal(bits(c.volume(0)), bits(f["vm0"]))
            if refine:
                want = P.compose(pair, 13, refine=True)
                np.testing.assert_array_equal(bits(c.volume(1)), bits(want["vm1"]))
        finally:
            c.close()


# ---- end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt,refine", [("sgm", 0), ("", 0), ("sgm", 1)], ids=["sgm", "wta", "sgm_refine"])
def test_end_to_end(fx, opt, refine):
    params = dict(optimization=opt, do_refine=refine, sgm_paths=4)
    plain = Ctx(fx["pair"], D, None, **params).cost()
    dw = Ctx(fx["pair"], D, DW, **params).cost()
    try:
        got = dw.finish(refine)
        single = plain.finish(refine)
        plain.cost()
        plain.set_volume(0, fx["vm0"])
        if refine:
            plain.set_volume(1, fx["vm1"])
        want = plain.finish(refine)
        np.testing.assert_array_equal(got, want)
        assert (got != single).any()
    finally:
        plain.close()
        dw.close()


def _batch_inputs(n):
    pairs = [P.make_input(H, W, D, i) for i in range(n)]
    return pairs, [np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in KEYS]


@pytest.fixture(scope="module")
def alone_maps():
    pairs, _ = _batch_inputs(3)
    maps, masks = [], []
    for p in pairs:
        sb = StereoBatch(D - 1, H, W, 1, cbca_double_win=True)
        try:
            sb.upload(*(p[k][None] for k in KEYS))
            maps.append(sb.run(0.3)[0].copy())
            masks.append(sb.get_cbca_dw_mask())
        finally:
            sb.close()
    return maps, masks


@pytest.mark.parametrize("sched", [dict(), dict(sub_batch=1, num_streams=2), dict(sub_batch=2, num_streams=1),
                                   dict(sub_batch=1, num_streams=3, fuse_cost_scan=0), dict(num_streams=4, sub_batch=1),
                                   dict(cap=8), dict(cap=8, fuse_cost_scan=0)],
                         ids=["default", "g1_s2", "g2_s1", "g1_s3_nofuse", "g1_s4", "pipelined", "pipelined_nofuse"])
def test_batch_of_three(alone_maps, sched):
    """Every pair gets its own mask: each map of the batch equals the map of the same pair run alone, under every
    schedule."""
    maps, masks = alone_maps
    pairs, stacked = _batch_inputs(3)
    for i, p in enumerate(pairs):   # the masks differ from pair to pair and are the restatement's
        np.testing.assert_array_equal(masks[i], P.compose(p, D, refine=False)["mask"])
    assert (masks[0] != masks[1]).any() and (masks[1] != masks[2]).any()
    sched = dict(sched)
    # (capacity 8 with 4-path SGM: the automatic two-group schedule, pipelined across calls)
    sb = StereoBatch(D - 1, H, W, sched.pop("cap", 3), cbca_double_win=True, **sched)
    try:
        sb.upload(*stacked)
        for _ in range(2):   # (a second run on the same context: the buffers are reused)
            got = sb.run(0.3)
            for i in range(3):
                np.testing.assert_array_equal(got[i], maps[i], err_msg=f"pair {i}")
        np.testing.assert_array_equal(sb.get_cbca_dw_mask(), masks[0])
    finally:
        sb.close()


def test_sm_run_equals_staged_calls(fx, alone_maps):
    """SolveAll's weight fused into both runs' last pass (sm_run) equals compose, then scale (the staged calls)."""
    c = Ctx(fx["pair"], D, DW).cost()
    try:
        np.testing.assert_array_equal(c.finish(), alone_maps[0][0])
    finally:
        c.close()


def test_enable_off_again(fx):
    plain = Ctx(fx["pair"], D, None).cost()
    c = Ctx(fx["pair"], D, DW).cost()
    try:
        single = plain.finish()
        on = c.finish()
        assert (on != single).any()
        c.config(0, *DW)
        with pytest.raises(_capi.SMError):
            c.cost().mask()
        np.testing.assert_array_equal(c.finish(), single)
        c.config(1, *DW)
        np.testing.assert_array_equal(c.cost().finish(), on)
    finally:
        plain.close()
        c.close()


def test_two_level_pyramid():
    """Each level composes its own volume before SolveAll (costCalculate per level): the double-window levels'
    combined volume and map equal those of plain levels that were handed the restatement's composed volumes."""
    md, Hp, Wp = 23, 48, 70
    imgs = P.make_input(Hp, Wp, md + 1, 3)
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", "CBCA", "sgm"
    dw_levels, plain_levels = [], []
    sc = 1
    for lvl in range(2):
        h, w = imgs["lgray"].shape
        want = P.compose(imgs, md + 1, refine=False,
                         win0=dict(arm_L=17 // sc, arm_L_out=34 // sc, arm_cT=20, arm_cT_out=6),
                         win1=dict(arm_L=23 // sc, arm_L_out=23 // sc, arm_cT=30, arm_cT_out=0))
        assert 0 < want["mask"].mean() < 1
        for dw, levels in ((True, dw_levels), (False, plain_levels)):
            prm = StereoMatching.Parameters(md, h, w, 13, 1, 2, 109, 10, "", sc)
            prm.cbca_double_win = dw
            sm = StereoMatching(imgs["lbgr"], imgs["rbgr"], imgs["lgray"], imgs["rgray"], None, None, None, None, prm,
                                keep_final_volume=True)
            sm.costCalculate()
            if dw:
                np.testing.assert_array_equal(bits(sm.vm[0]), bits(want["vm0"]), err_msg=f"level {lvl}")
            else:
                vol = np.ascontiguousarray(want["vm0"])
                _capi.check(sm._lib, sm._ctx, sm._lib.sm_set_volume(sm._ctx, 0, _capi.ptr(vol)))
            levels.append(sm)
        md, sc = md // 2 + 1, sc * 2
        imgs = {k: pyrDown(imgs[k]) for k in KEYS}
    SolveAll(dw_levels, 2, 0.3)
    SolveAll(plain_levels, 2, 0.3)
    np.testing.assert_array_equal(bits(dw_levels[0].vm[0]), bits(plain_levels[0].vm[0]))
    np.testing.assert_array_equal(dw_levels[0].dispOptimize(), plain_levels[0].dispOptimize())
