"""GPU parity of cross-based aggregation without arm intersection (sm_cbca_intersect_config(ctx, 0),
sm_cbca_ni.hip) against the restatement tests/pyref_cbca_ni.py and its fixtures tests/golden/cbca_ni/*.npz.

All comparisons are exact: volumes as f32 bit patterns, areas as int32, maps as int16.  The end-to-end
expectations are built on the GPU from code that is already pinned: a plain context takes the restatement's
volume(s) with sm_set_volume and runs sm_solve_all, sm_disp_optimize and sm_refine.
"""
import ctypes as C
import os

import numpy as np
import pytest

import pyref_cbca_ni as P
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi, pyrDown
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cbca_ni")
H, W, D = 40, 56, 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(name):
    f = dict(np.load(os.path.join(GOLDEN, f"cbca_ni_{name}.npz")))
    f["pair"] = {k: f[k] for k in KEYS}
    return f


class Ctx:
    """One pair through the reference-ordered C ABI; intersect None leaves the context as sm_create made it."""

    def __init__(self, pair, D, intersect=0, dw=None, **params):
        self.lib = _capi.load()
        self.H, self.W = pair["lgray"].shape
        self.D = D
        p = _capi.default_params(D - 1, self.H, self.W, **params)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(p), 0))
        if dw is not None:
            self.ok(self.lib.sm_cbca_double_config(self.ctx, 1, *dw))
        if intersect is not None:
            self.config(intersect)
        im = [np.ascontiguousarray(pair[k]) for k in KEYS]
        self.ok(self.lib.sm_set_images(self.ctx, _capi.ptr(im[0]), _capi.ptr(im[1]), self.W * 3, _capi.ptr(im[2]),
                                       _capi.ptr(im[3]), self.W))

    def ok(self, st):
        _capi.check(self.lib, self.ctx, st)

    def config(self, intersect):
        self.ok(self.lib.sm_cbca_intersect_config(self.ctx, intersect))

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

    def area(self, view=0):
        a = np.full((self.H, self.W), -1, np.int32)
        self.ok(self.lib.sm_get_cbca_area(self.ctx, view, _capi.ptr(a)))
        return a

    def area_status(self, view=0):
        a = np.empty((self.H, self.W), np.int32)
        return self.lib.sm_get_cbca_area(self.ctx, view, _capi.ptr(a))

    def arms(self, view=0):
        a = np.empty((self.H, self.W, 4), np.uint16)
        self.ok(self.lib.sm_get_arms(self.ctx, view, _capi.ptr(a)))
        return a

    def mask(self):
        m = np.full((self.H, self.W), 255, np.uint8)
        self.ok(self.lib.sm_get_cbca_dw_mask(self.ctx, _capi.ptr(m)))
        return m

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
    return load("main")


# ---- volumes and areas ----------------------------------------------------------------------------------

def test_fixture_both_views(fx):
    c = Ctx(fx["pair"], D, do_refine=1).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        np.testing.assert_array_equal(bits(c.volume(1)), bits(fx["vm1"]))
        np.testing.assert_array_equal(c.area(0), fx["area0"])
        np.testing.assert_array_equal(c.area(1), fx["area1"])
    finally:
        c.close()


def test_fixture_view0_only(fx):
    c = Ctx(fx["pair"], D, do_refine=0).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        np.testing.assert_array_equal(c.area(0), fx["area0"])
        assert c.area_status(1) == _capi.SM_EINVAL   # no second view without do_refine
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 3])
def test_iterations(fx, n):
    """Three iterations run V then H in the odd one."""
    c = Ctx(fx["pair"], D, cbca_iterations=n).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx[f"vm0_n{n}"]))
    finally:
        c.close()


def test_zero_iterations_leave_the_raw_costs(fx):
    off = Ctx(fx["pair"], D, cbca_iterations=0).cost()
    on = Ctx(fx["pair"], D, None, cbca_iterations=0).cost()
    try:
        raw = P.pieces(fx["pair"], D, views=1)[0][0]
        np.testing.assert_array_equal(bits(off.volume(0)), bits(on.volume(0)))
        np.testing.assert_array_equal(bits(off.volume(0)), bits(raw))
        assert off.area_status() == _capi.SM_ESTATE   # no iteration ran
    finally:
        off.close()
        on.close()


@pytest.mark.parametrize("params", [dict(fuse_cost_scan=0), dict(fuse_cost_scan=1), dict(fuse_norm_scan=0),
                                    dict(fuse_norm_scan=1), dict(fuse_cost_scan=0, fuse_norm_scan=1)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_volume_settings(fx, params):
    """The intersecting form's fused sweeps are not part of this path: the settings change nothing."""
    c = Ctx(fx["pair"], D, do_refine=1, optimization="sgm", **params).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        np.testing.assert_array_equal(bits(c.volume(1)), bits(fx["vm1"]))
        ref = Ctx(fx["pair"], D, do_refine=1, optimization="sgm").cost()
        try:
            np.testing.assert_array_equal(c.finish(True), ref.finish(True))
        finally:
            ref.close()
    finally:
        c.close()


def test_odd_shape():
    """23 x 37 x 13: neither D nor W * D is a multiple of 4 (one float per thread)."""
    f = load("odd")
    c = Ctx(f["pair"], 13, do_refine=1).cost()
    try:
        for v in (0, 1):
            np.testing.assert_array_equal(bits(c.volume(v)), bits(f[f"vm{v}"]))
            np.testing.assert_array_equal(c.area(v), f[f"area{v}"])
    finally:
        c.close()


def test_d_across_a_wave():
    """10 x 72 x 70: a pixel's disparities span more than one 64-lane chunk."""
    pair = P.make_input(10, 72, 70, 0)
    want = P.aggregate(pair, 70, 2, refine=False)
    c = Ctx(pair, 70).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(want["vm0"]))
        np.testing.assert_array_equal(c.area(0), want["area0"])
    finally:
        c.close()


def test_minimum_shape():
    """2 x 2 x 1 with arm_l = arm_l_out = 0 and no minimum arm: every region is one pixel and the output is the raw
    cost.  With the reference's minimum arm of 1 the arms reach the neighbour: the restatement on the device's
    arms."""
    bgr = np.array([[[10, 200, 30], [12, 198, 33]], [[11, 203, 29], [240, 5, 90]]], np.uint8)
    pair = {"lbgr": bgr, "rbgr": bgr[:, ::-1].copy()}
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    raw_c = Ctx(pair, 1, cbca_iterations=0, arm_l=0, arm_l_out=0, arm_min_l=0).cost()
    c = Ctx(pair, 1, arm_l=0, arm_l_out=0, arm_min_l=0).cost()
    m = Ctx(pair, 1, arm_l=0, arm_l_out=0).cost()
    try:
        raw = raw_c.volume(0)
        assert (c.arms(0) == 0).all()
        np.testing.assert_array_equal(bits(c.volume(0)), bits(raw))
        np.testing.assert_array_equal(c.area(0), np.ones((2, 2), np.int32))
        want, want_area = P.cbca_ni(raw, m.arms(0), 2)
        assert (m.arms(0) == 1).any()
        np.testing.assert_array_equal(bits(m.volume(0)), bits(want))
        np.testing.assert_array_equal(m.area(0), want_area)
    finally:
        raw_c.close()
        c.close()
        m.close()


def test_arms_longer_than_the_image():
    """A constant-colour pair with arm_l = arm_l_out = 84: every arm ends at the border, `inner` is false everywhere
    and every area is 16 * 24 after one iteration."""
    Hc, Wc, Dc = 16, 24, 8
    pair = {"lbgr": np.full((Hc, Wc, 3), 97, np.uint8), "rbgr": np.full((Hc, Wc, 3), 97, np.uint8),
            "lgray": np.full((Hc, Wc), 97, np.uint8), "rgray": np.full((Hc, Wc), 97, np.uint8)}
    win = dict(arm_L=84, arm_L_out=84, arm_cT=20, arm_cT_out=6)
    want = P.aggregate(pair, Dc, 1, win=win, refine=False)
    for inner in P.inner_masks(want["armsL"]):
        assert not inner.any()
    c = Ctx(pair, Dc, cbca_iterations=1, arm_l=84, arm_l_out=84).cost()
    try:
        np.testing.assert_array_equal(c.arms(0), want["armsL"])
        np.testing.assert_array_equal(c.area(0), np.full((Hc, Wc), Hc * Wc, np.int32))
        np.testing.assert_array_equal(bits(c.volume(0)), bits(want["vm0"]))
    finally:
        c.close()


def test_second_cost_string(fx):
    """"AD": costs that are not censusGrad's go through the cost volume kernel into the same aggregation."""
    want = P.aggregate(fx["pair"], D, 2, cost="AD")
    assert (bits(want["vm0"]) != bits(fx["vm0"])).any()
    c = Ctx(fx["pair"], D, cost_method="AD", do_refine=1).cost()
    try:
        np.testing.assert_array_equal(bits(c.volume(0)), bits(want["vm0"]))
        np.testing.assert_array_equal(bits(c.volume(1)), bits(want["vm1"]))
        np.testing.assert_array_equal(c.area(0), fx["area0"])   # the areas do not depend on the costs
    finally:
        c.close()


# ---- end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt,refine", [("sgm", 0), ("", 0), ("sgm", 1)], ids=["sgm", "wta", "sgm_refine"])
def test_end_to_end(fx, opt, refine):
    params = dict(optimization=opt, do_refine=refine, sgm_paths=4)
    plain = Ctx(fx["pair"], D, None, **params).cost()
    ni = Ctx(fx["pair"], D, 0, **params).cost()
    sb = StereoBatch(D - 1, H, W, 1, cbca_intersect=False, **params)
    try:
        got = ni.finish(refine)
        isect = plain.finish(refine)
        plain.cost()
        plain.set_volume(0, fx["vm0"])
        if refine:
            plain.set_volume(1, fx["vm1"])
        want = plain.finish(refine)
        np.testing.assert_array_equal(got, want)
        assert (got != isect).any()
        # sm_run (SolveAll's weight fused into the last normalising write) equals the staged calls
        sb.upload(*(fx["pair"][k][None] for k in KEYS))
        np.testing.assert_array_equal(sb.run(0.3)[0], got)
        np.testing.assert_array_equal(sb.get_cbca_area(0), fx["area0"])
    finally:
        plain.close()
        ni.close()
        sb.close()


def test_double_window_without_intersection(fx):
    """CBCA() sends both windows through the same cbca_core: both runs use the view's own arms of their window,
    two iterations each; the mask and the selection are the double window's."""
    dwf = dict(np.load(os.path.join(ROOT, "tests", "golden", "cbca_dw", "cbca_dw_main.npz")))
    for k in KEYS:
        np.testing.assert_array_equal(dwf[k], fx[k])
    want = P.double_window(fx["pair"], D, refine=True)
    np.testing.assert_array_equal(want["mask"], dwf["mask"])
    assert (bits(want["vm0"]) != bits(dwf["vm0"])).any() and (bits(want["vm0"]) != bits(fx["vm0"])).any()
    for extra in (dict(), dict(cbca_iterations=3)):   # (the double window's literal 2, whatever cbca_iterations says)
        c = Ctx(fx["pair"], D, 0, dw=DW_ARGS, do_refine=1, **extra).cost()
        try:
            np.testing.assert_array_equal(c.mask(), dwf["mask"])
            np.testing.assert_array_equal(bits(c.volume(0)), bits(want["vm0"]))
            np.testing.assert_array_equal(bits(c.volume(1)), bits(want["vm1"]))
            np.testing.assert_array_equal(c.area(0), fx["area0"])   # the last run is window 0's
        finally:
            c.close()


DW_ARGS = (23, 23, 30, 0, 5.0)


def _batch_inputs(n):
    pairs = [P.make_input(H, W, D, i) for i in range(n)]
    return pairs, [np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in KEYS]


@pytest.fixture(scope="module")
def alone_maps():
    pairs, _ = _batch_inputs(3)
    maps = []
    for p in pairs:
        sb = StereoBatch(D - 1, H, W, 1, cbca_intersect=False)
        try:
            sb.upload(*(p[k][None] for k in KEYS))
            maps.append(sb.run(0.3)[0].copy())
        finally:
            sb.close()
    assert (maps[0] != maps[1]).any() and (maps[1] != maps[2]).any()
    return maps


@pytest.mark.parametrize("sched", [dict(), dict(sub_batch=1, num_streams=2), dict(sub_batch=2, num_streams=1),
                                   dict(sub_batch=1, num_streams=3, fuse_cost_scan=0), dict(num_streams=4, sub_batch=1),
                                   dict(cap=8), dict(cap=8, fuse_cost_scan=0)],
                         ids=["default", "g1_s2", "g2_s1", "g1_s3_nofuse", "g1_s4", "pipelined", "pipelined_nofuse"])
def test_batch_of_three(alone_maps, sched):
    """Each map of the batch equals the map of the same pair run alone, under every schedule; a second run on the
    same context gives the same maps."""
    _, stacked = _batch_inputs(3)
    sched = dict(sched)
    sb = StereoBatch(D - 1, H, W, sched.pop("cap", 3), cbca_intersect=False, **sched)
    try:
        sb.upload(*stacked)
        for _ in range(2):
            got = sb.run(0.3)
            for i in range(3):
                np.testing.assert_array_equal(got[i], alone_maps[i], err_msg=f"pair {i}")
    finally:
        sb.close()


def test_switching(fx):
    plain = Ctx(fx["pair"], D, None).cost()
    c = Ctx(fx["pair"], D, 0).cost()
    try:
        isect_vol = plain.volume(0)
        isect = plain.finish()
        np.testing.assert_array_equal(bits(c.volume(0)), bits(fx["vm0"]))
        off = c.finish()
        assert (off != isect).any()
        c.config(1)
        assert c.area_status() == _capi.SM_ESTATE
        c.cost()
        assert c.area_status() == _capi.SM_ESTATE
        np.testing.assert_array_equal(bits(c.volume(0)), bits(isect_vol))
        np.testing.assert_array_equal(c.finish(), isect)
        c.config(0)
        np.testing.assert_array_equal(c.cost().finish(), off)
        np.testing.assert_array_equal(c.area(0), fx["area0"])
    finally:
        plain.close()
        c.close()


def test_profile_names(fx):
    """The kernels run under `_ni` names with algorithmic bytes (8 B per element each)."""
    sb = StereoBatch(D - 1, H, W, 1, cbca_intersect=False)
    try:
        sb.upload(*(fx["pair"][k][None] for k in KEYS))
        sb.profile(True)
        sb.run(0.3)
        sb.synchronize()
        stats = sb.profile_read()
    finally:
        sb.close()
    # two iterations: H, V (normalising), then V, H (normalising)
    ni = {n: s for n, s in stats.items() if n.endswith("_ni")}
    assert set(ni) == {"cbca_h_prefix_ni", "cbca_v_prefix_ni", "cbca_h_window_ni", "cbca_v_window_ni",
                       "cbca_h_window_norm_ni", "cbca_v_window_norm_ni"}
    assert "cost_volume" in stats and not any(n.startswith("cbca_") and n not in ni for n in stats)
    for n, s in ni.items():
        assert s["launches"] == (2 if "prefix" in n else 1) and s["bytes_per_launch"] == H * W * D * 8.0, (n, s)


def test_two_level_pyramid():
    """Each level aggregates its own volume before SolveAll (one context per level, arm limits divided by the
    level's scale): the levels' combined volume and map equal those of plain levels that were handed the
    restatement's volumes."""
    md, Hp, Wp = 23, 48, 70
    imgs = P.make_input(Hp, Wp, md + 1, 3)
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", "CBCA", "sgm"
    ni_levels, plain_levels = [], []
    sc = 1
    for lvl in range(2):
        h, w = imgs["lgray"].shape
        want = P.aggregate(imgs, md + 1, 2, refine=False,
                           win=dict(arm_L=17 // sc, arm_L_out=34 // sc, arm_cT=20, arm_cT_out=6))
        for off, levels in ((True, ni_levels), (False, plain_levels)):
            prm = StereoMatching.Parameters(md, h, w, 13, 1, 2, 109, 10, "", sc)
            prm.cbca_intersect = not off
            sm = StereoMatching(imgs["lbgr"], imgs["rbgr"], imgs["lgray"], imgs["rgray"], None, None, None, None, prm,
                                keep_final_volume=True)
            sm.costCalculate()
            if off:
                np.testing.assert_array_equal(bits(sm.vm[0]), bits(want["vm0"]), err_msg=f"level {lvl}")
            else:
                assert (bits(sm.vm[0]) != bits(want["vm0"])).any()
                vol = np.ascontiguousarray(want["vm0"])
                _capi.check(sm._lib, sm._ctx, sm._lib.sm_set_volume(sm._ctx, 0, _capi.ptr(vol)))
            levels.append(sm)
        md, sc = md // 2 + 1, sc * 2
        imgs = {k: pyrDown(imgs[k]) for k in KEYS}
    SolveAll(ni_levels, 2, 0.3)
    SolveAll(plain_levels, 2, 0.3)
    np.testing.assert_array_equal(bits(ni_levels[0].vm[0]), bits(plain_levels[0].vm[0]))
    np.testing.assert_array_equal(ni_levels[0].dispOptimize(), plain_levels[0].dispOptimize())
