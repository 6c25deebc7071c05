"""GPU parity of refine()'s peak-ratio check, background fill and sub-pixel map (sm_refine_ext.hip) against the
restatement tests/pyref_refine_ext.py.

All comparisons are exact: maps as int16, mask bytes, float maps as f32 bit patterns.  The single stages run on
crafted volumes and maps (sm_set_volume / sm_set_disp under optimization "", every other stage off, LRmaxDiff
huge and DP[1] = 0 so that the LR check only turns negative values and d > u into -1); the pipeline cases compare
with the restatement composed with the C oracle's stages, on the oracle's own volume and maps.

BGIpol's width 1 of the issue's list is covered on the host only (tests/test_refine_ext_host.py): sm_create refuses
cols < 2.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref_refine_ext as R
from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


class Ctx:
    """One pair through the reference-ordered C ABI.  crafted=True: optimization "" on AD costs without
    aggregation, refine()'s four existing stages reduced to the LR check with LRmaxDiff = 1e9."""

    def __init__(self, H, W, D, pair=None, crafted=True, **over):
        self.lib = _capi.load()
        self.H, self.W, self.D = H, W, D
        if crafted:
            over = dict(dict(cost_method="AD", aggregation=0, optimization=0, lr_max_diff=1e9, do_region_vote=0,
                             do_proper_ipol=0, do_last_median_blur=0), **over)
        p = _capi.default_params(D - 1, H, W, do_refine=1, **over)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(p), 0))
        if pair is None:
            z = np.zeros((H, W, 3), np.uint8)
            pair = dict(lbgr=z, rbgr=z, lgray=z[:, :, 0].copy(), rgray=z[:, :, 0].copy())
        a = [np.ascontiguousarray(pair[k]) for k in KEYS]
        self.ok(self.lib.sm_set_images(self.ctx, _capi.ptr(a[0]), _capi.ptr(a[1]), W * 3, _capi.ptr(a[2]), _capi.ptr(a[3]), W))
        self.ok(self.lib.sm_cost_calculate(self.ctx))

    def ok(self, st):
        _capi.check(self.lib, self.ctx, st)

    def config(self, do_pkr=False, ratio=0.1, disp_pkr=-64, do_bg=False, depth=1000, do_se=False, mode=0):
        self.ok(self.lib.sm_refine_ext_config(self.ctx, int(do_pkr), float(ratio), disp_pkr, int(do_bg), depth, int(do_se), mode))

    def set_volume(self, vol):
        vol = np.ascontiguousarray(vol, np.float32)
        assert vol.shape == (self.H, self.W, self.D)
        self.ok(self.lib.sm_set_volume(self.ctx, 0, _capi.ptr(vol)))

    def optimize(self, reg_lambda=None):
        if reg_lambda is not None:
            self.ok(self.lib.sm_solve_all(self.ctx, 1, reg_lambda))
        self.ok(self.lib.sm_disp_optimize(self.ctx, None))

    def set_disp(self, d0, d1=None):
        for view, m in ((0, d0), (1, d1)):
            if m is not None:
                self.ok(self.lib.sm_set_disp(self.ctx, view, _capi.ptr(np.ascontiguousarray(m, np.int16))))

    def get_disp(self, view):
        out = np.empty((self.H, self.W), np.int16)
        self.ok(self.lib.sm_get_disp(self.ctx, view, _capi.ptr(out)))
        return out

    def volume(self):
        out = np.empty((self.H, self.W, self.D), np.float32)
        self.ok(self.lib.sm_get_volume(self.ctx, 0, _capi.ptr(out)))
        return out

    def refine(self):
        dp = np.empty((self.H, self.W), np.int16)
        self.ok(self.lib.sm_refine(self.ctx, _capi.ptr(dp)))
        return dp

    def mask(self):
        out = np.full((self.H, self.W), 255, np.uint8)
        self.ok(self.lib.sm_get_pkr_mask(self.ctx, _capi.ptr(out)))
        return out

    def se(self):
        out = np.full((self.H, self.W), np.nan, np.float32)
        self.ok(self.lib.sm_get_subpixel(self.ctx, _capi.ptr(out)))
        return out

    def close(self):
        self.lib.sm_destroy(self.ctx)


def _lr_only(d0):
    """What the crafted contexts' LR check leaves of d0 (DP[1] = 0, LRmaxDiff = 1e9): d < 0 or u - d < 0 -> -1."""
    O = _oracle()
    H, W = d0.shape
    cfg = O.config(H, W, 15, do_refine=1, lr_max_diff=1e9)
    return O.lr_check(d0, np.zeros((H, W), np.int16), cfg)


def _map(rng, H, W, dmax, hole_rate, holes=(-1, -32)):
    """Valid values <= u (they survive the LR check) with holes at the given rate."""
    d = np.minimum(rng.integers(0, dmax + 1, (H, W)), np.arange(W)[None, :]).astype(np.int16)
    h = rng.random((H, W)) < hole_rate
    d[h] = rng.choice(np.array(holes, np.int16), size=int(h.sum()))
    return d


# ---- PKR ---------------------------------------------------------------------------------------------

def _pkr_volume(rng, H, W, D):
    """Costs in [4, 8) with the two smallest of every pixel set from a list of (c0, c1) cases placed at random
    disparities: ratios on both sides of 0.1, duplicated minima, c1 == 0 with c0 == 0 and c0 < 0, a negative pair."""
    vol = (rng.random((H, W, D)) * 4 + 4).astype(f32)
    one = f32(1)
    cases = [(one, one), (f32(0.9), one), (np.nextafter(f32(0.9), f32(2)), one), (f32(0.95), one), (f32(0.5), one),
             (f32(0), f32(0)), (f32(-1), f32(0)), (f32(0), f32(3)), (f32(-2), f32(-1.9)), (f32(2), f32(2.1)),
             (f32(1.9), f32(2.2)), (f32(3), f32(3.3)), (f32(3), np.nextafter(f32(3.3), f32(0))), (f32(1e-30), f32(1.05e-30))]
    pick = rng.integers(0, len(cases), (H, W))
    for v in range(H):
        for u in range(W):
            c0, c1 = cases[pick[v, u]]
            a, b = rng.choice(D, 2, replace=False)
            vol[v, u, a], vol[v, u, b] = c0, c1
    if D >= 4:   # a triple minimum and minima in the first and last slot
        vol[0, 0, :3] = 2
        vol[0, 1, 0], vol[0, 1, D - 1] = 1, 1.05
        # c0 < 0 over zeros of both signs: the ratio is -inf (marked) or +inf by the FIRST zero in d order
        for u, (za, zb) in ((2, (-0.0, 0.0)), (3, (0.0, -0.0))):
            vol[0, u] = 5
            vol[0, u, 1], vol[0, u, D - 2], vol[0, u, D - 1] = za, zb, -1
    return vol, pick


@pytest.mark.parametrize("D", [2, 13, 60, 64, 65, 130, 260])
def test_pkr(D):
    H, W = 24, 40
    rng = np.random.default_rng(7 * D)
    vol, pick = _pkr_volume(rng, H, W, D)
    d0 = _map(rng, H, W, D - 1, 0.2)
    want_mask = R.cal_pkr(vol)
    frac = want_mask.mean()
    assert 0.05 < frac < 0.95, frac
    if D >= 4:
        assert want_mask[0, 2] == 1 and want_mask[0, 3] == 0
    below = np.arange(H)[:, None] * np.ones(W, int)[None, :] > 0   # (row 0 holds the extra pixels)
    assert want_mask[below & (pick == 0)].all()                                                   # duplicated minima
    assert not want_mask[below & (pick == 5)].any() and not want_mask[below & (pick == 6)].any()   # c1 == 0
    post = _lr_only(d0)
    want = R.sign_dp(post, want_mask)
    c = Ctx(H, W, D)
    try:
        with pytest.raises(_capi.SMError):   # no mask before a refine with the stage on
            c.mask()
        c.set_volume(vol)
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        c.config(do_pkr=True)
        got = c.refine()
        mask = c.mask()
        np.testing.assert_array_equal(mask, want_mask)
        np.testing.assert_array_equal(got, want)
        assert (got[post < 0] == post[post < 0]).all() and (got == -64).any()   # holes stay, marks exist
        np.testing.assert_array_equal(bits(c.volume()), bits(vol))              # calPKR works on a clone
        # another ratio and mark value
        c.set_disp(d0)
        c.config(do_pkr=True, ratio=0.5, disp_pkr=-7)
        got = c.refine()
        m2 = R.cal_pkr(vol, f32(0.5))
        np.testing.assert_array_equal(c.mask(), m2)
        np.testing.assert_array_equal(got, R.sign_dp(post, m2, -7))
        # off again: the LR check alone, and no mask
        c.set_disp(d0)
        c.config()
        np.testing.assert_array_equal(c.refine(), post)
        with pytest.raises(_capi.SMError):
            c.mask()
    finally:
        c.close()


# ---- BGIpol ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [2, 63, 64, 65, 130, 200])
def test_bg_ipol(W):
    """Rows with 10 %, 60 % and 100 % holes at depths 0, 1, 3 and 1000."""
    H = 9
    rng = np.random.default_rng(W)
    d0 = np.concatenate([_map(rng, 3, W, 50, r, holes=(-1,)) for r in (0.1, 0.6, 1.0)])
    if W > 2:
        d0[0, 0], d0[1, W - 1], d0[3, :2], d0[4, W - 2:] = -1, -1, -1, -1   # holes at both borders
    post = _lr_only(d0)
    c = Ctx(H, W, 64)
    try:
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        for depth in (0, 1, 3, 1000):
            c.set_disp(d0)
            c.config(do_bg=True, depth=depth)
            got = c.refine()
            want = R.bg_ipol(post, depth)
            np.testing.assert_array_equal(got, want, err_msg=f"depth {depth}")
            if depth == 0:
                np.testing.assert_array_equal(got, post)
            if depth == 3 and W > 2:
                assert ((want >= 0) & (post < 0)).any() and (want < 0).any()
            assert (want[6:] < 0).all()   # rows of holes stay
    finally:
        c.close()


def test_bg_ipol_keeps_marks_and_batch_of_three():
    """A batch of three pairs with different maps (the LR check's own holes), depth 3; and PKR's marks, which
    BGIpol fills like any hole or leaves as they are."""
    O = _oracle()
    H, W, md, n = 30, 75, 15, 3
    batch = S.make_batch(n, H, W, md + 1, first_index=610)
    kw = dict(do_refine=1, do_region_vote=0, do_proper_ipol=0, do_last_median_blur=0)
    sb = StereoBatch(md, H, W, n, device=0, **kw)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        base = sb.run(0.3)
        sb.refine_ext_config(do_bg_ipol=True, bg_ipl_depth=3)
        filled = sb.run(0.3)
        sb.refine_ext_config(do_pkr=True, do_bg_ipol=True, bg_ipl_depth=2)
        both = sb.run(0.3)
        sb.refine_ext_config(do_pkr=True)
        marked = sb.run(0.3)
    finally:
        sb.close()
    assert (base[0] != base[1]).any() and (base[1] != base[2]).any()
    cfg = O.config(H, W, md, do_refine=1, do_region_vote=0, do_proper_ipol=0, do_last_median=0)
    for i in range(n):
        pair = {k: batch[k][i] for k in KEYS}
        np.testing.assert_array_equal(base[i], O.run_ex(pair, cfg)["disp"])
        want = R.bg_ipol(base[i], 3)
        np.testing.assert_array_equal(filled[i], want, err_msg=f"pair {i}")
        assert ((want >= 0) & (base[i] < 0)).any() and (want < 0).any()
        assert (marked[i] == -64).any()
        np.testing.assert_array_equal(both[i], R.bg_ipol(marked[i], 2), err_msg=f"pair {i}")


# ---- SE ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,W", [(3, 40), (16, 41), (65, 70)])
@pytest.mark.parametrize("mode", [R.SE_REFERENCE, R.SE_FLOAT])
def test_subpixel(D, W, mode):
    H = 24
    rng = np.random.default_rng(D + mode)
    vol = (rng.random((H, W, D)) * 3).astype(f32)
    vol[::3, ::2] = np.round(vol[::3, ::2] * 2) / 2   # halves: denom == 0 and diff == +-1 occur
    d0 = _map(rng, H, W, D - 1, 0.15)
    d0[:, D - 1:: 5] = D - 1
    d0[1::4, 3::4] = 0
    d0[2, :] = np.minimum(1, np.arange(W))          # whole border rows / columns of parabola pixels where D allows
    post = _lr_only(d0)
    assert (post == 0).any() and (post == D - 1).any() and (post < 0).any()
    raw = R.subpixel(post, vol, mode)
    want = R.median3_f32(raw)
    if D > 3:
        assert (raw != post).any() and (want != raw).any()
    c = Ctx(H, W, D)
    try:
        with pytest.raises(_capi.SMError):
            c.se()
        c.set_volume(vol)
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        c.config(do_se=True, mode=mode)
        got_dp = c.refine()
        got = c.se()
        np.testing.assert_array_equal(got_dp, post)   # DP[0] is not changed by the stage
        for name, sl in (("top", np.s_[0, :]), ("bottom", np.s_[H - 1, :]), ("left", np.s_[:, 0]), ("right", np.s_[:, W - 1])):
            np.testing.assert_array_equal(bits(got[sl]), bits(want[sl]), err_msg=name)
        np.testing.assert_array_equal(bits(got), bits(want))
        if mode == R.SE_REFERENCE:
            assert (got == np.trunc(got)).all()
    finally:
        c.close()


# ---- whole pipeline ------------------------------------------------------------------------------------

ALL_ON = dict(do_pkr=True, do_bg_ipol=True, do_subpixel=True)


def _expect(ctx, pair, mode=R.SE_REFERENCE, **cfg_kw):
    """The restatement composed with the oracle's stages, on the maps and the volume the context holds after
    sm_disp_optimize."""
    O = _oracle()
    cfg = O.config(ctx.H, ctx.W, ctx.D - 1, do_refine=1, **cfg_kw)
    d0, d1, vm = ctx.get_disp(0), ctx.get_disp(1), ctx.volume()
    return d0, d1, vm, R.refine_ext(O, cfg, d0, d1, O.arms(pair["lbgr"], cfg), pair["lbgr"], vm, do_pkr=True, do_bg=True,
                                    do_se=True, mode=mode)


@pytest.mark.parametrize("D,idx", [(16, 620), (64, 621)])
def test_pipeline_against_oracle(D, idx):
    """censusGrad + CBCA + sgm, all three stages on: the staged calls against pyref o oracle (the oracle's own
    path sum and maps), and sm_run against the staged calls, both SE forms."""
    O = _oracle()
    H, W = 40, 60
    pair = S.make_pair(H, W, D, idx)
    cfg = O.config(H, W, D - 1, do_refine=1)
    ref = O.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
    c = Ctx(H, W, D, pair, crafted=False)
    try:
        c.config(do_pkr=True, do_bg=True, do_se=True)
        c.optimize(0.3)
        d0, d1, vm, want = _expect(c, pair)
        np.testing.assert_array_equal(d0, ref["disp_raw"])
        np.testing.assert_array_equal(d1, ref["disp_right"])
        np.testing.assert_array_equal(bits(vm), bits(ref["final"]))   # SGM kept its path sum for the stages
        got = c.refine()
        np.testing.assert_array_equal(got, want["disp"])
        np.testing.assert_array_equal(c.mask(), want["mask"])
        np.testing.assert_array_equal(bits(c.se()), bits(want["se"]))
        assert 0 < want["mask"].mean() < 1 and (got != ref["disp"]).any() and (got >= 0).all()   # BGIpol leaves no hole here
    finally:
        c.close()
    for mode in (R.SE_REFERENCE, R.SE_FLOAT):
        sb = StereoBatch(D - 1, H, W, 1, device=0, do_refine=1, refine_ext=dict(ALL_ON, se_mode=mode))
        try:
            sb.upload(*(pair[k][None] for k in KEYS))
            run = sb.run(0.3)[0]
            np.testing.assert_array_equal(run, want["disp"])
            np.testing.assert_array_equal(sb.get_pkr_mask(), want["mask"])
            se = sb.download_subpixel()[0]
            if mode == R.SE_REFERENCE:
                np.testing.assert_array_equal(bits(se), bits(want["se"]))
            else:
                w2 = R.refine_ext(O, cfg, d0, d1, O.arms(pair["lbgr"], cfg), pair["lbgr"], vm, do_pkr=True, do_bg=True,
                                  do_se=True, mode=mode)
                np.testing.assert_array_equal(bits(se), bits(w2["se"]))
                assert (se != np.trunc(se)).any()
        finally:
            sb.close()


@pytest.mark.parametrize("name,over", [("wta", dict(optimization=0)), ("paths8", dict(sgm_paths=8)), ("vmtop", dict())])
def test_pipeline_variants(name, over):
    """optimization "", 8 paths and vmTop: the stages run on whatever maps and volume dispOptimize leaves."""
    H, W, D = 40, 60, 16
    pair = S.make_pair(H, W, D, 622)
    c = Ctx(H, W, D, pair, crafted=False, **over)
    try:
        if name == "vmtop":
            c.ok(c.lib.sm_vmtop_config(c.ctx, 1, 0, 3, float(f32(1.09)), 10, 1, 0))
        c.config(do_pkr=True, do_bg=True, do_se=True)
        c.optimize(0.3)
        _, _, _, want = _expect(c, pair)
        got = c.refine()
        np.testing.assert_array_equal(got, want["disp"])
        np.testing.assert_array_equal(c.mask(), want["mask"])
        np.testing.assert_array_equal(bits(c.se()), bits(want["se"]))
    finally:
        c.close()
    sb = StereoBatch(D - 1, H, W, 1, device=0, do_refine=1, refine_ext=ALL_ON, **over)
    try:
        if name == "vmtop":
            sb.vmtop_config(True, 0, 3, float(f32(1.09)), 10, True, False)
        sb.upload(*(pair[k][None] for k in KEYS))
        np.testing.assert_array_equal(sb.run(0.3)[0], want["disp"])
        np.testing.assert_array_equal(bits(sb.download_subpixel()[0]), bits(want["se"]))
    finally:
        sb.close()


@functools.lru_cache(maxsize=None)
def _three(H, W, D, first):
    """Three pairs and their expected outputs (single-pair staged contexts + the restatement)."""
    batch = S.make_batch(3, H, W, D, first_index=first)
    want = []
    for i in range(3):
        pair = {k: batch[k][i] for k in KEYS}
        c = Ctx(H, W, D, pair, crafted=False)
        try:
            c.config(do_pkr=True, do_bg=True, do_se=True)
            c.optimize(0.3)
            want.append(_expect(c, pair)[3])
        finally:
            c.close()
    return batch, want


@pytest.mark.parametrize("sub_batch,num_streams", [(0, 1), (1, 2), (2, 3), (1, 4), (2, 0)])
def test_schedules(sub_batch, num_streams):
    H, W, D = 40, 60, 16
    batch, want = _three(H, W, D, 630)
    sb = StereoBatch(D - 1, H, W, 3, device=0, do_refine=1, sub_batch=sub_batch, num_streams=num_streams, refine_ext=ALL_ON)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
        se = sb.download_subpixel()
        again = sb.run(0.3)
        np.testing.assert_array_equal(again, got)
        np.testing.assert_array_equal(sb.get_pkr_mask(), want[0]["mask"])
    finally:
        sb.close()
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i]["disp"], err_msg=f"pair {i}")
        np.testing.assert_array_equal(bits(se[i]), bits(want[i]["se"]), err_msg=f"pair {i}")


def test_compute_function_hands_the_override_on():
    """DistributedBatchRunner's compute function: refine_ext travels with the other overrides, and the block's float
    maps can be fetched from it."""
    from mystereomatching_amd.batch import hip_compute_fn
    H, W, D = 40, 60, 16
    batch, want = _three(H, W, D, 630)
    fn = hip_compute_fn(D - 1, H, W, 3, 0, do_refine=1, refine_ext=dict(ALL_ON, se_mode=R.SE_REFERENCE))
    try:
        got = fn({k: batch[k] for k in KEYS}, 0.3)
        se = fn.download_subpixel()
    finally:
        fn.close()
    for i in range(3):
        np.testing.assert_array_equal(np.asarray(got)[i], want[i]["disp"], err_msg=f"pair {i}")
        np.testing.assert_array_equal(bits(se[i]), bits(want[i]["se"]), err_msg=f"pair {i}")


def test_switches_off_and_state():
    """After a config call with all three off the maps are those of a context that never made the call; a stage
    switched on after sm_disp_optimize is refused by sm_refine under "sgm"; the getters need a refine."""
    O = _oracle()
    H, W, D = 40, 60, 16
    batch, _ = _three(H, W, D, 630)
    maps = []
    for call in (False, True):
        sb = StereoBatch(D - 1, H, W, 3, device=0, do_refine=1)
        try:
            if call:
                sb.refine_ext_config(**ALL_ON)
                sb.refine_ext_config()
            sb.upload(*(batch[k] for k in KEYS))
            maps.append(sb.run(0.3))
            if call:
                with pytest.raises(_capi.SMError):
                    sb.get_pkr_mask()
                with pytest.raises(_capi.SMError):
                    sb.download_subpixel()
        finally:
            sb.close()
    np.testing.assert_array_equal(maps[1], maps[0])
    cfg = O.config(H, W, D - 1, do_refine=1)
    for i in range(3):
        np.testing.assert_array_equal(maps[0][i], O.run_ex({k: batch[k][i] for k in KEYS}, cfg)["disp"])
    pair = {k: batch[k][0] for k in KEYS}
    c = Ctx(H, W, D, pair, crafted=False)
    try:
        c.optimize(0.3)
        with pytest.raises(_capi.SMError):   # SGM kept no path sum
            c.volume()
        c.config(do_pkr=True)
        with pytest.raises(_capi.SMError, match="switched on after"):
            c.refine()
        c.config(do_bg=True)                 # the fill reads no volume: sm_refine runs
        want = R.refine_ext(O, cfg, c.get_disp(0), c.get_disp(1), O.arms(pair["lbgr"], cfg), pair["lbgr"], None, do_bg=True)
        np.testing.assert_array_equal(c.refine(), want["disp"])
    finally:
        c.close()


def test_profile_names():
    H, W, D = 40, 60, 16
    batch, _ = _three(H, W, D, 630)
    sb = StereoBatch(D - 1, H, W, 3, device=0, do_refine=1, num_streams=1, refine_ext=ALL_ON)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.profile(True)
        sb.run(0.3)
        sb.synchronize()
        prof = sb.profile_read()
    finally:
        sb.close()
    npix, nvol = 3 * H * W, 3 * H * W * D
    assert prof["refine_pkr"]["bytes_per_launch"] == nvol * 4 + npix * 5
    assert prof["refine_bg_ipol"]["bytes_per_launch"] == npix * 8
    assert prof["refine_subpixel"]["bytes_per_launch"] == npix * 18
    assert prof["refine_median3_f32"]["bytes_per_launch"] == npix * 8
    for k in ("refine_pkr", "refine_bg_ipol", "refine_subpixel", "refine_median3_f32"):
        assert prof[k]["launches"] == 1, (k, prof[k])
