"""GPU parity of refine()'s discontinuity adjustment (sm_refine_da.hip) against the restatement tests/pyref_da.py.

All comparisons are exact: image planes and edge maps as bytes, maps as int16.  The image stages run on supplied
images (sm_da_run_image), the ordered pass on supplied edge maps (sm_set_da_edges), both on crafted contexts as in
tests/test_gpu_refine_ext.py (AD costs, no aggregation, optimization "", the other refine stages off, LRmaxDiff huge
and DP[1] = 0, so the LR check only turns negative values and d > u into -1: the holes -1 and -32 both reach the
stage as -1, and a value >= D has to sit at a column >= itself).  The pipeline cases compare with the restatement
composed with the C oracle's stages on the oracle's own volume and maps.

The meander of the hysteresis test is bars of value 8 in rows 4 + 8 k .. 7 + 8 k (k = 0 .. 7) over columns 4 .. 91,
joined by 4 x 12 posts alternately at the right (columns 80 .. 91) and left (columns 4 .. 15) ends.  On the
restatement it has 1242 candidates with and without the seed, 8 strong pixels with it, no edge without it and every
candidate an edge with it (the issue's prototype counted 1272 candidates on its own drawing of the meander, which
its prose does not pin down; the properties are the same).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref_da as DA
from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S
from test_gpu_refine_ext import Ctx, KEYS, _lr_only, _map, _oracle

pytestmark = pytest.mark.gpu
f32 = np.float32


class DaCtx(Ctx):
    def da_config(self, on=True, low=20, high=60, ks=84, kc=87):
        self.ok(self.lib.sm_refine_da_config(self.ctx, int(on), low, high, ks, kc))

    def run_image(self, img, first):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.H, self.W)
        out = [np.full((self.H, self.W), 0xAB, np.uint8) for _ in range(3)]
        ptrs = [_capi.ptr(o) if i >= first else None for i, o in enumerate(out)]
        self.ok(self.lib.sm_da_run_image(self.ctx, _capi.ptr(img), first, *ptrs))
        return out

    def set_edges(self, edges):
        self.ok(self.lib.sm_set_da_edges(self.ctx, None if edges is None else _capi.ptr(np.ascontiguousarray(edges, np.uint8))))

    def edges(self):
        out = np.full((self.H, self.W), 0xAB, np.uint8)
        self.ok(self.lib.sm_get_da_edges(self.ctx, _capi.ptr(out)))
        return out


# ---- image stages --------------------------------------------------------------------------------------

def _images():
    rng = np.random.default_rng(11)
    noise = lambda h, w: rng.integers(0, 256, (h, w)).astype(np.uint8)
    ramp = (np.arange(33)[:, None] * 3 + np.arange(41)[None, :] * 2 + 40).astype(np.uint8)   # first bin 40
    steps = np.repeat(np.repeat(rng.integers(40, 200, (5, 6)), 7, 0), 7, 1)[:33, :41].astype(np.uint8)
    return {"3x3": noise(3, 3), "2x2": noise(2, 2), "33x41": noise(33, 41), "17x130": noise(17, 130),
            "constant": np.full((8, 9), 77, np.uint8), "offset_bin": ramp, "steps": steps}


@pytest.mark.parametrize("name", ["3x3", "2x2", "33x41", "17x130", "constant", "offset_bin", "steps"])
def test_image_stages(name):
    img = _images()[name]
    H, W = img.shape
    want = DA.image_stages(img, 0)
    if name == "constant":
        assert not want["edges"].any() and (want["eq"] == 77).all()
    if name in ("offset_bin", "steps"):
        assert img.min() >= 40 and want["eq"].min() == 0
    if name in ("33x41", "17x130", "steps"):
        assert 0 < (want["edges"] > 0).mean() < 1
    c = DaCtx(H, W, 16)
    try:
        eq, bl, ed = c.run_image(img, 0)               # chained
        np.testing.assert_array_equal(eq, want["eq"])
        np.testing.assert_array_equal(bl, want["blur"])
        np.testing.assert_array_equal(ed, want["edges"])
        for src in (img, want["eq"]):                  # the blur entered alone, on two images
            w1 = DA.image_stages(src, 1)
            eq, bl, ed = c.run_image(src, 1)
            assert (eq == 0xAB).all()                  # outputs before the entry are left alone
            np.testing.assert_array_equal(bl, w1["blur"])
            np.testing.assert_array_equal(ed, w1["edges"])
        for src in (img, want["blur"]):                # Canny entered alone: dense candidates on raw noise
            w2 = DA.image_stages(src, 2)
            _, bl, ed = c.run_image(src, 2)
            assert (bl == 0xAB).all()
            np.testing.assert_array_equal(ed, w2["edges"])
        # other thresholds (swapped on entry) and a kernel that sums to 256
        c.da_config(False, 90, 30, 85, 86)
        w3 = DA.image_stages(img, 0, 30, 90, 85, 86)
        eq, bl, ed = c.run_image(img, 0)
        np.testing.assert_array_equal(bl, w3["blur"])
        np.testing.assert_array_equal(ed, w3["edges"])
    finally:
        c.close()


def _meander(seed):
    img = np.zeros((64, 96), np.uint8)
    for k in range(8):
        img[4 + 8 * k:8 + 8 * k, 4:92] = 8
    for k in range(7):
        c0 = 80 if k % 2 == 0 else 4
        img[8 + 8 * k:12 + 8 * k, c0:c0 + 12] = 8
    if seed:
        img[4:8, 4:6] = 30
    return img


@pytest.mark.parametrize("seed", [False, True])
def test_hysteresis_across_blocks(seed):
    """One weak component that winds through every tile of the image: a strong seed in one corner decides all of
    it.  A block-local propagation gets this wrong."""
    img = _meander(seed)
    edges, cand, strong = DA.canny(img)
    assert cand.sum() == 1242
    assert strong.sum() == (8 if seed else 0)
    assert (edges > 0).sum() == (1242 if seed else 0)
    assert cand[4:8].any() and cand[60:].any() and cand[:, :16].any() and cand[:, 80:].any()
    c = DaCtx(64, 96, 16)
    try:
        _, _, got = c.run_image(img, 2)
        np.testing.assert_array_equal(got, edges)
        _, _, again = c.run_image(img, 2)
        np.testing.assert_array_equal(again, got)
    finally:
        c.close()


# ---- the ordered pass alone ------------------------------------------------------------------------------

def _ordered_case(name, H, W, D=16):
    rng = np.random.default_rng(sum(map(ord, name)) + H * 131 + W)
    vol = rng.random((H, W, D)).astype(f32)
    d0 = _map(rng, H, W, D - 1, 0.0)
    edges = np.full((H, W), 255, np.uint8)
    if name == "random_edges":
        edges = np.where(rng.random((H, W)) < 0.5, 255, 0).astype(np.uint8)
    elif name == "negative_costs":
        vol = (rng.random((H, W, D)) * 2 - 1).astype(f32)
        vol[rng.random((H, W, D)) < 0.1] = -1           # the value the second side refuses
    elif name == "nan_costs":
        vol[rng.random((H, W, D)) < 0.15] = np.nan
    elif name == "holes":
        d0 = _map(rng, H, W, D - 1, 0.2)
    elif name == "beyond_d":
        big = (rng.random((H, W)) < 0.1) & (np.arange(W)[None, :] >= D + 3)
        d0[big] = rng.integers(D, D + 4, int(big.sum())).astype(np.int16)
        assert big.any()
    return vol, d0, edges


@pytest.mark.parametrize("H,W", [(33, 41), (17, 130)])
@pytest.mark.parametrize("name", ["all_edges", "random_edges", "negative_costs", "nan_costs", "holes", "beyond_d"])
def test_ordered_pass(name, H, W):
    D = 16
    vol, d0, edges = _ordered_case(name, H, W, D)
    post = _lr_only(d0)
    if name == "holes":
        assert (post < 0).any()
    if name == "beyond_d":
        assert (post >= D).any()
    if name == "all_edges":   # every interior pixel has direction 4: each anti-diagonal is one chain
        assert all(DA.direction_of(edges, h, w) == 4 for h in range(1, H - 1) for w in range(1, W - 1))
    stats = {}
    want = DA.adjust(post, edges, vol, stats)
    assert stats["chained"] >= 1 and stats["changed"] > 0, stats
    c = DaCtx(H, W, D)
    try:
        c.set_volume(vol)
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        c.da_config(True)
        c.set_edges(edges)
        got = c.refine()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(c.edges(), edges)
        if name == "all_edges":
            # back to Canny's own map, then off: the LR check alone
            c.set_edges(None)
            c.set_disp(d0)
            w2, e2 = DA.discontinuity_adjust(post, vol)
            np.testing.assert_array_equal(c.refine(), w2)
            np.testing.assert_array_equal(c.edges(), e2)
            c.set_disp(d0)
            c.da_config(False)
            np.testing.assert_array_equal(c.refine(), post)
            with pytest.raises(_capi.SMError):
                c.edges()
    finally:
        c.close()


def test_small_maps_change_nothing():
    """rows < 3: no interior.  The image stages still run."""
    H, W, D = 2, 40, 16
    rng = np.random.default_rng(5)
    d0 = _map(rng, H, W, D - 1, 0.1)
    post = _lr_only(d0)
    c = DaCtx(H, W, D)
    try:
        c.set_volume(rng.random((H, W, D)).astype(f32))
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        c.da_config(True)
        np.testing.assert_array_equal(c.refine(), post)
        np.testing.assert_array_equal(c.edges(), DA.image_stages(DA.to_u8(post))["edges"])
    finally:
        c.close()


# ---- the whole stage -------------------------------------------------------------------------------------

def _piecewise(rng, H, W, D):
    d = np.full((H, W), rng.integers(2, 8), np.int64)
    for _ in range(6):
        h0, w0 = rng.integers(0, H - 4), rng.integers(0, W - 4)
        d[h0:h0 + rng.integers(4, H), w0:w0 + rng.integers(4, W)] = rng.integers(0, D)
    out = rng.random((H, W)) < 0.10
    d[out] = rng.integers(0, D, int(out.sum()))
    d = np.minimum(d, np.arange(W)[None, :]).astype(np.int16)
    d[rng.random((H, W)) < 0.05] = -1
    return d


@pytest.mark.parametrize("H,W", [(33, 41), (64, 96)])
@pytest.mark.parametrize("kind", ["noise", "piecewise"])
def test_whole_stage(kind, H, W):
    D = 64
    rng = np.random.default_rng(H + (7 if kind == "noise" else 0))
    vol = rng.random((H, W, D)).astype(f32)
    d0 = _map(rng, H, W, D - 1, 0.05) if kind == "noise" else _piecewise(rng, H, W, D)
    post = _lr_only(d0)
    stats = {}
    want, edges = DA.discontinuity_adjust(post, vol, stats=stats)
    assert stats["changed"] > 0 and 0 < (edges > 0).mean() < 1, stats
    c = DaCtx(H, W, D)
    try:
        with pytest.raises(_capi.SMError):   # no edge map before a refine with the stage on
            c.edges()
        c.set_volume(vol)
        c.optimize()
        c.set_disp(d0, np.zeros((H, W), np.int16))
        c.da_config(True)
        got = c.refine()
        np.testing.assert_array_equal(c.edges(), edges)
        np.testing.assert_array_equal(got, want)
    finally:
        c.close()


# ---- whole pipeline ----------------------------------------------------------------------------------------

HP, WP, DP_ = 33, 41, 16


@functools.lru_cache(maxsize=None)
def _three(first=650):
    """Three pairs and, from the oracle's own path sum and maps, the expected maps with the stage off and on."""
    O = _oracle()
    batch = S.make_batch(3, HP, WP, DP_, first_index=first)
    cfg = O.config(HP, WP, DP_ - 1, do_refine=1)
    want = []
    for i in range(3):
        pair = {k: batch[k][i] for k in KEYS}
        ref = O.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
        args = (O, cfg, ref["disp_raw"], ref["disp_right"], O.arms(pair["lbgr"], cfg), pair["lbgr"], ref["final"])
        want.append({"pair": pair, "off": ref["disp"], "on": DA.refine_da(*args), "all": DA.refine_da(*args, do_pkr=True, do_bg=True, do_se=True)})
        np.testing.assert_array_equal(DA.refine_da(*args, do_da=False)["disp"], ref["disp"])
    assert any((w["on"]["disp"] != w["off"]).any() for w in want)
    return batch, want


def test_pipeline_against_oracle():
    """censusGrad + CBCA + sgm + Do_refine with the adjustment: the staged calls and sm_run against pyref o oracle;
    then with PKR, BGIpol and SE on as well (the order of the stages)."""
    batch, want = _three()
    w = want[0]
    c = DaCtx(HP, WP, DP_, w["pair"], crafted=False)
    try:
        c.da_config(True)
        c.optimize(0.3)
        np.testing.assert_array_equal(c.refine(), w["on"]["disp"])
        np.testing.assert_array_equal(c.edges(), w["on"]["edges"])
    finally:
        c.close()
    sb = StereoBatch(DP_ - 1, HP, WP, 1, device=0, do_refine=1, refine_da=dict(on=True),
                     refine_ext=dict(do_pkr=True, do_bg_ipol=True, do_subpixel=True))
    try:
        sb.upload(*(w["pair"][k][None] for k in KEYS))
        np.testing.assert_array_equal(sb.run(0.3)[0], w["all"]["disp"])
        np.testing.assert_array_equal(sb.get_da_edges(), w["all"]["edges"])
        np.testing.assert_array_equal(sb.get_pkr_mask(), w["all"]["mask"])
        np.testing.assert_array_equal(sb.download_subpixel()[0].view(np.uint32), w["all"]["se"].view(np.uint32))
    finally:
        sb.close()
    assert (w["all"]["disp"] != w["on"]["disp"]).any()


@pytest.mark.parametrize("sub_batch,num_streams", [(0, 1), (1, 1), (1, 2), (2, 2)])
def test_schedules(sub_batch, num_streams):
    batch, want = _three()
    sb = StereoBatch(DP_ - 1, HP, WP, 3, device=0, do_refine=1, sub_batch=sub_batch, num_streams=num_streams)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        off = sb.run(0.3)                      # the stage off: today's maps
        sb.refine_da_config(True)
        got = sb.run(0.3)
        edges = sb.get_da_edges()
        again = sb.run(0.3)
        sb.refine_da_config(False)
        off2 = sb.run(0.3)
    finally:
        sb.close()
    np.testing.assert_array_equal(again, got)
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(edges, want[0]["on"]["edges"])
    for i in range(3):
        np.testing.assert_array_equal(off[i], want[i]["off"], err_msg=f"pair {i}")
        np.testing.assert_array_equal(got[i], want[i]["on"]["disp"], err_msg=f"pair {i}")


def test_state():
    batch, want = _three()
    c = DaCtx(HP, WP, DP_, want[0]["pair"], crafted=False)
    try:
        with pytest.raises(_capi.SMError) as e:
            c.edges()
        assert e.value.status == _capi.SM_ESTATE
        c.optimize(0.3)
        c.da_config(True)                      # SGM kept no path sum
        with pytest.raises(_capi.SMError, match="switched on after") as e:
            c.refine()
        assert e.value.status == _capi.SM_ESTATE
        c.ok(c.lib.sm_cost_calculate(c.ctx))   # again, with the stage on from the start
        c.optimize(0.3)
        np.testing.assert_array_equal(c.refine(), want[0]["on"]["disp"])
    finally:
        c.close()
    lib = _capi.load()
    p = _capi.default_params(DP_ - 1, HP, WP, do_refine=1, optimization="so")
    ctx = C.c_void_p()
    _capi.check(lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0))
    try:
        assert lib.sm_refine_da_config(ctx, 1, 20, 60, 84, 87) == _capi.SM_EINVAL
        assert b"so" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_profile_names():
    batch, _ = _three()
    sb = StereoBatch(DP_ - 1, HP, WP, 3, device=0, do_refine=1, num_streams=1, refine_da=dict(on=True))
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.profile(True)
        sb.run(0.3)
        sb.synchronize()
        prof = sb.profile_read()
    finally:
        sb.close()
    names = ("hist", "equalize", "blur", "sobel", "nms", "link", "mark", "edges", "dir", "adjust")
    for k in names:   # a fixed number of launches: one each, whatever the data
        assert prof["refine_da_" + k]["launches"] == 1, (k, prof.get("refine_da_" + k))
    assert sorted(k for k in prof if k.startswith("refine_da_")) == sorted("refine_da_" + k for k in names)


def test_python_facade_and_compute_function():
    """StereoMatching with the class attribute set gives the C ABI's maps and leaves the edge map in DA_Edge;
    DistributedBatchRunner's compute function hands refine_da on."""
    from mystereomatching_amd import SolveAll, StereoMatching
    from mystereomatching_amd.batch import hip_compute_fn
    batch, want = _three()
    w = want[0]
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_discontinuityAdjust)
    try:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine = "censusGrad", "CBCA", "sgm", True
        for on in (True, False):
            cls.Do_discontinuityAdjust = on
            p = w["pair"]
            sm = StereoMatching(p["lbgr"], p["rbgr"], p["lgray"], p["rgray"], None, None, None, None,
                                StereoMatching.Parameters(DP_ - 1, HP, WP))
            sm.costCalculate()
            SolveAll([sm], 1, 0.3)
            sm.dispOptimize()
            np.testing.assert_array_equal(sm.refine(), w["on"]["disp"] if on else w["off"])
            if on:
                np.testing.assert_array_equal(sm.DA_Edge, w["on"]["edges"])
            else:
                assert sm.DA_Edge is None
    finally:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_discontinuityAdjust = saved
    fn = hip_compute_fn(DP_ - 1, HP, WP, 3, 0, do_refine=1, refine_da=dict(on=True))
    try:
        got = np.asarray(fn({k: batch[k] for k in KEYS}, 0.3))
        edges = fn.get_da_edges()
    finally:
        fn.close()
    np.testing.assert_array_equal(edges, want[0]["on"]["edges"])
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i]["on"]["disp"], err_msg=f"pair {i}")


def test_cpp_facade(tmp_path):
    """tests/cpp/da_facade_check.cpp: the C++ facade with Do_discontinuityAdjust set gives the C ABI's maps (the
    facade reads its gray images from the colour files, so the expectation is a StereoBatch on those)."""
    import os
    import subprocess
    from test_cpp_facade import _compile, write_ppm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "da_facade_check")
    _compile(os.path.join(root, "tests", "cpp", "da_facade_check.cpp"), exe)
    H, W, MD = 40, 56, 15
    p = S.make_pair(H, W, MD + 1, 640)
    write_ppm(tmp_path / "l.ppm", p["lbgr"])
    write_ppm(tmp_path / "r.ppm", p["rbgr"])
    want = {}
    sb = StereoBatch(MD, H, W, 1, device=0, do_refine=1)
    try:
        sb.upload(*(p[k][None] for k in KEYS))
        want[0] = sb.run(0.3)[0].copy()
        sb.refine_da_config(True)
        want[1] = sb.run(0.3)[0].copy()
        edges = sb.get_da_edges()
    finally:
        sb.close()
    assert (want[0] != want[1]).any() and edges.any()
    for on in (1, 0):
        dp, ed = tmp_path / f"dp{on}", tmp_path / f"edge{on}"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(MD), str(on), str(dp), str(ed)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "canny 20 60 taps 84 87" in r.stdout
        np.testing.assert_array_equal(np.fromfile(dp, np.int16).reshape(H, W), want[on])
        if on:
            np.testing.assert_array_equal(np.fromfile(ed, np.uint8).reshape(H, W), edges)
