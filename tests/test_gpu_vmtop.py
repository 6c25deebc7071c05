"""GPU parity of dispOptimize's Do_vmTop branch (sm_vmtop.hip) against the restatement tests/pyref_vmtop.py.

All comparisons are exact: maps as int16, candidate tables as f32 bit patterns (entries past a pixel's count read
as 0 on both sides).  Select alone and the decision methods run on crafted volumes put into vm[0] with
sm_set_volume under optimization ""; the end-to-end cases compare with the restatement applied to the C oracle's
summed volume.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pyref
import pyref_vmtop as V
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import synthetic as S
from test_cpp_facade import _compile, write_ppm

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vmtop")
f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


class Ctx:
    """One pair through the reference-ordered C ABI with optimization "": crafted volumes go into vm[0]."""

    def __init__(self, H, W, D, bgr=None):
        self.lib = _capi.load()
        self.H, self.W, self.D = H, W, D
        p = _capi.default_params(D - 1, H, W, cost_method="AD", aggregation=0, optimization=0)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(p), 0))
        if bgr is None:
            bgr = np.zeros((H, W, 3), np.uint8)
        bgr = np.ascontiguousarray(bgr)
        gray = np.ascontiguousarray(bgr[:, :, 1])
        self.ok(self.lib.sm_set_images(self.ctx, _capi.ptr(bgr), _capi.ptr(bgr), W * 3, _capi.ptr(gray), _capi.ptr(gray), W))
        self.ok(self.lib.sm_cost_calculate(self.ctx))

    def ok(self, st):
        _capi.check(self.lib, self.ctx, st)

    def config(self, *args):
        self.ok(self.lib.sm_vmtop_config(self.ctx, *args))

    def run(self, vol, num=None):
        """The map of `vol`, and its candidate table when num is given."""
        vol = np.ascontiguousarray(vol, np.float32)
        assert vol.shape == (self.H, self.W, self.D)
        self.ok(self.lib.sm_set_volume(self.ctx, 0, _capi.ptr(vol)))
        dp = np.empty((self.H, self.W), np.int16)
        self.ok(self.lib.sm_disp_optimize(self.ctx, _capi.ptr(dp)))
        back = np.empty_like(vol)
        self.ok(self.lib.sm_get_volume(self.ctx, 0, _capi.ptr(back)))
        np.testing.assert_array_equal(bits(back), bits(vol))   # vm[i] itself is not modified
        if num is None:
            return dp
        tab = np.full((self.H, self.W, num + 1, 2), np.nan, np.float32)
        self.ok(self.lib.sm_get_top_disp(self.ctx, 0, _capi.ptr(tab)))
        return dp, tab

    def close(self):
        self.lib.sm_destroy(self.ctx)


# ---- select alone -----------------------------------------------------------------------------------

def _contents(H, W, D, seed):
    """(name, volume, thres): the cases the selection can get wrong."""
    rng = np.random.default_rng(seed)
    out = [("equal_pos", np.full((H, W, D), 7, f32), 1.09),
           ("zero", np.zeros((H, W, D), f32), 1.09),
           ("equal_neg", np.full((H, W, D), -3, f32), 1.09),
           ("neg", -(rng.integers(1, 9, (H, W, D)).astype(f32)), 0.5)]
    v = rng.integers(5, 9, (H, W, D)).astype(f32)
    v[:, :, 0] = 2
    out.append(("min_first", v, 4.0))
    v = rng.integers(5, 9, (H, W, D)).astype(f32)
    v[:, :, D - 1] = 2
    out.append(("min_last", v, 4.0))
    # equal minima on both sides of a lane's four disparities, of the 16-lane row's 64 and of every later chunk
    v = rng.integers(5, 9, (H, W, D)).astype(f32)
    for d in (3, 4, 15, 16, 59, 60, 63, 64, 67, 127, 128, 191, 192, 255):
        if d < D:
            v[:, :, d] = np.where(rng.random((H, W)) < 0.7, 3, v[:, :, d])
    out.append(("ties", v, 1.5))
    # signed halves: the threshold multiply and compare on both signs, -0 among them
    v = (rng.integers(-6, 7, (H, W, D)) * 0.5).astype(f32)
    v[rng.random((H, W, D)) < 0.1] = -0.0
    out.append(("signed", v, 0.75))
    out.append(("random", rng.random((H, W, D)).astype(f32) + f32(0.5), 1.2))
    return out


@pytest.mark.parametrize("num", [1, 2, 6, 8])
@pytest.mark.parametrize("H,W,D", [(20, 28, 10), (9, 13, 60), (7, 3, 64), (6, 5, 132), (5, 4, 256)])
def test_select_tables(H, W, D, num):
    c = Ctx(H, W, D)
    try:
        for name, vol, thres in _contents(H, W, D, 31 * D + num):
            c.config(1, 0, num, thres, 10, 1, 0)
            _, got = c.run(vol, num)
            want, counts = V.select(vol, num, f32(thres))
            np.testing.assert_array_equal(got[:, :, num, 0], counts.astype(f32), err_msg=name)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=name)
            if name in ("equal_pos",):   # more candidates asked for than distinct costs: the lowest d's, in order
                assert (counts == min(num, D)).all()
                assert (got[:, :, :min(num, D), 0] == np.arange(min(num, D), dtype=f32)).all()
            if name in ("zero", "equal_neg"):   # firstV <= 0 with thres > 1
                assert (counts == 1).all()
    finally:
        c.close()


# ---- the decision methods on the fixtures ---------------------------------------------------------

def _fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"vmtop_{name}.npz")))


@pytest.mark.parametrize("name", ["mix", "mix_m8", "case2", "rows", "signed"])
def test_decide_fixtures(name):
    fx = _fixture(name)
    H, W, D = fx["vol"].shape
    num, thres, ts = int(fx["num"]), float(fx["thres"]), int(fx["ts"])
    c = Ctx(H, W, D, fx["bgr"])
    try:
        for key in sorted(k for k in fx if k.startswith("map_")):
            m, cir2, col = int(key[4]), int(key[5]), int(key[6])
            c.config(1, m, num, thres, ts, cir2, col)
            dp, tab = c.run(fx["vol"], num)
            np.testing.assert_array_equal(bits(tab), bits(fx["table"]), err_msg=key)
            np.testing.assert_array_equal(dp, fx[key], err_msg=key)
    finally:
        c.close()


@pytest.mark.parametrize("cir2,col", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_decide_longest_chain_transposed(cir2, col):
    """The all-case-2 33 x 41 volume transposed (41 x 33): the ordered pass's other aspect, t up to W + 2 H - 3."""
    fx = _fixture("case2")
    vol = np.ascontiguousarray(fx["vol"].transpose(1, 0, 2))
    bgr = np.ascontiguousarray(fx["bgr"].transpose(1, 0, 2))
    H, W, D = vol.shape
    num, thres, ts = int(fx["num"]), float(fx["thres"]), int(fx["ts"])
    table, counts = V.select(vol, num, f32(thres))
    want, cnt = V.decide(table, counts, bgr, 0, ts, cir2, col)
    if cir2:
        assert cnt["case2"] == (H - 1) * (W - 1)
    c = Ctx(H, W, D, bgr)
    try:
        c.config(1, 0, num, thres, ts, cir2, col)
        np.testing.assert_array_equal(c.run(vol), want)
        for m in (1, 2):
            c.config(1, m, num, thres, ts, cir2, col)
            np.testing.assert_array_equal(c.run(vol), V.decide(table, counts, bgr, m)[0], err_msg=f"method {m}")
    finally:
        c.close()


def test_disabled_again_is_the_plain_wta():
    fx = _fixture("mix")
    H, W, D = fx["vol"].shape
    c = Ctx(H, W, D, fx["bgr"])
    try:
        plain = c.run(fx["vol"])
        np.testing.assert_array_equal(plain, pyref.wta(fx["vol"]))
        c.config(1, 0, int(fx["num"]), float(fx["thres"]), int(fx["ts"]), 1, 0)
        on = c.run(fx["vol"])
        np.testing.assert_array_equal(on, fx["map_010"])
        assert (on != plain).any()
        c.config(0, 0, int(fx["num"]), float(fx["thres"]), int(fx["ts"]), 1, 0)
        np.testing.assert_array_equal(c.run(fx["vol"]), plain)
    finally:
        c.close()


# ---- end to end -----------------------------------------------------------------------------------

VT = dict(method=0, num=3, thres=float(np.float32(1.09)), ts=10, has_cir2=True, cir3_color_limit=False)


@functools.lru_cache(maxsize=None)
def _batch(H, W, D, n, first):
    batch = S.make_batch(n, H, W, D, first_index=first)
    return {k: batch[k] for k in KEYS}


def _vt(vol, lbgr, vt):
    return V.vmtop(vol, lbgr, vt["num"], f32(vt["thres"]), vt["method"], vt["ts"], vt["has_cir2"], vt["cir3_color_limit"])


@functools.lru_cache(maxsize=None)
def _want(H, W, D, n, first, i, opt, paths, agg, refine, vt_key):
    """Pair i's expected map: the restatement on the oracle's volume after SolveAll (and SGM)."""
    O = _oracle()
    vt = dict(vt_key)
    batch = _batch(H, W, D, n, first)
    pair = {k: batch[k][i] for k in KEYS}
    cfg = O.config(H, W, D - 1, optimization=opt, sgm_paths=paths, aggregation=agg, do_refine=int(refine))
    ref = O.run_ex(pair, cfg, dumps=("final", "agg_right") if refine else ("final",))
    d0 = _vt(ref["final"], pair["lbgr"], vt)
    if refine:
        v1 = pyref.solve_all(ref["agg_right"])
        if opt == 1:
            v1 = pyref.sgm(v1, pair["rbgr"], paths=paths)
        d1 = _vt(v1, pair["lbgr"], vt)   # I_c[0] for view 1 as well
        d0 = pyref.refine(d0, d1, pyref.arms(pair["lbgr"]), pair["lbgr"], D)
    d0.setflags(write=False)
    return d0


def _key(vt):
    return tuple(sorted(vt.items()))


E2E = [dict(optimization=1, sgm_paths=4), dict(optimization=1, sgm_paths=8), dict(optimization=0),
       dict(optimization=1, sgm_paths=4, aggregation=2), dict(optimization=1, sgm_paths=4, do_refine=1)]


@pytest.mark.parametrize("H,W,D", [(30, 44, 32), (21, 30, 200)])
@pytest.mark.parametrize("cfg", E2E, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_end_to_end_batch(H, W, D, cfg):
    """sm_run on 3 pairs: 4 and 8 paths, "", GF (signed costs), do_refine (both views, the refined map)."""
    n, first = 3, 930
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, **cfg)
    try:
        sb.vmtop_config(True, **VT)
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
        tab = sb.get_top_disp(0)
    finally:
        sb.close()
    args = (cfg["optimization"], cfg.get("sgm_paths", 4), cfg.get("aggregation", 1), bool(cfg.get("do_refine")), _key(VT))
    for i in range(n):
        np.testing.assert_array_equal(got[i], _want(H, W, D, n, first, i, *args), err_msg=f"pair {i}")
    assert (tab[:, :, VT["num"], 0] >= 1).all()


@pytest.mark.parametrize("sub_batch,num_streams", [(2, 2), (1, 3)])
def test_schedules(sub_batch, num_streams):
    H, W, D, n, first = 29, 41, 16, 5, 940
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, sub_batch=sub_batch, num_streams=num_streams)
    try:
        sb.vmtop_config(True, **VT)
        sb.upload(*(batch[k] for k in KEYS))
        first_run = sb.run(0.3)
        second = sb.run(0.3)
    finally:
        sb.close()
    np.testing.assert_array_equal(second, first_run)
    for i in range(n):
        np.testing.assert_array_equal(first_run[i], _want(H, W, D, n, first, i, 1, 4, 1, False, _key(VT)), err_msg=f"pair {i}")


def test_pipelined_default_with_async_downloads():
    """batch_capacity 8, num_streams 0: two groups pipelined across calls, the new kernels between each group's
    SGM and its map copy.  Three calls with asynchronous downloads, then vmTop off: today's maps."""
    import torch
    H, W, D, n, first = 29, 41, 16, 8, 950
    batch = _batch(H, W, D, n, first)
    O = _oracle()
    sb = StereoBatch(D - 1, H, W, n, device=0)
    try:
        assert sb.params.num_streams == 0
        sb.vmtop_config(True, **VT)
        sb.upload(*(batch[k] for k in KEYS))
        outs = [torch.empty((n, H, W), dtype=torch.int16, pin_memory=True).numpy() for _ in range(3)]
        for o in outs:
            sb.run(0.3, download=False)
            sb.download_async(o)
        sb.synchronize()
        sb.vmtop_config(False, **VT)
        plain = sb.run(0.3)
    finally:
        sb.close()
    for i in range(n):
        want = _want(H, W, D, n, first, i, 1, 4, 1, False, _key(VT))
        for o in outs:
            np.testing.assert_array_equal(o[i], want, err_msg=f"pair {i}")
        pair = {k: batch[k][i] for k in KEYS}
        np.testing.assert_array_equal(plain[i], O.run_ex(pair, O.config(H, W, D - 1))["disp"], err_msg=f"pair {i}")


def test_so_ignores_vmtop():
    H, W, D, n, first = 30, 44, 32, 3, 930
    batch = _batch(H, W, D, n, first)
    maps = []
    for on in (False, True):
        sb = StereoBatch(D - 1, H, W, n, device=0, optimization=2)
        try:
            if on:
                sb.vmtop_config(True, **VT)
            sb.upload(*(batch[k] for k in KEYS))
            maps.append(sb.run(0.3))
        finally:
            sb.close()
    np.testing.assert_array_equal(maps[1], maps[0])


def test_reference_ordered_api():
    """param.Do_vmTop through costCalculate -> SolveAll -> dispOptimize, M, lamc and ts from the constructor."""
    H, W, D, first = 30, 44, 32, 930
    batch = _batch(H, W, D, 3, first)
    pair = {k: batch[k][1] for k in KEYS}
    prm = StereoMatching.Parameters(D - 1, H, W, 13, 1, 3, 109, 10)
    prm.Do_vmTop = True
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_LRConsis)
    cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_LRConsis = "censusGrad", "CBCA", "sgm", False, True
    try:
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm, device=0)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        got = sm.dispOptimize()
    finally:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_LRConsis = saved
    np.testing.assert_array_equal(got, _want(H, W, D, 3, first, 1, 1, 4, 1, False, _key(VT)))


def test_profile_names():
    H, W, D, n, first = 29, 41, 16, 5, 940
    batch = _batch(H, W, D, n, first)
    sb = StereoBatch(D - 1, H, W, n, device=0, num_streams=1)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.profile(True)
        for m in (0, 1):
            sb.vmtop_config(True, **dict(VT, method=m))
            sb.run(0.3)
        sb.synchronize()
        names = {k: v["launches"] for k, v in sb.profile_read().items()}
    finally:
        sb.close()
    for k in ("vmtop_select", "vmtop_decide0_a", "vmtop_decide0_b", "vmtop_decide12"):
        assert names.get(k, 0) >= 1, names
    assert "wta" not in names


def test_cpp_facade(tmp_path):
    """tests/cpp/vmtop_facade_check.cpp: Parameters(maxDisp, h, w, 13, 1, M, lamc, ts) with Do_vmTop set."""
    src = os.path.join(ROOT, "tests", "cpp", "vmtop_facade_check.cpp")
    exe = str(tmp_path / "vmtop_facade_check")
    _compile(src, exe)
    H, W, md = 20, 26, 15
    pair = S.make_pair(H, W, md + 1, 970)
    pair = {k: pair[k] for k in ("lbgr", "rbgr")}
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    maps = {}
    for method in (-1, 0, 2):
        out = tmp_path / f"dp{method}.i16"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(md), "3", "113", "9", str(method),
                            "1", "0", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"vmTop_thres_bits {int(bits(np.float32(113 * 0.01)).item()):08x}" in r.stdout
        got = np.fromfile(out, np.int16).reshape(H, W)
        sb = StereoBatch(md, H, W, 1, device=0, num_streams=1)
        try:
            if method >= 0:
                sb.vmtop_config(True, method, 3, float(np.float32(113 * 0.01)), 9, True, False)
            sb.upload(*(pair[k][None] for k in KEYS))
            want = sb.run(0.3)[0]
        finally:
            sb.close()
        np.testing.assert_array_equal(got, want)
        maps[method] = got
    assert (maps[0] != maps[-1]).any()   # the branch reached the kernels
