"""GPU: the cross-scale pyramid (PY_LVL 2-8, main_.cpp:131-158) inside the batch path -- sm_pyramid_config + sm_run
through StereoBatch, hip_compute_fn and DistributedBatchRunner.  Bit-exact against oracle.run_pyr, against
pyref.solve_all_pyr over the oracle's per-level volumes, and against the staged one-context-per-level path
(StereoMatching / pyrDown / SolveAll) for what run_pyr does not cover.
"""
import functools

import numpy as np
import pytest

import pyref
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, pyrDown
from mystereomatching_amd import synthetic as S
from mystereomatching_amd.batch import DistributedBatchRunner, hip_compute_fn

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def _pair(batch, i):
    return {k: batch[k][i] for k in KEYS}


def _oracle_maps(oracle, batch, H, W, md, L, **cfg_kw):
    cfg = oracle.config(H, W, md, **cfg_kw)
    return np.stack([oracle.run_pyr(_pair(batch, i), cfg, L) for i in range(batch["lgray"].shape[0])])


def _run(sb, batch, n=None):
    n = batch["lgray"].shape[0] if n is None else n
    sb.upload(*(batch[k][:n] for k in KEYS))
    return sb.run(0.3)


# ---- 1. maps against oracle.run_pyr --------------------------------------------------------------

# (L, H, W, maxdisp, n, do_refine, first pair index, oracle config, StereoBatch overrides)
MAP_CASES = [
    pytest.param(2, 40, 52, 15, 3, 0, 1000, {}, {}, id="L2-odd-group-split"),
    pytest.param(3, 40, 52, 15, 2, 1, 1010, {}, {}, id="L3-both-views"),
    pytest.param(3, 61, 77, 22, 2, 0, 1020, {}, {}, id="L3-D23-scalar-tail"),
    pytest.param(4, 33, 41, 63, 2, 1, 1030, {}, {}, id="L4-D64-refine"),
    pytest.param(2, 16, 18, 255, 1, 0, 1040, {}, {}, id="L2-D256"),
    pytest.param(3, 5, 7, 3, 2, 0, 1050, {}, {}, id="L3-smallest"),
    pytest.param(8, 300, 260, 63, 2, 0, 1060, {}, {}, id="L8-deepest"),
    pytest.param(2, 21, 34, 22, 2, 0, 1070, dict(cost="Census", aggregation=0, optimization=0),
                 dict(cost_method="Census", aggregation="", optimization=""), id="L2-census-wta"),
    pytest.param(2, 40, 52, 15, 2, 0, 1080, dict(cost="ADCensus", optimization=2),
                 dict(cost_method="ADCensus", optimization="so"), id="L2-adcensus-so"),
    pytest.param(2, 40, 52, 15, 2, 0, 1090, dict(sgm_paths=8), dict(sgm_paths=8), id="L2-sgm8"),
]


@pytest.mark.parametrize("L,H,W,md,n,refine,first,okw,skw", MAP_CASES)
def test_maps_equal_run_pyr(oracle, L, H, W, md, n, refine, first, okw, skw):
    batch = S.make_batch(n, H, W, md + 1, first_index=first)
    want = _oracle_maps(oracle, batch, H, W, md, L, do_refine=refine, **okw)
    # the condition on the oracle alone: the pyramid changes a map (nothing changes at the smallest legal one)
    flat = _oracle_maps(oracle, batch, H, W, md, 1, do_refine=refine, **okw)
    differs = int((want != flat).sum())
    print(f"L={L} {H}x{W} maxdisp {md}: {differs} / {want.size} px differ from PY_LVL 1")
    if (H, W) != (5, 7):
        assert differs > 0
    sb = StereoBatch(md, H, W, n, do_refine=refine, py_lvl=L, **skw)
    try:
        assert sb.pyramid_levels == L
        got = _run(sb, batch)
        for i in range(n):
            np.testing.assert_array_equal(got[i], want[i], err_msg=f"pair {i}")
    finally:
        sb.close()


# ---- 2. volumes and level inputs -----------------------------------------------------------------

def _oracle_levels(oracle, pair, H, W, md, L, refine):
    """Per level: the pyrDown'ed pair, the oracle's config (arm limits / 2^s, maxdisp / 2 + 1) and aggregated volumes."""
    out, p = [], {k: pair[k] for k in KEYS}
    for s in range(L):
        cfg = oracle.config(H, W, md, arm_L=17 >> s, arm_L_out=34 >> s, do_refine=refine, optimization=0)
        r = oracle.run_ex(p, cfg, dumps=("agg", "agg_right") if refine else ("agg",))
        out.append(dict(pair=p, cfg=cfg, agg=[r["agg"]] + ([r["agg_right"]] if refine else [])))
        p = {k: oracle.pyr_down(v) for k, v in p.items()}
        H, W, md = (H + 1) // 2, (W + 1) // 2, md // 2 + 1
    return out


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("L,H,W,md", [(3, 9, 10, 23), (2, 21, 34, 22)])
def test_volumes_and_level_inputs(oracle, L, H, W, md, refine):
    batch = S.make_batch(2, H, W, md + 1, first_index=1100 + H)
    lv = _oracle_levels(oracle, _pair(batch, 0), H, W, md, L, refine)
    sb = StereoBatch(md, H, W, 2, optimization="", do_refine=refine, py_lvl=L)
    try:
        _run(sb, batch)
        for v in range(1 + refine):
            want = pyref.solve_all_pyr([l["agg"][v] for l in lv])
            np.testing.assert_array_equal(sb.pyramid_level_volume(0, v).view(np.uint32), want.view(np.uint32), err_msg=f"view {v}")
        for s in range(1, L):
            p, cfg = lv[s]["pair"], lv[s]["cfg"]
            for v, (g, c) in enumerate((("lgray", "lbgr"), ("rgray", "rbgr"))):
                np.testing.assert_array_equal(sb.pyramid_level_census(s, v), oracle.census(p[g], cfg), err_msg=f"census {s} {v}")
                np.testing.assert_array_equal(sb.pyramid_level_arms(s, v), oracle.arms(p[c], cfg), err_msg=f"arms {s} {v}")
            for v in range(1 + refine):   # a coarse level's own aggregated volume, through sm_pyramid_level
                np.testing.assert_array_equal(sb.pyramid_level_volume(s, v).view(np.uint32), lv[s]["agg"][v].view(np.uint32))
        with pytest.raises(ValueError):
            sb.pyramid_level_volume(L)
    finally:
        sb.close()


def test_level_context_takes_only_getters():
    from mystereomatching_amd import _capi
    import ctypes as C
    sb = StereoBatch(15, 24, 30, 1, py_lvl=2)
    try:
        lib = sb._lib
        lvl = C.c_void_p(lib.sm_pyramid_level(sb._ctx, 1))
        for st in (lib.sm_synchronize(lvl), lib.sm_run(lvl, 1, 0.3, None), lib.sm_pyramid_config(lvl, 1),
                   lib.sm_cbca_intersect_config(lvl, 0), lib.sm_destroy(lvl)):
            assert st == _capi.SM_ESTATE
        assert lib.sm_pyramid_level(lvl, 0) is None
        assert sb.pyramid_levels == 2
    finally:
        sb.close()


# ---- 3. batched equals staged for what run_pyr does not cover ------------------------------------

def _staged(batch, md, L, agg, opt="sgm", refine=False, prm=None, cls=None):
    """main_.cpp:131-166 through the one-context-per-level API, pair by pair."""
    saved = {k: getattr(StereoMatching, k) for k in dict(cls or {}, costcalculation=0, aggregation=0, optimization=0, Do_refine=0)}
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", agg, opt
    StereoMatching.Do_refine = refine
    for k, v in (cls or {}).items():
        setattr(StereoMatching, k, v)
    try:
        maps = []
        for i in range(batch["lgray"].shape[0]):
            imgs, levels, m, sc = _pair(batch, i), [], md, 1
            for _ in range(L):
                H, W = imgs["lgray"].shape
                p = StereoMatching.Parameters(m, H, W, 13, 1, 2, 109, 10, "", sc)
                for k, v in (prm or {}).items():
                    setattr(p, k, v)
                sm = StereoMatching(imgs["lbgr"], imgs["rbgr"], imgs["lgray"], imgs["rgray"], None, None, None, None, p)
                sm.costCalculate()
                levels.append(sm)
                m, sc = m // 2 + 1, sc * 2
                imgs = {k: pyrDown(v) for k, v in imgs.items()}
            SolveAll(levels, L, 0.3)
            dp = levels[0].dispOptimize()
            maps.append(levels[0].refine() if refine else dp)
        return np.stack(maps)
    finally:
        for k, v in saved.items():
            setattr(StereoMatching, k, v)


VMTOP_THRES = float(np.float32(109 * 0.01))

# (H, W, aggregation, staged class attributes, staged Parameters fields, refine, StereoBatch overrides)
STAGED_CASES = [
    pytest.param(24, 30, "GF", {}, {}, False, dict(aggregation="GF"), id="GF-ximgproc"),
    pytest.param(40, 44, "GF", dict(MY_GUIDE=True), {}, False, dict(aggregation="GF", gf_mode=1), id="GF-my-guide"),
    pytest.param(24, 30, "NL", {}, {}, False, dict(aggregation="NL"), id="NL"),
    pytest.param(24, 30, "FIF", {}, {}, False, dict(aggregation="FIF"), id="FIF"),
    pytest.param(24, 30, "AWS", dict(AWS_RADIUS_V=3, AWS_RADIUS_U=3), {}, False,
                 dict(aggregation="AWS", aws_radius_v=3, aws_radius_u=3), id="AWS-r3"),
    pytest.param(24, 30, "BF", {}, {}, False, dict(aggregation="BF"), id="BF"),
    pytest.param(24, 30, "GFNL", {}, {}, False, dict(aggregation="GFNL"), id="GFNL"),
    pytest.param(24, 30, "CBCA", {}, dict(cbca_double_win=True), False, dict(cbca_double_win=True), id="cbca-double-win"),
    pytest.param(24, 30, "CBCA", {}, dict(cbca_intersect=False), False, dict(cbca_intersect=False), id="cbca-no-intersect"),
    pytest.param(24, 30, "CBCA", dict(Do_calPKR=True, Do_discontinuityAdjust=True), dict(Do_vmTop=True), True,
                 dict(do_refine=1, refine_ext=dict(do_pkr=True), refine_da=dict(on=True)), id="vmtop-pkr-da"),
]


@pytest.mark.parametrize("H,W,agg,cls,prm,refine,skw", STAGED_CASES)
def test_batched_equals_staged(H, W, agg, cls, prm, refine, skw):
    L, md, n = 2, 15, 2
    batch = S.make_batch(n, H, W, md + 1, first_index=1200)
    want = _staged(batch, md, L, agg, refine=refine, prm=prm, cls=cls)
    sb = StereoBatch(md, H, W, n, py_lvl=L, **skw)
    try:
        if prm.get("Do_vmTop"):
            sb.vmtop_config(True, 0, 2, VMTOP_THRES, 10)
        got = _run(sb, batch)
        np.testing.assert_array_equal(got, want)
        # the pyramid took part: the same context without it gives another map
        sb.pyramid_config(1)
        assert (_run(sb, batch) != want).any()
    finally:
        sb.close()


def test_config_order_and_level_refusal():
    """The aggregation-side config calls reach every level whichever order they and pyramid_config come in, and a
    setting a level cannot take fails with the level named and nothing changed."""
    from mystereomatching_amd import _capi
    L, md, n, H, W = 2, 15, 2, 24, 30
    batch = S.make_batch(n, H, W, md + 1, first_index=1200)
    maps = []
    for first in (True, False):
        sb = StereoBatch(md, H, W, n, py_lvl=L if first else 1)
        try:
            sb.cbca_double_config(True)
            sb.cbca_intersect_config(False)
            if not first:
                sb.pyramid_config(L)
            maps.append(_run(sb, batch))
        finally:
            sb.close()
    np.testing.assert_array_equal(maps[0], maps[1])
    sb = StereoBatch(md, H, W, n, aggregation="BF", py_lvl=L)
    try:
        ref = _run(sb, batch)
        with pytest.raises(_capi.SMError, match="level 1"):
            sb.bf_config(26, 12)       # 24 rows take a 26-row window (one reflection), level 1's 12 rows do not
        np.testing.assert_array_equal(_run(sb, batch), ref)
        sb.bf_config(5, 7)
        assert (_run(sb, batch) != ref).any()
    finally:
        sb.close()


# ---- 4. schedules --------------------------------------------------------------------------------

SCHED = dict(H=30, W=52, md=15, cap=10, L=2)


@functools.lru_cache(maxsize=None)
def _sched_sets():
    from oracle import oracle as O
    O.load()
    c = SCHED
    sets = [S.make_batch(c["cap"], c["H"], c["W"], c["md"] + 1, first_index=1300 + 20 * s) for s in range(2)]
    return sets, [_oracle_maps(O, b, c["H"], c["W"], c["md"], c["L"]) for b in sets]


@pytest.mark.parametrize("num_streams,sub_batch", [(1, 0), (2, 0), (0, 0), (2, 3)])
def test_schedules_give_the_same_maps(num_streams, sub_batch):
    import torch
    c = SCHED
    sets, want = _sched_sets()
    dev = [{k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in KEYS} for b in sets]
    torch.cuda.synchronize()
    sb = StereoBatch(c["md"], c["H"], c["W"], c["cap"], num_streams=num_streams, sub_batch=sub_batch, py_lvl=c["L"])
    try:
        ns = (10, 7, 10)
        outs = [torch.full((n, c["H"], c["W"]), -5, dtype=torch.int16, pin_memory=True).numpy() for n in ns]
        for i, n in enumerate(ns):
            sb.upload_async(*(dev[i % 2][k][:n] for k in KEYS))
            sb.run(0.3, download=False)
            sb.download_async(outs[i])
            if i >= 1:
                sb.download_wait(1)
                np.testing.assert_array_equal(outs[i - 1], want[(i - 1) % 2][:ns[i - 1]], err_msg=f"call {i - 1}")
            sb.upload_wait()
        sb.download_wait(0)
        np.testing.assert_array_equal(outs[2], want[0])
    finally:
        sb.close()


# ---- 5. reconfiguration on a live context --------------------------------------------------------

def test_reconfigure_live_context(oracle):
    H, W, md, n = 40, 52, 15, 2
    batch = S.make_batch(n, H, W, md + 1, first_index=1400)
    sb = StereoBatch(md, H, W, n)
    fresh = StereoBatch(md, H, W, n)
    try:
        for L in (1, 3, 1, 2):
            sb.pyramid_config(L)
            assert sb.pyramid_levels == L
            got = _run(sb, batch)
            np.testing.assert_array_equal(got, _oracle_maps(oracle, batch, H, W, md, L), err_msg=f"PY_LVL {L}")
            if L == 1:
                np.testing.assert_array_equal(got, _run(fresh, batch))
    finally:
        sb.close()
        fresh.close()


# ---- 6. the runner -------------------------------------------------------------------------------

def test_runner_run_many(oracle):
    H, W, md, n, L = 30, 52, 15, 4, 2
    batches = [S.make_batch(n, H, W, md + 1, first_index=1500 + 10 * i) for i in range(3)]
    fn = hip_compute_fn(md, H, W, n, device=0, py_lvl=L)
    try:
        got = DistributedBatchRunner(fn).run_many(batches, max_disp=md, reg_lambda=0.3)
        for g, b in zip(got, batches):
            np.testing.assert_array_equal(g, _oracle_maps(oracle, b, H, W, md, L))
    finally:
        fn.close()


# ---- 7. profile ----------------------------------------------------------------------------------

@pytest.mark.parametrize("num_streams,groups", [(1, 1), (0, 2)])
def test_profile_names_and_launch_counts(num_streams, groups):
    H, W, md, n, L, steps = 30, 52, 15, 8, 3, 2
    batch = S.make_batch(n, H, W, md + 1, first_index=1600)
    sb = StereoBatch(md, H, W, n, num_streams=num_streams, py_lvl=L)
    try:
        sb.profile(True)
        for _ in range(steps):
            _run(sb, batch)
        sb.synchronize()
        prof = sb.profile_read()
        for name in ("pyr_down@1", "pyr_down@2", "solve_all_pyr"):
            assert prof[name]["launches"] == groups * steps, (name, prof.get(name))
        for s in (1, 2):
            assert any(k.startswith("cbca_") and k.endswith(f"@{s}") for k in prof), sorted(prof)
            assert f"prep@{s}" in prof
        assert not any(k.endswith("@0") or k.endswith("@3") for k in prof)
    finally:
        sb.close()
