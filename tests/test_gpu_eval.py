"""The per-stage error table on the GPU (sm_eval_config): the batch path with three pairs against the CPU chain of
tests/pyref_stages.py -- stage names, every kept stage map, the counts against numpy, sum_sq against
sm_eval_stage_host bit for bit, the final map against the same run with evaluation off -- over the optimisers and
refine() configurations, schedules, the pyramid, the off state and the facades.

The chain of configurations A-D and F is computed on the CPU alone (the C oracle's maps and path sum, then the
restatements).  For E (vmTop) it starts from the maps of single-pair staged contexts, and for G (the pyramid) from
the batch's own stage 0 and DP[1] of pair 0: the oracle exposes neither selection nor the pyramid's raw maps."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import pyref_outlier as OC
import pyref_stages as PS
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import evaluate as E
from mystereomatching_amd import synthetic as S
from test_gpu_refine_ext import KEYS, Ctx, _oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
D, N, FIRST = 16, 3, 705
SHAPES = [(33, 41), (47, 91), (40, 70)]     # odd npix below one block; several blocks, odd npix; even npix
THRES = (1.0, 2.0)
DA_ARGS = dict(on=True, canny_low=20, canny_high=60, blur_side=84, blur_centre=87)

# name -> (sm_params overrides, StereoBatch's config dicts, the chain's switches)
CONFIGS = {
    "A": (dict(do_refine=1, rv_s=3), dict(refine_ext=dict(do_pkr=True, do_bg_ipol=True), refine_da=DA_ARGS),
          dict(do_pkr=True, do_bg=True, do_da=True)),
    "B": (dict(do_refine=1, rv_s=3, do_proper_ipol=0), dict(refine_ext=dict(do_pkr=True, do_bg_ipol=True), refine_da=DA_ARGS),
          dict(do_pkr=True, do_bg=True, do_da=True)),
    "C": (dict(do_refine=1), dict(refine_outlier=dict(classify=True, rv_combine=True, interpolate_type=3)),
          dict(classify=True, rv=True, itype=3)),
    "D": (dict(do_refine=1, optimization="so"), {}, {}),
    "E": (dict(do_refine=1), {}, {}),
    "F": (dict(), {}, {}),
}
VMTOP = (True, 0, 3, float(f32(1.09)), 10, True, False)


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    batch = S.make_batch(N, H, W, D, first_index=FIRST)
    rng = np.random.default_rng(H * 1000 + W)
    disc = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), (N, H, W))
    disc[1] = 0                                              # one pair's disc region is empty
    masks = [np.ascontiguousarray(batch["nonocc"]), np.full((N, H, W), 255, np.uint8), disc]
    return batch, np.ascontiguousarray(batch["gt"], f32), masks


def _oracle_cfg(O, H, W, over):
    kw = {k: v for k, v in over.items() if k != "optimization"}
    if "do_last_median_blur" in kw:
        kw["do_last_median"] = kw.pop("do_last_median_blur")
    if over.get("optimization") == "so":
        kw["optimization"] = 2
    return O.config(H, W, D - 1, **kw)


@functools.lru_cache(maxsize=None)
def _chains(name, H, W):
    """The CPU chain [(stage, map)] of every pair."""
    O = _oracle()
    over, _, sw = CONFIGS[name]
    batch, _, _ = _inputs(H, W)
    cfg = _oracle_cfg(O, H, W, over)
    refine = bool(over.get("do_refine"))
    out = []
    for i in range(N):
        pair = {k: batch[k][i] for k in KEYS}
        if name == "E":
            c = Ctx(H, W, D, pair, crafted=False)
            try:
                c.ok(c.lib.sm_vmtop_config(c.ctx, *[int(v) if not isinstance(v, float) else v for v in VMTOP]))
                c.optimize(0.3)
                d0, d1, vm = c.get_disp(0), c.get_disp(1), None
            finally:
                c.close()
        else:
            dumps = ("disp_raw", "disp_right", "final") if refine and name != "D" else (("disp_raw", "disp_right") if refine else ())
            ref = O.run_ex(pair, cfg, dumps=dumps)
            d0 = ref["disp_raw"] if refine else ref["disp"]
            d1, vm = ref.get("disp_right"), ref.get("final")
        arms = O.arms(pair["lbgr"], cfg) if refine else None
        ch = PS.chain(O, cfg, d0, d1, arms, pair["lbgr"], vm, refine=refine, vote=OC.vote_hv_rows,
                      name0=PS.stage0_name(over.get("optimization", "sgm"), name == "E"), **sw)
        if refine and name not in ("C", "E"):   # nothing extra in D; A and B end where the oracle's refine() would not
            assert (name != "D") or np.array_equal(ch[-1][1], ref["disp"])
        out.append(ch)
    return out


def _batch(H, W, over, cfgs, eval_kw=None, **more):
    sb = StereoBatch(D - 1, H, W, N, device=0, **over, **cfgs, **more)
    if eval_kw is not None:
        sb.eval_config(**eval_kw)
    return sb


def _check_table(tab, maps_of, gt, masks, names):
    """tab [N][S][3] against numpy's exact counts and sm_eval_stage_host's sum, on the maps maps_of(stage)[pair]."""
    assert list(tab.names) == names and tab.shape == (N, len(names), 3)
    for s in range(len(names)):
        maps = maps_of(s)
        for i in range(N):
            m = [mk[i] for mk in masks]
            want = PS.stage_err(maps[i], gt[i], m, THRES)
            host = E.eval_stage_host(maps[i], gt[i], PS.pack(maps[i].shape, m), THRES)
            for r in range(3):
                g, w = tab[i, s, r], want[r]
                where = (names[s], i, r)
                assert (int(g["count"]), int(g["invalid"])) == (w["count"], w["invalid"]), where
                assert [int(x) for x in g["bad"]] == w["bad"] + [0, 0], where
                assert np.float64(g["sum_sq"]).tobytes() == np.float64(host[r]["sum_sq"]).tobytes(), where
                assert g.tobytes() == np.asarray(host)[r].tobytes(), where


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configurations(name, H, W):
    over, cfgs, sw = CONFIGS[name]
    chains = _chains(name, H, W)
    names = [n for n, _ in chains[0]]
    O = _oracle()
    assert names == PS.stage_names(_oracle_cfg(O, H, W, over), over.get("optimization", "sgm"), name == "E",
                                   bool(over.get("do_refine")), sw.get("do_pkr", False), sw.get("do_bg", False), sw.get("do_da", False))
    # the chain alone, before the GPU is looked at: every stage the configuration is there for changes a pixel somewhere
    ch = {n: sum(PS.changed(c).get(n, 0) for c in chains) for n in names[1:]}
    if name == "A":
        assert all(ch[n] > 0 for n in ("od", "PKR", "RV0", "RV1", "pi", "da", "mb")) and ch["BG"] == 0, ch
    if name == "B":
        assert all(ch[n] > 0 for n in ("od", "PKR", "RV0", "RV1", "BG", "da", "mb")), ch
    if name == "C":
        od = np.stack([dict(c)["od"] for c in chains])
        assert ch["RV0"] > 0 and (od == -32).any() and (od == -48).any(), ch
    if name in ("D", "E"):
        assert ch["od"] > 0 and ch["mb"] > 0, ch
    batch, gt, masks = _inputs(H, W)
    sb = _batch(H, W, over, cfgs, dict(keep_maps=True, thresholds=THRES))
    try:
        if name == "E":
            sb.vmtop_config(*VMTOP)
        sb.upload(*(batch[k] for k in KEYS))
        sb.upload_truth(gt, *masks)
        assert sb.stage_names() == names                     # before the run: what it would record
        final = sb.run(0.3)
        assert sb.stage_names() == names
        kept = [sb.stage_maps(s) for s in range(len(names))]
        tab = sb.stage_errors()
        sb.eval_config(False)
        np.testing.assert_array_equal(sb.run(0.3), final)    # the same run with evaluation off
        with pytest.raises(_capi.SMError) as e:
            sb.stage_errors()
        assert e.value.status == _capi.SM_ESTATE
    finally:
        sb.close()
    for s, n in enumerate(names):
        for i in range(N):
            np.testing.assert_array_equal(kept[s][i], chains[i][s][1], err_msg=f"stage {n} pair {i}")
    np.testing.assert_array_equal(final, kept[-1])
    _check_table(tab, lambda s: [chains[i][s][1] for i in range(N)], gt, masks, names)
    assert int(tab["count"][1, :, 2].max()) == 0 and (tab.pbm()[1, :, 2] == 0).all() and (tab.rms()[1, :, 2] == 0).all()
    assert (tab["count"][:, :, 1] == H * W).all()
    if name == "C":
        assert (tab["invalid"][:, names.index("od"), 1] > 0).all()
    assert (tab["bad"][..., 2:] == 0).all()


def test_pyramid():
    """G: py_lvl = 2 at 40 x 70.  The table is level 0's; the last stage is the oracle's pyramid result; pair 0's
    refine() chain from the batch's own stage 0 and DP[1]."""
    H, W = 40, 70
    O = _oracle()
    batch, gt, masks = _inputs(H, W)
    cfg = O.config(H, W, D - 1, do_refine=1)
    sb = _batch(H, W, dict(do_refine=1), {}, dict(keep_maps=True, thresholds=THRES), py_lvl=2)
    try:
        lvl = sb._lib.sm_pyramid_level(sb._ctx, 1)
        assert sb._lib.sm_eval_config(C.c_void_p(lvl), 1, 0, 1, (C.c_float * 1)(1.0)) == _capi.SM_ESTATE   # a level context
        assert sb._lib.sm_upload_truth(C.c_void_p(lvl), 1, _capi.ptr(gt), None, None, None) == _capi.SM_ESTATE
        sb.upload(*(batch[k] for k in KEYS))
        sb.upload_truth(gt, *masks)
        sb.profile(True)
        final = sb.run(0.3)
        names = sb.stage_names()
        kept = [sb.stage_maps(s) for s in range(len(names))]
        tab = sb.stage_errors()
        d1 = sb.get_disp(1)
        prof = sb.profile_read()
    finally:
        sb.close()
    assert names == ["wta", "od", "RV0", "RV1", "pi", "mb"]
    assert prof["eval_stage"]["launches"] == len(names) and not any(k.startswith("eval_") and "@" in k for k in prof)
    for i in range(N):
        np.testing.assert_array_equal(final[i], O.run_pyr({k: batch[k][i] for k in KEYS}, cfg, 2), err_msg=f"pair {i}")
    np.testing.assert_array_equal(final, kept[-1])
    ch = PS.chain(O, cfg, kept[0][0], d1, O.arms(batch["lbgr"][0], cfg), batch["lbgr"][0])
    for s, (n, m) in enumerate(ch):
        np.testing.assert_array_equal(kept[s][0], m, err_msg=n)
    _check_table(tab, lambda s: kept[s], gt, masks, names)


def _run_a(H, W, num_streams, sub_batch, keep=False):
    over, cfgs, _ = CONFIGS["A"]
    batch, gt, masks = _inputs(H, W)
    sb = _batch(H, W, over, cfgs, dict(keep_maps=keep, thresholds=THRES), num_streams=num_streams, sub_batch=sub_batch)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.upload_truth(gt, *masks)
        sb.profile(True)
        sb.run(0.3, download=False)
        first = np.asarray(sb.stage_errors()).tobytes()
        prof = sb.profile_read()
        sb.run(0.3, download=False)
        second = np.asarray(sb.stage_errors()).tobytes()
    finally:
        sb.close()
    return first, second, prof


def test_schedules_and_repeats():
    """A under one and two streams and under sub-batches of one pair: the table's bytes are the same, and the same
    again from a second run of each schedule."""
    H, W = 47, 91
    tables = []
    for num_streams, sub_batch, groups in ((1, 0, 1), (2, 0, 1), (1, 1, 3), (2, 1, 3)):
        first, second, prof = _run_a(H, W, num_streams, sub_batch)
        assert first == second, (num_streams, sub_batch)
        tables.append(first)
        S_ = 9
        assert prof["eval_stage"]["launches"] == S_ * groups and prof["eval_final"]["launches"] == 2 * groups
        assert prof["eval_stage"]["bytes_per_launch"] == (N // groups) * H * W * 7
    assert all(t == tables[0] for t in tables[1:])
    _, _, prof = _run_a(H, W, 1, 0, keep=True)
    assert prof["eval_stage"]["bytes_per_launch"] == N * H * W * 9


def test_evaluation_off_and_missing_truth():
    H, W = 40, 70
    over, cfgs, _ = CONFIGS["A"]
    batch, gt, masks = _inputs(H, W)
    sb = _batch(H, W, over, cfgs)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.profile(True)
        off = sb.run(0.3)
        sb.synchronize()
        assert not any(k.startswith("eval_") for k in sb.profile_read())
        with pytest.raises(_capi.SMError) as e:
            sb.stage_errors()
        assert e.value.status == _capi.SM_ESTATE
        sb.eval_config(True, thresholds=(1.0,))
        with pytest.raises(_capi.SMError) as e:               # evaluation on, no truth
            sb.run(0.3)
        assert e.value.status == _capi.SM_ESTATE and "sm_upload_truth" in str(e.value)
        sb.upload_truth(gt[:2], *(m[:2] for m in masks))
        with pytest.raises(_capi.SMError) as e:               # fewer truth planes than pairs
            sb.run(0.3)
        assert e.value.status == _capi.SM_ESTATE and "sm_upload_truth" in str(e.value)
        with pytest.raises(_capi.SMError) as e:               # no run with evaluation on yet
            sb.stage_errors()
        assert e.value.status == _capi.SM_ESTATE
        sb.upload_truth(gt, masks[0], None, masks[2])         # the `all` region absent
        np.testing.assert_array_equal(sb.run(0.3), off)
        tab = sb.stage_errors()
        assert (tab["count"][:, :, 1] == 0).all() and (tab["count"][:, :, 0] > 0).all()
        with pytest.raises(_capi.SMError) as e:               # keep_maps was off
            sb.stage_maps(0)
        assert e.value.status == _capi.SM_ESTATE
    finally:
        sb.close()


def test_staged_calls_record_their_own_stages():
    """sm_disp_optimize records stage 0, sm_refine the rest; the rows are the batch's for the same pair."""
    H, W = 40, 70
    batch, gt, masks = _inputs(H, W)
    pair = {k: batch[k][0] for k in KEYS}
    c = Ctx(H, W, D, pair, crafted=False)
    try:
        th = (C.c_float * 2)(*THRES)
        c.ok(c.lib.sm_eval_config(c.ctx, 1, 1, 2, th))
        c.ok(c.lib.sm_upload_truth(c.ctx, 1, _capi.ptr(gt[0]), *[_capi.ptr(np.ascontiguousarray(m[0])) for m in masks]))
        c.optimize(0.3)
        assert c.lib.sm_eval_stage_count(c.ctx) == 1 and c.lib.sm_eval_stage_name(c.ctx, 0) == b"wta"
        one = np.zeros((1, 1, 3), _capi.STAGE_ERR_DTYPE)
        c.ok(c.lib.sm_get_stage_errors(c.ctx, 1, _capi.ptr(one)))
        d0 = c.get_disp(0)
        c.refine()
        S_ = c.lib.sm_eval_stage_count(c.ctx)
        names = [c.lib.sm_eval_stage_name(c.ctx, i).decode() for i in range(S_)]
        allr = np.zeros((1, S_, 3), _capi.STAGE_ERR_DTYPE)
        c.ok(c.lib.sm_get_stage_errors(c.ctx, 1, _capi.ptr(allr)))
        m0 = np.zeros((H, W), np.int16)
        c.ok(c.lib.sm_get_stage_maps(c.ctx, 1, 0, _capi.ptr(m0)))
    finally:
        c.close()
    assert names == ["wta", "od", "RV0", "RV1", "pi", "mb"]
    np.testing.assert_array_equal(m0, d0)
    assert one[0, 0].tobytes() == allr[0, 0].tobytes()
    sb = _batch(H, W, dict(do_refine=1), {}, dict(thresholds=THRES))
    try:
        sb.upload(*(batch[k] for k in KEYS))
        sb.upload_truth(gt, *masks)
        sb.run(0.3, download=False)
        assert np.asarray(sb.stage_errors())[0].tobytes() == allr[0].tobytes()
    finally:
        sb.close()


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(f"P5\n{img.shape[1]} {img.shape[0]}\n255\n".encode() + np.ascontiguousarray(img, np.uint8).tobytes())


def test_facades(tmp_path):
    """Both facades' stageErrors on one pair give the batch's rows (errorThreshold = 1; `all` absent)."""
    import subprocess
    from test_cpp_facade import _compile, write_ppm
    H, W = 40, 70
    batch, gt, masks = _inputs(H, W)
    p = {k: batch[k][0] for k in KEYS}
    gti = np.clip(np.rint(gt[0]), 0, 255).astype(np.uint8)   # what a disparity PNG holds
    dt = gti.astype(f32)
    sb = StereoBatch(D - 1, H, W, 1, device=0, do_refine=1, eval=dict(thresholds=(1.0,)))
    try:
        sb.upload(*(p[k][None] for k in KEYS))
        sb.upload_truth(dt[None], masks[0][:1], None, masks[2][:1])
        sb.run(0.3, download=False)
        rows = E.err_rows(sb.stage_errors()[0], (True, False, True))
    finally:
        sb.close()
    assert len(rows) == 6 * 2 and rows[0][:2] == ("wta", "nonocc") and rows[-1][:2] == ("mb", "disc")
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_stageErrors)
    try:
        cls.costcalculation, cls.aggregation, cls.optimization = "censusGrad", "CBCA", "sgm"
        cls.Do_refine, cls.Do_stageErrors = True, True
        sm = cls(p["lbgr"], p["rbgr"], p["lgray"], p["rgray"], dt, None, masks[0][0], masks[2][0], param=cls.Parameters(D - 1, H, W))
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        sm.dispOptimize()
        assert [r[0] for r in sm.stageErrors()] == ["wta", "wta"]
        sm.refine()
        assert sm.stage_errors() == rows
        # calErr stays what it was, and agrees on the final map within the float sum's error
        cal = sm.calErr()
        assert cal["nonocc"][0] == rows[-2][2] and abs(cal["nonocc"][1] - rows[-2][3]) <= 1e-3 * rows[-2][3]
    finally:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_stageErrors = saved
    exe = str(tmp_path / "eval_facade_check")
    _compile(os.path.join(ROOT, "tests", "cpp", "eval_facade_check.cpp"), exe)
    write_ppm(tmp_path / "l.ppm", p["lbgr"])
    write_ppm(tmp_path / "r.ppm", p["rbgr"])
    _write_pgm(tmp_path / "gt.pgm", gti)
    _write_pgm(tmp_path / "nonocc.pgm", masks[0][0])
    _write_pgm(tmp_path / "disc.pgm", masks[2][0])
    r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(D - 1), str(tmp_path / "gt.pgm"),
                        str(tmp_path / "nonocc.pgm"), str(tmp_path / "disc.pgm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.splitlines() == E.format_err_lines(rows)


def test_eval_tool_prints_one_line_per_stage(tmp_path, monkeypatch, capsys):
    """tools/sm_eval.py --stages on a Middlebury-layout folder: the JSON line, then one err-txt line per stage."""
    import importlib.util
    import json
    from PIL import Image
    H, W = 90, 120
    p = S.make_pair(H, W, 60, 17)
    d = tmp_path / "teddy"
    d.mkdir()
    Image.fromarray(p["lbgr"][..., ::-1]).save(d / "im2.png")
    Image.fromarray(p["rbgr"][..., ::-1]).save(d / "im6.png")
    Image.fromarray(np.clip(p["gt"] * 4, 0, 255).astype(np.uint8)).save(d / "disp2.png")
    Image.fromarray(p["nonocc"]).save(d / "nonocc.png")
    spec = importlib.util.spec_from_file_location("sm_eval", os.path.join(ROOT, "tools", "sm_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    saved = (StereoMatching.Do_refine, StereoMatching.Do_stageErrors)
    try:
        monkeypatch.setattr(sys, "argv", ["sm_eval.py", str(tmp_path), "--objects", "teddy", "--refine", "--stages"])
        tool.main()
    finally:
        StereoMatching.Do_refine, StereoMatching.Do_stageErrors = saved
    out = capsys.readouterr().out.splitlines()
    rec = json.loads(out[0])
    assert [ln.split("\t")[0] for ln in out[1:]] == ["wta", "od", "RV0", "RV1", "pi", "mb"]
    for ln in out[1:]:
        f = ln.split("\t")
        assert f[1] == "nonocc" and f[2].startswith("PBM: ") and f[3].startswith("RMS: ") and len(f) == 5 and f[4] == ""
    # the last line is the final map's: calErr's own figure for it, to the digits printed
    assert abs(float(out[-1].split("\t")[2][5:]) - rec["bad1.0_nonocc"] / 100) < 1e-5
