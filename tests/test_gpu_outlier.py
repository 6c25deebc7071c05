"""GPU parity of refine()'s outlier classification (sm_refine_oc.hip: the classifying LR check and RV_combine_BG)
against the restatement tests/pyref_outlier.py.  Every comparison is exact: int16 maps and mask bytes.

The single stages run on crafted maps through sm_set_disp under the "crafted" context of test_gpu_refine_ext.py
(optimization "" on AD costs, every other stage off).  refine() always starts with the LR check, so a hole's class is
crafted through it: with LRmaxDiff = 1e9 a pixel fails only for d < 0 or d > u, and a failed pixel u is a mismatch
exactly where DP[1](u) = 0 is planted (DP[1] = -1 elsewhere); -64 holes come from the peak-ratio stage on a crafted
volume (a flat cost row is marked), -1 holes from the plain LR check with classification off.  A valid value must
be <= its column to survive the LR check.  Arms come from sm_get_arms and are fed to the restatement.

The pipeline cases compare with the restatement composed with the C oracle's stages on the maps and the volume the
context holds after sm_disp_optimize.
"""
import functools

import numpy as np
import pytest

import pyref_outlier as P
import pyref_refine_ext as RX
from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S
from test_gpu_refine_ext import KEYS, Ctx, _oracle

pytestmark = pytest.mark.gpu

f32 = np.float32
OCC, MIS, PKR = P.DISP_OCC, P.DISP_MIS, P.DISP_PKR


def outlier(c, classify=False, rv=False, itype=0, disp_mis=MIS):
    c.ok(c.lib.sm_refine_outlier_config(c.ctx, int(classify), disp_mis, int(rv), itype))


def lrc_mask(c):
    out = np.full((c.H, c.W), 7, np.uint8)
    c.ok(c.lib.sm_get_lrc_mask(c.ctx, _capi.ptr(out)))
    return out


def arms_of(c):
    out = np.empty((c.H, c.W, 4), np.uint16)
    c.ok(c.lib.sm_get_arms(c.ctx, 0, _capi.ptr(out)))
    return out


# ---- the classifying LR check ------------------------------------------------------------------------------

def _classify_maps(rng, H, W, D):
    """DP0 / DP1 with -1, 0, d > u, D - 1 and, in DP1, values >= D."""
    vals0 = np.array([-1, 0, 1, D - 1, D // 2, 2 * W], np.int64)
    d0 = np.where(rng.random((H, W)) < 0.5, rng.integers(0, D, (H, W)), rng.choice(vals0, (H, W))).astype(np.int16)
    vals1 = np.array([-1, 0, D - 1, D, D + 3, 1], np.int64)
    d1 = np.where(rng.random((H, W)) < 0.5, rng.integers(0, D, (H, W)), rng.choice(vals1, (H, W))).astype(np.int16)
    return d0, d1


@pytest.mark.parametrize("H,W,D", [(2, 2, 2), (3, 63, 16), (4, 64, 16), (5, 65, 70), (3, 130, 64), (2, 300, 256)])
def test_classify(H, W, D):
    rng = np.random.default_rng(100 * W + D)
    d0, d1 = _classify_maps(rng, H, W, D)
    seen = set()
    for maxdiff in (0.0, 1.0, 1e9):
        c = Ctx(H, W, D, lr_max_diff=maxdiff)
        try:
            c.optimize()
            with pytest.raises(_capi.SMError):   # no mask before a classifying refine
                lrc_mask(c)
            c.set_disp(d0, d1)
            outlier(c, classify=True)
            got = c.refine()
            mask = lrc_mask(c)
            want, wmask = P.lr_classify(d0, d1, D, maxdiff)
            np.testing.assert_array_equal(mask, wmask, err_msg=f"maxdiff {maxdiff}")
            np.testing.assert_array_equal(got, want, err_msg=f"maxdiff {maxdiff}")
            np.testing.assert_array_equal(want, P.lr_classify(d0, d1, D, maxdiff, scatter=True)[0])
            assert set(np.unique(mask)) <= {0, 255} and ((mask == 255) == (got < 0)).all()
            assert (got[mask == 0] == d0[mask == 0]).all()
            seen |= set(np.unique(got[got < 0]).tolist())
            # other labels
            c.set_disp(d0, d1)
            outlier(c, classify=True, disp_mis=-1)
            got = c.refine()
            np.testing.assert_array_equal(got, P.lr_classify(d0, d1, D, maxdiff, disp_mis=-1)[0])
            # every failed pixel a mismatch (DP1 = 0: x + 0 == u), then none (DP1 = -1: nothing scatters)
            for fill, label in ((0, MIS), (-1, OCC)):
                d1c = np.full((H, W), fill, np.int16)
                c.set_disp(d0, d1c)
                outlier(c, classify=True)
                got = c.refine()
                np.testing.assert_array_equal(got, P.lr_classify(d0, d1c, D, maxdiff)[0])
                assert (got < 0).any() and (got[got < 0] == label).all()
            # off again: the plain check, and no mask
            c.set_disp(d0, d1)
            outlier(c)
            np.testing.assert_array_equal(c.refine(), _oracle().lr_check(d0, d1, _oracle().config(H, W, D - 1, do_refine=1, lr_max_diff=maxdiff)))
            with pytest.raises(_capi.SMError):
                lrc_mask(c)
        finally:
            c.close()
    if W > 2:
        assert seen == {OCC, MIS}


# ---- RV_combine_BG on crafted maps ---------------------------------------------------------------------------

def _uniform(H, W):
    z = np.full((H, W, 3), 90, np.uint8)
    return dict(lbgr=z, rbgr=z, lgray=z[:, :, 0].copy(), rgray=z[:, :, 0].copy())


def _blocks(H, W):
    """Flat colour blocks with edges inside the 64 x 4 tiles and at columns 20, 45, 63 | 64 and rows 7, 18, 29: the
    arms end there."""
    img = np.zeros((H, W, 3), np.uint8)
    for i, (v0, v1) in enumerate(((0, 7), (7, 18), (18, 29), (29, H))):
        for j, (u0, u1) in enumerate(((0, 20), (20, 45), (45, 64), (64, W))):
            img[v0:v1, u0:u1] = (40 + 50 * ((i + j) % 4), 200 - 45 * ((2 * i + j) % 4), 30 + 70 * ((i + 3 * j) % 3))
    g = img[:, :, 1].copy()
    return dict(lbgr=img, rbgr=img, lgray=g, rgray=g)


def _craft(rng, H, W, D, hole_rate, dvals, pkr_rate=0.25, mis_rate=0.5, noise=0.25, over_d=False):
    """Returns (d0, d1, vol, pkr_pixels): d0 has valid values <= u concentrated on `dvals` by 6-row x 16-column
    cells (so that votes pass and fail), holes (-5) at hole_rate; DP1 plants a mismatch at mis_rate of the columns;
    the volume is flat (marked by the peak-ratio stage) on pkr_rate of the pixels."""
    vv, uu = np.mgrid[0:H, 0:W]
    cell = (vv // 6) * 7 + uu // 16
    base = np.asarray(dvals)[cell % len(dvals)]
    d0 = np.where(rng.random((H, W)) < noise, rng.integers(0, D, (H, W)), base)
    if over_d:   # values >= D that survive the LR check: counted in validNum, in no bin
        d0 = np.where(rng.random((H, W)) < 0.1, D + rng.integers(0, 9, (H, W)), d0)
    d0 = np.minimum(d0, uu).astype(np.int16)
    d0[rng.random((H, W)) < hole_rate] = -5
    d1 = np.where(rng.random((H, W)) < mis_rate, 0, -1).astype(np.int16)
    flat = rng.random((H, W)) < pkr_rate
    vol = np.full((H, W, D), 5, f32)
    vol[:, :, 0] = 1
    vol[flat] = 3
    return d0, d1, vol, flat


def _crafted_expect(d0, d1, flat, arms, D, classify, pkr, rounds, itype, rv_s, depth, stats=None):
    """The crafted context's refine(): LR check (LRmaxDiff 1e9), peak-ratio marks, RV_combine_BG rounds."""
    H, W = d0.shape
    if classify:
        d, mask = P.lr_classify(d0, d1, D, 1e9)
    else:
        O = _oracle()
        d, mask = O.lr_check(d0, d1, O.config(H, W, D - 1, do_refine=1, lr_max_diff=1e9)), None
    labelled = d
    if pkr:
        d = RX.sign_dp(d, flat.astype(np.uint8))
    for _ in range(rounds):
        d = P.rv_combine(d, arms, D, rv_s, 0.4, itype, depth, stats=stats, vote=P.vote_hv_rows)
    return d, mask, labelled


def _rv_case(pair, H, W, D, itype, cases, dvals, over_d=False):
    rng = np.random.default_rng(1000 * itype + H + D)
    filled = kept = carried = 0
    classes = set()
    for hole_rate, rv_s, depth, classify, rounds in cases:
        d0, d1, vol, flat = _craft(rng, H, W, D, hole_rate, dvals, over_d=over_d)
        c = Ctx(H, W, D, pair, do_region_vote=1, region_vote_nums=rounds, rv_s=rv_s)
        try:
            c.set_volume(vol)
            c.optimize()
            arms = arms_of(c)
            c.set_disp(d0, d1)
            c.config(do_pkr=True, depth=depth)
            outlier(c, classify=classify, rv=True, itype=itype)
            got = c.refine()
            np.testing.assert_array_equal(c.mask(), flat.astype(np.uint8))
            stats = {}
            want, wmask, labelled = _crafted_expect(d0, d1, flat, arms, D, classify, True, rounds, itype, rv_s, depth, stats)
            msg = f"type {itype} holes {hole_rate} rv_s {rv_s} depth {depth} classify {classify}"
            np.testing.assert_array_equal(got, want, err_msg=msg)
            if classify:
                np.testing.assert_array_equal(lrc_mask(c), wmask)
            before = RX.sign_dp(labelled, flat.astype(np.uint8))
            classes |= set(np.unique(before[before < 0]).tolist())
            filled += int(((before < 0) & (want >= 0)).sum())
            kept += int((want < 0).sum())
            carried += stats["carried"]
            assert (want[want < 0] == before[want < 0]).all()   # an unfilled hole keeps its label
        finally:
            c.close()
    return arms, filled, kept, carried, classes


# (hole rate, rv_s, depth, classify, rounds)
RV_CASES = [(0.05, 20, 1000, True, 1), (0.6, 0, 1, True, 2), (0.6, 20, 0, True, 1), (0.3, 20, 1000, False, 1)]


@pytest.mark.parametrize("itype", [0, 1, 2, 3])
def test_rv_combine_uniform_d256(itype):
    """A uniform 75 x 75 image: arms of 34, so a 69 x 69 region (4761 pixels) in the middle: counts above 255 in a
    256-bin histogram."""
    H = W = 75
    arms, filled, kept, carried, classes = _rv_case(_uniform(H, W), H, W, 256, itype, RV_CASES, dvals=(3, 9, 3, 20, 3, 3, 31, 3, 9))
    a = arms[37, 37].astype(int)
    assert (a == 34).all() and (a[0] + a[1] + 1) * (a[2] + a[3] + 1) == 4761
    assert filled > 100 and kept > 100
    assert classes == {-1, OCC, MIS, PKR}
    if itype >= 2:
        assert carried > 0


@pytest.mark.parametrize("itype", [0, 1, 2, 3])
def test_rv_combine_blocks(itype):
    """40 x 70 of flat colour blocks: arms that end inside the tile and at the 64-column tile edge; values >= D."""
    H, W, D = 40, 70, 16
    pair = _blocks(H, W)
    arms, filled, kept, carried, classes = _rv_case(pair, H, W, D, itype, RV_CASES, dvals=(2, 7, 7, 11, 0), over_d=True)
    # (an arm crosses an edge by the minimum arm length, 1)
    assert arms[10, 62, 1] == 1 and arms[10, 64, 0] == 1 and arms[10, 30, 0] == 10 and arms[10, 30, 2] == 3
    assert filled > 100 and kept > 50
    assert classes == {-1, OCC, MIS, PKR}
    if itype >= 2:
        assert carried > 0


def _vote_ctx(H, W, D, rv_s, itype=0):
    c = Ctx(H, W, D, _uniform(H, W), do_region_vote=1, region_vote_nums=1, rv_s=rv_s, arm_l=2, arm_l_out=2)
    c.optimize()
    return c


def test_vote_boundaries_and_ties():
    """Ratio boundaries (2 of 5 is not above 0.4f, 3 of 7 is), validNum == rv_s against rv_s + 1, the lowest
    disparity on a tie: a 5 x 5 region (arms of 2 on a uniform image) around one mismatch hole."""
    H, W, D = 9, 40, 16
    v, u = 4, 20

    def run(vals, rv_s):
        """vals: the valid values of the hole's region, row-major from its top-left; the rest are holes."""
        c = _vote_ctx(H, W, D, rv_s)
        try:
            arms = arms_of(c)
            assert (arms[v - 2:v + 3, u] == 2).all()
            d0 = np.full((H, W), -5, np.int16)
            cells = [(a, b) for a in range(v - 2, v + 3) for b in range(u - 2, u + 3) if (a, b) != (v, u)]
            for (a, b), x in zip(cells, vals):
                d0[a, b] = x
            d1 = np.full((H, W), -1, np.int16)
            d1[v, u] = 0                                # the hole is a mismatch, the others occlusions
            c.set_disp(d0, d1)
            outlier(c, classify=True, rv=True, itype=2)   # occlusions take bg at depth 0: nothing
            c.config(depth=0)
            got = c.refine()
            want, _, _ = _crafted_expect(d0, d1, None, arms, D, True, False, 1, 2, rv_s, 0)
            np.testing.assert_array_equal(got, want)
            assert got[v, u - 3] == OCC
            return int(got[v, u])
        finally:
            c.close()

    assert run([7, 7, 1, 2, 3], 0) == MIS               # 2 of 5: (float)2 / 5 > 0.4f is false
    assert run([7, 7, 7, 1, 2, 3, 4], 0) == 7           # 3 of 7
    assert run([7, 7, 7, 7, 7], 5) == MIS               # validNum == rv_s
    assert run([7, 7, 7, 7, 7, 7], 5) == 7              # rv_s + 1
    assert run([9, 4, 9, 4, 1], 0) == MIS               # a tie of 2 of 5
    assert run([9, 4, 9, 4], 0) == 4                    # a tie above the ratio: the lowest disparity
    assert run([12, 3, 12, 3, 3, 12], 0) == 3


# ---- the carry of types 2 and 3 ------------------------------------------------------------------------------

@pytest.mark.parametrize("itype", [2, 3])
def test_carry_placements(itype):
    """-64 holes first in the image, first in a row, at columns 63 / 64 and as a run; what they take is the result of
    the last classified hole before them, across a row end, -1 at the start of the image."""
    H, W, D = 6, 130, 16
    uu = np.arange(W)[None, :] * np.ones((H, 1), int)
    d0 = np.minimum(5, uu).astype(np.int16)
    d1 = np.full((H, W), -1, np.int16)
    flat = np.zeros((H, W), bool)
    flat[0, 0] = flat[0, 1] = True                      # before any classified hole: stay
    d0[0, 5] = -5                                       # an occlusion, filled by bg (4)
    flat[0, 6:10] = True                                # a run: all take 4
    flat[0, 63] = flat[0, 64] = True
    d0[0, 100] = -5
    d0[0, 99], d0[0, 101] = 2, 8                        # bg: min(8, 2) = 2
    flat[1, 0] = True                                   # first in its row: takes 2 across the row end
    d0[2, 64:] = -5                                     # a row end of occlusions: the last one has no right value
    d0[2, 63] = 9
    flat[3, 0] = flat[3, 63] = flat[3, 64] = True       # take 9
    d0[4, :] = -5                                       # a row of occlusions, unfilled at depth 1000 (no valid value)
    flat[5, 0] = flat[5, 70] = True                     # the last result is -1: stay
    vol = np.full((H, W, D), 5, f32)
    vol[:, :, 0] = 1
    vol[flat] = 3
    c = Ctx(H, W, D, _uniform(H, W), do_region_vote=1, region_vote_nums=1, rv_s=0)
    try:
        c.set_volume(vol)
        c.optimize()
        arms = arms_of(c)
        c.set_disp(d0, d1)
        c.config(do_pkr=True)
        outlier(c, classify=True, rv=True, itype=itype)
        got = c.refine()
        stats = {}
        want, _, _ = _crafted_expect(d0, d1, flat, arms, D, True, True, 1, itype, 0, 1000, stats)
        np.testing.assert_array_equal(got, want)
    finally:
        c.close()
    if itype == 2:   # (type 3 lets the vote in on occlusions; the expectations below are type 2's)
        # (0, 5): the values are min(5, u), the marks at 6..9 are holes: bg = min(left 4, right 5 at column 10) = 4
        assert got[0, 0] == PKR and got[0, 1] == PKR and (got[0, 5:10] == 4).all() and got[0, 63] == 4 and got[0, 64] == 4
        assert got[0, 100] == 2 and got[1, 0] == 2 and (got[3, [0, 63, 64]] == 9).all()
        assert (got[4] == OCC).all() and got[5, 0] == PKR and got[5, 70] == PKR
        assert stats["carried"] == 10


# ---- whole pipeline ------------------------------------------------------------------------------------------

# chosen on the CPU (the C oracle's "sgm" and "so" maps + the restatement), for every mode below: >= 20 pixels of
# each class, and a DISP_OCC hole that properIpol fills with a value the closest-colour rule would not give
PIPE = {(40, 70, 16): 705, (96, 128, 32): 701}


def _pipe_state(H, W, D, so, ext):
    """One pair through sm_disp_optimize; the maps, the volume, the arms."""
    pair = S.make_pair(H, W, D, PIPE[(H, W, D)])
    over = dict(optimization=2) if so else {}
    c = Ctx(H, W, D, pair, crafted=False, **over)
    if ext:
        c.config(do_pkr=True, do_bg=True, do_se=True)
        c.ok(c.lib.sm_refine_da_config(c.ctx, 1, 20, 60, 84, 87))
    c.optimize(0.3)
    d0, d1 = c.get_disp(0), c.get_disp(1)
    vm = c.volume() if ext else None
    return pair, c, d0, d1, vm


@pytest.mark.parametrize("H,W,D", sorted(PIPE))
@pytest.mark.parametrize("mode", ["sgm", "ext", "so"])
def test_pipeline_against_restatement(H, W, D, mode):
    """censusGrad + CBCA + sgm (or "so") with do_refine: classification alone, then with RV_combine_BG for every
    type; `ext` adds the peak-ratio check, BGIpol, the discontinuity adjustment and the sub-pixel map."""
    O = _oracle()
    ext = mode == "ext"
    pair, c, d0, d1, vm = _pipe_state(H, W, D, mode == "so", ext)
    try:
        cfg = O.config(H, W, D - 1, do_refine=1)
        arms = O.arms(pair["lbgr"], cfg)
        np.testing.assert_array_equal(arms_of(c), arms)
        kw = dict(do_pkr=ext, do_bg=ext, do_da=ext, do_se=ext, vote=P.vote_hv_rows)
        base = None
        for classify, rv, itype in [(True, False, 0)] + [(True, True, t) for t in range(4)] + [(False, True, 0)]:
            c.set_disp(d0, d1)
            outlier(c, classify=classify, rv=rv, itype=itype)
            got = c.refine()
            stats = {}
            want = P.refine_outlier(O, cfg, d0, d1, arms, pair["lbgr"], vm, classify=classify, rv=rv, itype=itype,
                                    stats=stats, **kw)
            msg = f"classify {classify} rv {rv} type {itype}"
            np.testing.assert_array_equal(got, want["disp"], err_msg=msg)
            if classify:
                np.testing.assert_array_equal(lrc_mask(c), want["mask"], err_msg=msg)
                lab = want["labelled"]
                assert (lab == OCC).sum() >= 20 and (lab == MIS).sum() >= 20, ((lab == OCC).sum(), (lab == MIS).sum())
                if not rv:   # the classification-only step: properIpol's DISP_OCC rule decides somewhere
                    assert stats["occ_rule_differs"] >= 1
                    base = got
            if ext:
                np.testing.assert_array_equal(c.mask(), want["pkr_mask"], err_msg=msg)
                np.testing.assert_array_equal(c.se().view(np.uint32), want["se"].view(np.uint32), err_msg=msg)
        # both off: the parent's refine
        c.set_disp(d0, d1)
        outlier(c)
        off = c.refine()
        np.testing.assert_array_equal(off, P.refine_outlier(O, cfg, d0, d1, arms, pair["lbgr"], vm, **kw)["disp"])
        if base is not None:
            assert (base != off).any()
    finally:
        c.close()


# ---- schedules, batches, the facades ---------------------------------------------------------------------------

ON = dict(classify=True, rv_combine=True, interpolate_type=3)
HS, WS, DS = 40, 70, 16


@functools.lru_cache(maxsize=None)
def _three():
    """Three pairs and what single-pair staged contexts + the restatement give for them, with the peak-ratio
    check on (its -64 holes are the carry's customers)."""
    O = _oracle()
    batch = S.make_batch(3, HS, WS, DS, first_index=710)
    cfg = O.config(HS, WS, DS - 1, do_refine=1)
    want = []
    for i in range(3):
        pair = {k: batch[k][i] for k in KEYS}
        c = Ctx(HS, WS, DS, pair, crafted=False)
        try:
            c.config(do_pkr=True)
            c.optimize(0.3)
            stats = {}
            w = P.refine_outlier(O, cfg, c.get_disp(0), c.get_disp(1), O.arms(pair["lbgr"], cfg), pair["lbgr"], c.volume(),
                                 classify=True, rv=True, itype=3, do_pkr=True, vote=P.vote_hv_rows)
            # the first round's carry, for the batch test below
            d = RX.sign_dp(w["labelled"], w["pkr_mask"])
            P.rv_combine(d, O.arms(pair["lbgr"], cfg), DS, cfg.rv_s, cfg.rv_ratio, 3, stats=stats, vote=P.vote_hv_rows)
            w["carried"] = stats["carried"]
            want.append(w)
        finally:
            c.close()
    return batch, want


@pytest.mark.parametrize("sub_batch,num_streams", [(0, 1), (1, 2), (1, 1), (0, 2)])
def test_schedules(sub_batch, num_streams):
    batch, want = _three()
    sb = StereoBatch(DS - 1, HS, WS, 3, device=0, do_refine=1, sub_batch=sub_batch, num_streams=num_streams,
                     refine_ext=dict(do_pkr=True), refine_outlier=ON)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
        mask = sb.get_lrc_mask()
        np.testing.assert_array_equal(sb.run(0.3), got)
    finally:
        sb.close()
    np.testing.assert_array_equal(mask, want[0]["mask"])
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i]["disp"], err_msg=f"pair {i}")
    assert sum(w["carried"] for w in want) > 0


def test_pyramid_level_0_only():
    """py_lvl 2: the switches concern level 0's refine; every schedule gives the same maps."""
    batch, _ = _three()
    maps = []
    for sub_batch, num_streams in ((0, 1), (1, 2)):
        sb = StereoBatch(DS - 1, HS, WS, 3, device=0, do_refine=1, sub_batch=sub_batch, num_streams=num_streams,
                         refine_outlier=ON, py_lvl=2)
        try:
            sb.upload(*(batch[k] for k in KEYS))
            sb.profile(True)
            maps.append(sb.run(0.3))
            sb.synchronize()
            prof = sb.profile_read()
        finally:
            sb.close()
        assert "refine_lr_classify" in prof and not any(k.startswith("refine_") and "@" in k for k in prof)
    np.testing.assert_array_equal(maps[0], maps[1])


CARRY_PAIRS = (725, 730, 745)   # chosen on the CPU: see test_carry_stays_inside_its_pair


def test_carry_stays_inside_its_pair():
    """A batch of three pairs, each of which begins (raster order) with a hole of neither class and ends its scan with
    a filled classified hole: were the carry to cross a pair boundary, the next pair's leading holes would be filled.
    LRmaxDiff = 1e9 leaves few LR failures, ratio_PKR = 0.3 marks many pixels, the pairs' first holes among them; one RV_combine_BG round of type 3
    and nothing after it, so the map shows the round's result."""
    O = _oracle()
    kw = dict(do_refine=1, lr_max_diff=1e9, region_vote_nums=1, do_proper_ipol=0, do_last_median_blur=0)
    cfg = O.config(HS, WS, DS - 1, do_refine=1, lr_max_diff=1e9, region_vote_nums=1, do_proper_ipol=0, do_last_median=0)
    pairs = [S.make_pair(HS, WS, DS, i) for i in CARRY_PAIRS]
    want = []
    for pair in pairs:
        c = Ctx(HS, WS, DS, pair, crafted=False, **{k: v for k, v in kw.items() if k != "do_refine"})
        try:
            c.config(do_pkr=True, ratio=0.3)
            c.optimize(0.3)
            arms = O.arms(pair["lbgr"], cfg)
            w = P.refine_outlier(O, cfg, c.get_disp(0), c.get_disp(1), arms, pair["lbgr"], c.volume(), classify=True, rv=True,
                                 itype=3, do_pkr=True, pkr_ratio=0.3, vote=P.vote_hv_rows)
            stats = {}
            d = RX.sign_dp(w["labelled"], w["pkr_mask"])
            r = P.rv_combine(d, arms, DS, cfg.rv_s, cfg.rv_ratio, 3, stats=stats, vote=P.vote_hv_rows)
            np.testing.assert_array_equal(r, w["disp"])
            first = int(np.flatnonzero(d.ravel() < 0)[0])       # the pair's first hole in raster order
            assert d.ravel()[first] == PKR and stats["last"] >= 0 and stats["carried"] > 0, (int(d.ravel()[first]), stats)
            assert w["disp"].ravel()[first] == PKR              # before the pair's first classified hole: stays
            want.append(w["disp"])
        finally:
            c.close()
    sb = StereoBatch(DS - 1, HS, WS, 3, device=0, refine_ext=dict(do_pkr=True, pkr_ratio=0.3), refine_outlier=ON, **kw)
    try:
        sb.upload(*(np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in KEYS))
        got = sb.run(0.3)
    finally:
        sb.close()
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"pair {i}")


def test_switches_off_change_nothing():
    """Both switches off (after having been on): the parent's maps, and none of the new profile names.  The maps are
    compared with the C oracle's refine() on three pairs (what the recorded refine fixtures hold, computed here),
    and, on the recorded fixture tests/golden/large_teddy_refine_d64.npz itself, with its map."""
    O = _oracle()
    batch, _ = _three()
    sb = StereoBatch(DS - 1, HS, WS, 3, device=0, do_refine=1, num_streams=1)
    try:
        sb.refine_outlier_config(**ON)
        sb.refine_outlier_config()
        sb.upload(*(batch[k] for k in KEYS))
        sb.profile(True)
        got = sb.run(0.3)
        sb.synchronize()
        prof = sb.profile_read()
        with pytest.raises(_capi.SMError):
            sb.get_lrc_mask()
        assert not any(k in prof for k in ("refine_lr_classify", "refine_rv_combine", "refine_rv_carry"))
        assert prof["refine_lr_check"]["launches"] == 1 and prof["refine_region_vote"]["launches"] == 2
        sb.refine_outlier_config(**ON)
        sb.profile_reset()
        sb.run(0.3)
        sb.synchronize()
        prof = sb.profile_read()
    finally:
        sb.close()
    cfg = O.config(HS, WS, DS - 1, do_refine=1)
    for i in range(3):
        np.testing.assert_array_equal(got[i], O.run_ex({k: batch[k][i] for k in KEYS}, cfg)["disp"])
    npix = 3 * HS * WS
    # (a name stays in the table once registered: the replaced launches are there with no launch)
    assert prof["refine_lr_check"]["launches"] == 0 and prof["refine_region_vote"]["launches"] == 0
    assert prof["refine_lr_classify"]["launches"] == 1 and prof["refine_lr_classify"]["bytes_per_launch"] == npix * 7
    assert prof["refine_rv_combine"]["launches"] == 2 and prof["refine_rv_combine"]["bytes_per_launch"] == npix * 6
    assert prof["refine_rv_carry"]["launches"] == 2 and prof["refine_rv_carry"]["bytes_per_launch"] == npix * 6 + 3 * HS * 4


def test_switches_off_recorded_refine_fixture():
    """tests/golden/large_teddy_refine_d64.npz (the oracle's refined Teddy-shaped map, the fixture of
    test_gpu_large_fixtures.py): a context whose switches were on and are off again gives it bit for bit, with the
    parent's refine launches only."""
    import os
    from test_gpu_large_fixtures import _diff_msg, _load, _pair
    z, ov = _load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "large_teddy_refine_d64.npz"))
    assert ov.get("do_refine") == 1
    pair, H, W, md = _pair(z)
    sb = StereoBatch(md, H, W, 1, device=0, num_streams=1, **ov)
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        sb.refine_outlier_config(**ON)
        on = sb.run(0.3)[0].copy()
        sb.refine_outlier_config()
        sb.profile(True)
        got = sb.run(0.3)[0]
        sb.synchronize()
        prof = sb.profile_read()
    finally:
        sb.close()
    assert np.array_equal(got, z["disp"]), _diff_msg(got, z["disp"])
    assert (on != got).any()
    assert not any(k in prof for k in ("refine_lr_classify", "refine_rv_combine", "refine_rv_carry"))
    assert prof["refine_lr_check"]["launches"] == 1 and prof["refine_region_vote"]["launches"] == 2


def test_facades(tmp_path):
    """The Python facade's statics and tests/cpp/outlier_facade_check.cpp give the C ABI's maps and mask."""
    import os
    import subprocess
    from mystereomatching_amd import SolveAll, StereoMatching
    from test_cpp_facade import _compile, write_ppm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    H, W, MD = 40, 56, 15
    p = S.make_pair(H, W, MD + 1, 720)
    sb = StereoBatch(MD, H, W, 1, device=0, do_refine=1, refine_outlier=dict(classify=True, rv_combine=True, interpolate_type=2))
    try:
        sb.upload(*(p[k][None] for k in KEYS))
        want = sb.run(0.3)[0].copy()
        wmask = sb.get_lrc_mask()
    finally:
        sb.close()
    assert wmask.any()
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG)
    try:
        cls.costcalculation, cls.aggregation, cls.optimization = "censusGrad", "CBCA", "sgm"
        cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG = True, True, True
        prm = cls.Parameters(MD, H, W)
        assert prm.interpolateType == 0 and prm.DISP_MIS == -48
        prm.interpolateType = 2
        sm = cls(p["lbgr"], p["rbgr"], p["lgray"], p["rgray"], param=prm)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        sm.dispOptimize()
        np.testing.assert_array_equal(sm.refine(), want)
        np.testing.assert_array_equal(sm.LRC_Err_Mask, wmask)
    finally:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.LRC_CLASSIFY, cls.RV_COMBINE_BG = saved
    # (the C++ facade reads its gray images from the colour files; the synthetic pair's are that conversion)
    exe = str(tmp_path / "outlier_facade_check")
    _compile(os.path.join(root, "tests", "cpp", "outlier_facade_check.cpp"), exe)
    write_ppm(tmp_path / "l.ppm", p["lbgr"])
    write_ppm(tmp_path / "r.ppm", p["rbgr"])
    dp, mk = tmp_path / "dp", tmp_path / "mask"
    r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(MD), "1", "1", "2", str(dp), str(mk)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DISP_MIS -48 interpolateType 2" in r.stdout
    np.testing.assert_array_equal(np.fromfile(dp, np.int16).reshape(H, W), want)
    np.testing.assert_array_equal(np.fromfile(mk, np.uint8).reshape(H, W), wmask)
