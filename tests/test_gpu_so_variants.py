"""GPU parity of the scan-line optimiser variants (sm_so_config): so_R2L (cpp:6683-6826) and so_T2D (cpp:6580-6681).

Every case reads the volumes dispOptimize is about to see back from the context (vm[0], vm[1]), runs the variant on
the GPU and compares the maps of both views with the numpy restatement (tests/pyref_so.py, pinned to the C oracle in
tests/test_so_variants_host.py) on those volumes and the LEFT colour image.  R2L with keep_final_volume: the
accumulated volume's bits; T2D: vm[view] after dispOptimize has the bits it had before.

Two conditions keep the comparisons from passing vacuously and are asserted on every make_pair input that is large
enough to show them (SIZEABLE: at least 16 steps along the scan, 12 lines and 10 disparities): the variant's map
differs from so's; and so_T2D's accumulated volume has a negative column minimum at >= 10 % of the pixels (an unsigned
minimum goes wrong exactly there) wherever the input can give one, see NEGATIVE_AT_OWN_PENALTIES.  The tiny shapes
(D = 1, two rows) cannot show either.
"""
import numpy as np
import pytest

import degenerate
import pyref_so as P
from mystereomatching_amd import StereoBatch, StereoMatching, SolveAll
from mystereomatching_amd import synthetic as S
from test_so_variants_host import oracle_so

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
# (H, W, D) for so_R2L; so_T2D takes the list with H and W exchanged
R2L_SHAPES = [(5, 3, 10), (2, 2, 1), (31, 57, 16), (9, 70, 100), (17, 150, 128), (13, 300, 256),
              (6, 1100, 256), (7, 2100, 64),                            # the trace in global memory
              (4, 63, 16), (4, 64, 16), (4, 65, 16), (4, 129, 16)]      # the map's 64-wide flush groups
T2D_SHAPES = [(W, H, D) for H, W, D in R2L_SHAPES]
PYREF = {"so": P.so, "so_R2L": P.so_r2l, "so_T2D": P.so_t2d}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Statics:
    """StereoMatching's class-level selectors for one block, restored afterwards."""

    NAMES = ("costcalculation", "aggregation", "optimization", "Do_refine", "SO_VARIANT", "SO_PN")

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: getattr(StereoMatching, k) for k in self.NAMES}
        for k, v in self.kw.items():
            setattr(StereoMatching, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(StereoMatching, k, v)


def staged(pair, H, W, D, variant, pn=None, keep=False, refine=False, cost="censusGrad"):
    """costCalculate + SolveAll, the volumes read back, dispOptimize [+ refine] with the variant: dict(vol = [vm[0],
    vm[1]] before dispOptimize, dp = [DP[0], DP[1]], after = the volumes after dispOptimize, refined)."""
    with Statics(costcalculation=cost, aggregation="CBCA", optimization="so", Do_refine=refine, SO_VARIANT=variant, SO_PN=pn):
        prm = StereoMatching.Parameters(D - 1, H, W)
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm,
                            keep_final_volume=keep)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        vol = sm.vm
        sm.dispOptimize()
        out = dict(vol=vol, dp=[sm.DP[0].copy(), sm.DP[1].copy()], after=sm.vm, arms=sm.HVL[0])
        if refine:
            out["refined"] = sm.refine().copy()
    assert len(vol) == 2
    return out


def sizeable(steps, lines, D):
    return steps >= 16 and lines >= 12 and D >= 10


@pytest.mark.parametrize("H,W,D", R2L_SHAPES)
def test_r2l_reference_order(H, W, D):
    pair = S.make_pair(H, W, D, 800 + H + W)
    r = staged(pair, H, W, D, "so_R2L", keep=True)
    for view in (0, 1):
        dp, acc = P.so_r2l(r["vol"][view], pair["lbgr"])
        np.testing.assert_array_equal(r["dp"][view], dp, err_msg=f"view {view}")
        np.testing.assert_array_equal(bits(r["after"][view]), bits(acc), err_msg=f"view {view}: accumulated volume")
        if sizeable(W, H, D):
            assert (dp != P.so(r["vol"][view], pair["lbgr"])[0]).mean() > 0.05


def check_t2d(H, W, D, pn, want_negative):
    pair = S.make_pair(H, W, D, 900 + H + W)
    r = staged(pair, H, W, D, "so_T2D", pn=pn, keep=True)
    for view in (0, 1):
        dp, acc = P.so_t2d(r["vol"][view], pair["lbgr"], *(pn or P.T2D_PN))
        np.testing.assert_array_equal(r["dp"][view], dp, err_msg=f"view {view}")
        # the reference runs on a clone (vm_res): vm[view] keeps the aggregated volume bit for bit
        np.testing.assert_array_equal(bits(r["after"][view]), bits(r["vol"][view]), err_msg=f"view {view}: vm changed")
        if sizeable(H, W, D):
            assert (dp != P.so(r["vol"][view], pair["lbgr"])[0]).mean() > 0.05
        if want_negative:
            neg = (acc.min(axis=2) < 0).mean()
            print(f"T2D {H}x{W}x{D} view {view}: negative column minimum at {100 * neg:.1f} % of the pixels")
            assert (r["vol"][view] >= 0).all() and neg >= 0.10


# With the function's own 0.3 / 0.9 the accumulated costs go negative only where make_pair's volumes have costs near 0:
# every image of this list that is at least 31 columns wide (37 - 39 % of the pixels at (57, 31, 16), 30 % at
# (26, 71, 32), 15 % at (40, 60, 64)).  The images of 4 - 17 columns - the global-trace, ragged-D, K = 2 / 4 and
# flush-group shapes - have no cost under 0.5 (the border's costs), each row adds at least that and takes off at most
# 0.9, and the restatement on the oracle's volumes measures 0.0 - 1.2 % negative column minima there.  So the
# assertion at the function's penalties is gated on the image's width, and every kernel path of those narrow shapes
# follows once more with 2.0 / 6.0, where 98.6 - 100 % of the column minima are negative.
NEGATIVE_AT_OWN_PENALTIES = [(57, 31, 16), (26, 71, 32), (40, 60, 64)]


@pytest.mark.parametrize("H,W,D", T2D_SHAPES + NEGATIVE_AT_OWN_PENALTIES[1:])
def test_t2d_reference_order(H, W, D):
    assert ((H, W, D) in NEGATIVE_AT_OWN_PENALTIES) == (W >= 31 and D > 1)
    check_t2d(H, W, D, None, (H, W, D) in NEGATIVE_AT_OWN_PENALTIES)


@pytest.mark.parametrize("H,W,D", [(70, 9, 100), (150, 17, 128), (300, 13, 256), (1100, 6, 256), (2100, 7, 64), (129, 4, 16)])
def test_t2d_signed_minima_on_every_kernel_path(H, W, D):
    """Ragged D, K = 2 and 4, the trace in global memory (K = 4 and K = 1) and a partial last flush group, each with
    accumulated costs below zero at nearly every pixel."""
    check_t2d(H, W, D, (2.0, 6.0), True)


def test_r2l_against_the_oracle_on_mirrored_input(oracle):
    """so_R2L at so's penalties is the mirror of so on the mirrored volume and image: smo_so itself is the yardstick
    here, not the restatement."""
    H, W, D = 26, 71, 32
    pair = S.make_pair(H, W, D, 600)
    r = staged(pair, H, W, D, "so_R2L", pn=P.SO_PN, keep=True)
    for view in (0, 1):
        dp, acc = oracle_so(oracle, r["vol"][view][:, ::-1], pair["lbgr"][:, ::-1])
        np.testing.assert_array_equal(r["dp"][view], dp[:, ::-1])
        np.testing.assert_array_equal(bits(r["after"][view]), bits(acc[:, ::-1]))


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
def test_penalties_are_arguments(variant):
    H, W, D = 21, 40, 24
    pair = S.make_pair(H, W, D, 41)
    pn = (0.75, 2.0)
    r = staged(pair, H, W, D, variant, pn=pn)
    d = staged(pair, H, W, D, variant)
    for view in (0, 1):
        np.testing.assert_array_equal(r["dp"][view], PYREF[variant](r["vol"][view], pair["lbgr"], *pn)[0])
    assert (r["dp"][0] != d["dp"][0]).any()


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
@pytest.mark.parametrize("kind", ["constant", "vstripes"])
def test_ties_take_the_first_index(variant, kind):
    H, W, D = 23, 70, 20
    pair = degenerate.TIE_INPUTS[kind](H, W)
    r = staged(pair, H, W, D, variant)
    for view in (0, 1):
        np.testing.assert_array_equal(r["dp"][view], PYREF[variant](r["vol"][view], pair["lbgr"])[0], err_msg=f"view {view}")
    if kind == "constant":
        assert not r["dp"][0].any()


@pytest.fixture(scope="module")
def batch3():
    H, W, D, n = 26, 71, 32, 3
    pairs = [S.make_pair(H, W, D, 600 + i) for i in range(n)]
    vols = [staged(p, H, W, D, "so")["vol"] for p in pairs]
    want = {v: [[PYREF[v](vols[i][view], pairs[i]["lbgr"])[0] for view in (0, 1)] for i in range(n)] for v in PYREF}
    for v in ("so_R2L", "so_T2D"):
        assert all((want[v][i][0] != want["so"][i][0]).mean() > 0.05 for i in range(n))
    return H, W, D, pairs, degenerate.batch(pairs), want


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
def test_batch_schedules(batch3, variant):
    """A batch of 3 under sub_batch 1 and 2 with 1 and 2 streams: the same maps (the right view's of pair 0 too)."""
    H, W, D, pairs, st, want = batch3
    b = StereoBatch(D - 1, H, W, 3, optimization="so", so_variant=variant)
    try:
        b.upload(*(st[k] for k in KEYS))
        for streams, sub in ((0, 0), (1, 1), (1, 2), (2, 1), (2, 2)):
            b.set_schedule(streams, sub)
            out = b.run()
            for i in range(3):
                np.testing.assert_array_equal(out[i], want[variant][i][0], err_msg=f"pair {i} streams {streams} sub_batch {sub}")
            np.testing.assert_array_equal(b.get_disp(1), want[variant][0][1])
    finally:
        b.close()


def test_switching_on_a_live_context(batch3):
    H, W, D, pairs, st, want = batch3
    b = StereoBatch(D - 1, H, W, 3, optimization="so")
    try:
        b.upload(*(st[k] for k in KEYS))
        first = b.run().copy()
        for variant in ("so", "so_T2D", "so_R2L", "so"):
            b.so_config(variant)
            out = b.run()
            for i in range(3):
                np.testing.assert_array_equal(out[i], want[variant][i][0], err_msg=f"{variant} pair {i}")
        np.testing.assert_array_equal(out, first)
    finally:
        b.close()


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
def test_eval_stage_0_is_named_so(batch3, variant):
    """The table's stage 0 keeps the name "so" (the literal at cpp:1102) and carries the variant's map."""
    H, W, D, pairs, st, want = batch3
    b = StereoBatch(D - 1, H, W, 3, optimization="so", so_variant=variant, eval=dict(keep_maps=True, thresholds=(1.0,)))
    try:
        b.upload(*(st[k] for k in KEYS))
        b.upload_truth(np.stack([p["gt"] for p in pairs]).astype(np.float32), np.stack([p["nonocc"] for p in pairs]))
        out = b.run()
        assert b.stage_names()[0] == "so"
        kept = b.stage_maps(0)
        for i in range(3):
            np.testing.assert_array_equal(kept[i], want[variant][i][0])
            np.testing.assert_array_equal(out[i], want[variant][i][0])
    finally:
        b.close()


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
def test_with_refine(oracle, variant):
    """do_refine = 1: both views aggregated, the variant on both, refine() on those maps (the oracle's stages)."""
    H, W, D = 40, 66, 24
    pair = S.make_pair(H, W, D, 77)
    r = staged(pair, H, W, D, variant, refine=True)
    d0, d1 = (PYREF[variant](r["vol"][view], pair["lbgr"])[0] for view in (0, 1))
    np.testing.assert_array_equal(r["dp"][0], d0)
    np.testing.assert_array_equal(r["dp"][1], d1)
    cfg = oracle.config(H, W, D - 1, optimization=2, do_refine=1)
    ref = oracle.refine(d0, d1, r["arms"], pair["lbgr"], cfg)
    np.testing.assert_array_equal(r["refined"], ref)
    assert (ref != d0).any()
    b = StereoBatch(D - 1, H, W, 1, optimization="so", do_refine=1, so_variant=variant)
    try:
        b.upload(*(pair[k][None] for k in KEYS))
        np.testing.assert_array_equal(b.run()[0], ref)
    finally:
        b.close()


@pytest.mark.parametrize("variant", ["so_R2L", "so_T2D"])
def test_pyramid(variant):
    """py_lvl = 2: the variant runs at level 0 on the combined volume, which neither variant changes without
    keep_final_volume."""
    H, W, D = 40, 70, 32
    pair = S.make_pair(H, W, D, 52)
    b = StereoBatch(D - 1, H, W, 1, optimization="so", so_variant=variant, py_lvl=2)
    try:
        b.upload(*(pair[k][None] for k in KEYS))
        out = b.run()
        vol = b.pyramid_level_volume(0, 0)
        np.testing.assert_array_equal(out[0], PYREF[variant](vol, pair["lbgr"])[0])
        assert (out[0] != P.so(vol, pair["lbgr"])[0]).mean() > 0.05
    finally:
        b.close()
