"""The C oracle against the independent numpy restatement (tests/pyref.py) on small inputs.

Both restate the reference.  For the default pipeline (census, arms, censusGrad / Census costs, CBCA, SGM, WTA, so)
the oracle is also held to the reference's own functions (tests/test_ref_core.py, oracle/ref_core.mk); for everything
else here agreement of two independent restatements is the pin available.  Bit-exact comparisons throughout.
"""
import numpy as np
import pytest

from mystereomatching_amd import synthetic as S
from tests import pyref


def tiny_pair(H, W, D, idx, smooth=False):
    p = S.make_pair(H, W, D, idx)
    if smooth:  # quantise colours so cross arms grow long
        for k in ("lbgr", "rbgr"):
            p[k] = (p[k] // 64 * 64).astype(np.uint8)
        p["lgray"], p["rgray"] = S.bgr_to_gray(p["lbgr"]), S.bgr_to_gray(p["rbgr"])
    return p


CASES = [(9, 13, 5, 0, False), (12, 17, 8, 1, True), (7, 20, 12, 2, False), (16, 11, 6, 3, True)]


@pytest.mark.parametrize("H,W,D,idx,smooth", CASES)
def test_census_codes(oracle, H, W, D, idx, smooth):
    p = tiny_pair(H, W, D, idx, smooth)
    cfg = oracle.config(H, W, D - 1)
    for g in ("lgray", "rgray"):
        np.testing.assert_array_equal(oracle.census(p[g], cfg), pyref.census_words(pyref.census(p[g])))


@pytest.mark.parametrize("H,W,D,idx,smooth", CASES)
def test_arms(oracle, H, W, D, idx, smooth):
    p = tiny_pair(H, W, D, idx, smooth)
    cfg = oracle.config(H, W, D - 1)
    for k in ("lbgr", "rbgr"):
        np.testing.assert_array_equal(oracle.arms(p[k], cfg), pyref.arms(p[k]))


@pytest.mark.parametrize("cost", ["censusGrad", "Census", "ADCensus", "AD"])
@pytest.mark.parametrize("H,W,D,idx,smooth", CASES[:3])
def test_pipeline_bitexact(oracle, cost, H, W, D, idx, smooth):
    p = tiny_pair(H, W, D, idx, smooth)
    cfg = oracle.config(H, W, D - 1, cost=cost)
    got = oracle.run(p, cfg, dumps=True)
    ref = pyref.pipeline(p, D - 1, cost=cost)
    for k in ("cost", "agg", "final"):
        np.testing.assert_array_equal(got[k].view(np.uint32), ref[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(got["disp"], ref["disp"])


def test_right_view_cost(oracle):
    H, W, D = 10, 14, 7
    p = tiny_pair(H, W, D, 5)
    cfg = oracle.config(H, W, D - 1)
    got = oracle.cost_volume(p, cfg, view=1)
    bl, br = pyref.census(p["lgray"]), pyref.census(p["rgray"])
    gx0, gy0 = pyref.grads(p["lgray"])
    gx1, gy1 = pyref.grads(p["rgray"])
    ref = pyref.fuse(pyref.census_cost(bl, br, D, view=1),
                     pyref.grad_cost(gx0, gx1, gy0, gy1, pyref.arms(p["rbgr"]), D, view=1), 13, 1)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_sgm_8_paths(oracle):
    H, W, D = 9, 12, 6
    p = tiny_pair(H, W, D, 6)
    cfg = oracle.config(H, W, D - 1, sgm_paths=8)
    got = oracle.run(p, cfg, dumps=True)
    ref = pyref.pipeline(p, D - 1, paths=8)
    np.testing.assert_array_equal(got["final"].view(np.uint32), ref["final"].view(np.uint32))
    np.testing.assert_array_equal(got["disp"], ref["disp"])


def test_solve_all_weight(oracle):
    # OpenCV 1x1 float invert: (float)(1.0 / (double)(1 + 0.3f)) = 0x3f44ec4f
    w = np.float32(oracle.solve_all_weight(0.3))
    assert w.view(np.uint32) == 0x3F44EC4F


def test_reflect101(oracle):
    lib = oracle.load()
    for n in (1, 2, 3, 5):
        for p in range(-9, 14):
            assert lib.smo_reflect101(p, n) == pyref.reflect101(p, n)


# ---- refine() path (Do_refine = 1): right-view CBCA/SGM and the refinement stages ----------

@pytest.mark.parametrize("H,W,D,idx,smooth", [(10, 15, 6, 7, True), (12, 16, 8, 8, False)])
def test_refine_pipeline_bitexact(oracle, H, W, D, idx, smooth):
    p = tiny_pair(H, W, D, idx, smooth)
    cfg = oracle.config(H, W, D - 1, do_refine=1)
    got = oracle.run_ex(p, cfg, dumps=("agg", "agg_right", "disp_raw", "disp_right"))
    ref = pyref.pipeline(p, D - 1, refine_on=True)
    np.testing.assert_array_equal(got["agg"].view(np.uint32), ref["agg"].view(np.uint32))
    np.testing.assert_array_equal(got["agg_right"].view(np.uint32), ref["agg_right"].view(np.uint32))
    np.testing.assert_array_equal(got["disp_raw"], ref["disp_raw"])
    np.testing.assert_array_equal(got["disp_right"], ref["disp_right"])
    np.testing.assert_array_equal(got["disp"], ref["disp"])


def _noisy_map(H, W, D, seed, invalid=0.3, occ=False):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, D, size=(H // 4 + 1, W // 4 + 1))
    dp = np.kron(base, np.ones((4, 4), np.int64))[:H, :W]
    dp = np.where(rng.random((H, W)) < invalid, -32 if occ else -1, dp)
    if occ:
        dp = np.where(rng.random((H, W)) < 0.1, -1, dp)
    return dp.astype(np.int16)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_refine_stages_vs_pyref(oracle, seed):
    H, W, D = 23, 31, 9
    p = tiny_pair(H, W, D, 20 + seed, smooth=True)
    cfg = oracle.config(H, W, D - 1)
    aL = oracle.arms(p["lbgr"], cfg)
    d0, d1 = _noisy_map(H, W, D, seed, 0.1), _noisy_map(H, W, D, seed + 100, 0.1)
    np.testing.assert_array_equal(oracle.lr_check(d0, d1, cfg), pyref.lr_check(d0, d1))
    dm = _noisy_map(H, W, D, seed + 7, 0.4)
    np.testing.assert_array_equal(oracle.region_vote(dm, aL, cfg), pyref.region_vote(dm, aL, D))
    # uniform colour => long arms: the vote fills a hole only where every valid neighbour agrees
    # (hist / validNum is an integer division, cpp:7270)
    aU = oracle.arms(np.full((H, W, 3), 90, np.uint8), cfg)
    flat = np.full((H, W), 3, np.int16)
    flat[::5, ::3] = -1
    got = oracle.region_vote(flat, aU, cfg)
    np.testing.assert_array_equal(got, pyref.region_vote(flat, aU, D))
    assert (got == 3).all()
    mixed = flat.copy()
    mixed[0, 1] = 5          # one dissenting neighbour in every region: no hole is filled
    got = oracle.region_vote(mixed, aU, cfg)
    np.testing.assert_array_equal(got, pyref.region_vote(mixed, aU, D))
    np.testing.assert_array_equal(got, mixed)
    for occ in (False, True):
        dq = _noisy_map(H, W, D, seed + 11, 0.5, occ)
        np.testing.assert_array_equal(oracle.proper_ipol(dq, p["lbgr"], cfg), pyref.proper_ipol(dq, p["lbgr"]))
    dq = _noisy_map(H, W, D, seed + 13, 0.2)
    np.testing.assert_array_equal(oracle.median3(dq), pyref.median3(dq))
    np.testing.assert_array_equal(oracle.refine(d0, d1, aL, p["lbgr"], cfg),
                                  pyref.refine(d0, d1, aL, p["lbgr"], D))


def test_proper_ipol_colour_255_never_wins(oracle):
    # minDifColor starts at 255 with a strict '>' (cpp:7470-7477): a neighbour whose colour
    # differs by exactly 255 is never taken, so the pixel keeps its invalid value.
    H, W, D = 5, 6, 4
    bgr = np.zeros((H, W, 3), np.uint8)
    bgr[2, 2] = 255
    dp = np.full((H, W), 2, np.int16)
    dp[2, 2] = -1
    cfg = oracle.config(H, W, D - 1)
    out = oracle.proper_ipol(dp, bgr, cfg)
    assert out[2, 2] == -1
    np.testing.assert_array_equal(out, pyref.proper_ipol(dp, bgr))


# ---- cross-scale pyramid (PY_LEV > 1): pyrDown, SolveAll weights, whole pipeline -------------

@pytest.mark.parametrize("shape", [(9, 13, 3), (10, 14), (2, 3, 3), (3, 2), (17, 8, 3), (5, 5)])
def test_pyr_down(oracle, shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    np.testing.assert_array_equal(oracle.pyr_down(img), pyref.pyr_down(img))


def test_pyr_down_constant_and_ramp(oracle):
    flat = np.full((7, 11, 3), 200, np.uint8)
    np.testing.assert_array_equal(oracle.pyr_down(flat), np.full((4, 6, 3), 200, np.uint8))
    ramp = np.tile(np.arange(16, dtype=np.uint8) * 10, (6, 1))
    np.testing.assert_array_equal(oracle.pyr_down(ramp), pyref.pyr_down(ramp))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("lam", [0.3, 0.1, 1.0])
def test_pyr_weights(oracle, L, lam):
    """L <= 3: OpenCV's closed-form invert in double; L > 3: LUImpl<float> (pyref._lu_inv_row0)."""
    np.testing.assert_array_equal(oracle.pyr_weights(L, lam).view(np.uint32), pyref.pyr_weights(L, lam).view(np.uint32))
    if L == 1:
        assert oracle.pyr_weights(1, 0.3).view(np.uint32)[0] == 0x3F44EC4F   # the PY_LVL = 1 weight


def test_pyr_weights_lu_close_to_exact_inverse(oracle):
    """The float LU row stays within a few float ulps of the float64 inverse (row sums 1)."""
    for L in range(4, 9):
        for lam in (0.1, 0.3, 1.0, 4.0):
            M = np.zeros((L, L))
            for s in range(L):
                M[s, s] = 1 + lam if s in (0, L - 1) else 1 + 2 * lam
                if s:
                    M[s, s - 1] = -lam
                if s < L - 1:
                    M[s, s + 1] = -lam
            np.testing.assert_allclose(oracle.pyr_weights(L, lam), np.linalg.inv(M)[0], rtol=0, atol=5e-7)
    with pytest.raises(ValueError):
        oracle.pyr_weights(9, 0.3)


@pytest.mark.parametrize("L,H,W,md", [(2, 14, 21, 7), (3, 20, 26, 9), (4, 34, 40, 15)])
def test_pyramid_pipeline(oracle, L, H, W, md):
    p = tiny_pair(H, W, md + 1, 31 + L, smooth=True)
    cfg = oracle.config(H, W, md)
    np.testing.assert_array_equal(oracle.run_pyr(p, cfg, L), pyref.pipeline_pyr(p, md, L))
    # PY_LEV = 1 through the pyramid driver is the plain pipeline
    np.testing.assert_array_equal(oracle.run_pyr(p, cfg, 1), oracle.run(p, cfg)["disp"])


# ---- scan-line optimisation "so" (cpp:6272-6394, optimization == "so") ---------------------

@pytest.mark.parametrize("H,W,D,idx", [(7, 19, 6, 1), (9, 23, 11, 2)])
def test_so_bitexact(oracle, H, W, D, idx):
    p = tiny_pair(H, W, D, 60 + idx)
    cfg = oracle.config(H, W, D - 1, optimization=2)
    got = oracle.run(p, cfg, dumps=True)
    ref_vm, ref_dp = pyref.so(pyref.solve_all(pyref.pipeline(p, D - 1)["agg"]), p["lbgr"])
    np.testing.assert_array_equal(got["final"].view(np.uint32), ref_vm.view(np.uint32))
    np.testing.assert_array_equal(got["disp"], ref_dp)
    # refine with "so": DP[1] from vm[1] with the LEFT colours (so() reads I[0] only)
    cfgr = oracle.config(H, W, D - 1, optimization=2, do_refine=1)
    r = oracle.run_ex(p, cfgr, dumps=("agg_right", "disp_right"))
    _, ref_d1 = pyref.so(pyref.solve_all(r["agg_right"]), p["lbgr"])
    np.testing.assert_array_equal(r["disp_right"], ref_d1)
    # without refine "so" still runs on both views (num = Do_LRConsis ? 2 : 1, cpp:1093): DP[1]
    # from the raw right cost volume (CBCA and SolveAll touch vm[1] only with Do_refine)
    n = oracle.run_ex(p, cfg, dumps=("right", "disp_right"))
    np.testing.assert_array_equal(n["disp"], got["disp"])
    _, ref_n1 = pyref.so(n["right"], p["lbgr"])
    np.testing.assert_array_equal(n["disp_right"], ref_n1)
