"""CPU: the oracle of the default pipeline against the reference's OWN functions, bit for bit, stage by stage.

oracle/ref_core.mk cuts the reference's cost, arm, CBCA, SGM, WTA and scan-line functions out of a reference
checkout and compiles them behind our driver and a minimal cv::Mat into oracle/_ref/ref_core_driver (not in
git); oracle/ref_core.py runs it.  Every stage of the restatement is fed the reference build's own output of
the stage before and must return the reference build's output of that stage, every bit:
    oracle.census          genCensusCode_NC_Sur (h:867-934)
    oracle.arms            calArms<uchar> -> calHorVerDis<uchar>, judgeColorDif (cpp:5354-5392, 2958-3050, 2847-2856)
    oracle.cost_volume     censusGrad -> grad -> calGrad, calGrad_y, calgradvm; censusCal -> gen_cenVM_XOR,
                           HammingDistance; gen_vm_from2vm_exp (cpp:25-48, 603-656, 271-455, 807-892, 3566-3590)
    oracle.cbca            cbca_core -> genTrueHorVerArms, gen1DCumu, cal1DCost, genfinalVm_cbca
    pyref_cbca_ni.cbca_ni  the same with Parameters::cbca_intersect = false
    oracle.solve_all       the one-level sum of SolveAll with the driver's weight
    oracle.sgm             sgm -> costScan -> updateCost<float>, min4; gen_sgm_vm (4 and 8 paths, leftFirst both ways)
    oracle.wta             gen_dispFromVm
    oracle.so, pyref_so.so_r2l / so_t2d, pyref_so_float.*   so, so_R2L, so_T2D (finite, signed and NaN volumes)
Every case runs with two fill bytes for the build's new buffers and counts only if both runs agree
(ref_core.run_defined); the stand-alone sanitizer build runs the whole list once more.

With a reference checkout beside the repository and no binary the tests FAIL (build() should have made it); with
neither they skip, and test_oracle_matches_recorded_reference still compares the oracle with
tests/golden/ref_core.npz, outputs of the binary recorded by tests/golden/make_ref_core.py.  The same script
records what tests/test_gpu_ref_core.py expects (tests/golden/ref_core_gpu.npz); the last tests keep both current."""
import os
import sys

import numpy as np
import pytest

import pyref_cbca_ni
import pyref_so
import pyref_so_float as PF
import ref_core_cases as K
import so_float_cases as SC
from oracle import ref_core as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = pytest.mark.parametrize("kind,H,W,D", K.CPU_CASES)
TWINS = {"so": pyref_so.so, "so_R2L": pyref_so.so_r2l, "so_T2D": pyref_so.so_t2d}


def need_binary(binary=R.BINARY):
    if R.available(binary):
        return
    if R.checkout_present():
        pytest.fail(f"a reference checkout is at {R.reference_dir()} but {binary} is not built: "
                    "build() (make -C oracle -f ref_core.mk all asan) must produce it")
    pytest.skip("no reference checkout and no oracle/_ref binary; tests/golden/ref_core.npz stands in")


def eq(got, want, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = K.bits(got), K.bits(want)
    np.testing.assert_array_equal(got, want, err_msg=msg)


def arms4(a):
    return np.ascontiguousarray(a[..., :4])


# ---- stage by stage ------------------------------------------------------------------------------------------

@CASES
def test_census_codes(oracle, kind, H, W, D):
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
    cfg = oracle.config(H, W, D - 1)
    for view, g in enumerate(("lgray", "rgray")):
        eq(oracle.census(p[g], cfg), c["census"][view], f"view {view}")


@CASES
def test_arms(oracle, kind, H, W, D):
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
    cfg = oracle.config(H, W, D - 1)
    for view, g in enumerate(("lbgr", "rbgr")):
        ref = c["arms"][view]
        eq(oracle.arms(p[g], cfg), arms4(ref), f"view {view}")
        np.testing.assert_array_equal(ref[..., 4], ref[..., :4].sum(axis=2, dtype=np.uint16))   # cpp:3031-3043
    if kind == "flat" and min(H, W) >= 36:
        a = c["arms"][0][..., :4]
        assert int(a[..., :2].max()) == 34 and int(a[..., 2:].max()) == 34, "the flat pair is there for arms at the cap L_out"


@pytest.mark.parametrize("cost", ["censusGrad", "Census"])
@CASES
def test_cost_volume(oracle, kind, H, W, D, cost):
    need_binary()
    p = K.pair(kind, H, W, D)
    ref = K.chain(kind, H, W, D, cost=cost)["cost"]
    cfg = oracle.config(H, W, D - 1, cost=cost)
    for view in (0, 1):
        eq(oracle.cost_volume(p, cfg, view), ref[view], f"view {view}")


def test_gradients_reach_their_bounds():
    """The 0 / 255 pair: gray steps of +-255 (calGrad's edge columns and rows take the full difference)."""
    kind, H, W, D = K.CPU_CASES[-1]
    assert kind == "binary"
    g = K.pair(kind, H, W, D)["lgray"].astype(np.int32)
    assert abs(g[:, 1] - g[:, 0]).max() == 255 or abs(g[:, -1] - g[:, -2]).max() == 255 or abs(np.diff(g, axis=1)).max() == 255
    assert abs(np.diff(g, axis=0)).max() == 255


@pytest.mark.parametrize("intersect", [True, False], ids=["intersect", "no_intersect"])
@pytest.mark.parametrize("iters", [1, 2, 3, 4])
@CASES
def test_cbca(oracle, kind, H, W, D, iters, intersect):
    need_binary()
    c = K.chain(kind, H, W, D)
    ref = K.chain(kind, H, W, D, iters=iters, intersect=intersect)
    cfg = oracle.config(H, W, D - 1, cbca_iters=iters)
    aL, aR = arms4(c["arms"][0]), arms4(c["arms"][1])
    for view in (0, 1):
        eq(ref["cost"][view], c["cost"][view])            # the same input on both sides
        if intersect:
            got = oracle.cbca(c["cost"][view], aL, aR, cfg, view)
        else:
            got = pyref_cbca_ni.cbca_ni(c["cost"][view], (aL, aR)[view], iters)[0]
        eq(got, ref["agg"][view], f"view {view}")


@CASES
def test_solve_all_scale(oracle, kind, H, W, D):
    need_binary()
    c = K.chain(kind, H, W, D)
    assert K.solve_all_weight() == oracle.solve_all_weight(K.REG_LAMBDA)
    cfg = oracle.config(H, W, D - 1)
    for view in (0, 1):
        eq(oracle.solve_all(c["agg"][view], cfg), c["scaled"][view], f"view {view}")


@pytest.mark.parametrize("paths", [4, 8])
@CASES
def test_sgm(oracle, kind, H, W, D, paths):
    """sgm(vm[0], true) reads I_c[0] for D1, sgm(vm[1], false) I_c[1] (h:2219-2224): the pair's two images differ,
    so the wrong image would show.  8 paths: DESIGN section 2, row a15-a16 (sm_params.sgm_paths); the recipe's one edited line
    hands sgm() the count, the direction table is the reference's."""
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D, paths=paths)
    cfg = oracle.config(H, W, D - 1, sgm_paths=paths)
    for view, g in enumerate(("lbgr", "rbgr")):
        eq(oracle.sgm(c["scaled"][view], p[g], cfg), c["sgm"][view], f"view {view}")


@pytest.mark.parametrize("kind,H,W,D", [K.CPU_CASES[3], K.CPU_CASES[8]])
def test_sgm_left_first_chooses_the_image(oracle, kind, H, W, D):
    """leftFirst alone decides the image: vm[0] with leftFirst = false must read I_c[1], vm[1] with true I_c[0]."""
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
    cfg = oracle.config(H, W, D - 1)
    s0, s1 = c["scaled"]
    o = R.run_defined(p, D, [("setvm", 0, s0), ("setvm", 1, s1), ("sgm", 0, 4, False), ("sgm", 1, 4, True)])
    eq(oracle.sgm(s0, p["rbgr"], cfg), o[2][0])
    eq(oracle.sgm(s1, p["lbgr"], cfg), o[3][0])
    assert (K.bits(o[2][0]) != K.bits(c["sgm"][0])).any()     # the image matters on this pair


@CASES
def test_wta(oracle, kind, H, W, D):
    need_binary()
    c = K.chain(kind, H, W, D)
    cfg = oracle.config(H, W, D - 1)
    for view in (0, 1):
        eq(oracle.wta(c["sgm"][view], cfg), c["disp"][view], f"view {view}")
    if D > 1 and H * W > 100:
        assert len(np.unique(c["disp"][0])) > 1


@pytest.mark.parametrize("H,W,D", [(7, 9, 1), (5, 8, 2), (9, 11, 70), (6, 10, 200), (12, 33, 16)])
def test_wta_first_minimum_and_nan(oracle, H, W, D):
    """gen_dispFromVm's rule by itself (K.wta_volume): the first of equal minima (-0 against +0 too), NaN at d = 0 and
    elsewhere never taken, -1 for a pixel of NaN or of FLT_MAX only.  The SGM sums of test_wta have no ties."""
    need_binary()
    vol = K.wta_volume(H, W, D)
    ref = R.wta(vol)
    eq(oracle.wta(vol, oracle.config(H, W, D - 1)), ref)
    num = np.where(np.isnan(vol), np.inf, vol)
    tied = (num == num.min(axis=2, keepdims=True)).sum(axis=2) > 1
    assert tied.mean() > 0.3 or D == 1
    if D > 1:
        # the inputs tell the rules apart: the last minimum, and a NaN-first arg-min, give other maps
        last = D - 1 - np.argmin(num[..., ::-1], axis=2)
        assert (last != np.argmin(num, axis=2)).mean() > 0.3
        assert (np.argmin(vol, axis=2)[np.isfinite(num).any(axis=2)] != ref[np.isfinite(num).any(axis=2)]).any()
    assert (ref == -1).any() and (ref[H // 2] == -1).all()
    assert np.isnan(vol[..., 0]).any() and (D == 1 or np.isnan(vol[..., 1:]).any())


@pytest.mark.parametrize("H,W,D", [(40, 24, 2), (9, 40, 16), (5, 70, 65)])
def test_so_ties_on_the_penalty_grid(oracle, H, W, D):
    """so()'s four candidates tie (K.so_tie_volume): prev[d], prev[d - 1] + Pn2, prev[d + 1] + Pn2, min + Pn3 are taken in
    that order on strict <.  oracle.so and the twin against the reference build, map and accumulated costs."""
    need_binary()
    vol = K.so_tie_volume(H, W, D)
    rng = np.random.default_rng(H + W)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img[::2, : W // 2] = img[::2, :1]                              # every other row: no halving on its left half
    pn2 = np.float32(1.2)
    first = vol[:, 0]
    assert (first[:, :-1] + pn2 == first[:, 1:]).any() and (first[:, :-1] + pn2 / 2 == first[:, 1:]).any()
    dp, acc = R.so(vol, img, "so")
    odp, oacc = oracle.so(vol, img, oracle.config(H, W, D - 1))
    eq(odp, dp), eq(oacc, acc)
    tdp, tacc = pyref_so.so(vol, img)
    eq(np.asarray(tdp, np.int16), dp), eq(np.asarray(tacc, np.float32), acc)


@pytest.mark.parametrize("variant", K.VARIANTS)
@CASES
def test_so_variants(oracle, kind, H, W, D, variant):
    """so* on the reference build's own scaled CBCA volumes (costs >= +0), both views, I[0] = the left image.
    so_T2D at W > 1 runs with fill 0 only: DESIGN section 25, finding 1."""
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
    cfg = oracle.config(H, W, D - 1)
    for view, (dp, acc) in enumerate(K.so_chain(kind, H, W, D, variant)):
        vol = c["scaled"][view]
        tdp, tacc = TWINS[variant](vol, p["lbgr"])
        eq(np.asarray(tdp, np.int16), dp, f"twin, view {view}")
        eq(np.asarray(tacc, np.float32), acc, f"twin, view {view}")
        if variant == "so":
            odp, oacc = oracle.so(vol, p["lbgr"], cfg)
            eq(odp, dp, f"oracle, view {view}")
            eq(oacc, acc, f"oracle, view {view}")


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("kind,H,W,D", [c for c in K.CPU_CASES if c[1] >= 3 and c[3] >= 2])
def test_so_variants_signed_and_nan(oracle, kind, H, W, D, variant):
    """Signed costs, -0 / +0 minima and NaN at index 0 and elsewhere (tests/so_float_cases.py) through the reference
    build, against the twins and, for so, oracle.so: the maps are equal, and the accumulated costs bit for bit
    wherever they are not NaN (which NaN a sum yields is the one thing the format leaves open; PF.same_floats --
    the one comparison here that is not on every bit)."""
    need_binary()
    p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
    vol = SC.craft(c["scaled"][0], 31 + H + D, lines="cols" if variant == "so_T2D" else "rows")
    assert np.isnan(vol[..., 0]).any() and np.isnan(vol[..., 1:]).any() and (vol < 0).any()
    dp, acc = R.so(vol, p["lbgr"], variant)
    tdp, tacc = SC.FUNCS[variant](vol, p["lbgr"])
    eq(np.asarray(tdp, np.int16), dp)
    assert PF.same_floats(np.asarray(tacc, np.float32), acc)
    if variant == "so":
        odp, oacc = oracle.so(vol, p["lbgr"], oracle.config(H, W, D - 1))
        eq(odp, dp, "oracle")
        assert PF.same_floats(oacc, acc)
    steps, lines = (H, W) if variant == "so_T2D" else (W, H)
    if SC.sizeable(steps, lines, D):
        SC.assert_not_vacuous(variant, vol, p["lbgr"])


@pytest.mark.parametrize("H,W,D", K.T2D_W1_CASES)
def test_so_t2d_single_column(H, W, D):
    """W = 1: so_T2D reads nothing it has not written, so both fill bytes run and must agree (run_defined)."""
    need_binary()
    vol, img = K.t2d_w1_volume(H, D)
    dp, acc = R.so(vol, img, "so_T2D")
    tdp, tacc = pyref_so.so_t2d(vol, img)
    eq(np.asarray(tdp, np.int16), dp)
    eq(np.asarray(tacc, np.float32), acc)
    vol = SC.craft(vol, 5, lines="cols")
    dp, acc = R.so(vol, img, "so_T2D")
    tdp, tacc = PF.so_t2d(vol, img)
    eq(np.asarray(tdp, np.int16), dp)
    assert PF.same_floats(np.asarray(tacc, np.float32), acc)


# ---- the reference build alone: the checks are not vacuous, the domain is what the wrapper says -----------------------

def test_wrapper_domain():
    need_binary()
    vol, img = np.zeros((4, 3, 5), np.float32), np.zeros((4, 3, 3), np.uint8)
    with pytest.raises(R.RefCoreError, match="so_T2D"):
        R.run(R.blank_pair(4, 3, img), 5, [("setvm", 0, vol), ("so", 0, "so_T2D")], fill=0xFF)
    R.run(R.blank_pair(4, 3, img), 5, [("setvm", 0, vol), ("so", 0, "so_T2D")], fill=0)
    with pytest.raises(R.RefCoreError, match="H, W >= 2"):
        R.cost(R.blank_pair(1, 8), 4)
    with pytest.raises(R.RefCoreError, match="512"):
        R.wta(np.zeros((2, 2, 513), np.float32))


def test_fill_byte_is_live():
    """The build's new buffers carry the fill byte and run_defined notices a result that depends on it: vm[1] as
    the constructor creates it (cpp:2081), never written, through gen_dispFromVm -- +0 everywhere gives disparity
    0, NaN everywhere leaves the loop's initial -1."""
    need_binary()
    p = R.blank_pair(3, 4)
    assert (R.run(p, 3, [("wta", 1)], fill=0x00)[0][0] == 0).all()
    assert (R.run(p, 3, [("wta", 1)], fill=0xFF)[0][0] == -1).all()
    with pytest.raises(R.RefCoreError, match="never wrote"):
        R.run_defined(p, 3, [("wta", 1)])


@pytest.mark.parametrize("kind,H,W,D", [K.CPU_CASES[3], K.CPU_CASES[8]])
def test_reference_is_sensitive(kind, H, W, D):
    """The reference build alone: the listed misreadings would show on these inputs -- the two views' census
    codes, arms and volumes differ, intersecting and plain CBCA differ, 4 and 8 paths differ, the three scan-line
    maps differ."""
    need_binary()
    c = K.chain(kind, H, W, D)
    assert (c["census"][0] != c["census"][1]).mean() > 0.2
    assert (c["arms"][0] != c["arms"][1]).any()
    assert (K.bits(c["cost"][0]) != K.bits(c["cost"][1])).mean() > 0.2
    assert (K.bits(c["agg"][0]) != K.bits(K.chain(kind, H, W, D, intersect=False)["agg"][0])).mean() > 0.2
    assert (K.bits(c["sgm"][0]) != K.bits(K.chain(kind, H, W, D, paths=8)["sgm"][0])).mean() > 0.9
    maps = [K.so_chain(kind, H, W, D, v)[0][0] for v in K.VARIANTS]
    assert (maps[0] != maps[1]).any() and (maps[0] != maps[2]).any()


# ---- the stand-alone sanitizer build ------------------------------------------------------------------------------

def test_sanitizer_build_is_clean_over_the_case_list():
    """oracle/_ref/ref_core_driver_asan (make -f ref_core.mk asan: -fsanitize=address,undefined, its own main, run on
    its own) over every pipeline and scan-line case above, each fill byte: it must finish, and with the plain
    build's bits."""
    need_binary(R.BINARY_ASAN)
    for kind, H, W, D in K.CPU_CASES:
        p, c = K.pair(kind, H, W, D), K.chain(kind, H, W, D)
        ops = [("census",), ("arms",), ("cost", "censusGrad"), ("cbca", 2), ("scale", K.solve_all_weight()),
               ("sgm", 0, 8, True), ("sgm", 1, 4, False), ("wta", 0), ("wta", 1)]
        o = R.run_defined(p, D, ops, binary=R.BINARY_ASAN, timeout=600)
        eq(o[3][0], c["agg"][0]), eq(o[6][0], c["sgm"][1]), eq(o[8][0], c["disp"][1])
        R.run_defined(p, D, [("cost", "Census"), ("cbca", 3)], intersect=False, binary=R.BINARY_ASAN, timeout=600)
        crafted = SC.craft(c["scaled"][0], 31 + H + D) if H >= 3 and D >= 2 else c["scaled"][0]
        for variant in K.VARIANTS:
            ops = [("setvm", 0, c["scaled"][0]), ("setvm", 1, crafted), ("so", 0, variant), ("so", 1, variant)]
            o = R.run_defined(p, D, ops, binary=R.BINARY_ASAN, timeout=600)
            eq(o[2][0], K.so_chain(kind, H, W, D, variant)[0][0])
    for H, W, D in K.T2D_W1_CASES:
        vol, img = K.t2d_w1_volume(H, D)
        R.so(vol, img, "so_T2D", binary=R.BINARY_ASAN)
    for H, W, D in K.GPU_WTA:
        eq(R.wta(K.wta_volume(H, W, D), binary=R.BINARY_ASAN), R.wta(K.wta_volume(H, W, D)))
    vol = K.so_tie_volume(9, 40, 16)
    eq(R.so(vol, np.zeros((9, 40, 3), np.uint8), "so", binary=R.BINARY_ASAN)[0], R.so(vol, np.zeros((9, 40, 3), np.uint8), "so")[0])


# ---- the recordings ------------------------------------------------------------------------------------------------

def _make_ref_core():
    sys.path.insert(0, GOLDEN_DIR)
    try:
        import make_ref_core
    finally:
        sys.path.pop(0)
    return make_ref_core


def test_oracle_matches_recorded_reference(oracle):
    """Runs everywhere: every stage of the oracle against outputs of the reference build recorded in
    tests/golden/ref_core.npz, each stage fed the recorded output of the stage before."""
    z = np.load(os.path.join(GOLDEN_DIR, "ref_core.npz"))
    assert int(z["n_cases"]) == len(K.GOLDEN_CASES) >= 3
    for i, (kind, H, W, D) in enumerate(K.GOLDEN_CASES):
        g = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        p = K.pair(kind, H, W, D)
        assert K.sha256(*(p[k] for k in R.KEYS)) == str(g["in_sha256"]), "the inputs differ from the recorded ones"
        cfg = oracle.config(H, W, D - 1)
        aL, aR = arms4(g["arms0"]), arms4(g["arms1"])
        for view, (gray, bgr) in enumerate((("lgray", "lbgr"), ("rgray", "rbgr"))):
            eq(oracle.census(p[gray], cfg), g[f"census{view}"])
            eq(oracle.arms(p[bgr], cfg), arms4(g[f"arms{view}"]))
            eq(oracle.cost_volume(p, cfg, view), g[f"cost{view}"])
            eq(oracle.cost_volume(p, oracle.config(H, W, D - 1, cost="Census"), view), g[f"census_cost{view}"])
            eq(oracle.cbca(g[f"cost{view}"], aL, aR, cfg, view), g[f"agg{view}"])
            eq(pyref_cbca_ni.cbca_ni(g[f"cost{view}"], (aL, aR)[view], 2)[0], g[f"agg_ni{view}"])
            eq(oracle.solve_all(g[f"agg{view}"], cfg), g[f"scaled{view}"])
            eq(oracle.sgm(g[f"scaled{view}"], p[bgr], cfg), g[f"sgm{view}"])
            eq(oracle.sgm(g[f"scaled{view}"], p[bgr], oracle.config(H, W, D - 1, sgm_paths=8)), g[f"sgm8_{view}"])
            eq(oracle.wta(g[f"sgm{view}"], cfg), g[f"disp{view}"])
        for variant in K.VARIANTS:
            tdp, tacc = TWINS[variant](g["scaled0"], p["lbgr"])
            eq(np.asarray(tdp, np.int16), g[f"{variant}_disp"])
            eq(np.asarray(tacc, np.float32), g[f"{variant}_acc"])
            tdp, tacc = SC.FUNCS[variant](g[f"{variant}_crafted"], p["lbgr"])
            eq(np.asarray(tdp, np.int16), g[f"{variant}_crafted_disp"])
            assert PF.same_floats(np.asarray(tacc, np.float32), g[f"{variant}_crafted_acc"])
        odp, oacc = oracle.so(g["scaled0"], p["lbgr"], cfg)
        eq(odp, g["so_disp"]), eq(oacc, g["so_acc"])


def test_recordings_are_current():
    """Both recordings are what the binary gives today on the inputs make_ref_core.py generates."""
    need_binary()
    m = _make_ref_core()
    for now, path in ((m.record(), m.OUT), (m.record_gpu(), m.OUT_GPU)):
        z = np.load(path)
        assert sorted(now) == sorted(z.files)
        for k in z.files:
            np.testing.assert_array_equal(np.asarray(now[k]), z[k], err_msg=k)


def test_recorded_gpu_cases_are_complete():
    """Runs everywhere: tests/golden/ref_core_gpu.npz names every array of every case of ref_core_cases.gpu_keys() on
    today's inputs; an array kept in full has the recorded digest; every stage has >= 3 cases, and the cbca and sgm
    stages one with D > 128.  That is not the whole of the D > 128 condition: the GPU shapes of the cost and so
    stages are the issue's own (D 16 - 100 and 32), so for those stages D > 128 survives on the CPU side only -- the
    cases (5, 260, 200) and (12, 258, 256) of K.CPU_CASES, each through run_defined, and (6, 18, 130) recorded in
    ref_core.npz."""
    z = dict(np.load(os.path.join(GOLDEN_DIR, "ref_core_gpu.npz")))
    keys = K.gpu_keys()
    assert sorted(k[3:] for k in z if k.startswith("in_")) == sorted(keys)
    for key, spec in keys.items():
        assert K.gpu_input_digest(spec) == str(z[f"in_{key}"]), key
        names = str(z[f"names_{key}"]).split(",")
        for n in names:
            assert f"sha_{key}_{n}" in z, (key, n)
            if f"arr_{key}_{n}" in z:
                assert K.sha256(z[f"arr_{key}_{n}"]) == str(z[f"sha_{key}_{n}"]), (key, n)
    stage_cases = {"cost": [s for s in keys.values() if s[0] == "cost"], "cbca": [s for s in keys.values() if s[0] == "cbca"],
                   "sgm": [s for s in keys.values() if s[0] == "sgm"], "so": [s for s in keys.values() if s[0] == "so"],
                   "wta": [s for s in keys.values() if s[0] == "wta"]}
    for stage, specs in stage_cases.items():
        assert len(specs) >= 3, stage
    for stage in ("cbca", "sgm", "wta"):
        assert any(s[4] > 128 for s in stage_cases[stage]), stage
