"""refine()'s discontinuity adjustment without a GPU: the restatement's (tests/pyref_da.py) building blocks on
hand-computed cases, sm_refine_da_config's argument checks on a device-less context, the symbol tables, and the
facades' plumbing through a recording stand-in for the library."""
import ctypes as C
import os
import re
from collections import deque

import numpy as np
import pytest

import pyref_da as DA
from mystereomatching_amd import StereoBatch, StereoMatching, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the restated OpenCV forms ---------------------------------------------------------------------

def test_taps_derive_from_sigma_4():
    assert DA.gaussian_taps(4.0, 3) == (84, 87, 84)
    assert sum(DA.gaussian_taps()) == 255                      # not 256: a constant image of 255 blurs to 253
    assert (DA.BLUR_SIDE, DA.BLUR_CENTRE) == (84, 87) == _capi.REFINE_DA_DEFAULTS[2:]
    assert (DA.CANNY_LOW, DA.CANNY_HIGH) == (20, 60) == _capi.REFINE_DA_DEFAULTS[:2]
    assert DA.cv_round(0.5) == 0 and DA.cv_round(1.5) == 2 and DA.cv_round(2.5) == 2


def test_lut_rounding_by_hand():
    # bins 3, 5, 9 hold 2, 1, 1 pixels: scale = 255 / (4 - 2) = 127.5; sums 1, 2 -> 127.5 (half to even: 128), 255
    hist = [0] * 256
    hist[3], hist[5], hist[9] = 2, 1, 1
    lut = DA.equalize_lut(hist, 4)
    assert lut[3] == 0 and lut[5] == 128 and lut[9] == 255 and lut[4] == 0 and lut[8] == 128 and lut[255] == 255
    # 2, 2, 1: scale = 255 / 3 = 85 in float; sums 2, 3 -> 170, 255
    hist = [0] * 256
    hist[0], hist[1], hist[200] = 2, 2, 1
    lut = DA.equalize_lut(hist, 5)
    assert (lut[0], lut[1], lut[200]) == (0, 170, 255)
    # half-to-even on the other side: scale = 255 / 2, sum 1 -> 127.5 -> 128; with 6 bins of one pixel beyond the
    # first, scale = 42.5: sums 1..6 -> 42.5 (42), 85, 127.5 (128), 170, 212.5 (212), 255
    hist = [0] * 256
    for b in range(10, 17):
        hist[b] = 1
    lut = DA.equalize_lut(hist, 7)
    assert [lut[b] for b in range(10, 17)] == [0, 42, 85, 128, 170, 212, 255]
    img = np.array([[3, 3], [5, 9]], np.uint8)
    np.testing.assert_array_equal(DA.equalize(img), [[0, 0], [128, 255]])


def test_equalise_constant_and_offset_first_bin():
    for v in (0, 7, 255):
        img = np.full((5, 6), v, np.uint8)
        assert DA.equalize_lut(np.bincount(img.ravel(), minlength=256), img.size) is None
        np.testing.assert_array_equal(DA.equalize(img), img)
    img = np.full((4, 4), 40, np.uint8)
    img[0, 0] = 41
    out = DA.equalize(img)
    assert out[0, 0] == 255 and (out.ravel()[1:] == 0).all()


def test_to_u8_clamps():
    np.testing.assert_array_equal(DA.to_u8(np.array([[-32, -1, 0, 255, 256, 3000]], np.int16)), [[0, 0, 0, 255, 255, 255]])


def test_blur_by_hand():
    assert (DA.blur(np.full((4, 5), 255, np.uint8)) == 253).all()      # (255 * 255 * 255 + 32768) >> 16
    assert (DA.blur(np.full((4, 5), 255, np.uint8), 85, 86) == 255).all()   # a kernel that sums to 256
    one = np.zeros((5, 5), np.uint8)
    one[2, 2] = 200
    want = np.zeros((5, 5), np.int64)
    want[1:4, 1:4] = np.array([[84 * 84, 84 * 87, 84 * 84], [87 * 84, 87 * 87, 87 * 84], [84 * 84, 84 * 87, 84 * 84]]) * 200
    np.testing.assert_array_equal(DA.blur(one), (want + 32768) >> 16)
    corner = np.zeros((3, 3), np.uint8)
    corner[1, 1] = 200                          # reflected: the corner sees the centre through both sides, twice
    assert DA.blur(corner)[0, 0] == (168 * 168 * 200 + 32768) >> 16
    # 2 x 2: -1 -> 1 and len -> len - 2 = 0 both fold onto the other pixel
    img = np.array([[10, 200], [60, 90]], np.uint8)
    r = np.array([[87 * 10 + 168 * 200, 87 * 200 + 168 * 10], [87 * 60 + 168 * 90, 87 * 90 + 168 * 60]])
    want = np.array([[87 * r[0, 0] + 168 * r[1, 0], 87 * r[0, 1] + 168 * r[1, 1]],
                     [87 * r[1, 0] + 168 * r[0, 0], 87 * r[1, 1] + 168 * r[0, 1]]])
    np.testing.assert_array_equal(DA.blur(img), (want + 32768) >> 16)
    assert [DA.reflect101(i, 5) for i in (-1, 0, 4, 5)] == [1, 0, 4, 3] and DA.reflect101(-1, 1) == DA.reflect101(1, 1) == 0


def _cand(mag_row, dx_sign=1):
    """Candidates of a one-row gradient field with dy = 0 (the left / right sector)."""
    dx = np.array([mag_row], np.int32) * dx_sign
    return DA.candidates(dx, np.zeros_like(dx), 20)[0][0]


def test_nms_ties():
    # left / right sector: `>` against the left neighbour, `>=` against the right one
    np.testing.assert_array_equal(_cand([0, 50, 50, 0]), [False, True, False, False])   # the left one of a tie wins
    np.testing.assert_array_equal(_cand([0, 50, 0]), [False, True, False])
    np.testing.assert_array_equal(_cand([50, 50]), [True, False])                       # outside is 0
    np.testing.assert_array_equal(_cand([0, 50, 50, 0], -1), [False, True, False, False])   # the sign of dx changes nothing
    np.testing.assert_array_equal(_cand([21, 20]), [True, False])                       # m > low is strict
    # up / down sector likewise
    dy = np.array([[0], [50], [50], [0]], np.int32)
    np.testing.assert_array_equal(DA.candidates(np.zeros_like(dy), dy, 20)[0][:, 0], [False, True, False, False])
    # the diagonal is `>` on both sides: a tie suppresses both; s follows the sign of dx ^ dy
    dx = np.zeros((3, 3), np.int32)
    dx[0, 0] = dx[1, 1] = 30
    dy = dx.copy()
    assert not DA.candidates(dx, dy, 20)[0][1, 1]            # s = +1: compares (0, 0) and (2, 2)
    assert DA.candidates(dx, -dy, 20)[0][1, 1]               # s = -1: compares (0, 2) and (2, 0), both 0
    # sector boundaries: tan 22.5 and tan 67.5 in 15-bit fixed point
    x = 100
    for y, sector in ((41, "h"), (42, "d"), (241, "d"), (242, "v")):
        assert ((y << 15) < x * 13573) == (sector == "h")
        assert ((y << 15) > x * 13573 + (x << 16)) == (sector == "v")


def _components_edges(cand, strong):
    """Components of the candidate mask that hold a strong pixel, a second way."""
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        lab, _ = ndimage.label(cand, structure=np.ones((3, 3), int))
        keep = np.unique(lab[strong])
        return np.where(np.isin(lab, keep[keep > 0]), 255, 0).astype(np.uint8)
    H, W = cand.shape
    out = np.zeros((H, W), np.uint8)
    seen = np.zeros((H, W), bool)
    for h0 in range(H):
        for w0 in range(W):
            if not cand[h0, w0] or seen[h0, w0]:
                continue
            comp, q = [], deque([(h0, w0)])
            seen[h0, w0] = True
            while q:
                h, w = q.popleft()
                comp.append((h, w))
                for a in range(max(h - 1, 0), min(h + 2, H)):
                    for b in range(max(w - 1, 0), min(w + 2, W)):
                        if cand[a, b] and not seen[a, b]:
                            seen[a, b] = True
                            q.append((a, b))
            if any(strong[p] for p in comp):
                for p in comp:
                    out[p] = 255
    return out


@pytest.mark.parametrize("seed,low,high", [(1, 20, 60), (2, 5, 200), (3, 60, 20), (4, 0, 0)])
def test_restatement_properties(seed, low, high):
    rng = np.random.default_rng(seed)
    img = DA.blur(DA.blur(rng.integers(0, 256, (33, 41)).astype(np.uint8)))
    edges, cand, strong = DA.canny(img, low, high)
    assert set(np.unique(edges)) <= {0, 255}
    assert ((edges > 0) <= cand).all()                       # edges are candidates
    assert ((edges > 0) >= strong).all()
    np.testing.assert_array_equal(edges, _components_edges(cand, strong))
    if seed == 2:
        assert 0 < (edges > 0).sum() < cand.sum()            # hysteresis dropped some, kept some
    if seed == 3:
        np.testing.assert_array_equal(edges, DA.canny(img, high, low)[0])   # thresholds in the wrong order are swapped


def test_direction_decision():
    E = np.zeros((3, 3), np.uint8)
    E[1, 1] = 255
    assert DA.direction_of(E, 1, 1) == -1
    for on, want in ((((0, 0), (2, 2)), 4), (((0, 2), (2, 0)), 0), (((0, 1), (2, 1)), 6), (((1, 0), (1, 2)), 2),
                     (((0, 1),), -1),            # above only: the nested if leaves -1, the left / right test is not reached
                     (((0, 0), (1, 2)), -1),     # likewise with a left (upper-left) and a right neighbour
                     (((1, 0), (2, 2)), 2), (((0, 2), (2, 2)), 6)):
        F = E.copy()
        for p in on:
            F[p] = 255
        assert DA.direction_of(F, 1, 1) == want, on


def test_adjust_asymmetry_and_order():
    H, W, D = 3, 5, 4
    E = np.full((H, W), 255, np.uint8)       # every interior pixel: direction 4, sides (h-1, w+1) and (h+1, w-1)
    vm = np.full((H, W, D), 5, f32)
    d = np.full((H, W), 1, np.int16)
    d[0, 2], d[2, 0] = 2, 3                  # the two sides of (1, 1)
    # first side: -0.5 is refused (cost1 >= 0), second side: -0.5 is accepted (cost2 != -1), -1 is not
    vm[0, 2, 2], vm[2, 0, 3] = -0.5, -0.5
    assert DA.adjust(d, E, vm)[1, 1] == 3
    vm[2, 0, 3] = -1
    assert DA.adjust(d, E, vm)[1, 1] == 1
    vm[0, 2, 2] = 4
    assert DA.adjust(d, E, vm)[1, 1] == 2
    vm[0, 2, 2] = np.nan                     # a NaN compares false everywhere
    assert DA.adjust(d, E, vm)[1, 1] == 1
    vm[1, 1, 1] = np.nan
    vm[0, 2, 2] = 0
    assert DA.adjust(d, E, vm)[1, 1] == 1
    # a chain: (1, 3) takes 2 from (0, 4); (1, 2)'s first side is (0, 3), its second (2, 1)
    vm = np.full((H, W, D), 5, f32)
    d = np.full((H, W), 1, np.int16)
    d[0, 4] = 2
    vm[0, 4, 2] = 1
    stats = {}
    out = DA.adjust(d, E, vm, stats)
    assert out[1, 3] == 2 and stats["changed"] == 1 and stats["chained"] == 0
    # holes are left alone and read as cost -1; a disparity >= D reads as -1 too (the documented deviation)
    d = np.full((H, W), 1, np.int16)
    d[1, 1], d[0, 2], d[2, 0] = -32, 2, 9
    np.testing.assert_array_equal(DA.adjust(d, E, np.zeros((H, W, D), f32)), d)
    # maps with fewer than three rows or columns have no interior
    small = np.ones((2, 7), np.int16)
    np.testing.assert_array_equal(DA.adjust(small, np.full((2, 7), 255, np.uint8), np.zeros((2, 7, D), f32)), small)


# ---- the C ABI (validation is host code) -----------------------------------------------------------

def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx


OK_ARGS = (1, 20, 60, 84, 87)


@pytest.mark.parametrize("args,msg", [
    ((1, -1, 60, 84, 87), b"canny_low"), ((1, 32768, 60, 84, 87), b"canny_low"),
    ((1, 20, -1, 84, 87), b"canny_high"), ((0, 20, 32768, 84, 87), b"canny_high"),
    ((1, 20, 60, -1, 87), b"blur_side"), ((1, 20, 60, 84, -1), b"blur_centre"),
    ((1, 20, 60, 85, 87), b"blur_side"), ((1, 20, 60, 0, 257), b"blur_centre"), ((1, 20, 60, 2 ** 30, 2 ** 30), b"2 * side"),
])
def test_refine_da_config_messages(args, msg):
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1))
    try:
        assert lib.sm_refine_da_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_refine_da_config(None, *OK_ARGS) == _capi.SM_EINVAL


def test_refine_da_config_needs_do_refine_and_refuses_so():
    lib, ctx = _create(_capi.default_params(15, 32, 32))
    try:
        assert lib.sm_refine_da_config(ctx, *OK_ARGS) == _capi.SM_EINVAL
        assert b"do_refine" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1, optimization="so"))
    try:
        for args in (OK_ARGS, (0, 20, 60, 84, 87)):
            assert lib.sm_refine_da_config(ctx, *args) == _capi.SM_EINVAL
            assert b"so" in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_null_arguments():
    lib = _capi.load()
    assert lib.sm_get_da_edges(None, None) == _capi.SM_EINVAL
    assert lib.sm_set_da_edges(None, None) == _capi.SM_EINVAL
    assert lib.sm_da_run_image(None, None, 0, None, None, None) == _capi.SM_EINVAL


def test_symbol_tables_and_sm_params():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in ("sm_refine_da_config", "sm_get_da_edges", "sm_da_run_image", "sm_set_da_edges"):
        assert fn in declared and hasattr(lib, fn)
    sig = dict((n, a) for n, _, a in _capi.SIGNATURES)
    assert sig["sm_refine_da_config"][1:] == [C.c_int32] * 5
    assert sig["sm_da_run_image"][2] == C.c_int32
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216
    assert not any("da_" in n or "canny" in n for n, _ in _capi.sm_params._fields_)
    assert "Do_discontinuityAdjust is built" in hdr


# ---- the facades -------------------------------------------------------------------------------------

class Recorder:
    """Stands in for the loaded library: every entry point returns SM_OK and is recorded with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("sm_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return _capi.SM_OK
        return fn

    def named(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    real = _capi.load()
    r.sm_params_default = real.sm_params_default          # host-only: fills the struct
    monkeypatch.setattr(_capi, "load", lambda: r)
    return r


def test_python_facade_defaults():
    assert StereoMatching.Do_discontinuityAdjust is False
    assert tuple(StereoMatching.DA_CANNY) == (20, 60) and tuple(StereoMatching.DA_BLUR_TAPS) == (84, 87)
    for fn in ("refine_da_config", "get_da_edges"):
        assert callable(getattr(StereoBatch, fn))


def test_stereo_batch_plumbing(rec):
    sb = StereoBatch(15, 32, 40, 2, do_refine=1, refine_da=dict(on=True, canny_low=10, blur_centre=88))
    assert [a[1:] for a in rec.named("sm_refine_da_config")] == [(1, 10, 60, 84, 88)]
    sb.refine_da_config(False)
    assert rec.named("sm_refine_da_config")[-1][1:] == (0, 20, 60, 84, 87)
    e = sb.get_da_edges()
    assert e.shape == (32, 40) and e.dtype == np.uint8 and len(rec.named("sm_get_da_edges")) == 1
    sb._ctx = None
    rec.calls.clear()
    sb = StereoBatch(15, 32, 40, 2, do_refine=1)          # without the override the entry point is not called
    assert not rec.named("sm_refine_da_config")
    sb._ctx = None


def test_compute_function_hands_the_override_on(rec):
    batch = pytest.importorskip("mystereomatching_amd.batch")
    fn = batch.hip_compute_fn(15, 32, 40, 2, 0, do_refine=1, refine_da=dict(on=True))
    assert [a[1:] for a in rec.named("sm_refine_da_config")] == [(1, 20, 60, 84, 87)]
    assert fn.get_da_edges().shape == (32, 40)


def test_stereo_matching_plumbing(rec):
    cls = StereoMatching
    saved = (cls.Do_refine, cls.Do_discontinuityAdjust, cls.DA_CANNY)
    z3, z1 = np.zeros((32, 40, 3), np.uint8), np.zeros((32, 40), np.uint8)
    try:
        for refine, da, want in ((True, True, [(1, 30, 90, 84, 87)]), (True, False, []), (False, True, [])):
            rec.calls.clear()
            cls.Do_refine, cls.Do_discontinuityAdjust, cls.DA_CANNY = refine, da, (30, 90)
            sm = cls(z3, z3, z1, z1, param=cls.Parameters(15, 32, 40))
            assert [a[1:] for a in rec.named("sm_refine_da_config")] == want
            if refine:
                sm.refine()
                assert (sm.DA_Edge is not None) == da and len(rec.named("sm_get_da_edges")) == int(da)
            sm._ctx = None
    finally:
        cls.Do_refine, cls.Do_discontinuityAdjust, cls.DA_CANNY = saved


def test_cpp_facade_source_and_docs():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("inline static bool Do_discontinuityAdjust = false;", "Mat DA_Edge;",
                 "sm_refine_da_config(ctx_, 1, da_canny_low, da_canny_high, da_blur_side, da_blur_centre)",
                 "sm_get_da_edges(ctx_, DA_Edge.ptr<uint8_t>())"):
        assert decl in src, decl
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "Do_discontinuityAdjust" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "unpinned" in design and "sm_refine_da.hip" in design


def test_da_facade_check_compiles(tmp_path):
    """tests/cpp/da_facade_check.cpp builds against the facade and the library (its maps are compared on the GPU in
    tests/test_gpu_da.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "da_facade_check.cpp"), str(tmp_path / "da_facade_check"))
