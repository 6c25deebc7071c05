"""GPU parity of aggregation "AWS" against the numpy twin (tests/pyref_aws.py), bit for bit.

AWS(), the branch without JBF_STANDARD (stereoMatching.cpp:5711-5792): both images' Lab planes,
the 35 x 35 adaptive support weights and the out-of-place aggregation of both views (sm_aws.hip).
The synthetic pairs are heavily textured: as generated the mean weight is about 0.03 and almost
only the centre tap counts, so a mis-indexed tap would pass unseen.  Every shape therefore also
runs with the colours compressed to 128 + (x - 128) // 16, and the test asserts with the twin that
each image's mean weight is then >= 0.25 (a condition on the inputs, not a tolerance).
Kernel layout (sm_aws.hip): a block covers one row, 32 adjacent u (four waves of 8) and 64
adjacent d; the weights are computed band by band of image rows (SM_AWS_BAND_BYTES shrinks the
band so that small images span several bands).
PARITY UNPINNED: the Lab planes restate OpenCV's 8-bit BGR2Lab.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref
import pyref_aws as A
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
AWS = 7
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def compressed(pair):
    return {k: (128 + (pair[k].astype(np.int32) - 128) // 16).astype(np.uint8) for k in KEYS}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.load()
    return O


@functools.lru_cache(maxsize=None)
def _case(H, W, D, rv, ru, idx, comp, gamma_c=5.0):
    """The pair, both views' raw cost volumes and the twin's volumes, masks and weights (once)."""
    O = _oracle()
    pair = S.make_pair(H, W, D, idx)
    pair = compressed(pair) if comp else {k: pair[k] for k in KEYS}
    cfg = O.config(H, W, D - 1)
    cost = [O.cost_volume(pair, cfg, view=v) for v in (0, 1)]
    want, ok, wt = A.aws(cost, pair["lbgr"], pair["rbgr"], rv, ru, f32(gamma_c))
    for a in cost + want:
        a.setflags(write=False)
    return pair, cost, want, ok, [float(w.mean()) for w in wt]


class Ctx:
    """One AWS context through the C ABI (do_refine = 1: both views are aggregated)."""

    def __init__(self, H, W, D, **over):
        self.lib = _capi.load()
        self.shape = (H, W, D)
        p = _capi.default_params(D - 1, H, W, aggregation=AWS, optimization=0, do_refine=1, **over)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(p), 0))

    def config(self, rv, ru, gamma_c):
        _capi.check(self.lib, self.ctx, self.lib.sm_aws_config(self.ctx, rv, ru, gamma_c))

    def volumes(self, pair):
        H, W, D = self.shape
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        _capi.check(self.lib, self.ctx, self.lib.sm_set_images(self.ctx, _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3,
                                                               _capi.ptr(a["lgray"]), _capi.ptr(a["rgray"]), W))
        _capi.check(self.lib, self.ctx, self.lib.sm_cost_calculate(self.ctx))
        out = []
        for view in (0, 1):
            got = np.empty((H, W, D), f32)
            _capi.check(self.lib, self.ctx, self.lib.sm_get_volume(self.ctx, view, _capi.ptr(got)))
            out.append(got)
        return out

    def lab(self, view):
        H, W, _ = self.shape
        got = np.empty((H, W, 3), np.uint8)
        _capi.check(self.lib, self.ctx, self.lib.sm_get_aws_lab(self.ctx, view, _capi.ptr(got)))
        return got

    def close(self):
        self.lib.sm_destroy(self.ctx)


def _check_volumes(H, W, D, rv, ru, idx, gamma_c=5.0, variants=(False, True)):
    for comp in variants:
        pair, cost, want, ok, means = _case(H, W, D, rv, ru, idx, comp, gamma_c)
        if comp and gamma_c == 5.0:
            print(f"{H}x{W}x{D} r {rv},{ru} compressed: mean weight {means[0]:.3f} / {means[1]:.3f}")
            assert min(means) >= 0.25, means
        c = Ctx(H, W, D)
        try:
            c.config(rv, ru, gamma_c)
            got = c.volumes(pair)
            labs = [c.lab(v) for v in (0, 1)]
        finally:
            c.close()
        for v, img in ((0, "lbgr"), (1, "rbgr")):
            np.testing.assert_array_equal(labs[v], A.bgr2lab(pair[img]), err_msg=f"Lab of view {v}")
            # elements with u1 >= W or u2 < 0 keep the raw cost bits
            out = ~ok[v]
            np.testing.assert_array_equal(bits(got[v])[:, out], bits(cost[v])[:, out], err_msg=f"view {v}: raw elements")
            np.testing.assert_array_equal(bits(got[v]), bits(want[v]), err_msg=f"compressed {comp} view {v}")


# H, W, D, rv, ru, seed
SHAPES = [(2, 2, 1, 17, 17, 800),       # every tap reflects repeatedly
          (3, 5, 2, 1, 1, 801),         # smallest radius
          (20, 37, 8, 17, 17, 802),     # full window, small D
          (37, 41, 16, 17, 17, 803),    # just past one window each way
          (6, 70, 65, 17, 17, 804),     # D one past a wave, W > D
          (5, 9, 64, 17, 17, 805),      # W < D: mostly pass-through
          (9, 19, 256, 17, 17, 806),    # large D
          (4, 6, 1024, 2, 2, 807),      # the D limit
          (40, 24, 16, 17, 0, 808),     # 1-D window, rows only
          (40, 24, 16, 0, 17, 809),     # 1-D window, columns only
          (12, 50, 64, 5, 3, 810),      # unequal radii
          (7, 5, 3, 0, 0, 811),         # identity
          # tile edges of the kernel: 8 u per wave, 32 u per block, 64 d per block
          (3, 31, 5, 2, 17, 812),       # one pixel short of a block's 32 u
          (3, 32, 5, 2, 17, 813),       # exactly one block
          (3, 33, 66, 2, 17, 814),      # one pixel and two disparities past a block
          (2, 9, 3, 1, 17, 815),        # one pixel past a wave's 8 u
          (2, 72, 130, 1, 4, 816)]      # three blocks along u, three along d


@pytest.mark.parametrize("H,W,D,rv,ru,idx", SHAPES)
def test_aws_volume_bits(H, W, D, rv, ru, idx):
    """Both views, as generated and compressed: uint32 equality with the twin."""
    _check_volumes(H, W, D, rv, ru, idx)


def test_aws_identity_window_returns_the_raw_costs():
    pair, cost, want, ok, _ = _case(7, 5, 3, 0, 0, 811, True)
    for v in (0, 1):   # one tap of weight 1: numer / denom = cost * 1 / 1
        np.testing.assert_array_equal(bits(want[v]), bits(cost[v]))


@pytest.mark.parametrize("gamma_c", [0.5, 50.0])
def test_aws_gamma(gamma_c):
    _check_volumes(12, 21, 8, 17, 17, 820, gamma_c=gamma_c)


def test_aws_rows_end_inside_a_weight_band(monkeypatch):
    """A band budget of 1 MB holds two rows at W = 41 (2 x 1225 x 41 x 4 B per image row): 37 rows
    are 18 bands and one row of a 19th; and the default budget again in the same process."""
    monkeypatch.setenv("SM_AWS_BAND_BYTES", str(1 << 20))
    _check_volumes(37, 41, 16, 17, 17, 803, variants=(True,))
    monkeypatch.setenv("SM_AWS_BAND_BYTES", "1")   # less than one row: one row per band
    _check_volumes(20, 37, 8, 17, 17, 802, variants=(True,))


PALETTE = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)], np.uint8)


@pytest.mark.parametrize("kind", ["random", "palette"])
def test_aws_lab_plane(kind):
    """sm_get_aws_lab against the twin: random colours, and the six saturated colours (whose
    weights underflow to subnormal products), with the volumes of the same images."""
    H, W, D = 9, 14, 4
    rng = np.random.default_rng(830)
    pair = {k: S.make_pair(H, W, D, 830)[k] for k in KEYS}
    for k in ("lbgr", "rbgr"):
        pair[k] = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) if kind == "random"
                   else PALETTE[rng.integers(0, 6, (H, W))])
    O = _oracle()
    cfg = O.config(H, W, D - 1)
    cost = [O.cost_volume(pair, cfg, view=v) for v in (0, 1)]
    want, _, _ = A.aws(cost, pair["lbgr"], pair["rbgr"], 4, 6)
    c = Ctx(H, W, D)
    try:
        c.config(4, 6, 5.0)
        got = c.volumes(pair)
        for v, img in ((0, "lbgr"), (1, "rbgr")):
            np.testing.assert_array_equal(c.lab(v), A.bgr2lab(pair[img]))
            np.testing.assert_array_equal(bits(got[v]), bits(want[v]))
    finally:
        c.close()


def test_aws_config_between_two_runs():
    """sm_aws_config on a live context: the second run's volumes are the twin's for the new constants."""
    H, W, D = 12, 21, 8
    first = _case(H, W, D, 17, 17, 820, True)
    second = _case(H, W, D, 5, 3, 820, True, 2.0)
    assert (bits(first[2][0]) != bits(second[2][0])).mean() > 0.5
    c = Ctx(H, W, D)
    try:
        got = c.volumes(first[0])        # the defaults: 17, 17, 5
        for v in (0, 1):
            np.testing.assert_array_equal(bits(got[v]), bits(first[2][v]))
        c.config(5, 3, 2.0)
        got = c.volumes(first[0])
        for v in (0, 1):
            np.testing.assert_array_equal(bits(got[v]), bits(second[2][v]))
    finally:
        c.close()


# ---- maps through sm_run: n = 3, 20 x 37 x 16, radius 17 -------------------------------------
MH, MW, MD, MN = 20, 37, 16, 3


@functools.lru_cache(maxsize=None)
def _map_case():
    """The batch (compressed colours), and per pair the twin's volumes after SolveAll."""
    O = _oracle()
    batch = S.make_batch(MN, MH, MW, MD, first_index=840)
    batch = {k: (128 + (batch[k].astype(np.int32) - 128) // 16).astype(np.uint8) for k in KEYS}
    cfg = O.config(MH, MW, MD - 1)
    vols = []
    for i in range(MN):
        pair = {k: batch[k][i] for k in KEYS}
        cost = [O.cost_volume(pair, cfg, view=v) for v in (0, 1)]
        want, _, _ = A.aws(cost, pair["lbgr"], pair["rbgr"])
        vols.append([pyref.solve_all(w) for w in want])
    return batch, vols


def _want_map(i, opt, paths=4, refine=False):
    batch, vols = _map_case()
    pair = {k: batch[k][i] for k in KEYS}

    def view(v):
        vm, img = vols[i][v], pair[("lbgr", "rbgr")[v]]
        if opt == "sgm":
            return pyref.wta(pyref.sgm(vm, img, paths=paths))
        if opt == "so":
            return pyref.so(vm, pair["lbgr"])[1]   # so reads I_c[0] for both views (cpp:1098)
        return pyref.wta(vm)

    d0 = view(0)
    if refine:
        d0 = pyref.refine(d0, view(1), pyref.arms(pair["lbgr"]), pair["lbgr"], MD)
    return d0


MAPS = [dict(optimization=0),                                   # WTA
        dict(optimization=1, sgm_paths=4),
        dict(optimization=1, sgm_paths=8),
        dict(optimization=2),                                   # so
        dict(optimization=1, sgm_paths=4, do_refine=1),
        dict(optimization=1, sgm_paths=4, sub_batch=1, num_streams=1),
        dict(optimization=1, sgm_paths=4, sub_batch=2, num_streams=2),
        dict(optimization=1, sgm_paths=4, sub_batch=1, num_streams=2, do_refine=1)]


@pytest.mark.parametrize("cfg", MAPS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_aws_maps(cfg):
    """sm_run (SolveAll's scale in the aggregation's store, raw elements included): the maps of the
    twin's volumes through pyref's optimisers; two runs of one context agree."""
    batch, _ = _map_case()
    sb = StereoBatch(MD - 1, MH, MW, MN, device=0, aggregation="AWS", **cfg)
    try:
        sb.upload(*(batch[k] for k in KEYS))
        got = sb.run(0.3)
        again = sb.run(0.3)
    finally:
        sb.close()
    np.testing.assert_array_equal(again, got)
    opt = {0: "wta", 1: "sgm", 2: "so"}[cfg["optimization"]]
    for i in range(MN):
        want = _want_map(i, opt, cfg.get("sgm_paths", 4), bool(cfg.get("do_refine")))
        np.testing.assert_array_equal(got[i], want, err_msg=f"pair {i}")


def test_aws_reference_ordered_api():
    """costCalculate -> SolveAll([sm], 1, 0.3) -> dispOptimize with the class selectors and constants."""
    batch, _ = _map_case()
    pair = {k: batch[k][0] for k in KEYS}
    O = _oracle()
    StereoMatching.aggregation, StereoMatching.AWS_RADIUS_V, StereoMatching.AWS_GAMMA_C = "AWS", 6, 3.0
    try:
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None,
                            StereoMatching.Parameters(MD - 1, MH, MW), device=0)
        sm.costCalculate()
        vol = sm.vm[0]
        SolveAll([sm], 1, 0.3)
        got = sm.dispOptimize()
    finally:
        StereoMatching.aggregation, StereoMatching.AWS_RADIUS_V, StereoMatching.AWS_GAMMA_C = "CBCA", 17, 5.0
    cost = O.cost_volume(pair, O.config(MH, MW, MD - 1))
    want, _, _ = A.aws([cost, None], pair["lbgr"], pair["rbgr"], 6, 17, f32(3.0))
    np.testing.assert_array_equal(bits(vol), bits(want[0]))
    np.testing.assert_array_equal(got, pyref.wta(pyref.sgm(pyref.solve_all(want[0]), pair["lbgr"], paths=4)))
