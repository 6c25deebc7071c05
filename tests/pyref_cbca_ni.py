"""cbca_core with Parameters::cbca_intersect == false (stereoMatching.cpp:5585-5666) restated in numpy on top of
the C oracle's pieces: the original cross-based aggregation of Zhang et al.

    per view LOR, on vm[LOR] with HVL[LOR] (the left image's arms for view 0, the right image's for view 1):
    for k in 0 .. N - 1:
        area = ones(h, w)                                   int32, per pixel (cpp:5606)
        two 1-D passes, H then V for even k, V then H for odd k; a pass along its axis x:
            gen1DCumu (cpp:3896-3926)   S(x) = S(x - 1) + vm(x), f32, in scan order; A likewise of area
            cal1DCost (h:1643-1715)     tail / head = the pixel's own arm pair of the direction
                                        ((left, right) for H, (up, down) for V), pt = x - tail - 1,
                                        out = pt >= 0 ? S(x + head) - S(pt) : S(x + head), the same for area
        genfinalVm_cbca (cpp:3969-3992) vm(v, u, d) /= (float)area(v, u)

The raw costs and the arms come from the oracle (O.cost_volume, O.arms), as tests/pyref_cbca_dw.compose takes
them; the aggregation is tests/pyref.cbca's with the arms broadcast over d and a 2-D area.
"""
import numpy as np

import pyref_cbca_dw as DW
from oracle import oracle as O

f32 = np.float32
WIN0 = dict(DW.WIN0)
make_input = DW.make_input
wta = DW.wta


def cbca_ni(vm: np.ndarray, arms: np.ndarray, iters: int = 2):
    """vm H x W x D f32, arms H x W x 4 (left, right, up, down) of the view's own image -> (volume, area int32)."""
    H, W, D = vm.shape
    A = np.asarray(arms).astype(np.int64)
    vm = np.ascontiguousarray(vm, f32).copy()
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    area = np.ones((H, W), np.int64)

    def pass1d(vm, area, horiz):
        axis = 1 if horiz else 0
        S = np.add.accumulate(vm, axis=axis, dtype=f32)   # sequential: S(x) = S(x - 1) + vm(x)
        Ar = np.add.accumulate(area, axis=axis)
        tail = A[..., 0] if horiz else A[..., 2]
        head = A[..., 1] if horiz else A[..., 3]
        if horiz:
            pt = uu - tail - 1
            hi, ti = (vv, uu + head), (vv, np.maximum(pt, 0))
        else:
            pt = vv - tail - 1
            hi, ti = (vv + head, uu), (np.maximum(pt, 0), uu)
        inner = pt >= 0
        out = np.where(inner[:, :, None], (S[hi] - S[ti]).astype(f32), S[hi]).astype(f32)
        return out, np.where(inner, Ar[hi] - Ar[ti], Ar[hi])

    for it in range(iters):
        area = np.ones((H, W), np.int64)
        for horiz in ((True, False) if it % 2 == 0 else (False, True)):
            vm, area = pass1d(vm, area, horiz)
        vm = (vm / area.astype(f32)[:, :, None]).astype(f32)
    return vm, area.astype(np.int32)


def inner_masks(arms: np.ndarray):
    """(inner of the H pass, inner of the V pass) of an H x W x 4 arm array."""
    a = np.asarray(arms).astype(np.int64)
    H, W = a.shape[:2]
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return uu - a[..., 0] - 1 >= 0, vv - a[..., 2] - 1 >= 0


def pieces(pair: dict, D: int, cost: str = "censusGrad", win=None, views: int = 2):
    """(raw cost volumes per view, [left arms, right arms]) from the oracle with window `win`."""
    H, W = pair["lgray"].shape
    cfg = O.config(H, W, D - 1, cost, **dict(WIN0 if win is None else win))
    raw = [O.cost_volume(pair, cfg, view) for view in range(views)]
    return raw, [O.arms(pair["lbgr"], cfg), O.arms(pair["rbgr"], cfg)]


def aggregate(pair: dict, D: int, iters: int = 2, cost: str = "censusGrad", win=None, refine: bool = True) -> dict:
    """dict(vm0, area0 [, vm1, area1], raw0 [, raw1], armsL, armsR)."""
    raw, arms = pieces(pair, D, cost, win, 2 if refine else 1)
    out = {"armsL": arms[0], "armsR": arms[1]}
    for view, r in enumerate(raw):
        out[f"raw{view}"] = r
        out[f"vm{view}"], out[f"area{view}"] = cbca_ni(r, arms[view], iters)
    return out


def double_window(pair: dict, D: int, refine: bool = False, cost: str = "censusGrad") -> dict:
    """The double window with both runs without intersection: window 1 and window 0 (two iterations each) on the
    raw costs made with window 0's settings, composed with combine2Vm_4's mask."""
    H, W = pair["lgray"].shape
    raw, arms0 = pieces(pair, D, cost, DW.WIN0, 2 if refine else 1)
    cfg1 = O.config(H, W, D - 1, cost, **DW.WIN1)
    arms1 = [O.arms(pair["lbgr"], cfg1), O.arms(pair["rbgr"], cfg1)]
    mask = DW.mask_from_arms(arms0[0])
    out = {"mask": mask}
    for view, r in enumerate(raw):
        small, large = cbca_ni(r, arms0[view], 2)[0], cbca_ni(r, arms1[view], 2)[0]
        out[f"vm{view}"] = np.where(mask.astype(bool)[:, :, None], large, small)
    return out
