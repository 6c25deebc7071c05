"""CBCA()'s double-window branch (Parameters::cbca_double_win, stereoMatching.cpp:4337-4357) restated on top of
the C oracle and tests/pyref_box.py.

    vm2 = clone(vm)
    arms from window 1 (cbca_crossL[1] = 23, cbca_crossL_out[1] = 23, cbca_cTresh[1] = 30, cbca_cTresh_out[1] = 0)
    cbca_core(vm2, 2)
    arms from window 0 (17 / 34 / 20 / 6); cbca_core(vm, 2)
    combine2Vm_4 (cpp:4273-4331):
        arm_Lst(v, u) = max of the four window-0 arms of HVL[0] (the LEFT image), as float
        boxFilter(arm_Lst, 3 x 3)              normalised, BORDER_REFLECT_101, double sums
        arm_Mask = arm_Lst < 5; a masked pixel takes all d_ costs of vm2, for view 0 and, with Do_refine, view 1

Both aggregations start from ONE raw cost volume (`vm2 = clone(vm)`): costCalculate made it before CBCA() ran, and
censusGrad's gradient term took its adaptive weights from window 0's arms (grad(), cpp:630-633).  A whole oracle
run with window 1's arm settings would compute those weights from window 1's arms, so the oracle is used in
pieces instead: its cost volume with window 0's settings, its arms for each window, and its cbca_core
(smo_cbca_view) twice on copies of that volume, two iterations each (the literal 2 of cpp:4344, 4347).
"""
import ctypes as C

import numpy as np

import pyref_box
from mystereomatching_amd import synthetic as S
from oracle import oracle as O

WIN0 = dict(arm_L=17, arm_L_out=34, arm_cT=20, arm_cT_out=6)
WIN1 = dict(arm_L=23, arm_L_out=23, arm_cT=30, arm_cT_out=0)
ARM_LEN_THRES = 5.0


def soften(pair: dict) -> dict:
    """The test input: the left two thirds of the columns of both colour images replaced by their 5 x 5 integer
    box mean (edge padding, floor division); the gray images follow.  Long arms there, short ones in the rest."""
    out = dict(pair)
    for k in ("lbgr", "rbgr"):
        a = pair[k].astype(np.int32)
        H, W = a.shape[:2]
        p = np.pad(a, ((2, 2), (2, 2), (0, 0)), mode="edge")
        s = np.zeros_like(a)
        for dy in range(5):
            for dx in range(5):
                s += p[dy:dy + H, dx:dx + W]
        b = pair[k].copy()
        b[:, :W * 2 // 3] = (s // 25).astype(np.uint8)[:, :W * 2 // 3]
        out[k] = b
    out["lgray"], out["rgray"] = S.bgr_to_gray(out["lbgr"]), S.bgr_to_gray(out["rbgr"])
    return out


def make_input(H: int, W: int, D: int, index: int = 0) -> dict:
    return soften(S.make_pair(H, W, D, index))


def arm_max(arms: np.ndarray) -> np.ndarray:
    """H x W x 4 arm lengths -> the longest of the four, int64."""
    return np.asarray(arms).astype(np.int64).max(axis=2)


def nine_sum(m: np.ndarray) -> np.ndarray:
    """Sum of the 3 x 3 neighbourhood with BORDER_REFLECT_101, in integers."""
    H, W = m.shape
    ri = [pyref_box.reflect101(y, H) for y in range(-1, H + 1)]
    ci = [pyref_box.reflect101(x, W) for x in range(-1, W + 1)]
    p = m[ri][:, ci]
    return sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3))


def mask_from_arms(arms_left0: np.ndarray, thres: float = ARM_LEN_THRES) -> np.ndarray:
    """arm_Mask as combine2Vm_4 computes it: cv::boxFilter's float result compared with armLthres."""
    lst = arm_max(arms_left0).astype(np.float32)
    return (pyref_box.box_filter(lst, 3, 3) < np.float32(thres)).astype(np.uint8)


def mask_int(arms_left0: np.ndarray, isum: int = 45) -> np.ndarray:
    """The integer form of the predicate for the reference's threshold 5: nine-term sum < 45."""
    return (nine_sum(arm_max(arms_left0)) < isum).astype(np.uint8)


def compose(pair: dict, D: int, refine: bool = True, cost: str = "censusGrad", thres: float = ARM_LEN_THRES,
            win0=None, win1=None) -> dict:
    """dict(mask, arms (window 0, left), vm0, vm1 (composed), small0, small1, large0, large1)."""
    H, W = pair["lgray"].shape
    win0, win1 = dict(WIN0 if win0 is None else win0), dict(WIN1 if win1 is None else win1)
    lib = O.load()
    lib.smo_cbca_view.argtypes = [C.POINTER(O.Config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.smo_cbca_view.restype = None
    cfg0 = O.config(H, W, D - 1, cost, cbca_iters=2, **win0)
    raw = [O.cost_volume(pair, cfg0, view) for view in range(2 if refine else 1)]
    vols = {}
    for name, win in (("small", win0), ("large", win1)):
        cfg = O.config(H, W, D - 1, cost, cbca_iters=2, **win)
        aL, aR = O.arms(pair["lbgr"], cfg), O.arms(pair["rbgr"], cfg)
        for view, r in enumerate(raw):
            vol = r.copy()
            lib.smo_cbca_view(C.byref(cfg), vol.ctypes.data, aL.ctypes.data, aR.ctypes.data, view)
            vols[name + str(view)] = vol
    arms = O.arms(pair["lbgr"], cfg0)
    mask = mask_from_arms(arms, thres)
    out = {"mask": mask, "arms": arms, **vols}
    sel = mask.astype(bool)[:, :, None]
    out["vm0"] = np.where(sel, vols["large0"], vols["small0"])
    if refine:
        out["vm1"] = np.where(sel, vols["large1"], vols["small1"])   # the LEFT mask for the right view as well
    return out


def wta(vol: np.ndarray) -> np.ndarray:
    return np.argmin(vol, axis=2).astype(np.int16)   # the first minimum, as gen_dispFromVm
