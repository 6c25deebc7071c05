"""bad-t evaluator of the reference (calErr, stereoMatching.h:1748-1825).

A pixel counts when mask == 255; it is an error when DP < 0 or |DT - DP| > t.  The reference
reports t = errorThreshold = 1 (h:225); BASELINE.json asks for t = 2 as well.  RMS follows the
reference: the float sum adds pow(dif, 2) per valid pixel and 2 per invalid one, in raster order
— evaluated by sm_cal_err in libsm_hip.so with exactly that arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

REGIONS = ("nonocc", "all", "disc")   # I_mask order (cpp:2073-2075)


def cal_err(DP: np.ndarray, DT: np.ndarray, mask: np.ndarray, thres: float = 1.0):
    """Return (PBM, RMS) over mask == 255 (one region of calErr)."""
    dp = np.ascontiguousarray(DP, np.int16)
    dt = np.ascontiguousarray(DT, np.float32)
    m = np.ascontiguousarray(mask, np.uint8)
    if not (dp.shape == dt.shape == m.shape) or dp.ndim != 2:
        raise ValueError("DP, DT and mask must be H x W arrays of one shape")
    lib = _capi.load()
    pbm, rms = C.c_float(), C.c_float()
    st = lib.sm_cal_err(_capi.ptr(dp), _capi.ptr(dt), _capi.ptr(m), dp.shape[0], dp.shape[1], float(thres),
                        C.byref(pbm), C.byref(rms))
    _capi.check(lib, None, st, "sm_cal_err")
    return float(pbm.value), float(rms.value)


def cal_err_regions(DP, DT, masks: dict, thres: float = 1.0) -> dict:
    """calErr over every available region: {region: (PBM, RMS)} (h:1760-1799)."""
    return {r: cal_err(DP, DT, masks[r], thres) for r in REGIONS if masks.get(r) is not None}


# ---- the per-stage error table (sm_eval_config): saveFromDisp -> calErr at every stage, on the GPU ----------------

class StageErrors(np.ndarray):
    """The error table as a structured array [..][stages][3 regions] of sm_stage_err records (count, invalid,
    bad[4], sum_sq) with the derived values of calErr; `names` are the stages' names."""

    names: tuple = ()

    def __array_finalize__(self, obj):
        self.names = getattr(obj, "names", ())

    def pbm(self, k: int = 0) -> np.ndarray:
        """PBM = (float)bad[k] / count, 0 where count == 0 (float32, as sm_cal_err)."""
        a = np.asarray(self)
        cnt = a["count"].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = a["bad"][..., k].astype(np.float32) / cnt
        return np.where(a["count"] == 0, np.float32(0), out).astype(np.float32)

    def rms(self) -> np.ndarray:
        """RMS = sqrtf((float)sum_sq / count), 0 where count == 0."""
        a = np.asarray(self)
        cnt = a["count"].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.sqrt(a["sum_sq"].astype(np.float32) / cnt)
        return np.where(a["count"] == 0, np.float32(0), out).astype(np.float32)


def stage_errors_array(raw: np.ndarray, names) -> StageErrors:
    out = np.ascontiguousarray(raw).view(StageErrors)
    out.names = tuple(names)
    return out


def pack_regions(shape, nonocc=None, all=None, disc=None) -> np.ndarray:
    """One byte per pixel, bit r set where mask r == 255 (I_mask's order); None is an absent region."""
    out = np.zeros(shape, np.uint8)
    for r, m in enumerate((nonocc, all, disc)):
        if m is not None:
            m = np.asarray(m)
            if m.shape != tuple(shape):
                raise ValueError("a region mask differs in shape from the maps")
            out |= ((m == 255).astype(np.uint8) << r).astype(np.uint8)
    return out


def eval_stage_host(DP, DT, region, thresholds=(1.0,)) -> StageErrors:
    """sm_eval_stage_host: the device's arithmetic for one map on the host -> records [3]."""
    dp = np.ascontiguousarray(DP, np.int16)
    dt = np.ascontiguousarray(DT, np.float32)
    rg = np.ascontiguousarray(region, np.uint8)
    if not (dp.shape == dt.shape == rg.shape) or dp.ndim != 2:
        raise ValueError("DP, DT and region must be H x W arrays of one shape")
    th = (C.c_float * len(thresholds))(*[float(t) for t in thresholds])
    out = np.zeros(3, _capi.STAGE_ERR_DTYPE)
    _capi.load().sm_eval_stage_host(_capi.ptr(dp), _capi.ptr(dt), _capi.ptr(rg), dp.shape[0], dp.shape[1], len(thresholds),
                                    th, _capi.ptr(out))
    return stage_errors_array(out, ())


def err_rows(table: StageErrors, present=(True, True, True), k: int = 0):
    """The err-txt rows of one pair's table [stages][3]: (procedure, region, PBM, RMS) per stage and present
    region, in calErr's order."""
    pbm, rms = table.pbm(k), table.rms()
    return [(name, REGIONS[r], float(pbm[s, r]), float(rms[s, r]))
            for s, name in enumerate(table.names) for r in range(3) if present[r]]


def format_err_lines(rows) -> list:
    """calErr's lines (h:1756, 1799, 1817): procedure, then `region\\tPBM: x\\tRMS: y\\t` per region, floats as an
    ostream prints them (%g)."""
    order = []
    for name, region, pbm, rms in rows:
        if not order or order[-1][0] != name or region in order[-1][1]:
            order.append((name, [], []))
        order[-1][1].append(region)
        order[-1][2].append(f"{region}\tPBM: {pbm:g}\tRMS: {rms:g}\t")
    return [name + "\t" + "".join(parts) for name, _, parts in order]
