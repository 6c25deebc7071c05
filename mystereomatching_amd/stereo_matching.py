"""Host-side mirror of the reference's ``class StereoMatching`` interface (stereoMatching.h:46-2738).

Same names, argument meaning and call order as ``main_.cpp`` uses them (main_.cpp:138-172):

    StereoMatching.costcalculation = "censusGrad"      # static selectors (h:51-53, main:15-17)
    param = StereoMatching.Parameters(maxDisp, h, w, lamCen, lamG, M, lamc, ts, csvName, disSc)
    sm = StereoMatching(I1_c, I2_c, I1, I2, DT, all_mask, nonocc_mask, disc_mask, param)
    sm.costCalculate()                                  # cost + CBCA (cpp:945-1021)
    SolveAll([sm], 1, 0.3)                              # cpp:2142-2208
    sm.dispOptimize()                                   # SGM + WTA (cpp:1046-1136)
    if StereoMatching.Do_refine: sm.refine()            # cpp:1138-1511 (main:165-166)
    disparity = sm.DP[0]                                # int16 H x W, -1 = invalid

All compute runs in libsm_hip.so on the GPU (no CPU fallback).  Errors are raised as
``SMError`` (the reference threw cv::Exception / called exit()).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _capi
from .evaluate import cal_err, err_rows, stage_errors_array


class StereoMatching:
    # static std::string selectors (h:51-54); process-global in the reference, read at ctor time here
    costcalculation: str = "censusGrad"
    aggregation: str = "CBCA"
    optimization: str = "sgm"
    object: str = ""

    # compile-time switches the hot path reads (h:57-83); like the reference's static consts they
    # are read when an object is constructed (set StereoMatching.Do_refine = True before it)
    Do_refine = False
    Do_LRConsis = True
    # `#define MY_GUIDE` (h:38, commented out in the shipped build): guideFilter's form, False =
    # cv::ximgproc::guidedFilter (cpp:4513), True = guideFilterCore_matlab (cpp:4509)
    MY_GUIDE = False
    # costCalculate's "FIF" branch calls FIF_Improve (cpp:1010-1012, `//FIF();` commented out):
    # True selects the plain form FIF (cpp:4541-4705) instead
    FIF_PLAIN = False
    # AWS()'s function-local constants (W_V_AWS, W_U_AWS cpp:5715; r_c h:1478), read with
    # aggregation = "AWS" (sm_aws_config)
    AWS_RADIUS_V, AWS_RADIUS_U, AWS_GAMMA_C = _capi.AWS_DEFAULTS
    # BF()'s literal Size(12, 12) (cpp:1038; height, width) and GFNL()'s literal variance threshold
    # (cpp:4470), read with aggregation = "BF" / "GFNL" (sm_bf_config, sm_gfnl_config)
    BF_KSIZE_V, BF_KSIZE_U = _capi.BF_DEFAULTS
    GFNL_VAR_THRESH = _capi.GFNL_VAR_THRESH
    Do_regionVote = True
    Do_properIpol = True
    Do_lastMedianBlur = True
    # three more of refine()'s stages (h:73-81; sm_refine_ext_config), off in the shipped build: the peak-ratio
    # check (calPKR + signDp_UsingPKR), the background fill (BGIpol) and the sub-pixel map (subpixelEnhancement +
    # its float median), which refine() leaves in self.SE.  SE_FLOAT keeps the float difference; False reproduces
    # the reference's `disp -= diff` on a short (cpp:6161)
    Do_calPKR = False
    Do_bgIpol = False
    Do_subpixelEnhancement = False
    SE_FLOAT = False
    PKR_RATIO = _capi.REFINE_EXT_DEFAULTS[0]   # calPKR's local ratio_PKR (cpp:4093)
    # refine()'s discontinuity adjustment (h:78; sm_refine_da_config), off in the shipped build: equalizeHist,
    # GaussianBlur and Canny on DP[0] as 8 bits, then the raster-order pass of cpp:6069-6135; refine() leaves the
    # edge map in self.DA_Edge.  DA_CANNY / DA_BLUR_TAPS are the literals of cpp:6063-6064 in the restated form
    Do_discontinuityAdjust = False
    DA_CANNY = _capi.REFINE_DA_DEFAULTS[:2]
    DA_BLUR_TAPS = _capi.REFINE_DA_DEFAULTS[2:]
    # two source switches of refine() (sm_refine_outlier_config), as commented out in the shipped build:
    # LRC_CLASSIFY = True runs LRConsistencyCheck (cpp:1367, 2284-2335: failed pixels become DISP_OCC / DISP_MIS and
    # refine() leaves the mask in self.LRC_Err_Mask) instead of LRConsistencyCheck_normal; RV_COMBINE_BG = True runs
    # RV_combine_BG (cpp:1408, 7146-7216: a float ratio, the filler chosen per class by Parameters.interpolateType)
    # instead of regionVote_my
    LRC_CLASSIFY = False
    RV_COMBINE_BG = False
    # which scan-line optimiser dispOptimize's "so" branch calls (cpp:1096-1100; sm_so_config): "so" (the shipped
    # call), "so_R2L" (cpp:6683-6826) or "so_T2D" (cpp:6580-6681, on a clone: vm[i] stays as aggregated); SO_PN
    # replaces the chosen function's Pn2 / Pn3 literals (None keeps them).  Read with optimization = "so"
    SO_VARIANT = "so"
    SO_PN = None
    # the reference's err txt (saveFromDisp -> calErr after dispOptimize and after refine()'s stages; sm_eval_config):
    # True (with DT given) builds the table on the GPU while dispOptimize and refine() run; stageErrors() returns
    # its rows.  Read when an object is constructed, like the switches above
    Do_stageErrors = False

    class Parameters:
        """StereoMatching::Parameters (h:85-351): the fields the hot path reads."""

        def __init__(self, maxDisp: int, h: int, w: int, lamCen: int = 13, lamG: int = 1, M: int = 2,
                     lamc: int = 109, ts: int = 10, errCsvName: str = "", disSc: int = 1):
            self.numDisparities = maxDisp + 1          # h:209
            self.W_U, self.W_V = 4, 3                  # h:206-207
            self.errorThreshold = 1                    # h:225
            self.census_channel = 1                    # h:229
            self.censusFunc = 3                        # h:244
            self.gradFuse_adpWgt = True                # h:245
            self.grad_use2direc = True                 # h:246
            self.cbca_minArmL = 1                      # h:259
            self.cbca_iterationNum = 2                 # h:260
            # h:262; False: the aggregation without arm intersection (sm_cbca_intersect_config), read when the
            # object is constructed and only by "CBCA"
            self.cbca_intersect = True
            self.cbca_crossL = [17, 23, 34]            # h:263-265
            self.cbca_crossL_out = [34, 23, 34]        # h:266-268
            self.cbca_cTresh = [20, 30, 30]            # h:269-271
            self.cbca_cTresh_out = [6, 0, 0]           # h:272-274
            # CBCA()'s double-window branch (h:144, 275; cpp:4337-4357; sm_cbca_double_config): window 1 is
            # index 1 of the four lists above; read when the object is constructed
            self.cbca_double_win = False
            # GF()'s switch (h:145, 276): both arms of the reference's branch run guideFilter(0, vm)
            # (cpp:4406-4418), so the field is accepted and changes nothing
            self.GF_double_win = False
            self.sgm_scanNum = 4                       # h:236 (the reference hard-codes 4, cpp:6214)
            self.sgm_P1, self.sgm_P2 = 1.0, 3.0        # ctor override for CBCA (cpp:2089-2091)
            self.sgm_corDifThres = 15                  # h:239
            self.sgm_reduCoeffi1 = 4                   # h:240
            self.lamCen, self.lamG = lamCen, lamG      # h:340-341
            self.ts, self.disSc = ts, disSc
            self.errCsvName = errCsvName
            self.vmTop_Num = M
            self.vmTop_thres = float(np.float32(lamc * 0.01))   # (float)(lamc_ * 0.01): double product (h:323)
            # dispOptimize's candidate-disparity selection (h:182-188, 320-326; sm_vmtop_config); read when
            # the object is constructed
            self.Do_vmTop = False
            self.vmTop_method = 0
            self.vmTop_thres_dirNum = 8                # carried; genDispFromTopCostVm2 does not read it
            self.vmTop_hasCir2 = True
            self.vmTop_cir3_doColorLimit = False
            self.rows, self.cols = h, w
            self.LRmaxDiff = 0.0                       # h:212
            self.DISP_OCC = -2 * 16                    # h:216
            self.DISP_MIS = -3 * 16                    # h:217
            self.DISP_PKR = -4 * 16                    # h:218
            self.interpolateType = 0                   # h:178, 310: RV_combine_BG's filler (RV_COMBINE_BG)
            self.bgIplDepth = 1000                     # h:311
            self.region_vote_nums = 2                  # h:306
            self.rv_ratio, self.rv_s = 0.4, 20         # refine(): rv_ratio[] / rv_s[] (cpp:1400-1401)

        def to_c(self, cost: str, aggregation: str, optimization: str, batch: int = 1,
                 compute_right_view: bool = False, keep_final_volume: bool = False,
                 do_refine: bool = False, switches=(True, True, True), my_guide: bool = False,
                 lr_consis: bool = True, fif_plain: bool = False) -> _capi.sm_params:
            if self.censusFunc not in (0, 3):
                raise ValueError("censusFunc must be 0 (plain census) or 3 (census + ring bits)")
            p = _capi.default_params(self.numDisparities - 1, self.rows, self.cols)
            p.cost_method = _capi.COST_METHODS[cost]
            p.aggregation = _capi.AGGREGATIONS[aggregation]
            p.optimization = _capi.OPTIMIZATIONS[optimization]
            p.census_ring = 1 if self.censusFunc == 3 else 0
            p.lam_cen, p.lam_g = float(self.lamCen), float(self.lamG)
            p.grad_adaptive = int(self.gradFuse_adpWgt)
            # calArms divides the arm limits by the level's scale (cpp:5367-5371)
            sc = self.disSc if self.disSc > 1 else 1
            p.arm_l, p.arm_l_out = int(self.cbca_crossL[0] / sc), int(self.cbca_crossL_out[0] / sc)
            p.arm_c_thresh, p.arm_c_thresh_out = self.cbca_cTresh[0], self.cbca_cTresh_out[0]
            p.arm_min_l = self.cbca_minArmL
            p.cbca_iterations = self.cbca_iterationNum
            p.sgm_paths = self.sgm_scanNum
            p.sgm_cor_dif_thres = self.sgm_corDifThres
            p.sgm_redu_coeff = self.sgm_reduCoeffi1
            p.batch_capacity = batch
            p.compute_right_view = int(compute_right_view)
            p.keep_final_volume = int(keep_final_volume)
            p.do_refine = int(do_refine)
            p.lr_max_diff = float(self.LRmaxDiff)
            p.disp_occ = int(self.DISP_OCC)
            p.region_vote_nums = int(self.region_vote_nums)
            p.rv_ratio, p.rv_s = float(self.rv_ratio), int(self.rv_s)
            p.do_region_vote, p.do_proper_ipol, p.do_last_median_blur = (int(x) for x in switches)
            p.gf_mode = 1 if my_guide else 0
            p.fif_mode = _capi.FIF_PLAIN if fif_plain else _capi.FIF_IMPROVE
            p.lr_consis = int(lr_consis)
            return p

        def cbca_double_args(self):
            """sm_cbca_double_config's arguments after `enable`: window 1 (calArms divides its arm limits by
            the level's scale too, cpp:5367-5371) and combine2Vm_4's armLthres = 5 (cpp:4297)."""
            sc = self.disSc if self.disSc > 1 else 1
            return (int(self.cbca_crossL[1] / sc), int(self.cbca_crossL_out[1] / sc), int(self.cbca_cTresh[1]),
                    int(self.cbca_cTresh_out[1]), _capi.CBCA_DW_DEFAULTS[4])

    def __init__(self, I1_c, I2_c, I1_g, I2_g, DT=None, all_mask=None, nonocc_mask=None, disc_mask=None,
                 param: Optional["StereoMatching.Parameters"] = None, device: int = 0,
                 keep_final_volume: bool = False, so_float_minima: Optional[bool] = None):
        """StereoMatching::StereoMatching (cpp:2058-2110).  Images: BGR u8 HxWx3, gray u8 HxW.

        so_float_minima: the scan-line optimisers' float-minima kernels (sm_create_ex).  None (default) is automatic:
        on where optimization "so" follows GF, GFNL or BF with inexact sums, which the reference runs without a
        switch; True / False force it."""
        I1_c, I2_c = np.ascontiguousarray(I1_c, np.uint8), np.ascontiguousarray(I2_c, np.uint8)
        I1_g, I2_g = np.ascontiguousarray(I1_g, np.uint8), np.ascontiguousarray(I2_g, np.uint8)
        h, w = I1_c.shape[:2]
        for im, nd in ((I1_c, 3), (I2_c, 3), (I1_g, 2), (I2_g, 2)):
            if im.ndim != nd or im.shape[:2] != (h, w) or (nd == 3 and im.shape[2] != 3):
                raise ValueError("images must be HxWx3 (colour) and HxW (gray) of one size")
        if param is None:
            raise ValueError("param is required")
        self.h_, self.w_ = h, w
        self.d_ = param.numDisparities
        self.param_ = param
        self.DT = DT
        self.I_mask = [nonocc_mask, all_mask, disc_mask]   # cpp:2073-2075
        self.I_c, self.I_g = [I1_c, I2_c], [I1_g, I2_g]
        self.DP: List[Optional[np.ndarray]] = [None, None]
        self._lib = _capi.load()
        if self.Do_refine and not self.Do_LRConsis:
            raise ValueError("Do_refine needs Do_LRConsis (refine() starts with the LR check, cpp:1364)")
        p = param.to_c(self.costcalculation, self.aggregation, self.optimization, my_guide=self.MY_GUIDE,
                       fif_plain=self.FIF_PLAIN,
                       compute_right_view=self.Do_LRConsis and self.Do_refine,
                       keep_final_volume=keep_final_volume, do_refine=self.Do_refine, lr_consis=self.Do_LRConsis,
                       switches=(self.Do_regionVote, self.Do_properIpol, self.Do_lastMedianBlur))
        self._refine_on = bool(self.Do_refine)
        # refine()'s volume-reading stages after "so" read vm[0] as so left it (the reference's so accumulates in
        # place): the context keeps it
        if self.optimization == "so" and self._refine_on and (self.Do_calPKR or self.Do_subpixelEnhancement or
                                                                self.Do_discontinuityAdjust):
            p.keep_final_volume = 1
        self._so_views2 = self.optimization == "so" and bool(self.Do_LRConsis)   # as passed to sm_create
        p.rows, p.cols = h, w
        ctx, st, entry = _capi.create(self._lib, p, device, so_float_minima)
        self._ctx = ctx
        _capi.check(self._lib, ctx, st, entry)
        if self.aggregation == "AWS":
            st = self._lib.sm_aws_config(ctx, int(self.AWS_RADIUS_V), int(self.AWS_RADIUS_U), float(self.AWS_GAMMA_C))
            _capi.check(self._lib, ctx, st, "sm_aws_config")
        if self.aggregation == "BF":
            st = self._lib.sm_bf_config(ctx, int(self.BF_KSIZE_V), int(self.BF_KSIZE_U))
            _capi.check(self._lib, ctx, st, "sm_bf_config")
        if self.aggregation == "GFNL":
            st = self._lib.sm_gfnl_config(ctx, float(self.GFNL_VAR_THRESH))
            _capi.check(self._lib, ctx, st, "sm_gfnl_config")
        if self.optimization == "so" and (self.SO_VARIANT != "so" or self.SO_PN is not None):
            if self.SO_VARIANT not in _capi.SO_VARIANTS:
                raise ValueError(f"SO_VARIANT must be one of {sorted(_capi.SO_VARIANTS)}")
            pn = (_capi.SO_PN_DEFAULT, _capi.SO_PN_DEFAULT) if self.SO_PN is None else self.SO_PN
            st = self._lib.sm_so_config(ctx, _capi.SO_VARIANTS[self.SO_VARIANT], float(pn[0]), float(pn[1]))
            _capi.check(self._lib, ctx, st, "sm_so_config")
        if param.Do_vmTop:
            st = self._lib.sm_vmtop_config(ctx, 1, int(param.vmTop_method), int(param.vmTop_Num), float(param.vmTop_thres),
                                           int(param.ts), int(param.vmTop_hasCir2), int(param.vmTop_cir3_doColorLimit))
            _capi.check(self._lib, ctx, st, "sm_vmtop_config")
        if param.cbca_double_win and self.aggregation == "CBCA":
            st = self._lib.sm_cbca_double_config(ctx, 1, *param.cbca_double_args())
            _capi.check(self._lib, ctx, st, "sm_cbca_double_config")
        if not param.cbca_intersect and self.aggregation == "CBCA":   # (only the CBCA functions read the field)
            st = self._lib.sm_cbca_intersect_config(ctx, 0)
            _capi.check(self._lib, ctx, st, "sm_cbca_intersect_config")
        self.SE: Optional[np.ndarray] = None            # refine()'s float map (Do_subpixelEnhancement)
        self.PKR_Err_Mask: Optional[np.ndarray] = None  # calPKR's mask (Do_calPKR)
        self._refine_ext = (bool(self.Do_calPKR), bool(self.Do_bgIpol), bool(self.Do_subpixelEnhancement))
        if self._refine_on and any(self._refine_ext):
            st = self._lib.sm_refine_ext_config(ctx, int(self.Do_calPKR), float(self.PKR_RATIO), int(param.DISP_PKR),
                                                int(self.Do_bgIpol), int(param.bgIplDepth), int(self.Do_subpixelEnhancement),
                                                _capi.SE_FLOAT if self.SE_FLOAT else _capi.SE_REFERENCE)
            _capi.check(self._lib, ctx, st, "sm_refine_ext_config")
        self.DA_Edge: Optional[np.ndarray] = None       # discontinuityAdjust's edge map (Do_discontinuityAdjust)
        self._refine_da = self._refine_on and bool(self.Do_discontinuityAdjust)
        if self._refine_da:
            st = self._lib.sm_refine_da_config(ctx, 1, int(self.DA_CANNY[0]), int(self.DA_CANNY[1]),
                                               int(self.DA_BLUR_TAPS[0]), int(self.DA_BLUR_TAPS[1]))
            _capi.check(self._lib, ctx, st, "sm_refine_da_config")
        self.LRC_Err_Mask: Optional[np.ndarray] = None  # LRConsistencyCheck's mask (LRC_CLASSIFY)
        self._outlier = (self._refine_on and bool(self.LRC_CLASSIFY), self._refine_on and bool(self.RV_COMBINE_BG))
        if any(self._outlier):
            st = self._lib.sm_refine_outlier_config(ctx, int(self._outlier[0]), int(param.DISP_MIS), int(self._outlier[1]),
                                                    int(param.interpolateType))
            _capi.check(self._lib, ctx, st, "sm_refine_outlier_config")
        self._stage_errors = bool(self.Do_stageErrors) and DT is not None
        if self._stage_errors:
            th = (C.c_float * 1)(float(param.errorThreshold))
            _capi.check(self._lib, ctx, self._lib.sm_eval_config(ctx, 1, 0, 1, th), "sm_eval_config")
            gt = np.ascontiguousarray(DT, np.float32)
            masks = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in self.I_mask]
            if gt.shape != (h, w) or any(m is not None and m.shape != (h, w) for m in masks):
                raise ValueError("DT and the masks must be HxW")
            st = self._lib.sm_upload_truth(ctx, 1, _capi.ptr(gt), *[None if m is None else _capi.ptr(m) for m in masks])
            _capi.check(self._lib, ctx, st, "sm_upload_truth")
        st = self._lib.sm_set_images(ctx, _capi.ptr(I1_c), _capi.ptr(I2_c), w * 3,
                                     _capi.ptr(I1_g), _capi.ptr(I2_g), w)
        _capi.check(self._lib, ctx, st, "sm_set_images")

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            self._lib.sm_destroy(ctx)
            self._ctx = None

    # -- pipeline stages ---------------------------------------------------------------
    def costCalculate(self):
        """Cost volume + aggregation (cpp:945-1021)."""
        _capi.check(self._lib, self._ctx, self._lib.sm_cost_calculate(self._ctx), "costCalculate")

    def dispOptimize(self):
        """SGM (or WTA only) -> DP[0], and DP[1] when Do_refine; "so" -> DP[0] and DP[1]
        (num = Do_LRConsis ? 2 : 1, cpp:1093) (cpp:1046-1136)."""
        dp = np.empty((self.h_, self.w_), np.int16)
        _capi.check(self._lib, self._ctx, self._lib.sm_disp_optimize(self._ctx, _capi.ptr(dp)), "dispOptimize")
        self.DP[0] = dp
        if self._refine_on or self._so_views2:
            d1 = np.empty((self.h_, self.w_), np.int16)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_disp(self._ctx, 1, _capi.ptr(d1)), "DP[1]")
            self.DP[1] = d1
        return dp

    def refine(self):
        """refine() (cpp:1138-1511): LR check against DP[1], [peak-ratio check,] region votes, proper
        interpolation, [background fill, discontinuity adjustment -> DA_Edge, sub-pixel map -> SE,] 3x3 median -> DP[0].  Needs Do_refine = True when
        the object was constructed."""
        dp = np.empty((self.h_, self.w_), np.int16)
        _capi.check(self._lib, self._ctx, self._lib.sm_refine(self._ctx, _capi.ptr(dp)), "refine")
        self.DP[0] = dp
        if self._refine_ext[0]:
            self.PKR_Err_Mask = np.empty((self.h_, self.w_), np.uint8)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_pkr_mask(self._ctx, _capi.ptr(self.PKR_Err_Mask)), "PKR_Err_Mask")
        if self._refine_ext[2]:
            self.SE = np.empty((self.h_, self.w_), np.float32)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_subpixel(self._ctx, _capi.ptr(self.SE)), "SE")
        if self._outlier[0]:
            self.LRC_Err_Mask = np.empty((self.h_, self.w_), np.uint8)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_lrc_mask(self._ctx, _capi.ptr(self.LRC_Err_Mask)), "LRC_Err_Mask")
        if self._refine_da:
            self.DA_Edge = np.empty((self.h_, self.w_), np.uint8)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_da_edges(self._ctx, _capi.ptr(self.DA_Edge)), "DA_Edge")
        return dp

    def pipeline(self):
        """pipeline() (cpp:1950-1981): costCalculate -> dispOptimize (no SolveAll)."""
        self.costCalculate()
        return self.dispOptimize()

    # -- state readback ------------------------------------------------------------------
    @property
    def vm(self) -> List[np.ndarray]:
        out = []
        for view in (0, 1):
            a = np.empty((self.h_, self.w_, self.d_), np.float32)
            st = self._lib.sm_get_volume(self._ctx, view, _capi.ptr(a))
            if st == _capi.SM_OK:
                out.append(a)
            elif view == 0:
                _capi.check(self._lib, self._ctx, st, "vm[0]")
        return out

    @property
    def HVL(self) -> List[np.ndarray]:
        out = []
        for view in (0, 1):
            a = np.empty((self.h_, self.w_, 4), np.uint16)
            _capi.check(self._lib, self._ctx, self._lib.sm_get_arms(self._ctx, view, _capi.ptr(a)), "HVL")
            out.append(a)
        return out

    def census_codes(self, view: int) -> np.ndarray:
        a = np.empty((self.h_, self.w_, 2), np.uint64)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_census(self._ctx, view, _capi.ptr(a)), "census")
        return a

    def calErr(self, DP=None, thres: Optional[float] = None):
        """bad-t ratio / RMS per mask region (h:1748-1825) -> {region: (PBM, RMS)}."""
        DP = self.DP[0] if DP is None else DP
        t = self.param_.errorThreshold if thres is None else thres
        res = {}
        for name, m in zip(("nonocc", "all", "disc"), self.I_mask):
            if m is not None and self.DT is not None:
                res[name] = cal_err(DP, self.DT, m, t)
        return res

    def stageErrors(self):
        """The err-txt rows of the last dispOptimize (+ refine): [(procedure, region, PBM, RMS)], one per stage at
        which the reference calls saveFromDisp<short, 0> and per region whose mask was given, against DT with
        errorThreshold (calErr, h:1748-1825).  Needs Do_stageErrors = True and DT when the object was constructed."""
        if not self._stage_errors:
            raise _capi.SMError(_capi.SM_ESTATE, "stageErrors needs StereoMatching.Do_stageErrors = True and DT at construction")
        return err_rows(_stage_table(self._lib, self._ctx, 1)[0], [m is not None for m in self.I_mask])

    stage_errors = stageErrors


def _stage_table(lib, ctx, n: int):
    """sm_get_stage_errors as a StageErrors array [n][stages][3] with the stages' names."""
    S = int(lib.sm_eval_stage_count(ctx))
    raw = np.zeros((n, max(S, 1), 3), _capi.STAGE_ERR_DTYPE)
    _capi.check(lib, ctx, lib.sm_get_stage_errors(ctx, n, _capi.ptr(raw)), "stage_errors")
    return stage_errors_array(raw, [lib.sm_eval_stage_name(ctx, i).decode() for i in range(S)])


def SolveAll(smPyr: Sequence[StereoMatching], PY_LVL: int, REG_LAMBDA: float):
    """SolveAll (cpp:2142-2208).  PY_LVL = 1 (main_.cpp:131) scales vm; PY_LVL in [2, 8] combines
    the pyramid levels smPyr[0..PY_LVL-1] (built with pyrDown, main_.cpp:134-156) into smPyr[0]."""
    sm = smPyr[0]
    if int(PY_LVL) == 1:
        st = sm._lib.sm_solve_all(sm._ctx, 1, float(REG_LAMBDA))
    else:
        arr = (C.c_void_p * int(PY_LVL))(*[s._ctx.value for s in smPyr[:int(PY_LVL)]])
        st = sm._lib.sm_solve_all_pyr(arr, int(PY_LVL), float(REG_LAMBDA))
    _capi.check(sm._lib, sm._ctx, st, "SolveAll")


def pyrDown(img, device: int = 0) -> np.ndarray:
    """cv::pyrDown (main_.cpp:145-154), on the GPU: u8 H x W or H x W x 3 images (the inputs and
    masks) or a float32 H x W image (the ground truth DT, main_.cpp:149)."""
    lib = _capi.load()
    if np.asarray(img).dtype == np.float32:
        a = np.ascontiguousarray(img, np.float32)
        if a.ndim != 2:
            raise ValueError("float pyrDown takes a 1-channel image")
        rows, cols = a.shape
        out = np.empty(((rows + 1) // 2, (cols + 1) // 2), np.float32)
        st = lib.sm_pyr_down_f32(device, _capi.ptr(a), rows, cols, _capi.ptr(out))
        _capi.check(lib, None, st, "pyrDown")
        return out
    a = np.ascontiguousarray(img, np.uint8)
    rows, cols = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    out = np.empty(((rows + 1) // 2, (cols + 1) // 2) + a.shape[2:], np.uint8)
    st = lib.sm_pyr_down(device, _capi.ptr(a), rows, cols, ch, _capi.ptr(out))
    _capi.check(lib, None, st, "pyrDown")
    return out


def _is_device_tensor(a) -> bool:
    return type(a).__module__.startswith("torch") and getattr(a, "is_cuda", False)


def _to_numpy(a):
    return a.numpy() if type(a).__module__.startswith("torch") else a


class StereoBatch:
    """n independent pairs of one size through the whole main_.cpp sequence in one set of launches."""

    def __init__(self, max_disp: int, rows: int, cols: int, batch: int, device: int = 0, **overrides):
        self._lib = _capi.load()
        overrides.setdefault("batch_capacity", batch)
        # "AWS"'s constants are not sm_params fields (sm_aws_config): aws_radius_v / _u, aws_gamma_c
        aws = [overrides.pop(k, d) for k, d in zip(("aws_radius_v", "aws_radius_u", "aws_gamma_c"), _capi.AWS_DEFAULTS)]
        # likewise "BF"'s window (sm_bf_config) and "GFNL"'s threshold (sm_gfnl_config)
        bf = [overrides.pop(k, d) for k, d in zip(("bf_ksize_v", "bf_ksize_u"), _capi.BF_DEFAULTS)]
        gfnl_thresh = overrides.pop("gfnl_var_thresh", _capi.GFNL_VAR_THRESH)
        # CBCA's double window (sm_cbca_double_config): cbca_double_win switches it on, cbca_double_args are
        # window 1's arm settings and the arm-length threshold (DistributedBatchRunner's compute function hands
        # both through with its other overrides)
        dw_on = bool(overrides.pop("cbca_double_win", False))
        dw_args = tuple(overrides.pop("cbca_double_args", _capi.CBCA_DW_DEFAULTS))
        # CBCA without arm intersection (sm_cbca_intersect_config): cbca_intersect=False switches to it
        intersect = bool(overrides.pop("cbca_intersect", True))
        # refine()'s extra stages (sm_refine_ext_config): refine_ext is a dict of refine_ext_config's arguments
        refine_ext = overrides.pop("refine_ext", None)
        # refine()'s discontinuity adjustment (sm_refine_da_config): refine_da is a dict of refine_da_config's arguments
        refine_da = overrides.pop("refine_da", None)
        # refine()'s outlier classification (sm_refine_outlier_config): refine_outlier is a dict of
        # refine_outlier_config's arguments
        refine_outlier = overrides.pop("refine_outlier", None)
        # the per-stage error table (sm_eval_config): eval is a dict of eval_config's arguments
        eval_cfg = overrides.pop("eval", None)
        # the scan-line optimiser behind optimization "so" (sm_so_config): so_variant is the reference's function
        # name, so_pn = (pn2, pn3) replaces its penalty literals
        so_variant = overrides.pop("so_variant", "so")
        so_pn = overrides.pop("so_pn", None)
        if so_variant not in _capi.SO_VARIANTS:
            raise ValueError(f"so_variant must be one of {sorted(_capi.SO_VARIANTS)}")
        # the cross-scale pyramid inside run() (sm_pyramid_config): py_lvl = PY_LEV of main_.cpp:131, applied last
        py_lvl = int(overrides.pop("py_lvl", 1))
        # the scan-line optimisers' float-minima kernels (sm_create_ex): None is automatic (on where "so" follows GF,
        # GFNL or BF with inexact sums, as the reference runs them), True / False force it
        so_float_minima = overrides.pop("so_float_minima", None)
        p = _capi.default_params(max_disp, rows, cols, **overrides)
        # refine()'s volume-reading stages after "so" read vm[0] as so left it: the context keeps it
        reads = bool(refine_ext and (dict(refine_ext).get("do_pkr") or dict(refine_ext).get("do_subpixel"))) or \
            bool(refine_da and dict(refine_da).get("on", True))
        if p.optimization == _capi.OPTIMIZATIONS["so"] and p.do_refine and reads:
            p.keep_final_volume = 1
        self.params = p
        self.shape = (rows, cols, p.num_disparities)
        ctx, st, entry = _capi.create(self._lib, p, device, so_float_minima)
        self._ctx = ctx
        _capi.check(self._lib, ctx, st, entry)
        if tuple(aws) != _capi.AWS_DEFAULTS:
            self.aws_config(*aws)
        if tuple(bf) != _capi.BF_DEFAULTS:
            self.bf_config(*bf)
        if gfnl_thresh != _capi.GFNL_VAR_THRESH:
            self.gfnl_config(gfnl_thresh)
        if dw_on:
            self.cbca_double_config(True, *dw_args)
        if not intersect:
            self.cbca_intersect_config(False)
        if so_variant != "so" or so_pn is not None:
            self.so_config(so_variant, so_pn)
        if refine_ext:
            self.refine_ext_config(**dict(refine_ext))
        if refine_da:
            self.refine_da_config(**dict(refine_da))
        if refine_outlier:
            self.refine_outlier_config(**dict(refine_outlier))
        if py_lvl != 1:
            self.pyramid_config(py_lvl)
        if eval_cfg:
            self.eval_config(**dict(eval_cfg))
        self.n = 0
        self._async_out = []   # buffers of download_async copies still in flight

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.sm_destroy(self._ctx)   # (waits for the context's streams)
            self._ctx = None
        getattr(self, "_async_out", []).clear()

    def __del__(self):
        self.close()

    def upload(self, lbgr, rbgr, lgray, rgray):
        """Stacked numpy arrays (host) or uint8 torch tensors already on the GPU (copied
        device-to-device; the caller's stream is synchronized first)."""
        if all(_is_device_tensor(a) for a in (lbgr, rbgr, lgray, rgray)):
            import torch
            ts = [a.contiguous() for a in (lbgr, rbgr, lgray, rgray)]
            if any(t.dtype != torch.uint8 for t in ts):
                raise TypeError("device images must be uint8 tensors")
            torch.cuda.current_stream(ts[0].device).synchronize()
            ptrs = [C.c_void_p(t.data_ptr()) for t in ts]
            n = ts[0].shape[0]
        else:
            arrs = [np.ascontiguousarray(_to_numpy(a), np.uint8) for a in (lbgr, rbgr, lgray, rgray)]
            ptrs = [_capi.ptr(a) for a in arrs]
            n = arrs[0].shape[0]
        st = self._lib.sm_upload_batch(self._ctx, n, *ptrs)
        _capi.check(self._lib, self._ctx, st, "sm_upload_batch")
        self.n = n

    def upload_async(self, lbgr, rbgr, lgray, rgray):
        """sm_upload_batch_async: contiguous uint8 device tensors (or page-locked host tensors)
        copied in behind the previous pipelined call's groups, without a join or a host wait.
        The sources must stay unchanged until upload_wait() returns."""
        ts = [a.contiguous() for a in (lbgr, rbgr, lgray, rgray)]
        import torch
        if any(t.dtype != torch.uint8 for t in ts):
            raise TypeError("images must be uint8 tensors")
        if any(t.data_ptr() != a.data_ptr() for t, a in zip(ts, (lbgr, rbgr, lgray, rgray))):
            raise ValueError("upload_async needs contiguous tensors (a copy would be freed before the upload)")
        n = ts[2].shape[0]
        if tuple(ts[2].shape[1:]) != self.shape[:2] or tuple(ts[0].shape[1:]) != self.shape[:2] + (3,):
            raise ValueError("upload_async: image shape differs from the context's")
        st = self._lib.sm_upload_batch_async(self._ctx, n, *[C.c_void_p(t.data_ptr()) for t in ts])
        _capi.check(self._lib, self._ctx, st, "sm_upload_batch_async")
        self.n = n

    def upload_wait(self):
        _capi.check(self._lib, self._ctx, self._lib.sm_upload_wait(self._ctx), "upload_wait")

    def download_wait(self, back: int = 0):
        """Host wait for the copies of the last (back 0) or previous (back 1) download_async."""
        _capi.check(self._lib, self._ctx, self._lib.sm_download_wait(self._ctx, int(back)), "download_wait")
        # (buffers of copies known done are released; the later one may still be in flight)
        del self._async_out[:max(0, len(self._async_out) - int(back))]

    def run(self, reg_lambda: float = 0.3, download: bool = True) -> Optional[np.ndarray]:
        out = np.empty((self.n, self.shape[0], self.shape[1]), np.int16) if download else None
        st = self._lib.sm_run(self._ctx, self.n, float(reg_lambda), _capi.ptr(out) if download else None)
        _capi.check(self._lib, self._ctx, st, "sm_run")
        return out

    def _map_dst(self, out, what: str):
        """C pointer of `out` after checking it can take the n int16 maps: a C-contiguous int16
        numpy array or torch tensor (host or device) of at least n*H*W elements."""
        need = self.n * self.shape[0] * self.shape[1]
        if type(out).__module__.startswith("torch"):
            import torch
            if out.dtype != torch.int16 or not out.is_contiguous() or out.numel() < need:
                raise ValueError(f"{what}: out must be a contiguous int16 tensor of at least n*H*W = {need} elements")
            return C.c_void_p(out.data_ptr())
        if not isinstance(out, np.ndarray) or out.dtype != np.int16 or not out.flags["C_CONTIGUOUS"] \
                or out.size < need:
            raise ValueError(f"{what}: out must be a C-contiguous int16 array of at least n*H*W = {need} elements")
        return _capi.ptr(out)

    def download(self, out=None):
        """The n int16 maps into a new numpy array, or into `out` (numpy, or an int16 torch
        tensor on the GPU: device-to-device copy)."""
        if out is None:
            out = np.empty((self.n, self.shape[0], self.shape[1]), np.int16)
        dst = self._map_dst(out, "download")
        _capi.check(self._lib, self._ctx, self._lib.sm_download_disp(self._ctx, self.n, dst), "download")
        return out

    def get_disp(self, view: int = 0) -> np.ndarray:
        """DP[view] of the first pair (sm_get_disp): DP[1] exists with do_refine or optimization "so"."""
        out = np.empty((self.shape[0], self.shape[1]), np.int16)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_disp(self._ctx, view, _capi.ptr(out)), "get_disp")
        return out

    def download_async(self, out):
        """sm_download_disp_async: the n maps into `out` (page-locked host memory, e.g. a
        pin_memory torch tensor's numpy view, or device memory) on the copy stream; complete after
        synchronize().  The next run's map-writing kernels wait for the copy.  `out` is checked like
        download()'s and kept referenced until synchronize() or close(), so the copy never writes
        into a freed buffer."""
        dst = self._map_dst(out, "download_async")
        _capi.check(self._lib, self._ctx, self._lib.sm_download_disp_async(self._ctx, self.n, dst), "download_async")
        self._async_out.append(out)
        return out

    def copy_ceiling(self, nbytes: int, reps: int = 5):
        """sm_copy_ceiling: (best, median) GB/s of a dwordx4 device copy of nbytes (read + write)."""
        best, med = C.c_double(), C.c_double()
        st = self._lib.sm_copy_ceiling(self._ctx, int(nbytes), int(reps), C.byref(best), C.byref(med))
        _capi.check(self._lib, self._ctx, st, "copy_ceiling")
        return best.value, med.value

    def aws_config(self, radius_v: int = 17, radius_u: int = 17, gamma_c: float = 5.0):
        """sm_aws_config: "AWS"'s window radii (each in [0, 17]) and gamma_c, from the next run on."""
        st = self._lib.sm_aws_config(self._ctx, int(radius_v), int(radius_u), float(gamma_c))
        _capi.check(self._lib, self._ctx, st, "aws_config")

    def bf_config(self, ksize_v: int = 12, ksize_u: int = 12):
        """sm_bf_config: "BF"'s window height and width (each in [1, 32]), from the next run on."""
        st = self._lib.sm_bf_config(self._ctx, int(ksize_v), int(ksize_u))
        _capi.check(self._lib, self._ctx, st, "bf_config")

    def gfnl_config(self, var_thresh: float = 400.0):
        """sm_gfnl_config: "GFNL"'s variance threshold (any finite value), from the next run on."""
        st = self._lib.sm_gfnl_config(self._ctx, float(var_thresh))
        _capi.check(self._lib, self._ctx, st, "gfnl_config")

    def cbca_double_config(self, enable: bool = True, arm_l2: int = 23, arm_l_out2: int = 23, arm_c_thresh2: int = 30,
                           arm_c_thresh_out2: int = 0, arm_len_thres: float = 5.0):
        """sm_cbca_double_config: CBCA()'s double-window branch (two aggregations, fused per pixel by the
        left image's window-0 arm lengths), from the next run on."""
        st = self._lib.sm_cbca_double_config(self._ctx, int(bool(enable)), int(arm_l2), int(arm_l_out2),
                                             int(arm_c_thresh2), int(arm_c_thresh_out2), float(arm_len_thres))
        _capi.check(self._lib, self._ctx, st, "cbca_double_config")

    def get_cbca_dw_mask(self) -> np.ndarray:
        """sm_get_cbca_dw_mask: the first pair's arm_Mask [H][W] of the last run with the double window on."""
        out = np.empty(self.shape[:2], np.uint8)
        st = self._lib.sm_get_cbca_dw_mask(self._ctx, _capi.ptr(out))
        _capi.check(self._lib, self._ctx, st, "get_cbca_dw_mask")
        return out

    def cbca_intersect_config(self, intersect: bool = True):
        """sm_cbca_intersect_config: False runs "CBCA" without arm intersection (the view's own arms, one area
        per pixel), from the next run on."""
        st = self._lib.sm_cbca_intersect_config(self._ctx, int(bool(intersect)))
        _capi.check(self._lib, self._ctx, st, "cbca_intersect_config")

    def get_cbca_area(self, view: int = 0) -> np.ndarray:
        """sm_get_cbca_area: the first pair's support areas [H][W] (int32) of the last run without arm
        intersection."""
        out = np.empty(self.shape[:2], np.int32)
        st = self._lib.sm_get_cbca_area(self._ctx, int(view), _capi.ptr(out))
        _capi.check(self._lib, self._ctx, st, "get_cbca_area")
        return out

    def pyramid_config(self, py_lvl: int = 1):
        """sm_pyramid_config: run() builds py_lvl pyramid levels per pair (pyrDown'ed inputs, halved disparity range
        and arm limits) and SolveAll combines them into level 0 before the optimiser; 1 = no pyramid."""
        _capi.check(self._lib, self._ctx, self._lib.sm_pyramid_config(self._ctx, int(py_lvl)), "pyramid_config")

    @property
    def pyramid_levels(self) -> int:
        return int(self._lib.sm_pyramid_levels(self._ctx))

    def _pyramid_level(self, level: int):
        """(borrowed context, (rows, cols, num_disparities)) of pyramid level `level`, after synchronize()."""
        ctx = self._lib.sm_pyramid_level(self._ctx, int(level))
        if not ctx:
            raise ValueError(f"pyramid level {level} out of range (py_lvl = {self.pyramid_levels})")
        self.synchronize()
        h, w, d = self.shape
        for _ in range(int(level)):
            h, w, d = (h + 1) // 2, (w + 1) // 2, (d - 1) // 2 + 2
        return C.c_void_p(ctx), (h, w, d)

    def pyramid_level_volume(self, level: int, view: int = 0) -> np.ndarray:
        """The first pair's vm[view] of pyramid level `level` after the last run (level 0: the combined volume)."""
        ctx, (h, w, d) = self._pyramid_level(level)
        out = np.empty((h, w, d), np.float32)
        _capi.check(self._lib, ctx, self._lib.sm_get_volume(ctx, int(view), _capi.ptr(out)), "pyramid_level_volume")
        return out

    def pyramid_level_arms(self, level: int, view: int = 0) -> np.ndarray:
        """The first pair's arms HVL[view] [H_s][W_s][4] of pyramid level `level` after the last run."""
        ctx, (h, w, _) = self._pyramid_level(level)
        out = np.empty((h, w, 4), np.uint16)
        _capi.check(self._lib, ctx, self._lib.sm_get_arms(ctx, int(view), _capi.ptr(out)), "pyramid_level_arms")
        return out

    def pyramid_level_census(self, level: int, view: int = 0) -> np.ndarray:
        """The first pair's census codes [H_s][W_s][2] (uint64) of pyramid level `level` after the last run."""
        ctx, (h, w, _) = self._pyramid_level(level)
        out = np.empty((h, w, 2), np.uint64)
        _capi.check(self._lib, ctx, self._lib.sm_get_census(ctx, int(view), _capi.ptr(out)), "pyramid_level_census")
        return out

    def refine_ext_config(self, do_pkr: bool = False, pkr_ratio: float = _capi.REFINE_EXT_DEFAULTS[0],
                          disp_pkr: int = _capi.REFINE_EXT_DEFAULTS[1], do_bg_ipol: bool = False,
                          bg_ipl_depth: int = _capi.REFINE_EXT_DEFAULTS[2], do_subpixel: bool = False,
                          se_mode: int = _capi.REFINE_EXT_DEFAULTS[3]):
        """sm_refine_ext_config: refine()'s peak-ratio check, background fill and sub-pixel map (all off by
        default), from the next run on; needs do_refine = 1 and, for do_pkr / do_subpixel with optimization "so",
        keep_final_volume = 1 (the constructor's refine_ext sets it)."""
        st = self._lib.sm_refine_ext_config(self._ctx, int(bool(do_pkr)), float(pkr_ratio), int(disp_pkr),
                                            int(bool(do_bg_ipol)), int(bg_ipl_depth), int(bool(do_subpixel)), int(se_mode))
        _capi.check(self._lib, self._ctx, st, "refine_ext_config")

    def refine_da_config(self, on: bool = True, canny_low: int = _capi.REFINE_DA_DEFAULTS[0],
                         canny_high: int = _capi.REFINE_DA_DEFAULTS[1], blur_side: int = _capi.REFINE_DA_DEFAULTS[2],
                         blur_centre: int = _capi.REFINE_DA_DEFAULTS[3]):
        """sm_refine_da_config: refine()'s discontinuity adjustment (off by default), from the next run on; needs
        do_refine = 1 and, with optimization "so", keep_final_volume = 1 (the constructor's refine_da sets it)."""
        st = self._lib.sm_refine_da_config(self._ctx, int(bool(on)), int(canny_low), int(canny_high), int(blur_side),
                                           int(blur_centre))
        _capi.check(self._lib, self._ctx, st, "refine_da_config")

    def get_da_edges(self) -> np.ndarray:
        """sm_get_da_edges: the first pair's edge map [H][W] (0 / 255) of the last run with the adjustment on."""
        out = np.empty(self.shape[:2], np.uint8)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_da_edges(self._ctx, _capi.ptr(out)), "get_da_edges")
        return out

    def so_config(self, variant: str = "so", pn=None):
        """sm_so_config: the scan-line optimiser that optimization "so" runs from the next run on — "so", "so_R2L"
        or "so_T2D" (the reference's function names) — and, with pn = (pn2, pn3), its penalties instead of the
        function's literals."""
        if variant not in _capi.SO_VARIANTS:
            raise ValueError(f"variant must be one of {sorted(_capi.SO_VARIANTS)}")
        pn2, pn3 = (_capi.SO_PN_DEFAULT, _capi.SO_PN_DEFAULT) if pn is None else pn
        st = self._lib.sm_so_config(self._ctx, _capi.SO_VARIANTS[variant], float(pn2), float(pn3))
        _capi.check(self._lib, self._ctx, st, "so_config")

    def refine_outlier_config(self, classify: bool = False, disp_mis: int = _capi.REFINE_OUTLIER_DEFAULTS[0],
                              rv_combine: bool = False, interpolate_type: int = _capi.REFINE_OUTLIER_DEFAULTS[1]):
        """sm_refine_outlier_config: refine()'s classifying LR check (DISP_OCC / DISP_MIS labels and LRC_Err_Mask)
        and RV_combine_BG in the region-vote rounds (both off by default), from the next run on; needs
        do_refine = 1."""
        st = self._lib.sm_refine_outlier_config(self._ctx, int(bool(classify)), int(disp_mis), int(bool(rv_combine)),
                                                int(interpolate_type))
        _capi.check(self._lib, self._ctx, st, "refine_outlier_config")

    def get_lrc_mask(self) -> np.ndarray:
        """sm_get_lrc_mask: the first pair's LRC_Err_Mask [H][W] (0 / 255) of the last run with classify on."""
        out = np.empty(self.shape[:2], np.uint8)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_lrc_mask(self._ctx, _capi.ptr(out)), "get_lrc_mask")
        return out

    def eval_config(self, on: bool = True, keep_maps: bool = False, thresholds=(1.0,)):
        """sm_eval_config: the reference's error table (calErr over nonocc / all / disc at every stage where it calls
        saveFromDisp) built on the GPU inside run(), against upload_truth's data; up to four thresholds; keep_maps
        also keeps every stage's maps (stage_maps).  Off by default."""
        th = (C.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
        st = self._lib.sm_eval_config(self._ctx, int(bool(on)), int(bool(keep_maps)), len(thresholds), th)
        _capi.check(self._lib, self._ctx, st, "eval_config")

    def upload_truth(self, gt, nonocc=None, all=None, disc=None):
        """sm_upload_truth: ground truth [n][H][W] float32 and the region masks [n][H][W] uint8 (255 = inside;
        None = region absent) of the uploaded pairs; stays until the next call."""
        g = np.ascontiguousarray(_to_numpy(gt), np.float32)
        if g.ndim != 3 or g.shape[1:] != self.shape[:2]:
            raise ValueError("upload_truth: gt must be [n][H][W]")
        ms = [None if m is None else np.ascontiguousarray(_to_numpy(m), np.uint8) for m in (nonocc, all, disc)]
        if any(m is not None and m.shape != g.shape for m in ms):
            raise ValueError("upload_truth: every mask must have gt's shape")
        st = self._lib.sm_upload_truth(self._ctx, g.shape[0], _capi.ptr(g), *[None if m is None else _capi.ptr(m) for m in ms])
        _capi.check(self._lib, self._ctx, st, "upload_truth")

    def stage_names(self):
        """The stages of the last run's table (before any run: what the next run would record)."""
        return [self._lib.sm_eval_stage_name(self._ctx, i).decode() for i in range(self._lib.sm_eval_stage_count(self._ctx))]

    def stage_errors(self):
        """sm_get_stage_errors: the last run's table, a structured array [n][stages][3] (count, invalid, bad[4],
        sum_sq) with .names, .pbm(k) and .rms()."""
        return _stage_table(self._lib, self._ctx, self.n)

    def stage_maps(self, stage: int) -> np.ndarray:
        """sm_get_stage_maps: the n maps [n][H][W] as they were at `stage` (eval_config with keep_maps)."""
        out = np.empty((self.n, self.shape[0], self.shape[1]), np.int16)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_stage_maps(self._ctx, self.n, int(stage), _capi.ptr(out)), "stage_maps")
        return out

    def get_pkr_mask(self) -> np.ndarray:
        """sm_get_pkr_mask: the first pair's PKR_Err_Mask [H][W] of the last run with do_pkr on."""
        out = np.empty(self.shape[:2], np.uint8)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_pkr_mask(self._ctx, _capi.ptr(out)), "get_pkr_mask")
        return out

    def download_subpixel(self, out=None):
        """sm_download_subpixel: the n float maps SE [n][H][W] of the last run with do_subpixel on, into a new
        numpy array or into `out` (a C-contiguous float32 numpy array, or a float32 torch tensor on the GPU)."""
        need = self.n * self.shape[0] * self.shape[1]
        if out is None:
            out = np.empty((self.n, self.shape[0], self.shape[1]), np.float32)
        if type(out).__module__.startswith("torch"):
            import torch
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < need:
                raise ValueError(f"download_subpixel: out must be a contiguous float32 tensor of at least {need} elements")
            dst = C.c_void_p(out.data_ptr())
        else:
            if not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"] or out.size < need:
                raise ValueError(f"download_subpixel: out must be a C-contiguous float32 array of at least {need} elements")
            dst = _capi.ptr(out)
        _capi.check(self._lib, self._ctx, self._lib.sm_download_subpixel(self._ctx, self.n, dst), "download_subpixel")
        return out

    def vmtop_config(self, enable: bool = True, method: int = 0, num: int = 2, thres: float = 1.09, ts: int = 10,
                     has_cir2: bool = True, cir3_color_limit: bool = False):
        """sm_vmtop_config: dispOptimize's Do_vmTop branch (candidate-disparity selection instead of the
        plain WTA after "sgm" / ""), from the next run on; num in [1, 8], method 0, 1 or 2."""
        st = self._lib.sm_vmtop_config(self._ctx, int(bool(enable)), int(method), int(num), float(thres), int(ts),
                                       int(bool(has_cir2)), int(bool(cir3_color_limit)))
        _capi.check(self._lib, self._ctx, st, "vmtop_config")
        self._vmtop_num = int(num)

    def get_top_disp(self, view: int = 0) -> np.ndarray:
        """sm_get_top_disp: the first pair's candidate table [H][W][num + 1][2] of the last run with vmTop on
        (num as given to vmtop_config)."""
        out = np.empty((self.shape[0], self.shape[1], getattr(self, "_vmtop_num", 2) + 1, 2), np.float32)
        _capi.check(self._lib, self._ctx, self._lib.sm_get_top_disp(self._ctx, view, _capi.ptr(out)), "get_top_disp")
        return out

    def set_schedule(self, num_streams: int = 0, sub_batch: int = 0):
        """sm_set_schedule: num_streams / sub_batch for the following runs on the same allocations
        (0 / 0 = the auto default); maps are identical under every schedule."""
        st = self._lib.sm_set_schedule(self._ctx, int(num_streams), int(sub_batch))
        _capi.check(self._lib, self._ctx, st, "set_schedule")
        self.params.num_streams, self.params.sub_batch = int(num_streams), int(sub_batch)

    def placement(self):
        """The first run's volume placement trials (sm_params.placement_trials): (pipeline ms of
        each candidate set, index of the set kept), or ([], -1) when none ran."""
        buf = (C.c_double * 8)()
        nt = self._lib.sm_placement_trials_ms(self._ctx, buf, 8)
        return [round(buf[i], 3) for i in range(max(0, min(nt, 8)))], int(self._lib.sm_placement_kept(self._ctx))

    def synchronize(self):
        _capi.check(self._lib, self._ctx, self._lib.sm_synchronize(self._ctx), "sync")
        self._async_out.clear()

    def profile(self, on: bool = True):
        self._lib.sm_profile_enable(self._ctx, int(on))

    def profile_reset(self):
        self._lib.sm_profile_reset(self._ctx)

    def profile_read(self):
        names = C.create_string_buffer(64 * 48)
        launches = (C.c_int64 * 64)()
        total = (C.c_double * 64)()
        byts = (C.c_double * 64)()
        cnt = C.c_int32()
        st = self._lib.sm_profile_read(self._ctx, 64, names, launches, total, byts, C.byref(cnt))
        _capi.check(self._lib, self._ctx, st, "profile_read")
        out = {}
        for i in range(min(cnt.value, 64)):
            nm = names.raw[i * 48:(i + 1) * 48].split(b"\0", 1)[0].decode()
            out[nm] = {"launches": launches[i], "total_ms": total[i], "bytes_per_launch": byts[i]}
        return out


def run_batch_multi(batches: Sequence[StereoBatch], lbgr, rbgr, lgray, rgray, reg_lambda: float = 0.3) -> np.ndarray:
    """sm_run_batch_multi: n host pairs split into contiguous blocks over the contexts of
    `batches` (one per GPU, or several on one), one host thread per context; returns [n,H,W] int16."""
    lib = _capi.load()
    arrs = [np.ascontiguousarray(_to_numpy(a), np.uint8) for a in (lbgr, rbgr, lgray, rgray)]
    n, H, W = arrs[2].shape
    out = np.empty((n, H, W), np.int16)
    ctxs = (C.c_void_p * len(batches))(*[b._ctx.value for b in batches])
    st = lib.sm_run_batch_multi(ctxs, len(batches), n, *[_capi.ptr(a) for a in arrs], float(reg_lambda), _capi.ptr(out))
    _capi.check(lib, batches[0]._ctx, st, "sm_run_batch_multi")
    for b in batches:
        b.n = 0   # each context now holds only its own block
    return out
