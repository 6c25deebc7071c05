/*
 * sm_capi.h — C-ABI of the MI355X stereo-matching back end (libsm_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path: the calls that
 * main_.cpp makes on class StereoMatching (reference main_.cpp:138-172) map one-to-one onto the
 * entry points below.  Plain pointers and sizes only; no exceptions, no exit(), no globals:
 * every call returns an sm_status and sm_last_error(ctx) holds the message.
 *
 * Reference interface each entry point replaces (paths relative to the reference root):
 *   sm_params_default  <- StereoMatching::Parameters::Parameters     stereoMatching.h:204-350
 *   sm_create          <- StereoMatching::StereoMatching (ctor)      stereoMatching.cpp:2058-2110
 *   sm_set_images      <- ctor image arguments I1_c,I2_c,I1_g,I2_g   stereoMatching.cpp:2063-2071
 *   sm_cost_calculate  <- StereoMatching::costCalculate              stereoMatching.cpp:945-1021
 *                         (aggregators: cbca cpp:5585-5666, guideFilter cpp:4492-4516, NL cpp:4892-4917,
 *                          FIF_Improve cpp:4707-4890 and its plain form FIF cpp:4541-4705,
 *                          AWS cpp:5692-5801 without JBF_STANDARD, h:1305-1350, 1472-1493, 1533-1548)
 *                          BF cpp:1023-1043, GFNL cpp:4421-4490)
 *   sm_aws_config      <- AWS()'s local constants W_V_AWS, W_U_AWS (cpp:5715) and r_c (h:1478)
 *   sm_bf_config       <- BF()'s literal Size(12, 12) (cpp:1038)
 *   sm_gfnl_config     <- GFNL()'s literal variance threshold 400 (cpp:4470)
 *   sm_get_gfnl_mask   <- member arm_Mask as GFNL() leaves it (cpp:4460, 4472)
 *   sm_solve_all       <- SolveAll(StereoMatching**&, PY_LVL, REG_LAMBDA)  stereoMatching.cpp:2142-2208
 *   sm_solve_all_pyr   <- the same with PY_LVL > 1 (one ctx per level)     stereoMatching.cpp:2142-2208
 *   sm_pyr_down        <- cv::pyrDown on the inputs                     main_.cpp:145-148
 *   sm_cal_err         <- StereoMatching::calErr (one region)          stereoMatching.h:1748-1825
 *   sm_disp_optimize   <- StereoMatching::dispOptimize + DP[0]       stereoMatching.cpp:1046-1136, h:2724
 *   sm_refine          <- StereoMatching::refine (Do_refine)         stereoMatching.cpp:1138-1511, main_.cpp:165-166
 *   sm_get_disp / sm_set_disp <- public member DP[view]              stereoMatching.h:2724
 *   sm_so_config       <- the call commented in at dispOptimize's "so" branch (cpp:1096-1100):
 *                         so cpp:6272-6394, so_R2L cpp:6683-6826, so_T2D cpp:6580-6681, and their Pn2 / Pn3 literals
 *   sm_vmtop_config    <- Parameters::Do_vmTop, vmTop_* and ts       stereoMatching.h:182-188, 201, 320-326
 *                         (dispOptimize cpp:1108-1128, selectTopCostFromVolumn h:2405-2461,
 *                          genDispFromTopCostVm2 cpp:1514-1885)
 *   sm_cbca_double_config <- Parameters::cbca_double_win, cbca_crossL[1] ..  stereoMatching.h:144, 263-275
 *                         (CBCA cpp:4333-4360, combine2Vm_4 cpp:4273-4331)
 *   sm_get_cbca_dw_mask <- member arm_Mask as combine2Vm_4 leaves it (cpp:4303-4318)
 *   sm_cbca_intersect_config <- Parameters::cbca_intersect                 stereoMatching.h:139, 262
 *                         (cbca_core cpp:5585-5666, gen1DCumu cpp:3896-3926, cal1DCost h:1643-1715)
 *   sm_get_cbca_area   <- cbca_core's local `area` after its last iteration (cpp:5606)
 *   sm_refine_ext_config <- static switches Do_calPKR, Do_bgIpol, Do_subpixelEnhancement (h:73-81),
 *                         calPKR's ratio_PKR (cpp:4093), Parameters::DISP_PKR (h:218), bgIplDepth (h:311)
 *                         (calPKR + signDp_UsingPKR cpp:4087-4140, BGIpol cpp:7323-7338 +
 *                          backgroundInterpolateCore cpp:7011-7043, subpixelEnhancement cpp:6138-6167)
 *   sm_get_pkr_mask    <- member PKR_Err_Mask as calPKR leaves it (cpp:1380)
 *   sm_get_subpixel / sm_download_subpixel <- refine()'s local SE after medianBlur(SE, SE, 3) (cpp:1484-1490)
 *   sm_refine_da_config <- static switch Do_discontinuityAdjust (h:78), the literals of cpp:6063-6064
 *                         (discontinuityAdjust cpp:6057-6136)
 *   sm_get_da_edges    <- discontinuityAdjust's local disp_E after Canny (cpp:6064)
 *   sm_refine_outlier_config <- the commented alternatives of refine() at cpp:1367 and cpp:1408,
 *                         Parameters::DISP_MIS (h:217), interpolateType (h:178, 310)
 *                         (LRConsistencyCheck cpp:2284-2335; RV_combine_BG cpp:7146-7216 with
 *                          cal_histogram_for_HV cpp:6830-6862, backgroundInterpolateCore cpp:6964-7043)
 *   sm_get_lrc_mask    <- member LRC_Err_Mask as LRConsistencyCheck leaves it (cpp:2291-2309)
 *   sm_eval_config, sm_upload_truth, sm_get_stage_errors, sm_get_stage_maps <- saveFromDisp<short, 0> -> calErr
 *                         after dispOptimize and the stages of refine() (cpp:588-601, 1102, 1131, 1373-1501;
 *                         h:1748-1825), DT and I_mask (cpp:2072-2075)
 *   sm_get_volume / sm_set_volume <- public member vm[view]       stereoMatching.h:2720
 *   sm_get_arms        <- public member HVL[view]                    stereoMatching.h:2717
 *   sm_destroy         <- delete smPsy[p]                            main_.cpp:173-178
 *   sm_run / sm_run_batch  <- the whole main_.cpp:139-163 sequence for n independent pairs
 *   sm_run_batch_multi     <- the same over several contexts / GPUs (one host thread each)
 *   sm_pyramid_config      <- PY_LEV and the per-level constructor arguments of main_.cpp:131-158, for sm_run
 * Threading: one sm_ctx per host thread; each ctx owns one HIP stream on its device.
 */
#ifndef SM_CAPI_H
#define SM_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SM_API __attribute__((visibility("default")))
#else
#define SM_API
#endif

typedef enum sm_status {
    SM_OK = 0,
    SM_EINVAL = 1,   /* bad argument / unsupported parameter combination */
    SM_ENOMEM = 2,   /* device or host allocation failed */
    SM_EHIP = 3,     /* HIP runtime error (launch, copy, sync) */
    SM_ESTATE = 4,   /* call out of order (e.g. optimize before cost) */
} sm_status;

/* static std::string costcalculation / aggregation / optimization selectors (h:51-53). */
typedef enum sm_cost_method {
    SM_COST_CENSUS_GRAD = 0, /* "censusGrad" (main:15; cpp:25-48) — default */
    SM_COST_CENSUS = 1,      /* "Census"     (cpp:975-976) */
    SM_COST_AD_CENSUS = 2,   /* "ADCensus"   (cpp:894-915, 5250-5277) */
    SM_COST_AD = 3,          /* "AD"         (cpp:954-955) */
    /* The remaining measures of costCalculate (cpp:954-987).  Left view, moving pixel u - d (the right view
     * mirrors it); fl = one fp32 rounding; constants that are literals in the reference's functions are fixed. */
    SM_COST_SD = 4,          /* "SD"  asdCal(vm, "SD", imgNum, 20) (cpp:954-955) -> gen_ad_sd_vm(.., AOS = 1, trunc)
                              * (cpp:2468-2509): min(fl(sum_c |L_c - R_c|^2 / 3), ad_trunc_ad), out of range
                              * ad_trunc_ad (the call and its argument are AD's) */
    SM_COST_BT = 5,          /* "BT"  bt (cpp:90-114): Birchfield-Tomasi on the gray images (calNeiMaxMin cpp:197-227,
                              * calCostForBT cpp:142-195): the smaller distance of one pixel's value to the other
                              * pixel's half-neighbour range; truncation and out-of-range value 20 */
    SM_COST_GRAD = 6,        /* "grad"  grad(vm, 500) (cpp:961-962, 603-656) -> calgradvm: the gradient term of
                              * censusGrad stored as is; reads grad_trunc and grad_adaptive; out of range
                              * (float)sqrt(2 grad_trunc^2) */
    /* 7 is reserved (rejected by sm_create): "ZNCC".  gen_NCC_vm (cpp:2419-2464) writes only the interior of an
     * uninitialised volume that transform_NCCVm2 (cpp:2692-2707) then reads whole, so the reference's output
     * is undefined on a border frame and there is nothing to match.  The gap is pinned by tests */
    SM_COST_TRUNC_AD = 8,    /* "TruncAD"  truncAD (cpp:788-805) -> gen_truncAD_vm (cpp:2511-2548):
                              * (float)min(sum_c |L_c - R_c|, 60) in integers, out of range 60 */
    SM_COST_AD_GRAD = 9,     /* "adGrad"  adGrad (cpp:50-70): A = AD with truncation 7, G = grad with truncation 2,
                              * fl(fl(A * (float)0.11) + fl(G * (float)(1 - 0.11))) (gen_vm_from2vm_fixWgt
                              * cpp:3767-3796); reads grad_adaptive */
    SM_COST_AD_CENSUS_GRAD = 10, /* "ADCensusGrad"  ADCensusGrad (cpp:917-943) -> gen_vm_from3vm_exp (cpp:3592-3652,
                              * called from cpp:5287): A = AD with truncation 255, C = the census cost, G = grad with
                              * truncation 500; m = (float)(0.5 A + 0.5 C), (float)(0.7 (1 - expf(-m / 1)) +
                              * 0.3 (1 - expf(-G / 2))) with the products and the sum in double.  The call's ARU
                              * arguments 30, 45, 15 are dead in the live line (cpp:3640); reads grad_adaptive and
                              * the census window */
} sm_cost_method;

typedef enum sm_aggregation {
    SM_AGG_NONE = 0,
    SM_AGG_CBCA = 1,         /* "CBCA" (main:16; cpp:1002-1003) — default */
    SM_AGG_GF = 2,           /* "GF"  guideFilter (cpp:4492-4516), form chosen by gf_mode.  Costs may be negative or NaN:
                              * sgm / WTA, and so through sm_create_ex with so_float_minima = 1 */
    SM_AGG_NL = 3,           /* "NL"  non-local MST tree filter (cpp:4892-4917, NL/NLCCA.cpp:27-96) */
    /* 4 is reserved (rejected by sm_create) */
    SM_AGG_FIF = 5,          /* "FIF" full-image guided filter: four weighted sweeps over the volume, form chosen
                              * by fif_mode (FIF_Improve cpp:4707-4890, FIF cpp:4541-4705) */
    /* 6 is reserved (rejected by sm_create) */
    SM_AGG_AWS = 7,          /* "AWS" adaptive support weights over a 35 x 35 window (cpp:5692-5801, the branch
                              * without JBF_STANDARD); window and gamma_c: sm_aws_config.  The Lab planes are
                              * OpenCV's 8-bit BGR2Lab restated (parity unpinned) */
    /* 8 is reserved (rejected by sm_create).  The gaps 4, 6 and 8 are deliberate and pinned by tests: do not
     * renumber or fill them */
    SM_AGG_BF = 9,           /* "BF" cv::boxFilter(vm[i], vm[i], -1, Size(12, 12)) on every view that exists
                              * (cpp:1023-1043): normalised, BORDER_REFLECT_101, anchor 6, i.e. offsets -6 .. +5;
                              * window: sm_bf_config.  Costs stay >= +0 while the sums are exact: every optimiser applies;
                              * with inexact sums (gradient cost methods, ad_trunc_ad off the 2^-25 grid) so needs
                              * sm_create_ex with so_float_minima = 1 */
    SM_AGG_GFNL = 10,        /* "GFNL" (cpp:4421-4490): vm[0] = NL where the left gray image's 19 x 19 variance is
                              * < 400 (sm_gfnl_config), else (float)(0.5 NL + 0.5 GF); vm[1] is GF's (do_refine).
                              * Reads gf_eps, gf_mode, nl_sigma; like GF, sgm / WTA, and so through sm_create_ex */
} sm_aggregation;

/* "FIF"'s two forms: */
typedef enum sm_fif_mode {
    SM_FIF_IMPROVE = 0,      /* FIF_Improve (cpp:4707-4890), what costCalculate calls (cpp:1010-1011): every sweep
                              * step takes the minimum over d - 1, d, d + 1 of the previous pixel (+ Pn off d) */
    SM_FIF_PLAIN = 1,        /* FIF (cpp:4541-4705): the previous pixel's cost at d only */
} sm_fif_mode;

/* guideFilter's two builds (stereoMatching.h:38 `//#define MY_GUIDE`): */
typedef enum sm_gf_mode {
    SM_GF_XIMGPROC = 0,      /* cv::ximgproc::guidedFilter(I, vm, vm, 9, 1e-4) (cpp:4513) — the shipped build */
    SM_GF_MY_GUIDE = 1,      /* guideFilterCore_matlab (cpp:4509, 4975-5104) — the MY_GUIDE build */
} sm_gf_mode;

typedef enum sm_optimization {
    SM_OPT_WTA = 0,          /* "" : WTA only (cpp:1104-1128) */
    SM_OPT_SGM = 1,          /* "sgm" (main:17; cpp:1051-1060) — default */
    SM_OPT_SO = 2,           /* "so" scan-line DP + backtrack (cpp:1091-1105, 6272-6394) */
} sm_optimization;

/* The subset of StereoMatching::Parameters (h:85-351) that the hot path reads, plus the
 * static selectors.  Field defaults come from sm_params_default (= the reference ctor). */
typedef struct sm_params {
    uint32_t struct_size;        /* = sizeof(sm_params), set by sm_params_default; sm_create refuses others */
    int32_t rows, cols;          /* h_, w_ */
    int32_t num_disparities;     /* numDisparities = maxDisp + 1 (h:209) */
    int32_t cost_method;         /* sm_cost_method */
    int32_t aggregation;         /* sm_aggregation */
    int32_t optimization;        /* sm_optimization */
    int32_t census_rv, census_ru;/* census window radii {3, 4} (cpp:815) */
    int32_t census_ring;         /* censusFunc == 3 -> 8 ring bits (h:244) */
    float lam_cen, lam_g;        /* lamCen = 13, lamG = 1 (main:56-57) */
    float grad_trunc;            /* 500 (cpp:34) */
    int32_t grad_adaptive;       /* gradFuse_adpWgt = 1 (h:245) */
    float lam_ad, lam_cen_adc;   /* ADCensus fusion constants 10, 30 (cpp:5270) */
    float ad_trunc_adc;          /* 1000 (cpp:905) */
    float ad_trunc_ad;           /* 20 (cpp:955) */
    int32_t arm_l, arm_l_out;    /* cbca_crossL[0] = 17, cbca_crossL_out[0] = 34 (h:263, 266) */
    int32_t arm_c_thresh, arm_c_thresh_out; /* cbca_cTresh[0] = 20, cbca_cTresh_out[0] = 6 */
    int32_t arm_min_l;           /* cbca_minArmL = 1 (h:259) */
    int32_t cbca_iterations;     /* cbca_iterationNum = 2 (h:260) */
    int32_t sgm_paths;           /* 4 (cpp:6214) or 8 (full table cpp:6207-6208) */
    float sgm_p1, sgm_p2;        /* 1.0, 3.0 (h:2234-2235) */
    int32_t sgm_cor_dif_thres;   /* 15 (h:239) */
    int32_t sgm_redu_coeff;      /* 4 (h:240) */
    int32_t compute_right_view;  /* build vm[1] too (Do_LRConsis, h:72); 0 = skip (unused downstream) */
    int32_t keep_final_volume;   /* write the SGM path-sum back into vm[0] (reference does); 0 = fuse into WTA */
    int32_t batch_capacity;      /* max pairs per sm_run call (device buffers sized for it) */
    /* refinement: Do_refine (h:70) = 1 runs vm[1] through CBCA / SolveAll / SGM / WTA as well
     * (cbca_core cpp:5592, SolveAll cpp:2178, dispOptimize cpp:1054) and refine() afterwards
     * (sm_refine; sm_run does both).  Stage switches and constants as in the reference. */
    int32_t do_refine;           /* Do_refine = 0 (h:70) */
    float lr_max_diff;           /* LRmaxDiff = 0 (h:212) */
    int32_t do_region_vote;      /* Do_regionVote = 1 (h:75) */
    int32_t region_vote_nums;    /* region_vote_nums = 2 (h:306): rounds of region vote and of properIpol */
    float rv_ratio;              /* rv_ratio[i] = 0.4 (cpp:1400); must be > 0 */
    int32_t rv_s;                /* rv_s[i] = 20 (cpp:1401) */
    int32_t do_proper_ipol;      /* Do_properIpol = 1 (h:76) */
    int32_t disp_occ;            /* DISP_OCC = -2 * 16 (h:216) */
    int32_t do_last_median_blur; /* Do_lastMedianBlur = 1 (h:80) */
    /* scheduling of sm_run (results are identical for every setting): */
    int32_t sub_batch;           /* run the n pairs in groups of k (0 = one group), stages back to back */
    int32_t num_streams;         /* 0 (default): auto -- with CBCA and a volume >= 256 MiB per pair (or
                                  * batch_capacity >= 8 with 4-path SGM and no refinement), two
                                  * streams and (sub_batch 0) two groups of n / 2 pairs; with SGM
                                  * and no refinement the groups are pipelined ACROSS calls: sm_run
                                  * returns with the second group still queued on the side stream
                                  * (about half a call behind the first), the next sm_run's groups
                                  * follow on their own streams, sm_download_disp_async copies each
                                  * group's maps after that group, and every other call first waits
                                  * for both; else one stream; 1: one stream; 2-4: groups alternate
                                  * over that many streams (group k + 1 starts after group k's first
                                  * CBCA sweep, or its aggregation without CBCA), joined per call */
    int32_t fuse_norm_scan;      /* CBCA: iteration k's normalising sweep fused with iteration k+1's
                                  * scan (one sweep, 8 B per element less): 1 = always, 0 = never,
                                  * -1 (default) = when the dedicated sweep for the reference's lag
                                  * applies (arm length 34, D % 64 == 0) or a pair's volume is
                                  * >= 256 MiB (measured faster there; the generic fused sweep is
                                  * slower at Teddy size) */
    /* alternative aggregators */
    float gf_eps;                /* gf_eps[0] = 0.0001 (h:298; radius gf_r[0] = 9, h:297) */
    int32_t gf_mode;             /* sm_gf_mode: SM_GF_XIMGPROC (default, the shipped build) or SM_GF_MY_GUIDE */
    double nl_sigma;             /* NLCCA sigma = 0.1 (NL/NLCCA.cpp:33): weights exp(-c / (255 sigma)) */
    int32_t lr_consis;           /* Do_LRConsis = 1 (h:72): "so" optimises both views, DP[1] = so(vm[1])
                                  * (num = Do_LRConsis ? 2 : 1, cpp:1093); 0: "so" builds and optimises
                                  * the left view only */
    int32_t placement_trials;    /* volume placement (results are identical for every setting): the
                                  * same kernels run 5-8 % apart on different device allocations of
                                  * the volumes -- same request counts, more DRAM credit stalls
                                  * (TCC_EA0_RDREQ_DRAM_CREDIT_STALL) -- so the first
                                  * sm_run of a context may time its own pipeline on k candidate
                                  * volume sets held at once and keep the fastest (k - 1 extra sets
                                  * of memory during that call only; fewer if they do not fit).
                                  * -1 (default) = 3 with CBCA + SGM and a volume >= 256 MiB per
                                  * pair, else off; 0 / 1 = off; 2-8 = k */
    int32_t fuse_cost_scan;      /* CBCA (results are identical for every setting): the first H scan
                                  * of a view computes its censusGrad costs itself, so that view's
                                  * cost volume is never written and read back (8 B per element
                                  * less).  Applies to the views CBCA runs on, with censusGrad,
                                  * >= 3 census words (more than 64 bits), lam_g == 1 and a grad_trunc
                                  * at which the select-free cost elements apply; everything else
                                  * keeps the cost-volume kernel.  1 = wherever eligible, 0 = never,
                                  * -1 (default) = wherever eligible (measured faster at every
                                  * bench shape, Teddy to full resolution) */
    /* aggregation "FIF" (read only with aggregation = SM_AGG_FIF) */
    int32_t fif_mode;            /* sm_fif_mode: SM_FIF_IMPROVE (default) or SM_FIF_PLAIN */
    float fif_eps;               /* eps = 0.08 (cpp:4713): weights exp(-|dI|^2 / eps^2) on I / 255; must be > 0 */
    float fif_pn;                /* Pn = 2 (cpp:4714): penalty of the d +/- 1 neighbours (FIF_Improve); >= +0 */
} sm_params;

typedef struct sm_ctx sm_ctx;

SM_API void sm_params_default(sm_params* p, int32_t max_disp, int32_t rows, int32_t cols);
SM_API sm_status sm_create(sm_ctx** out, const sm_params* p, int32_t hip_device);

/* sm_create with options that are not sm_params fields (the struct keeps its size).  sm_create(out, p, dev) is
 * sm_create_ex(out, p, NULL, dev); NULL means the defaults, under which every refusal and its text is sm_create's.
 *   so_float_minima = 1: the scan-line optimisers (so, so_R2L, so_T2D) take every minimum as the reference's C++
 *     loop does: m = c[0], i = 0; for d = 1 .. D-1: if (c[d] < m) { m = c[d]; i = d; } -- float compares, the first
 *     index of equal values (-0 == +0), a NaN at index 0 sticky ((NaN, 0) whatever follows), a NaN elsewhere never
 *     taken.  The forward step's compares are false when a side is NaN, so a NaN cost stays NaN along its line and
 *     is never chosen over a number.  Defined for finite costs of either sign, +-0 and NaN.  Where an accumulated
 *     cost kept with keep_final_volume is not NaN its bits are the reference's; NaN payloads and signs are not
 *     pinned.  With a +inf cost the reference's own backtrack leaves its trace (FLT_MAX < +inf selects d - 1 at
 *     d = 0 and d + 1 at d = D - 1); here the backtrack's disparity is clamped to [0, num_disparities), no access
 *     leaves the line's own trace and every other line (row for so / so_R2L, column for so_T2D) is unaffected; what
 *     the map holds on the affected line is unspecified.
 *     sm_create's four refusals of "so" fall away: after GF, after GFNL, and after BF with a gradient cost method or
 *     with ad_trunc_ad off the 2^-25 grid.  Every other check is unchanged.  After an aggregation whose costs are
 *     >= +0 the option is allowed too and gives the same maps and volumes from the float-minima kernels.  On a
 *     context whose optimization is not SM_OPT_SO it is accepted and changes nothing.
 * SM_EINVAL, with the field named in sm_last_error, for a struct_size other than sizeof(sm_create_opts) and for
 * so_float_minima outside {0, 1}: checked before sm_params and without a device. */
typedef struct sm_create_opts {
    uint32_t struct_size;        /* = sizeof(sm_create_opts), set by sm_create_opts_default */
    int32_t so_float_minima;     /* 0 (default): as sm_create.  1: see above */
} sm_create_opts;
SM_API void sm_create_opts_default(sm_create_opts* o);
SM_API sm_status sm_create_ex(sm_ctx** out, const sm_params* p, const sm_create_opts* opts, int32_t hip_device);
SM_API sm_status sm_destroy(sm_ctx* ctx);
SM_API const char* sm_last_error(const sm_ctx* ctx);
SM_API const char* sm_status_string(sm_status s);

/* Single-pair, reference-ordered API (pair slot 0).  Host buffers: BGR u8 rows of
 * `cstride` bytes, gray u8 rows of `gstride` bytes; copied to the device. */
SM_API sm_status sm_set_images(sm_ctx* ctx, const uint8_t* lbgr, const uint8_t* rbgr, size_t cstride,
                               const uint8_t* lgray, const uint8_t* rgray, size_t gstride);
SM_API sm_status sm_cost_calculate(sm_ctx* ctx);
SM_API sm_status sm_solve_all(sm_ctx* ctx, int32_t py_lev, float reg_lambda);
SM_API sm_status sm_disp_optimize(sm_ctx* ctx, int16_t* disp_out);
/* SolveAll(smPyr, PY_LVL, REG_LAMBDA) over PY_LVL in [1, 8] contexts, one per pyramid level
 * (main_.cpp:131-158): level s has rows (rows_{s-1} + 1) / 2, cols likewise, num_disparities
 * >= num_disparities_{s-1} / 2 + 1, the same pair count and device, and sm_cost_calculate done.
 * levels[0]'s volume(s) receive the cross-scale sum; the coarser levels are only read. */
SM_API sm_status sm_solve_all_pyr(sm_ctx* const* levels, int32_t py_lvl, float reg_lambda);
/* cv::pyrDown (u8, 1 or 3 channels, BORDER_REFLECT_101) on `hip_device`; src rows x cols, dst
 * ((rows + 1) / 2) x ((cols + 1) / 2); host or device pointers, synchronous.  (main_.cpp:145-148) */
SM_API sm_status sm_pyr_down(int32_t hip_device, const uint8_t* src, int32_t rows, int32_t cols, int32_t channels,
                             uint8_t* dst);
/* cv::pyrDown of a 1-channel f32 image (the ground truth DT, main_.cpp:149), same contract. */
SM_API sm_status sm_pyr_down_f32(int32_t hip_device, const float* src, int32_t rows, int32_t cols, float* dst);
/* refine() on DP[0] (needs do_refine = 1 at sm_create and a preceding sm_disp_optimize). */
SM_API sm_status sm_refine(sm_ctx* ctx, int16_t* disp_out);
SM_API sm_status sm_get_disp(sm_ctx* ctx, int32_t view, int16_t* dst);  /* DP[view], H*W int16; DP[1] exists
                                                                        * with do_refine or optimization "so"
                                                                        * (so runs on both views, cpp:1093) */
/* Overwrite DP[view] (the reference's DP is a public member, h:2724); after sm_disp_optimize. */
SM_API sm_status sm_set_disp(sm_ctx* ctx, int32_t view, const int16_t* src);
SM_API sm_status sm_get_volume(sm_ctx* ctx, int32_t view, float* dst);   /* H*W*D floats */
SM_API sm_status sm_get_arms(sm_ctx* ctx, int32_t view, uint16_t* dst);  /* H*W*4 (L,R,U,D) */

/* Batched, device-resident API.  Inputs are packed [n][H][W][3] (BGR) and [n][H][W] (gray) and may
 * be host or device pointers (unified addressing: e.g. a torch tensor already in HBM is copied
 * device-to-device).  A device source must be complete before the call (its stream synchronized). */
SM_API sm_status sm_upload_batch(sm_ctx* ctx, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr,
                                 const uint8_t* lgray, const uint8_t* rgray);
/* Run cost -> CBCA -> SolveAll(PY_LVL, reg_lambda) -> SGM -> WTA [-> refine] on the n uploaded pairs; PY_LVL is
 * 1 unless sm_pyramid_config set another (then every pair group first builds and aggregates its coarse levels).
 * Asynchronous on the ctx stream.  disp_out: host or device [n][H][W] int16 (synchronous copy) or
 * NULL to leave the maps on the device (read them with sm_download_disp). */
SM_API sm_status sm_run(sm_ctx* ctx, int32_t n, float reg_lambda, int16_t* disp_out);
/* The cross-scale pyramid of main_.cpp:131-158 inside sm_run / sm_run_batch / sm_run_batch_multi: py_lvl = PY_LEV in
 * [1, 8]; 1 (the default) is sm_run without a pyramid.  With py_lvl = L > 1 the context owns L - 1 level contexts --
 * ordinary contexts on the same device with the same batch_capacity, created as sm_create creates one, destroyed by
 * sm_destroy or the next sm_pyramid_config.  Level s >= 1 takes level 0's sm_params except (main_.cpp:138-148,
 * cpp:5367-5371): rows_s = (rows_{s-1} + 1) / 2 and cols_s likewise; num_disparities_s = (num_disparities_{s-1} - 1)
 * / 2 + 2; arm_l_s = arm_l / 2^s and arm_l_out_s = arm_l_out / 2^s; optimization "" (no optimiser or refine buffers;
 * do_refine still decides that vm[1] is built and combined), one stream, no placement trials.  fuse_cost_scan and
 * fuse_norm_scan are decided per level from its own size.  Memory: 1/8 + 1/64 + .. of level 0's volumes and planes.
 * sm_run then does, for every pair group on the group's stream: pyrDown of the group's colour and gray images of
 * both views, level by level (one launch per level); prep, cost volume(s) and aggregation of levels L - 1 .. 1;
 * level 0 with SolveAll not fused into its last aggregation store; SolveAll's cross-scale sum (cpp:2179-2203: from
 * 0.f, one rounded product and one rounded sum per level in level order, cy >>= 1, cx >>= 1, cd = (cd + 1) >> 1)
 * into level 0's vm[0] (and vm[1] with do_refine); level 0's optimiser and refine().  The maps are the same for every
 * schedule; the NL pipelined front is off.  Profile names of a level's launches end in @<level>
 * ("cbca_v_norm_scan@1"); the new launches are "pyr_down@<destination level>" and "solve_all_pyr[_r]".
 * sm_aws_config, sm_bf_config, sm_gfnl_config, sm_cbca_double_config (arm_l2 and arm_l_out2 divided by 2^s) and
 * sm_cbca_intersect_config apply to every level, whichever order they and this call come in; a level that cannot
 * take a setting fails that call with the level named and every level unchanged.  sm_so_config, sm_vmtop_config,
 * sm_refine_ext_config, sm_refine_da_config, sm_refine_outlier_config and sm_eval_config concern level 0 only.  The staged calls keep their contracts
 * (sm_solve_all refuses py_lev != 1; sm_solve_all_pyr takes one context per level).
 * Checked before any device call: py_lvl outside [1, 8] and a level that sm_create would refuse (rows or cols < 2,
 * an aggregation's minimum size, ..) are SM_EINVAL with the level and its reason in sm_last_error.  On a live
 * context the call joins a live pipeline and waits for the queued work first.  If a level cannot be allocated the
 * context is left at py_lvl = 1. */
SM_API sm_status sm_pyramid_config(sm_ctx* ctx, int32_t py_lvl);
/* Level `level`'s context, borrowed: level 0 is ctx itself; NULL when out of range.  For sm_get_volume, sm_get_arms,
 * sm_get_census, sm_get_cbca_area and sm_get_cbca_dw_mask on a coarse level after sm_run -- call
 * sm_synchronize(ctx) on the owner first.  Every other call on a level context returns SM_ESTATE. */
SM_API sm_ctx* sm_pyramid_level(sm_ctx* ctx, int32_t level);
SM_API int32_t sm_pyramid_levels(const sm_ctx* ctx);   /* PY_LVL of the context (1 without a pyramid) */
SM_API sm_status sm_download_disp(sm_ctx* ctx, int32_t n, int16_t* disp_out);
/* The same copy, enqueued on the ctx's copy stream behind the work queued so far, returning at
 * once: the next sm_run's disparity-writing kernels wait for it, so the copy overlaps the next
 * run's cost / aggregation work.  disp_out must be page-locked host memory (or device memory) and
 * stays in flight until sm_synchronize. */
SM_API sm_status sm_download_disp_async(sm_ctx* ctx, int32_t n, int16_t* disp_out);
/* A pipelined stream of calls without host waits in between (the batch runner's product path):
 * sm_upload_batch_async queues the copies of the next call's inputs behind the groups of the
 * previous call that read the same pairs (no join, no host wait; the sources must stay unchanged
 * until sm_upload_wait returns); sm_download_wait(ctx, back) waits on the host for the copies of
 * the last (back = 0) or the previous (back = 1) sm_download_disp_async -- neither joins the
 * pipeline. */
SM_API sm_status sm_upload_batch_async(sm_ctx* ctx, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr,
                                       const uint8_t* lgray, const uint8_t* rgray);
SM_API sm_status sm_upload_wait(sm_ctx* ctx);
SM_API sm_status sm_download_wait(sm_ctx* ctx, int32_t back);
SM_API sm_status sm_run_batch(sm_ctx* ctx, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr,
                              const uint8_t* lgray, const uint8_t* rgray, float reg_lambda,
                              int16_t* disp_out);
/* Multi-device batch (SURVEY §8b/§8e without torch.distributed): the n packed host pairs are split
 * into contiguous blocks of ceil(n / nctx), block i runs on ctxs[i] (each context on its own
 * device, or several on one), one host thread per context; disp_out receives all n maps in order.
 * Contexts must share rows / cols / num_disparities and hold batch_capacity >= the block size.
 * Returns the first failing context's status (its sm_last_error has the message). */
SM_API sm_status sm_run_batch_multi(sm_ctx* const* ctxs, int32_t nctx, int32_t n, const uint8_t* lbgr,
                                    const uint8_t* rbgr, const uint8_t* lgray, const uint8_t* rgray,
                                    float reg_lambda, int16_t* disp_out);
/* Change sm_params.num_streams / sub_batch of an existing context (same meaning and ranges as at
 * sm_create); applies from the next sm_run.  Results are identical for every schedule; this lets
 * one context (one set of device allocations) time schedules against each other. */
SM_API sm_status sm_set_schedule(sm_ctx* ctx, int32_t num_streams, int32_t sub_batch);
/* placement trials of the first sm_run (sm_params.placement_trials): the number of volume sets
 * timed (0: none ran), their pipeline times in ms (up to max), and the index of the set kept */
SM_API int32_t sm_placement_trials_ms(sm_ctx* ctx, double* ms, int32_t max);
SM_API int32_t sm_placement_kept(const sm_ctx* ctx);
SM_API sm_status sm_synchronize(sm_ctx* ctx);
SM_API void* sm_stream(sm_ctx* ctx);      /* the ctx's main hipStream_t, joined first: after a
                                             pipelined sm_run (num_streams 0, the default) the
                                             call's second group runs on a side stream until the
                                             next entry point joins it; sm_stream joins it, so work
                                             ordered after the returned stream sees the whole call.
                                             NULL on error (sm_last_error) */

/* Per-kernel timing with HIP events on the ctx stream. */
SM_API sm_status sm_profile_enable(sm_ctx* ctx, int32_t on);
/* Fills up to max entries: name (NUL-terminated, 48 chars max), launches, total ms,
 * algorithmic bytes per launch.  Returns the number of distinct kernels in *count. */
SM_API sm_status sm_profile_read(sm_ctx* ctx, int32_t max, char* names /* max*48 */, int64_t* launches,
                                 double* total_ms, double* bytes_per_launch, int32_t* count);
SM_API sm_status sm_profile_reset(sm_ctx* ctx);

/* calErr (stereoMatching.h:1748-1825) for one region mask: over pixels with mask == 255, an error
 * is DP < 0 or |DT - DP| > thres; *pbm = errors / count, *rms = sqrt(sum / count) where the float
 * sum adds pow(dif, 2) per valid pixel and 2 per invalid one, in raster order (host code, exact
 * reference arithmetic).  Host pointers; rows x cols, packed. */
SM_API sm_status sm_cal_err(const int16_t* disp, const float* gt, const uint8_t* mask, int32_t rows, int32_t cols,
                            float thres, float* pbm, float* rms);

/* "AWS"'s constants, function-local in the reference (W_V_AWS = W_U_AWS = 17, cpp:5715; r_c = 5, h:1478):
 * each radius in [0, 17], gamma_c finite and > 0.  Defaults 17, 17, 5.  Applies from the next
 * sm_cost_calculate / sm_run (buffers are sized for radius 17 at sm_create).  SM_EINVAL, with the
 * argument named in sm_last_error, on a bad value or a context whose aggregation is not SM_AGG_AWS. */
SM_API sm_status sm_aws_config(sm_ctx* ctx, int32_t radius_v, int32_t radius_u, float gamma_c);

/* "BF"'s window, a literal in the reference (Size(12, 12), cpp:1038; width = ksize_u, height = ksize_v): each
 * size in [1, 32], anchor ksize / 2 (an even window reaches one further up / left than down / right).  Defaults
 * 12, 12.  Applies from the next sm_cost_calculate / sm_run.  SM_EINVAL, with the argument named in
 * sm_last_error, on a size out of range, on an image too small for a single reflection
 * (rows < ksize_v / 2 + 1 or cols < ksize_u / 2 + 1), or on a context whose aggregation is not SM_AGG_BF. */
SM_API sm_status sm_bf_config(sm_ctx* ctx, int32_t ksize_v, int32_t ksize_u);

/* "GFNL"'s variance threshold, a literal in the reference (400, cpp:4470): any finite float.  The 19 x 19
 * window and the 0.5 / 0.5 blend are fixed.  Applies from the next sm_cost_calculate / sm_run.  SM_EINVAL on
 * a value that is not finite or on a context whose aggregation is not SM_AGG_GFNL. */
SM_API sm_status sm_gfnl_config(sm_ctx* ctx, float var_thresh);

/* Which scan-line optimiser dispOptimize's "so" branch runs: the reference holds four and chooses one by which call
 * is commented in (cpp:1096-1100).
 *   SM_SO_L2R  so (cpp:6272-6394), the shipped call: left to right along the rows, Pn2 = 1.2, Pn3 = 3.6.
 *   SM_SO_R2L  so_R2L (cpp:6683-6826): columns W-2 .. 0 with prev = vm(v, u+1), the discontinuity between I(v, u) and
 *              I(v, u+1), vm(v, u)[d] += cost_min in place, the backtrack from the first minimum of column 0 towards
 *              W-1.  Pn2 = 0.3, Pn3 = 0.9.
 *   SM_SO_T2D  so_T2D (cpp:6580-6681): per column, rows 1 .. H-1 with prev = vm(v-1, u), the discontinuity between
 *              I(v, u) and I(v-1, u), vm(v, u)[d] += (cost_min - c_min) with c_min = the row minimum + Pn3 (one
 *              rounded difference, one rounded sum; accumulated costs go negative), the backtrack upwards from the
 *              first minimum of the last row.  Pn2 = 0.3, Pn3 = 0.9.  The reference runs it on a clone (vm_res,
 *              cpp:1095): vm[view] is left untouched, with keep_final_volume too.
 * All three read the left colour image for both views, try prev[d], prev[d-1] + Pn2, prev[d+1] + Pn2, min + Pn3 in
 * that order on strict <, take the first index of a minimum, and halve Pn2 and Pn3 where the mean absolute channel
 * difference to the scan's previous pixel is > 15.  pn2 / pn3 replace the function's literals; SM_SO_PN_DEFAULT
 * keeps them.  so_change (cpp:6419-6578) is not built: it reads DP before anything has written it.
 * Not sm_params fields (the struct keeps its size): SM_SO_L2R with 1.2 / 3.6 by default, takes effect from the next
 * sm_disp_optimize / sm_run; with a pyramid the call concerns level 0 only.  keep_final_volume: SM_SO_R2L leaves its
 * accumulated volume in vm[view], as so does.  The eval table's stage 0 keeps the name "so" (cpp:1102).  Every
 * refusal that exists with "so" holds for all variants, and so does what sm_create_ex's so_float_minima lifts (after
 * GF, GFNL and inexact BF all three variants run, on their float-minima kernels).  The maps are the same for every schedule.  Profile names:
 * "so_r2l[_r]", "so_t2d[_r]".  SM_EINVAL, with the argument named in sm_last_error, for a variant outside [0, 2], a
 * penalty that is neither SM_SO_PN_DEFAULT nor finite and >= +0, or a context whose optimization is not SM_OPT_SO
 * (unless the call is the all-default one: SM_SO_L2R, SM_SO_PN_DEFAULT, SM_SO_PN_DEFAULT); the arguments are checked
 * without a device. */
enum { SM_SO_L2R = 0, SM_SO_R2L = 1, SM_SO_T2D = 2 };
#define SM_SO_PN_DEFAULT (-1.0f)      /* the chosen function's own literals */
SM_API sm_status sm_so_config(sm_ctx* ctx, int32_t variant, float pn2, float pn3);

/* dispOptimize's Do_vmTop branch (cpp:1108-1128), the candidate-disparity selection: after "sgm" or "" every pixel
 * keeps the `num` (vmTop_Num = M, main:62) cheapest disparities whose cost is < firstV * thres (vmTop_thres =
 * (float)(lamc * 0.01), h:323; selectTopCostFromVolumn, h:2405-2461) and genDispFromTopCostVm2 (cpp:1514-1885)
 * chooses among them with vmTop_method 0 (the default: pairs of candidates closer than ts, a cost-keyed
 * container, the 8 neighbours' candidates; vmTop_hasCir2, vmTop_cir3_doColorLimit), 1 or 2 (row-sequential).
 * Not sm_params fields (the struct keeps its size): off by default, takes effect from the next sm_disp_optimize /
 * sm_run.  With it on, SGM writes its path sum into vm[view] (as with keep_final_volume) and the selection reads
 * it; "" reads the volume after SolveAll; with do_refine both views are done and refine() runs on those maps;
 * "so" never reaches the branch, so the call is accepted there and changes nothing.  The maps are the same for
 * every schedule.  The candidate table is allocated on the first enabling call (batch_capacity pairs, every
 * view dispOptimize runs on).  SM_EINVAL, with the argument named in sm_last_error, for a method outside
 * [0, 2], a num outside [1, 8] or a thres that is not finite; the arguments are checked without a device.
 * Costs are expected finite and below FLT_MAX (the reference masks taken disparities with FLT_MAX). */
SM_API sm_status sm_vmtop_config(sm_ctx* ctx, int32_t enable, int32_t method, int32_t num, float thres, int32_t ts,
                                 int32_t has_cir2, int32_t cir3_color_limit);
/* Overwrite vm[view] of pair 0 (the reference's vm is a public member, h:2717), H*W*D floats; after
 * sm_cost_calculate.  sm_disp_optimize may then run (again) on it. */
SM_API sm_status sm_set_volume(sm_ctx* ctx, int32_t view, const float* src);
/* Pair 0's candidate table of `view` from the last sm_disp_optimize / sm_run with vmTop on, in the reference's
 * topDisp layout [H][W][num + 1][2] floats: (disparity, cost) per kept candidate, the count in [num][0];
 * entries the reference never writes read as 0. */
SM_API sm_status sm_get_top_disp(sm_ctx* ctx, int32_t view, float* dst);

/* CBCA()'s double-window branch (Parameters::cbca_double_win, cpp:4337-4357).  With it on, "CBCA" aggregates the
 * raw costs twice -- with the arms of window 1 (arm_l2 = cbca_crossL[1], arm_l_out2 = cbca_crossL_out[1],
 * arm_c_thresh2 = cbca_cTresh[1], arm_c_thresh_out2 = cbca_cTresh_out[1]; 23, 23, 30, 0 in the reference) into a
 * second volume, and with sm_params' window 0 in place -- and combine2Vm_4 (cpp:4273-4331) gives a pixel all its
 * costs from the window-1 volume where the 3 x 3 normalised box mean (BORDER_REFLECT_101) of "the longest of the
 * four window-0 arms" is < arm_len_thres (the literal 5 of cpp:4297).  As in the reference: both runs do two
 * iterations whatever cbca_iterations says (cbca_core(.., 2)); the mask comes from the LEFT image's arms for
 * both views (HVL[0]); window 0's arms are computed last, so sm_get_arms and refine() see them as without the
 * switch; arm_min_l applies to both windows.  Not sm_params fields (the struct keeps its size): off by default,
 * takes effect from the next sm_cost_calculate / sm_run.  The maps are the same for every schedule.  The second
 * arm planes, one second volume and the mask are allocated on the first enabling call (batch_capacity pairs);
 * a context that has had the switch on runs no placement trials.  SM_EINVAL, with the argument named in
 * sm_last_error, on a context whose aggregation is not SM_AGG_CBCA, for arm_l2 < 0, arm_l_out2 outside [0, 84],
 * a negative threshold or an arm_len_thres that is not finite; the arguments are checked without a device.
 * (Parameters::GF_double_win has no entry point: both arms of the reference's branch run guideFilter(0, vm),
 * cpp:4406-4418, so the facades accept the field and pass nothing on.) */
SM_API sm_status sm_cbca_double_config(sm_ctx* ctx, int32_t enable, int32_t arm_l2, int32_t arm_l_out2,
                                       int32_t arm_c_thresh2, int32_t arm_c_thresh_out2, float arm_len_thres);

/* Cross-based aggregation without arm intersection (Parameters::cbca_intersect = false, h:139, 262; cbca_core
 * cpp:5585-5666 with gen1DCumu cpp:3896-3926, cal1DCost h:1643-1715, genfinalVm_cbca cpp:3969-3992).  With
 * intersect = 0 the support region of a pixel comes from the arms of the view's own image alone (HVL[view]: the
 * left image's for vm[0], the right image's for vm[1]), is the same for every disparity, and has one int32 area
 * per pixel: every iteration starts from area = ones, runs two 1-D passes (H then V for an even iteration, V then
 * H for an odd one) -- a sequential f32 prefix sum along the axis, then per pixel S(x + head) - S(x - tail - 1), or
 * S(x + head) alone where x - tail - 1 < 0, and the same in integers for the area -- and divides by (float)area.
 * Default 1 (the intersecting form).  Not an sm_params field (the struct keeps its size); takes effect from the
 * next sm_cost_calculate / sm_run.  With 0: the costs always come from the cost volume kernel (every cost
 * method), fuse_cost_scan, fuse_norm_scan, sub_batch and num_streams change nothing in the maps,
 * cbca_iterations 0 .. 64 is honoured, the double window sends both of its runs through this form, profile names
 * end in "_ni"; sm_get_arms, refine() and the pyramid path work as before.  One more volume and the area planes
 * are allocated on the first call with 0 (batch_capacity pairs); a context that has had intersection off runs no
 * placement trials.  SM_EINVAL, with the argument named in sm_last_error, on a context whose aggregation is not
 * SM_AGG_CBCA and for a value outside {0, 1}; both are checked without a device. */
SM_API sm_status sm_cbca_intersect_config(sm_ctx* ctx, int32_t intersect);

/* subpixelEnhancement's two forms: */
typedef enum sm_se_mode {
    SM_SE_REFERENCE = 0,     /* the reference's `disp -= diff` on a short (cpp:6161): fl((float)d - diff) converted back
                              * to short, truncating toward zero, so SE holds integers (mostly d - 1 where diff > 0) */
    SM_SE_FLOAT = 1,         /* fl((float)d - diff) kept as a float: the sub-pixel disparity */
} sm_se_mode;

/* Three more stages of refine() (cpp:1347-1510), behind `static const bool` switches in the reference (h:73-81).
 * refine()'s order is LR check -> PKR -> region votes -> properIpol -> BGIpol -> SE -> last median.
 *   do_pkr       calPKR (cpp:4087-4126): c0, c1 = the smallest and second smallest (duplicates count) of a pixel's
 *                num_disparities costs in vm[0] as dispOptimize left it; PKR_Err_Mask = 1 where
 *                (c1 - c0) / c1 < pkr_ratio in float (ratio_PKR = 0.1f; 0 / 0 compares false); signDp_UsingPKR
 *                (cpp:4128-4140) then sets DP[0] = disp_pkr (DISP_PKR = -64) where the mask is set and DP[0] >= 0.
 *   do_bg_ipol   BGIpol (cpp:7323-7338): in raster order and IN PLACE every hole (DP[0] < 0) searches its row right,
 *                then left, up to bg_ipl_depth (bgIplDepth = 1000) steps each for the first value >= 0 and takes the
 *                only one found or the smaller of the two.  bg_ipl_depth = 0 fills nothing.
 *   do_subpixel  subpixelEnhancement (cpp:6138-6167) on DP[0] and vm[0], then medianBlur(SE, SE, 3): a float map
 *                per pair (se_mode: sm_se_mode), which the reference computes and drops; DP[0] is not changed.
 * Not sm_params fields (the struct keeps its size): all off by default, takes effect from the next
 * sm_disp_optimize / sm_refine / sm_run.  With do_pkr or do_subpixel and "sgm", SGM writes its path sum into
 * vm[0] (as with keep_final_volume) for the stages to read; "" leaves the volume after SolveAll.  The maps are the
 * same for every schedule.  The mask and the float maps are allocated on the first enabling call (batch_capacity
 * pairs).  SM_EINVAL, with the argument named in sm_last_error, on a context without do_refine, for a pkr_ratio
 * that is not finite, disp_pkr outside [-32768, -1], bg_ipl_depth outside [0, 32767], se_mode outside {0, 1},
 * do_pkr with num_disparities < 2 (the reference's second search writes slot -1), and do_pkr or do_subpixel with
 * optimization "so" and keep_final_volume = 0 (the reference's so rewrites vm in place, cpp:6299; this back end keeps
 * a trace instead).  With "so" and keep_final_volume = 1 the stages read vm[0] as the reference's refine() finds it:
 * the accumulated volume after so and so_R2L, the volume after SolveAll after so_T2D (which runs on a clone);
 * the arguments are checked without a device.  Do_discontinuityAdjust is built (sm_refine_da_config).  Not built:
 * Do_WM (reads a mask the shipped LR check never writes; with sm_refine_outlier_config's classify the mask exists,
 * but the stage still indexes a histogram with negative disparities) and Do_cbbi (needs floodFill and theRNG()). */
SM_API sm_status sm_refine_ext_config(sm_ctx* ctx, int32_t do_pkr, float pkr_ratio, int32_t disp_pkr, int32_t do_bg_ipol,
                                      int32_t bg_ipl_depth, int32_t do_subpixel, int32_t se_mode);
/* Pair 0's PKR_Err_Mask / float map SE of the last sm_refine / sm_run with the stage on: rows x cols bytes /
 * floats.  SM_ESTATE before that. */
SM_API sm_status sm_get_pkr_mask(sm_ctx* ctx, uint8_t* dst);
SM_API sm_status sm_get_subpixel(sm_ctx* ctx, float* dst);
/* The float maps of the first n pairs, [n][H][W], to a host or device pointer (synchronous). */
SM_API sm_status sm_download_subpixel(sm_ctx* ctx, int32_t n, float* dst);

/* refine()'s discontinuity adjustment (Do_discontinuityAdjust, h:78; discontinuityAdjust, cpp:6057-6136), "DA": per
 * pair on DP[0] and vm[0] as dispOptimize left it, after BGIpol and before the sub-pixel map and the last median
 * (cpp:1454-1497).  DP[0] clamped to 8 bits -> equalizeHist -> GaussianBlur(3 x 3, sigma 4) -> Canny(canny_low,
 * canny_high, 3, L1) gives an edge map; then, in raster order and IN PLACE over the interior, an edge pixel with a
 * direction (cpp:6079-6098) and DP >= 0 takes the disparity of the neighbour on either side of the edge whose cost
 * at its own disparity is lower (first side on cost >= 0, second side on cost != -1).  The three OpenCV calls are
 * restated in integers (the reference pins no OpenCV): the blur in OpenCV's 8.8 fixed-point form with
 * the taps (blur_side, blur_centre, blur_side) = (84, 87, 84), which are arguments so that a build whose kernel
 * sums to 256 can be matched.  One deviation: a disparity >= num_disparities in the map (possible only through
 * sm_set_disp) reads its cost as -1 where the reference reads outside the volume.  The imwrite of the edge image
 * is not reproduced.  rows < 3 or cols < 3 changes nothing.
 * Not sm_params fields (the struct keeps its size): off by default (20, 60, 84, 87 are the reference's values),
 * takes effect from the next sm_disp_optimize / sm_refine / sm_run.  With "sgm", SGM writes its path sum into
 * vm[0] for the stage to read, as for do_pkr; switched on after sm_disp_optimize ran without it, sm_refine returns
 * SM_ESTATE.  The maps are the same for every schedule; no launch count depends on the data and nothing is read
 * back.  The scratch is allocated on the first enabling call (batch_capacity pairs).  SM_EINVAL, with the argument
 * named in sm_last_error, on a context without do_refine, with optimization "so" and keep_final_volume = 0 (with 1
 * the stage reads vm[0] as for do_pkr), for a threshold outside
 * [0, 32767] (given in the wrong order they are swapped), a negative tap or 2 * blur_side + blur_centre > 256; the
 * arguments are checked without a device. */
SM_API sm_status sm_refine_da_config(sm_ctx* ctx, int32_t on, int32_t canny_low, int32_t canny_high, int32_t blur_side,
                                     int32_t blur_centre);
/* Pair 0's edge map (0 / 255) of the last sm_refine / sm_run with the stage on: rows x cols bytes.  SM_ESTATE
 * before that. */
SM_API sm_status sm_get_da_edges(sm_ctx* ctx, uint8_t* dst);

/* refine()'s outlier classification: two source switches of refine(), both off in the shipped build.
 *   classify     LRConsistencyCheck (cpp:2284-2335, LOR = 0; the commented call at cpp:1367) instead of
 *                LRConsistencyCheck_normal: with d = DP[0](v, u), a pixel fails when d < 0, u - d < 0 or
 *                (float)|d - DP[1](v, u - d)| > lr_max_diff (the same test); a failed pixel gets mask byte 255 and
 *                the label disp_mis (DISP_MIS = -48) if some d' in [0, min(num_disparities, u + 1)) has
 *                DP[1](v, u - d') == d', else sm_params.disp_occ (DISP_OCC = -32); passing pixels keep their value
 *                and get mask byte 0.  The DT-based counters, their cout lines and the imwrite are not reproduced.
 *   rv_combine   RV_combine_BG (cpp:7146-7216; the commented call at cpp:1408) instead of every regionVote_my round,
 *                under the same do_region_vote / region_vote_nums / rv_s / rv_ratio, Jacobi.  A hole (DP[0] < 0)
 *                takes, by interpolate_type (Parameters::interpolateType): 0 the vote rv; 1 the background value
 *                bg; 2 bg on a disp_occ hole, rv on a disp_mis hole; 3 on a disp_occ hole the smaller of rv and bg
 *                (the one that is >= 0 if only one is), rv on a disp_mis hole.  rv is cal_histogram_for_HV
 *                (cpp:6830-6862) over regionVote_my's region: -1 when validNum <= rv_s, else the first most frequent
 *                disparity if (float)hist[most] / validNum > rv_ratio (a float division, a strict compare), else -1.
 *                bg is backgroundInterpolateCore (cpp:6964-7043): the nearest value >= 0 within bg_ipl_depth columns
 *                right and left on the row, the smaller of those found, else -1; the depth is
 *                sm_refine_ext_config's bg_ipl_depth (1000 until that call), 0 finds nothing.  A result >= 0
 *                replaces the hole, otherwise the hole keeps its value, label included.  Types 2 and 3 assign
 *                nothing for a hole of neither class (DISP_PKR, or -1 without classify): the reference's `dp_`
 *                (cpp:7158) outlives both loops, so such a hole takes the result of the nearest earlier hole of
 *                either class in raster order within its pair and round (-1 before the first).  This is reproduced.
 *                One deviation: a value >= num_disparities in the map (possible only through sm_set_disp) counts in
 *                validNum and in no bin, where the reference indexes past its histogram.  The DT side channel is
 *                not reproduced.
 * Not sm_params fields (the struct keeps its size): both off by default, takes effect from the next sm_refine /
 * sm_run; with a pyramid the call concerns level 0 only.  No stage here reads a volume, so the call is allowed with
 * every optimiser, "so" included.  The maps are the same for every schedule, sub-batch and stream count; no launch
 * count depends on the data and nothing is read back.  The mask and the scratch are allocated on the first enabling
 * call (batch_capacity pairs).  SM_EINVAL, with the argument named in sm_last_error, on a context without do_refine,
 * for disp_mis outside [-32767, -1] or equal to disp_occ, interpolate_type outside [0, 3], or a switch outside
 * {0, 1}; the arguments are checked without a device. */
SM_API sm_status sm_refine_outlier_config(sm_ctx* ctx, int32_t classify, int32_t disp_mis, int32_t rv_combine,
                                          int32_t interpolate_type);
/* Pair 0's LRC_Err_Mask (0 / 255) of the last sm_refine / sm_run with classify on: rows x cols bytes.  SM_ESTATE
 * before that; SM_EINVAL for a null dst.  Both are decided without a device. */
SM_API sm_status sm_get_lrc_mask(sm_ctx* ctx, uint8_t* dst);

/* The reference's error table (saveFromDisp -> calErr, cpp:588-601, h:1748-1825), per pair and per stage, built on the
 * device inside sm_run / sm_disp_optimize / sm_refine.  Wherever the reference calls saveFromDisp<short, 0> -- after
 * dispOptimize and after the stages of refine() -- one launch ("eval_stage") reads the left map of every pair of the
 * group while it is still in cache, against the uploaded ground truth and region masks, and leaves one record per
 * (pair, stage, region); a second launch ("eval_final") sums the blocks' partial records.  Regions in I_mask's order:
 * nonocc, all, disc. */
typedef struct sm_stage_err {      /* one (pair, stage, region); 32 bytes */
    uint32_t count;                /* pixels with mask == 255 (calErr's sumNum) */
    uint32_t invalid;              /* of those, DP < 0 */
    uint32_t bad[4];               /* of those, DP < 0 or |DT - DP| > thres[k] (errorNumer); k >= nthres: 0 */
    double   sum_sq;               /* sum of dif^2 over valid pixels + 2 per invalid pixel (errorValueSum's terms) */
} sm_stage_err;
/* Not sm_params fields (the struct keeps its size): off by default; with it off nothing is launched or allocated.
 * on, keep_maps in {0, 1}; nthres in [1, 4] thresholds, each >= +0 and finite (calErr's `dif > THRES`).  keep_maps
 * also keeps every stage's maps (the same launch stores them).  The truth planes, the partial records, the table and
 * the snapshots are allocated on the enabling call (batch_capacity pairs, 7 + region_vote_nums stages at the most).
 * Stage list, from the settings as they are when the run starts, under the reference's names:
 *   "so" | "vmTop" (sm_vmtop_config on, optimiser not "so") | "wta" ("sgm" and ""): DP[0] as dispOptimize left it;
 *   with do_refine: "od" (after the LR check, either form), "PKR" (do_pkr), "RV0" .. "RV{k-1}" (do_region_vote,
 *   k = region_vote_nums), "pi" (do_proper_ipol, once after the last round), "BG" (do_bg_ipol, also at depth 0),
 *   "da" (the discontinuity adjustment), "mb" (do_last_median_blur).
 * The reference's "se" and the "mb" after it read the int16 map as floats (cpp:1487, 1492): undefined, left out.
 * sm_run records every stage; sm_disp_optimize records stage 0 and sm_refine the rest.  With sm_pyramid_config the
 * table is level 0's.  sum_sq is a double sum in a fixed order that sm_eval_stage_host restates: the table
 * is bit-identical from run to run and for every sub_batch / num_streams.  PBM = (float)bad[k] / count and
 * RMS = sqrtf((float)sum_sq / count), both 0 for count == 0 (as sm_cal_err; sm_cal_err stays the reference's float
 * accumulation in raster order).  SM_EINVAL with the argument named in sm_last_error; the arguments are checked
 * without a device.  SM_ESTATE on a pyramid level context. */
SM_API sm_status sm_eval_config(sm_ctx* ctx, int32_t on, int32_t keep_maps, int32_t nthres, const float* thres);
/* Ground truth DT ([n][H][W] floats) and the region masks ([n][H][W] bytes each) of the first n pairs, host
 * pointers; a NULL mask is an absent region (count 0: the reference's `continue`).  The masks are packed into one
 * byte per pixel, bit r set where mask_r == 255.  Synchronous, ordered like sm_upload_batch; the truth stays until
 * the next call.  A run of n pairs with evaluation on and fewer than n truth planes returns SM_ESTATE. */
SM_API sm_status sm_upload_truth(sm_ctx* ctx, int32_t n, const float* gt, const uint8_t* nonocc, const uint8_t* all,
                                 const uint8_t* disc);
/* The stages of the last run (before any run: what the next sm_run would record); NULL for a stage out of range. */
SM_API int32_t sm_eval_stage_count(const sm_ctx* ctx);
SM_API const char* sm_eval_stage_name(const sm_ctx* ctx, int32_t stage);
/* The table of the first n pairs of the last run, [n][stages][3], and (keep_maps) one stage's maps, [n][H][W]; both
 * synchronise like sm_download_disp.  SM_ESTATE before any run with evaluation on. */
SM_API sm_status sm_get_stage_errors(sm_ctx* ctx, int32_t n, sm_stage_err* out);
SM_API sm_status sm_get_stage_maps(sm_ctx* ctx, int32_t n, int32_t stage, int16_t* out);
/* The device's arithmetic on the host, in the same order, for one rows x cols map: `region` is the packed byte
 * plane (bit r = region r).  Defines sum_sq bit for bit; needs no device. */
SM_API void sm_eval_stage_host(const int16_t* disp, const float* gt, const uint8_t* region, int32_t rows, int32_t cols,
                               int32_t nthres, const float* thres, sm_stage_err out[3]);

/* Diagnostics used by the parity tests. */
/* CBCA's double window: pair 0's arm_Mask of the last sm_cost_calculate / sm_run, rows x cols bytes (1 where
 * vm[view] holds the window-1 costs). */
SM_API sm_status sm_get_cbca_dw_mask(sm_ctx* ctx, uint8_t* dst);
/* CBCA without arm intersection: pair 0's per-pixel support area of view `view` after the last iteration of the
 * last sm_cost_calculate / sm_run, rows x cols int32.  SM_ESTATE before that, or with intersection on. */
SM_API sm_status sm_get_cbca_area(sm_ctx* ctx, int32_t view, int32_t* dst);
/* "GFNL": pair 0's arm_Mask of the last sm_cost_calculate / sm_run, rows x cols bytes (1 where the variance
 * is below the threshold, i.e. where vm[0] is NL's value alone). */
SM_API sm_status sm_get_gfnl_mask(sm_ctx* ctx, uint8_t* dst);
/* The discontinuity adjustment's image stages on a supplied rows x cols 8-bit image, with sm_refine_da_config's
 * thresholds and taps: the image enters at first_stage 0 (equalizeHist), 1 (GaussianBlur) or 2 (Canny); out_eq,
 * out_blur and out_edges receive the stages' outputs (rows x cols bytes each).  NULL outputs are skipped, and so
 * are the outputs of stages before first_stage.  Uses pair 0's scratch: sm_get_da_edges gives SM_ESTATE after it
 * until the next refine. */
SM_API sm_status sm_da_run_image(sm_ctx* ctx, const uint8_t* src_u8, int32_t first_stage, uint8_t* out_eq,
                                 uint8_t* out_blur, uint8_t* out_edges);
/* The following sm_refine / sm_run calls use this rows x cols edge map (non-zero = edge) for every pair instead of
 * running the image stages; NULL returns to Canny's. */
SM_API sm_status sm_set_da_edges(sm_ctx* ctx, const uint8_t* edges);
/* "AWS": OpenCV's 8-bit BGR2Lab on the host (no device needed) with the tables the kernels use:
 * npix packed BGR pixels -> npix packed (L, a, b); and the H x W x 3 plane the device computed for
 * pair 0's image `view` in the last sm_cost_calculate / sm_run. */
SM_API void sm_bgr2lab_host(const uint8_t* bgr, size_t npix, uint8_t* lab);
SM_API sm_status sm_get_aws_lab(sm_ctx* ctx, int32_t view, uint8_t* dst);
SM_API float sm_expf_host(float x);   /* the device expf algorithm, evaluated on the host */
/* Device expf over the float bit patterns [first_bits, first_bits + n) into host out[n]. */
SM_API sm_status sm_expf_device_range(sm_ctx* ctx, uint32_t first_bits, uint32_t n, float* out);
SM_API sm_status sm_get_census(sm_ctx* ctx, int32_t view, uint64_t* dst); /* H*W*2 words */
/* CBCA's area division (div_area, sm_device.h) against IEEE division on the device: every
 * dividend mantissa at binary exponent `exp2` (a in [2^exp2, 2^(exp2+1))) for every divisor
 * 1 <= b <= bmax; *mismatches receives the number of differing results. */
SM_API sm_status sm_div_area_check(sm_ctx* ctx, int32_t exp2, int32_t bmax, uint64_t* mismatches);
/* Measured HBM ceiling: a dwordx4 copy between two fresh device buffers of `bytes`
 * each (rounded down to 16 KiB) on the ctx's device and stream, at three grid sizes, `reps` timed
 * launches each; GB/s counts read + write bytes.  Best and median over the samples. */
SM_API sm_status sm_copy_ceiling(sm_ctx* ctx, uint64_t bytes, int32_t reps, double* best_gbs, double* median_gbs);

#ifdef __cplusplus
}
#endif
#endif /* SM_CAPI_H */
