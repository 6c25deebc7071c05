// sm_validate.cpp — what a parameter set means, on the host alone (no HIP runtime call): the predicates on
// sm_params and on a context's feature settings, the proofs that license the kernels' shortcuts (bf_exact,
// cbca_div_safe, dw_int_threshold), validate, the defaults, the status strings and the cost look-up tables.
#include <math.h>
#include <string.h>

#include <cmath>

#include "sm_ctx.h"

int census_len(const sm_params& p) { return (2 * p.census_rv + 1) * (2 * p.census_ru + 1) + (p.census_ring ? 8 : 0); }

// the measures of sm_cost_ext.hip (SD .. ADCensusGrad) and, among them, those with a gradient term
bool cost_ext(const sm_params& p) { return p.cost_method >= SM_COST_SD; }
static bool cost_has_grad_ext(const sm_params& p) {
    return p.cost_method == SM_COST_GRAD || p.cost_method == SM_COST_AD_GRAD || p.cost_method == SM_COST_AD_CENSUS_GRAD;
}
static const char* cost_name(int m) {
    static const char* const names[] = {"censusGrad", "Census", "ADCensus", "AD", "SD", "BT", "grad", "?", "TruncAD", "adGrad",
                                        "ADCensusGrad"};
    return m >= 0 && m <= SM_COST_AD_CENSUS_GRAD ? names[m] : "?";
}
bool needs_census(const sm_params& p) {
    return cost_ext(p) ? p.cost_method == SM_COST_AD_CENSUS_GRAD : p.cost_method != SM_COST_AD;
}
bool needs_arms(const sm_params& p) {
    // grad() builds the arms for its adaptive weights (cpp:630-633)
    return p.cost_method == SM_COST_CENSUS_GRAD || cost_has_grad_ext(p) || p.aggregation == SM_AGG_CBCA ||
           p.do_refine;  // + regionVote (cpp:1393-1396)
}
// "so" runs on both views when Do_LRConsis (num = Do_LRConsis ? 2 : 1, cpp:1093, Do_LRConsis = 1,
// h:72; imgNum = Do_LRConsis ? 2 : 1 in costCalculate, cpp:952), so DP[1] = so(vm[1]) needs the
// right cost volume even without Do_refine
static bool so_views2(const sm_params& p) { return p.optimization == SM_OPT_SO && p.lr_consis; }
bool right_view(const sm_params& p) { return p.compute_right_view || p.do_refine || so_views2(p); }
int n_views(const sm_params& p) { return p.do_refine ? 2 : 1; }   // imgNum = Do_refine && Do_LRConsis ? 2 : 1
// views dispOptimize runs on: sgm / WTA num = Do_refine && Do_LRConsis ? 2 : 1 (cpp:1054, 1110);
// so num = Do_LRConsis ? 2 : 1 (cpp:1093) -- on vm[1] as costCalculate left it (CBCA and
// SolveAll touch vm[1] only with Do_refine, cpp:5592, 2178)
int opt_views(const sm_params& p) { return p.optimization == SM_OPT_SO ? (p.lr_consis ? 2 : 1) : n_views(p); }

// "GFNL" runs GF's and NL's code with their parameters and buffers
bool uses_gf(const sm_params& p) { return p.aggregation == SM_AGG_GF || p.aggregation == SM_AGG_GFNL; }
bool uses_nl(const sm_params& p) { return p.aggregation == SM_AGG_NL || p.aggregation == SM_AGG_GFNL; }

// "BF" keeps every cost >= +0 (as the SGM / WTA / so minima on bit patterns assume) because its
// sums are exact: every cost is 0 or a multiple of 2^-25 below 2^10, so a double holds
// any sum of <= 1024 of them.  Census costs are integers <= 136; AD costs are fl(s / 3), s <= 765
// an integer (0 or in [1/3, 255]: multiples of 2^-25), or ad_trunc_ad itself, which must then be
// such a multiple too; censusGrad and ADCensus costs are fl(t - e) with t = fl(2 - e0) in [1, 2] a
// multiple of 2^-23 and e in [0, 1]: a result >= 1/2 has ulp >= 2^-24, a smaller one has e > 1/2,
// a multiple of 2^-24, and is exact.  SD costs are fl(s / 3), s <= 195075 (0 or in [1/3, 2^16): multiples of
// 2^-25; their sums of <= 1024 stay below 2^26, 51 bits above 2^-25) or ad_trunc_ad, under AD's rule; BT costs
// are multiples of 1/2 <= 20, TruncAD costs integers <= 60.  The measures with a gradient term (grad, adGrad,
// ADCensusGrad) have no such proof.
bool bf_exact(const sm_params& p) {
    if (cost_has_grad_ext(p)) return false;
    if (p.cost_method != SM_COST_AD && p.cost_method != SM_COST_SD) return true;
    const float t = p.ad_trunc_ad;
    return t <= 1024.0f && std::ldexp(t, 25) == std::floor(std::ldexp(t, 25));
}

int cbca_lag(const sm_params& p) { return p.arm_l_out > p.arm_min_l ? p.arm_l_out : p.arm_min_l; }
// the double window's second arm set (window 1): its own maximum arm length
int cbca_lag2(const sm_ctx* c) { return c->dw_l_out > c->p.arm_min_l ? c->dw_l_out : c->p.arm_min_l; }
// cbca_core's iteration count: the double-window branch passes a literal 2 (cpp:4344, 4347) and never
// reads cbca_iterations
int cbca_iters(const sm_ctx* c) { return c->dw_on ? 2 : c->p.cbca_iterations; }
// refine()'s calPKR / subpixelEnhancement are on: they read vm[0] after dispOptimize
bool refine_reads_volume(const sm_ctx* c) { return c->p.do_refine && (c->rx_pkr || c->rx_se || c->da_on); }

// sm_refine_outlier_config's arguments against the context's parameters: the offending argument, named, or null.
// No stage behind the call reads a volume, so every optimiser is allowed ("so" included).
const char* outlier_config_error(const sm_params& p, int classify, int disp_mis, int rv_combine, int interpolate_type) {
    if (!p.do_refine) return "sm_refine_outlier_config: the context has do_refine = 0 (refine() never runs)";
    if (classify != 0 && classify != 1) return "classify must be 0 or 1 (LRConsistencyCheck instead of LRConsistencyCheck_normal)";
    if (rv_combine != 0 && rv_combine != 1) return "rv_combine must be 0 or 1 (RV_combine_BG instead of regionVote_my)";
    if (disp_mis < -32767 || disp_mis > -1) return "disp_mis must be in [-32767, -1] (DISP_MIS)";
    if (disp_mis == p.disp_occ) return "disp_mis must differ from disp_occ (the two classes share no label)";
    if (interpolate_type < 0 || interpolate_type > 3) return "interpolate_type must be in [0, 3] (interpolateType)";
    return nullptr;
}

// combine2Vm_4's predicate on the nine-term sum s of integer arm maxima is boxFilter's (float)(s * (1.0 / 9))
// (double sums, one rounding) < thres.  The product and its rounding are non-decreasing in s, so for every
// finite thres the predicate is `s < t` with t the first sum that fails it; the scan covers every sum the arm
// kernel can produce (arms <= 84: s <= 756) and so is the proof of the equivalence for the threshold at hand.
// The reference's 5.0f gives 45: s = 45 yields exactly 5.0f and is not selected.
int dw_int_threshold(float thres) {
    int t = 0;
    while (t <= 9 * 84 && (float)((double)t * (1.0 / 9)) < thres) t++;
    return t;
}

// Every dividend of iteration k's normalisation (genfinalVm_cbca, cpp:3969-3992) is 0 or
// >= 2^-110, so the area division needs no check for tiny dividends (sm_device.h div_area)?
// Costs are 0 or >= 2^f0: censusGrad / ADCensus fl(fl(2 - e0) - e1) with e0, e1 in [0, 1] is 0
// or >= 2^-24 (fl(2 - e0) = 1 gives 1 - e1 >= 2^-24 unless e1 = 1, else >= 1 + 2^-23 - 1);
// Census costs are integers; AD costs are 0 or >= min(1/3, trunc).  A prefix sum of values 0 or
// >= 2^f is 0 or >= 2^f, and a difference of two such sums is 0, the larger sum, or >= ulp(2^f)
// = 2^(f - 23); so iteration k's scan outputs are 0 or >= 2^(f_k - 23), its normalisation's
// dividends 0 or >= 2^(f_k - 46), and its quotients (areas < 2^15) 0 or >= 2^(f_k - 61) = f_{k+1}.
bool cbca_div_safe(const sm_params& p, int k) {
    int f0;
    if (p.cost_method == SM_COST_CENSUS_GRAD || p.cost_method == SM_COST_AD_CENSUS) {
        f0 = -24;
    } else if (p.cost_method == SM_COST_CENSUS) {
        f0 = 0;
    } else if (p.cost_method == SM_COST_AD) {   // AD: min(s / 3, trunc)
        if (p.ad_trunc_ad == 0.0f) return true;   // every cost is 0
        const float m = std::min(1.0f / 3.0f, p.ad_trunc_ad);
        f0 = std::ilogb(m);
    } else if (p.cost_method == SM_COST_SD) {   // SD: min(s / 3, trunc), s an integer
        if (p.ad_trunc_ad == 0.0f) return true;
        f0 = std::ilogb(std::min(1.0f / 3.0f, p.ad_trunc_ad));
    } else if (p.cost_method == SM_COST_BT) {   // multiples of 1/2
        f0 = -1;
    } else if (p.cost_method == SM_COST_TRUNC_AD) {   // integers
        f0 = 0;
    } else {
        return false;   // a cost method without a proof keeps the IEEE fallback
    }
    return f0 - 61 * k - 46 >= -110;
}

static bool nonneg(float x) { return x >= 0 && !std::signbit(x); }   // >= +0 (rejects NaN and -0.0)

// so_float_minima (sm_create_opts): the scan-line optimisers then take float minima, defined for signed and NaN
// costs, so the four refusals of "so" after GF, GFNL and inexact BF fall away; nothing else changes
sm_status validate(const sm_params& p, std::string& why, bool so_float_minima) {
    const bool so_unsigned = p.optimization == SM_OPT_SO && !so_float_minima;   // k_so's minima on bit patterns
    auto bad = [&](const char* m) { why = m; return SM_EINVAL; };
    if (p.rows < 2 || p.cols < 2) return bad("rows and cols must be >= 2 (calGrad reads I[1] and I[w-2])");
    if ((long long)p.rows * p.cols > (1LL << 30)) return bad("rows*cols too large");
    if (p.rows > 65535) return bad("rows must be <= 65535");
    if (p.num_disparities < 1 || p.num_disparities > 1024) return bad("num_disparities must be in [1, 1024]");
    // (7 is reserved: "ZNCC", whose reference output is undefined on a border frame)
    if (p.cost_method < 0 || p.cost_method > SM_COST_AD_CENSUS_GRAD || p.cost_method == 7) return bad("unknown cost_method");
    if (p.aggregation < 0 || p.aggregation > SM_AGG_GFNL || p.aggregation == 4 || p.aggregation == 6 || p.aggregation == 8)
        return bad("unknown aggregation");   // (4, 6, 8: reserved)
    if (p.aggregation == SM_AGG_BF) {
        // the default 12 x 12 window (anchor 6) with one REFLECT_101 reflection
        if (p.rows < 7 || p.cols < 7) return bad("aggregation BF needs rows, cols >= 7 (12 x 12 box, reflected border)");
        if (so_unsigned && cost_has_grad_ext(p)) {
            const std::string msg = std::string("aggregation BF with optimization so is not supported for cost_method ") + cost_name(p.cost_method) +
                  " (its box sums are not exact, so a filtered cost may be -0)";
            return bad(msg.c_str());
        }
        if (so_unsigned && !bf_exact(p))
            return bad("aggregation BF with optimization so needs ad_trunc_ad a multiple of 2^-25 and <= 1024 (exact sums)");
    }
    if (p.aggregation == SM_AGG_GFNL) {
        if (p.gf_mode != SM_GF_XIMGPROC && p.gf_mode != SM_GF_MY_GUIDE)
            return bad("aggregation GFNL: gf_mode must be 0 (ximgproc::guidedFilter) or 1 (MY_GUIDE)");
        if (p.gf_mode == SM_GF_MY_GUIDE && (p.rows < 19 || p.cols < 19))
            return bad("aggregation GFNL (MY_GUIDE) needs rows, cols >= 19 (box radius 9)");
        // the variance plane's 19 x 19 box with REFLECT_101 (one reflection); covers GF's >= 9 and NL's >= 3
        if (p.rows < 10 || p.cols < 10) return bad("aggregation GFNL needs rows, cols >= 10 (19 x 19 variance box, reflected border)");
        if (so_unsigned) return bad("aggregation GFNL (costs may be negative) supports optimization sgm or WTA");
        if (!(p.gf_eps > 0)) return bad("aggregation GFNL: gf_eps must be > 0");
        if (!(p.nl_sigma > 0)) return bad("aggregation GFNL: nl_sigma must be > 0");
        if (4.0 * (double)p.rows * (double)p.cols * (double)(p.batch_capacity > 0 ? p.batch_capacity : 1) >= 2147483647.0)
            return bad("aggregation GFNL: rows * cols * batch_capacity must stay below 2^29");
    }
    if (p.aggregation == SM_AGG_AWS) {   // the kernels' 32-bit offsets inside a volume row and a weight row
        if (p.cols > (1 << 21) || (long long)p.cols * p.num_disparities >= (1LL << 29))
            return bad("aggregation AWS needs cols <= 2^21 and cols * num_disparities < 2^29");
    }
    if (p.aggregation == SM_AGG_FIF) {
        if (p.fif_mode != SM_FIF_IMPROVE && p.fif_mode != SM_FIF_PLAIN)
            return bad("fif_mode must be 0 (FIF_Improve) or 1 (FIF, the plain form)");
        if (!(p.fif_eps > 0)) return bad("fif_eps must be > 0");
        // the sweeps keep every cost >= +0 (as SGM's and so's minima assume) only with Pn >= +0
        if (!nonneg(p.fif_pn)) return bad("fif_pn must be >= +0");
    }
    if (p.aggregation == SM_AGG_GF) {
        if (p.gf_mode != SM_GF_XIMGPROC && p.gf_mode != SM_GF_MY_GUIDE)
            return bad("gf_mode must be 0 (ximgproc::guidedFilter) or 1 (MY_GUIDE)");
        // MY_GUIDE: BoxFilter's windows need 2 r + 1 = 19 rows and columns (cpp:5156 asserts only
        // >= r, and reads outside the image below 2 r + 1); ximgproc: the reflected border of a
        // radius-9 box needs >= 9 (one reflection)
        if (p.gf_mode == SM_GF_MY_GUIDE && (p.rows < 19 || p.cols < 19))
            return bad("aggregation GF (MY_GUIDE) needs rows, cols >= 19 (box radius 9)");
        if (p.gf_mode == SM_GF_XIMGPROC && (p.rows < 9 || p.cols < 9))
            return bad("aggregation GF (ximgproc) needs rows, cols >= 9 (box radius 9, reflected border)");
        // the "so" optimiser's minima assume costs >= 0
        if (so_unsigned) return bad("aggregation GF (costs may be negative) supports optimization sgm or WTA");
        if (!(p.gf_eps > 0)) return bad("gf_eps must be > 0");
    }
    if (p.aggregation == SM_AGG_NL) {
        if (!(p.nl_sigma > 0)) return bad("nl_sigma must be > 0");
        // ctmf's 3x3 median asserts width >= 3 and height >= 3 (NL/ctmf.c:211-212).  That is not its whole
        // domain as mst() calls it (r = 1, memsize = rows * cols * 3, qx_mst_kruskals_image.cpp:174): the
        // stripe count divides by memsize / sizeof(Histogram) - 2 r in unsigned arithmetic (ctmf.c:414,
        // sizeof(Histogram) = 544), which is 0 for 363 <= rows * cols <= 543.  There the reference, built with
        // assertions, aborts at ctmf.c:211 (measured with the reference's own code, tests/test_ref_nl.py); built
        // without, it does not return.  Below 363 px the wrap-around yields one stripe and the filter works;
        // from 544 px it works as designed.  Inside the window this library (and the oracle) return the plain
        // clamped 3x3 median the reference gives everywhere else -- behaviour the reference does not have;
        // the sizes stay accepted.
        if (p.rows < 3 || p.cols < 3) return bad("aggregation NL needs rows, cols >= 3 (ctmf median)");
        // the GPU tree walk indexes the batch's tour arcs (4 per pixel) with 32-bit ints
        if (4.0 * (double)p.rows * (double)p.cols * (double)(p.batch_capacity > 0 ? p.batch_capacity : 1) >= 2147483647.0)
            return bad("aggregation NL: rows * cols * batch_capacity must stay below 2^29");
    }
    if (p.optimization < 0 || p.optimization > 2) return bad("unknown optimization");
    if (p.census_rv < 0 || p.census_ru < 0 || census_len(p) > 128) return bad("census code longer than 128 bits");
    if (p.arm_l_out < 0 || p.arm_l_out > 84 || p.arm_min_l < 0 || p.arm_min_l > 84 || p.arm_l < 0)
        return bad("arm lengths must be in [0, 84]");
    if (p.cbca_iterations < 0 || p.cbca_iterations > 64) return bad("cbca_iterations must be in [0, 64]");
    if (p.sgm_paths < 1 || p.sgm_paths > 8) return bad("sgm_paths must be in [1, 8]");
    if (p.sgm_redu_coeff == 0) return bad("sgm_redu_coeff must be non-zero");
    if (p.batch_capacity < 1) return bad("batch_capacity must be >= 1");
    if (p.sub_batch < 0 || p.num_streams < 0 || p.num_streams > 4) return bad("sub_batch >= 0 and num_streams in [0, 4] required");
    if (p.fuse_norm_scan < -1 || p.fuse_norm_scan > 1) return bad("fuse_norm_scan must be -1 (auto), 0 or 1");
    if (p.fuse_cost_scan < -1 || p.fuse_cost_scan > 1) return bad("fuse_cost_scan must be -1 (auto), 0 or 1");
    if (p.placement_trials < -1 || p.placement_trials > 8) return bad("placement_trials must be in [-1, 8]");
    // The kernels rely on every cost and path cost being >= +0 (SGM and WTA minima compare float
    // bit patterns as unsigned integers, sm_device.h), which these constants guarantee: fusion
    // terms 2 - exp(-C / lam) - exp(-G / lam) with C, G >= 0, truncations >= 0, P1, P2 >= 0.
    if (!(p.lam_cen > 0) || !(p.lam_g > 0) || !(p.lam_ad > 0) || !(p.lam_cen_adc > 0))
        return bad("fusion lambdas must be > 0");
    // -0.0 passes `>= 0` but its bit pattern 0x80000000 ranks above every positive cost in those
    // unsigned minima (the reference's std::min would treat it as 0), so it is rejected as well.
    // (GF, GFNL and inexact BF run SGM's float-minimum variants instead, which take costs of either
    // sign and volumes whose pixels are NaN at every disparity: sm_sgm.hip, keep_nan.)
    if (!nonneg(p.grad_trunc) || !nonneg(p.ad_trunc_adc) || !nonneg(p.ad_trunc_ad)) return bad("truncations must be >= +0");
    if (!nonneg(p.sgm_p1) || !nonneg(p.sgm_p2) || p.sgm_redu_coeff < 0) return bad("SGM penalties must be >= +0");
    if (p.do_refine) {
        if (!(p.rv_ratio > 0)) return bad("rv_ratio must be > 0");
        if (p.disp_occ == -32768) return bad("disp_occ = -32768 is reserved (properIpol's outside-the-image mark)");
        if (p.region_vote_nums < 0 || p.region_vote_nums > 64) return bad("region_vote_nums must be in [0, 64]");
    }
    return SM_OK;
}

void build_luts(sm_ctx* c) {
    const sm_params& p = c->p;
    for (int i = 0; i < 1024; i++) {
        c->lut_a[i] = 0;
        c->lut_b[i] = 0;
    }
    if (p.cost_method == SM_COST_CENSUS_GRAD) {
        for (int i = 0; i < 1024; i++) c->lut_a[i] = expf(-(float)i / p.lam_cen);    // cpp:3585, ARU0 = lamCen
    } else if (p.cost_method == SM_COST_AD_CENSUS) {
        for (int i = 0; i < 1024; i++) c->lut_a[i] = expf(-(float)i / p.lam_cen_adc); // census term, ARU1 = 30
        for (int s = 0; s < 1024; s++) {
            float ad = (float)s / 3;  // sum / channels (cpp:2504)
            if (p.ad_trunc_adc < ad) ad = p.ad_trunc_adc;
            c->lut_b[s] = expf(-ad / p.lam_ad);                                        // AD term, ARU0 = 10
        }
        c->ad_oor_exp = expf(-p.ad_trunc_adc / p.lam_ad);
    }
}

extern "C" {

void sm_create_opts_default(sm_create_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(sm_create_opts);
    o->so_float_minima = 0;
}

void sm_params_default(sm_params* p, int32_t max_disp, int32_t rows, int32_t cols) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(sm_params);
    p->rows = rows;
    p->cols = cols;
    p->num_disparities = max_disp + 1;  // h:209
    p->cost_method = SM_COST_CENSUS_GRAD;
    p->aggregation = SM_AGG_CBCA;
    p->optimization = SM_OPT_SGM;
    p->census_rv = 3;   // cpp:815
    p->census_ru = 4;
    p->census_ring = 1; // censusFunc = 3 (h:244)
    p->lam_cen = 13.0f;
    p->lam_g = 1.0f;
    p->grad_trunc = 500.0f;
    p->grad_adaptive = 1;
    p->lam_ad = 10.0f;
    p->lam_cen_adc = 30.0f;
    p->ad_trunc_adc = 1000.0f;
    p->ad_trunc_ad = 20.0f;
    p->arm_l = 17;
    p->arm_l_out = 34;
    p->arm_c_thresh = 20;
    p->arm_c_thresh_out = 6;
    p->arm_min_l = 1;
    p->cbca_iterations = 2;
    p->sgm_paths = 4;
    p->sgm_p1 = 1.0f;
    p->sgm_p2 = 3.0f;
    p->sgm_cor_dif_thres = 15;
    p->sgm_redu_coeff = 4;
    p->compute_right_view = 0;
    p->keep_final_volume = 0;
    p->batch_capacity = 1;
    p->do_refine = 0;           // h:70
    p->lr_max_diff = 0.0f;      // h:212
    p->do_region_vote = 1;      // h:75
    p->region_vote_nums = 2;    // h:306
    p->rv_ratio = 0.4f;         // cpp:1400
    p->rv_s = 20;               // cpp:1401
    p->do_proper_ipol = 1;      // h:76
    p->disp_occ = -2 * 16;      // h:216
    p->do_last_median_blur = 1; // h:80
    p->sub_batch = 0;
    p->num_streams = 0;        // auto (see sm_capi.h)
    p->fuse_norm_scan = -1;   // auto: fused where the lag-34 sweep applies or for volumes >= 256 MiB per pair
    p->fuse_cost_scan = -1;   // auto (see sm_capi.h)
    p->gf_eps = 0.0001f;        // gf_eps[0] = 1e-4 (h:298; guidedFilter / guideFilterCore_matlab, cpp:4509-4513)
    p->gf_mode = SM_GF_XIMGPROC;  // `//#define MY_GUIDE` (h:38): the shipped build calls ximgproc::guidedFilter
    p->nl_sigma = 0.1;          // NLCCA::aggreCV (NL/NLCCA.cpp:33)
    p->lr_consis = 1;           // Do_LRConsis (h:72)
    p->placement_trials = -1;   // auto (see sm_capi.h)
    p->fif_mode = SM_FIF_IMPROVE;   // costCalculate calls FIF_Improve (cpp:1010-1012)
    p->fif_eps = 0.08f;         // cpp:4713
    p->fif_pn = 2.0f;           // cpp:4714
}

const char* sm_status_string(sm_status s) {
    // (a C caller may pass any int: read the bits, never an out-of-range enum value)
    int32_t v;
    static_assert(sizeof(v) == sizeof(s), "sm_status is an int");
    memcpy(&v, &s, sizeof v);
    switch (v) {
        case SM_OK: return "ok";
        case SM_EINVAL: return "invalid argument";
        case SM_ENOMEM: return "out of memory";
        case SM_EHIP: return "HIP runtime error";
        case SM_ESTATE: return "call out of order";
    }
    return "unknown status";
}

}  // extern "C"
