// sm_eval_host.cpp — the host side of the per-stage error table (sm_eval_config): the stage list, the entry points,
// the launches that run_optimize and run_refine place at the stage boundaries, and sm_eval_stage_host, the kernels'
// arithmetic on the host (sm_eval_core.h).  The kernels are in sm_eval.hip.
#include <math.h>
#include <stdlib.h>

#include "sm_ctx.h"

// Where the reference calls saveFromDisp<short, 0> (cpp:1102, 1131, 1373-1501), under its names.  stage0: DP[0] as
// dispOptimize left it; refine: refine()'s stages, in its order.  run_refine's hooks follow the same conditions.
std::vector<std::string> eval_stage_names(const sm_ctx* c, bool stage0, bool refine) {
    const sm_params& p = c->p;
    std::vector<std::string> v;
    if (stage0) v.push_back(p.optimization == SM_OPT_SO ? "so" : (c->vt_on ? "vmTop" : "wta"));
    if (!refine) return v;
    v.push_back("od");
    if (c->rx_pkr) v.push_back("PKR");
    if (p.do_region_vote)
        for (int i = 0; i < p.region_vote_nums; i++) v.push_back("RV" + std::to_string(i));
    if (p.do_proper_ipol) v.push_back("pi");
    if (c->rx_bg) v.push_back("BG");
    if (c->da_on) v.push_back("da");
    if (p.do_last_median_blur) v.push_back("mb");
    return v;
}

sm_status eval_begin(sm_ctx* c, int n, bool stage0, bool refine) {
    if (!c->ev_on) return SM_OK;
    if (c->ev_truth_n < n)
        return fail(c, SM_ESTATE, "evaluation is on and " + std::to_string(c->ev_truth_n) + " truth planes are loaded for " +
                                      std::to_string(n) + " pairs: call sm_upload_truth first");
    if (stage0) {
        c->ev_names = eval_stage_names(c, true, refine);
    } else {
        if (c->ev_names.empty())
            return fail(c, SM_ESTATE, "sm_refine: evaluation was switched on after sm_disp_optimize (stage 0 is not recorded)");
        c->ev_names.resize(1);
        for (const std::string& s : eval_stage_names(c, false, true)) c->ev_names.push_back(s);
    }
    if ((int)c->ev_names.size() > c->ev_smax) return fail(c, SM_ESTATE, "evaluation: more stages than the table holds");
    c->ev_n = n;
    c->ev_kept = c->ev_keep;
    return SM_OK;
}

// One stage boundary: the group's maps `map` against the truth, into the partial records of `stage` (and, with
// keep_maps, into the stage's snapshots).  The map is read once.
sm_status run_eval_stage(sm_ctx* c, const Group& G, int stage, const int16_t* map) {
    if (stage < 0 || stage >= c->ev_smax) return fail(c, SM_ESTATE, "evaluation: stage index outside the table");
    sm::EvalArgs a{};
    a.disp = map;
    a.gt = G.slice(c->ev_gt, c->npix);
    a.reg = G.slice(c->ev_reg, c->npix);
    a.snap = c->ev_keep ? G.slice(c->ev_snap + (size_t)stage * c->ev_snap_stride, c->npix) : nullptr;
    a.npix = c->npix;
    a.nblk = c->ev_nblk;
    a.part_pair = (size_t)c->ev_smax * sm::EVAL_REGIONS * c->ev_nblk;
    a.part = G.slice(c->ev_part, a.part_pair);
    a.stage = stage;
    a.th = c->ev_th;
    const double bytes = (double)G.n * c->npix * (2 + 4 + 1 + (c->ev_keep ? 2 : 0));
    return timed(c, G.st, "eval_stage", bytes, [&] { sm::launch_eval_stage(a, G.n, G.st); });
}

// The partial records of stages [stage0, stage0 + nstages) of the group's pairs summed into the table
sm_status run_eval_final(sm_ctx* c, const Group& G, int stage0, int nstages) {
    if (nstages < 1) return SM_OK;
    const size_t per_pair = (size_t)c->ev_smax * sm::EVAL_REGIONS;
    const double bytes = (double)G.n * nstages * sm::EVAL_REGIONS * (c->ev_nblk + 1) * sizeof(sm_stage_err);
    return timed(c, G.st, "eval_final", bytes, [&] {
        sm::launch_eval_final(G.slice(c->ev_part, per_pair * c->ev_nblk), G.slice(c->ev_table, per_pair), c->ev_nblk,
                              c->ev_smax, stage0, nstages, G.n, G.st);
    });
}

static sm_status eval_alloc_truth(sm_ctx* c) {
    sm_status s;
    const size_t cap = (size_t)c->cap;
    if (!c->ev_gt && (s = dalloc(c, &c->ev_gt, cap * c->npix))) return s;
    if (!c->ev_reg && (s = dalloc(c, &c->ev_reg, cap * c->npix))) return s;
    return SM_OK;
}

extern "C" {

sm_status sm_eval_config(sm_ctx* c, int32_t on, int32_t keep_maps, int32_t nthres, const float* thres) {
    if (sm_status r = refuse_level(c)) return r;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (on < 0 || on > 1) return fail(c, SM_EINVAL, "sm_eval_config: on must be 0 or 1");
    if (keep_maps < 0 || keep_maps > 1) return fail(c, SM_EINVAL, "sm_eval_config: keep_maps must be 0 or 1");
    sm::EvalThres th = c->ev_th;
    if (on) {
        if (nthres < 1 || nthres > sm::EVAL_MAX_THRES) return fail(c, SM_EINVAL, "sm_eval_config: nthres must be in [1, 4]");
        if (!thres) return fail(c, SM_EINVAL, "sm_eval_config: thres is null");
        th = sm::EvalThres{{0.f, 0.f, 0.f, 0.f}, nthres};
        for (int k = 0; k < nthres; k++) {
            if (!(thres[k] >= 0.f) || !std::isfinite(thres[k]))
                return fail(c, SM_EINVAL, "sm_eval_config: thres[" + std::to_string(k) + "] must be >= +0 and finite");
            th.t[k] = thres[k];
        }
    }
    const bool live = c->st != nullptr;
    if (live && on) {
        sm_status s = check(c);
        if (s) return s;
        const size_t cap = (size_t)c->cap;
        c->ev_smax = 7 + std::max(c->p.region_vote_nums, 0);
        c->ev_nblk = sm::eval_blocks(c->npix);
        c->ev_snap_stride = (cap * c->npix + 7) / 8 * 8;
        const size_t slots = cap * (size_t)c->ev_smax * sm::EVAL_REGIONS;
        if ((s = eval_alloc_truth(c))) return s;
        if (!c->ev_part && (s = dalloc(c, &c->ev_part, slots * c->ev_nblk))) return s;
        if (!c->ev_table) {
            if ((s = dalloc(c, &c->ev_table, slots))) return s;
            HIP_TRY(c, hipMemsetAsync(c->ev_table, 0, slots * sizeof(sm_stage_err), c->st));
        }
        if (keep_maps && !c->ev_snap && (s = dalloc(c, &c->ev_snap, (size_t)c->ev_smax * c->ev_snap_stride))) return s;
    }
    c->ev_on = live && on;
    c->ev_keep = c->ev_on && keep_maps;
    c->ev_th = th;
    c->ev_names.clear();   // the table of an earlier run may hold other thresholds
    c->ev_n = 0;
    c->ev_kept = false;
    return SM_OK;
}

sm_status sm_upload_truth(sm_ctx* c, int32_t n, const float* gt, const uint8_t* nonocc, const uint8_t* all, const uint8_t* disc) {
    if (sm_status r = refuse_level(c)) return r;
    if (!gt) return fail(c, SM_EINVAL, "sm_upload_truth: gt is null");
    if (n < 1 || n > c->p.batch_capacity) return fail(c, SM_EINVAL, "sm_upload_truth: n must be in [1, batch_capacity]");
    sm_status s = check(c);
    if (s) return s;
    if ((s = eval_alloc_truth(c))) return s;
    const size_t count = (size_t)n * c->npix;
    uint8_t* packed = (uint8_t*)malloc(count ? count : 1);
    if (!packed) return fail(c, SM_ENOMEM, "sm_upload_truth: no host memory for the packed regions");
    sm::eval_pack_regions(count, nonocc, all, disc, packed);
    hipError_t e = hipMemcpyAsync(c->ev_gt, gt, count * sizeof(float), hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->ev_reg, packed, count, hipMemcpyHostToDevice, c->st);
    const hipError_t e2 = hipStreamSynchronize(c->st);   // (also on a failed copy: `packed` is released below)
    free(packed);
    if (e != hipSuccess || e2 != hipSuccess) return hip_fail(c, e != hipSuccess ? e : e2, "sm_upload_truth");
    c->ev_truth_n = n;
    return SM_OK;
}

int32_t sm_eval_stage_count(const sm_ctx* c) {
    if (!c) return 0;
    if (!c->ev_names.empty()) return (int32_t)c->ev_names.size();
    return (int32_t)eval_stage_names(c, true, c->p.do_refine != 0).size();
}

const char* sm_eval_stage_name(const sm_ctx* c, int32_t stage) {
    if (!c || stage < 0) return nullptr;
    if (!c->ev_names.empty()) return stage < (int32_t)c->ev_names.size() ? c->ev_names[stage].c_str() : nullptr;
    std::vector<std::string>& pv = const_cast<sm_ctx*>(c)->ev_preview;   // (the returned pointer needs a home)
    pv = eval_stage_names(c, true, c->p.do_refine != 0);
    return stage < (int32_t)pv.size() ? pv[stage].c_str() : nullptr;
}

sm_status sm_get_stage_errors(sm_ctx* c, int32_t n, sm_stage_err* out) {
    // the arguments and the state are checked before any device call
    if (sm_status r = refuse_level(c)) return r;
    if (!out || n < 1) return fail(c, SM_EINVAL, "sm_get_stage_errors: bad arguments");
    if (!c->ev_on || c->ev_names.empty())
        return fail(c, SM_ESTATE, "no error table yet (sm_eval_config, sm_upload_truth, then sm_run / sm_disp_optimize)");
    if (n > c->ev_n) return fail(c, SM_EINVAL, "sm_get_stage_errors: n exceeds the pairs of the last run");
    sm_status s = check(c);
    if (s) return s;
    const size_t row = c->ev_names.size() * sm::EVAL_REGIONS * sizeof(sm_stage_err);
    const size_t pitch = (size_t)c->ev_smax * sm::EVAL_REGIONS * sizeof(sm_stage_err);
    HIP_TRY(c, hipMemcpy2DAsync(out, row, c->ev_table, pitch, row, (size_t)n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

sm_status sm_get_stage_maps(sm_ctx* c, int32_t n, int32_t stage, int16_t* out) {
    if (sm_status r = refuse_level(c)) return r;
    if (!out || n < 1) return fail(c, SM_EINVAL, "sm_get_stage_maps: bad arguments");
    if (!c->ev_on || c->ev_names.empty() || !c->ev_kept)
        return fail(c, SM_ESTATE, "no stage maps yet (sm_eval_config with keep_maps, sm_upload_truth, then sm_run / sm_disp_optimize)");
    if (n > c->ev_n) return fail(c, SM_EINVAL, "sm_get_stage_maps: n exceeds the pairs of the last run");
    if (stage < 0 || stage >= (int32_t)c->ev_names.size()) return fail(c, SM_EINVAL, "sm_get_stage_maps: stage out of range");
    sm_status s = check(c);
    if (s) return s;
    HIP_TRY(c, hipMemcpyAsync(out, c->ev_snap + (size_t)stage * c->ev_snap_stride, (size_t)n * c->npix * sizeof(int16_t),
                              hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

void sm_eval_stage_host(const int16_t* disp, const float* gt, const uint8_t* region, int32_t rows, int32_t cols, int32_t nthres,
                        const float* thres, sm_stage_err out[3]) {
    if (!out) return;
    sm::EvalAcc z;
    sm::eval_zero(z);
    for (int r = 0; r < sm::EVAL_REGIONS; r++) out[r] = z.r[r];
    if (!disp || !gt || !region || !thres || rows < 1 || cols < 1 || nthres < 1 || nthres > sm::EVAL_MAX_THRES) return;
    sm::EvalThres th{{0.f, 0.f, 0.f, 0.f}, nthres};
    for (int k = 0; k < nthres; k++) th.t[k] = thres[k];
    sm::eval_stage_host(disp, gt, region, (size_t)rows * cols, th, out);
}

}  // extern "C"
