// sm_capi.cpp — C-ABI of libsm_hip.so: the context's life (sm_create, sm_destroy and the buffers they own),
// the entry points in the reference's StereoMatching call order (see include/sm_capi.h for the file:line of
// each reference interface), the pyramid weights, getters and setters (sm_download_subpixel among them, beside
// the stage it reads), the features' *_config calls (the aggregation-side ones over every pyramid level), the batch
// path's pyramid (sm_pyramid_config and the level contexts it owns), profiling, sm_cal_err and the diagnostics.  The batch
// path is sm_run.cpp, the stage drivers sm_stages.cpp and sm_stages_agg.cpp, parameter checks sm_validate.cpp.
// No exceptions cross the ABI.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cfloat>
#include <cmath>
#include <new>

#include "sm_ctx.h"

// The weight band of one stream: at most this many bytes, whatever the image height or the batch
// (both images' weights of as many image rows as fit; at least one row).
constexpr size_t AWS_BAND_BYTES = (size_t)256 << 20;

hipEvent_t get_event(sm_ctx* c) {
    if (!c->free_events.empty()) {
        hipEvent_t e = c->free_events.back();
        c->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int kernel_id(sm_ctx* c, const char* name, double bytes) {
    auto it = c->kidx.find(name);
    int id;
    if (it == c->kidx.end()) {
        id = (int)c->knames.size();
        c->kidx[name] = id;
        c->knames.push_back(name);
        c->kstat.emplace_back();
    } else {
        id = it->second;
    }
    c->kstat[id].bytes = bytes;
    return id;
}

namespace {

// The padded layout of an arm-plane set for CBCA sweeps of the given lag: front pad (V sweeps read rows
// i - lag >= -2 lag), the planes [cap][2 views][2 planes][npix] u32, tail pad (the fast V sweep's arm loads run
// up to lag + T rows past the last plane's end; sm_cbca.hip NsV clamps later tiles).  The pads hold zero arms
// (never written later): rows the sweeps read outside the planes then give zero-length windows, so every
// window slot stays inside the rings.
sm_status alloc_arm_planes(sm_ctx* c, int lag, uint8_t** alloc, uint8_t** planes, size_t* bytes) {
    const size_t cols = (size_t)c->p.cols;
    const size_t pad = (2 * (size_t)lag * cols * 4 + 255) / 256 * 256;
    const size_t tail = (size_t)(2 * lag + 64) * cols * 4;
    *bytes = (size_t)c->cap * 2 * 2 * c->npix * 4;
    sm_status s = dalloc(c, alloc, pad + *bytes + tail);
    if (s) return s;
    *planes = *alloc + pad;
    HIP_TRY(c, hipMemset(*alloc, 0, pad));
    HIP_TRY(c, hipMemset(*planes + *bytes, 0, tail));
    return SM_OK;
}

// the getters that only copy to the host and wait, on c->st
sm_status download_sync(sm_ctx* c, void* dst, const void* src, size_t bytes) {
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

void free_all(sm_ctx* c) {
    if (c->owner) c->nl_st = nullptr;   // (a level context's NL front stream is its owner's)
    for (void* q : c->allocs) hipFree(q);
    c->allocs.clear();
    // every stream is drained and destroyed (the main stream last) before the events its work recorded or waited for
    for (hipStream_t* st : {&c->nl_st, &c->cst, &c->xst[0], &c->xst[1], &c->xst[2], &c->st})
        if (*st) {
            hipStreamSynchronize(*st);
            hipStreamDestroy(*st);
            *st = nullptr;
        }
    for (hipEvent_t e : c->events) hipEventDestroy(e);
    c->events.clear();
    if (c->nl_offs_h) {
        hipHostFree(c->nl_offs_h);
        c->nl_offs_h = nullptr;
    }
    for (auto& r : c->recs) {
        if (r.start) hipEventDestroy(r.start);
        if (r.stop) hipEventDestroy(r.stop);
    }
    for (auto e : c->free_events) hipEventDestroy(e);
    c->recs.clear();
    c->free_events.clear();
}

}  // namespace

// sm_create; with `owner`, pyramid level `level` of that context (sm_pyramid_config), which needs no map or
// refine planes beyond DP[0]'s
static sm_status create_ctx(sm_ctx** out, const sm_params* p, const sm_create_opts* opts, int32_t hip_device, sm_ctx* owner, int level) {
    if (!out || !p) return SM_EINVAL;
    *out = nullptr;
    sm_ctx* c = new (std::nothrow) sm_ctx();
    if (!c) return SM_ENOMEM;
    *out = c;  // returned even on failure so sm_last_error works; caller must sm_destroy
    c->owner = owner;
    c->level = level;
    // the options first (NULL: the defaults), before any field of sm_params is read
    if (opts) {
        if (opts->struct_size != (uint32_t)sizeof(sm_create_opts))
            return fail(c, SM_EINVAL, "sm_create_opts.struct_size != sizeof(sm_create_opts): initialise the struct with "
                                      "sm_create_opts_default from this library's sm_capi.h");
        if (opts->so_float_minima != 0 && opts->so_float_minima != 1)
            return fail(c, SM_EINVAL, "sm_create_opts.so_float_minima must be 0 or 1");
        c->so_float_minima = opts->so_float_minima == 1;
    }
    // a struct from another version of sm_capi.h (or not filled by sm_params_default) is refused
    // before any field past struct_size is read
    if (p->struct_size != (uint32_t)sizeof(sm_params))
        return fail(c, SM_EINVAL, "sm_params.struct_size != sizeof(sm_params): initialise the struct with sm_params_default "
                                  "from this library's sm_capi.h");
    c->p = *p;
    c->device = hip_device;
    if (hipDeviceGetAttribute(&c->num_cu, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess || c->num_cu < 1)
        c->num_cu = 256;
    std::string why;
    if (validate(c->p, why, c->so_float_minima) != SM_OK) return fail(c, SM_EINVAL, why);
    int ndev = 0;
    HIP_TRY(c, hipGetDeviceCount(&ndev));
    if (hip_device < 0 || hip_device >= ndev) return fail(c, SM_EINVAL, "hip_device out of range");
    HIP_TRY(c, hipSetDevice(hip_device));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c->cap = p->batch_capacity;
    c->npix = (size_t)p->rows * p->cols;
    c->nvol = c->npix * (size_t)p->num_disparities;
    const size_t cap = c->cap;
    sm_status s;
    if ((s = dalloc(c, &c->bgr, cap * 2 * c->npix * 3 + 16))) return s;   // tail pad: prep's dword quads (load_quad_bgr)
    if ((s = dalloc(c, &c->gray, cap * 2 * c->npix))) return s;
    if ((s = dalloc(c, &c->code, cap * 2 * c->npix))) return s;
    if ((s = alloc_arm_planes(c, cbca_lag(*p), &c->arms_alloc, &c->arms, &c->arms_bytes))) return s;
    // volumes carry a tail: vectorised SGM lanes past D read (never write) into it, and the fast V
    // sweep's tiles that straddle the last rows read up to CBCA_VM_TAIL_ROWS rows past them
    const size_t vpad = 1024 + (size_t)sm::CBCA_VM_TAIL_ROWS * p->cols * p->num_disparities;
    c->vtail = vpad;
    if ((s = dalloc(c, &c->vm0, cap * c->nvol + vpad))) return s;
    if (right_view(*p))
        if ((s = dalloc(c, &c->vm1, cap * c->nvol + vpad))) return s;
    if (p->optimization == SM_OPT_SGM && p->sgm_paths > 1)
        if ((s = dalloc(c, &c->acc, cap * c->nvol + vpad))) return s;
    if (p->optimization == SM_OPT_SGM && sm::sgm_ck_ok(p->num_disparities, p->sgm_paths)) {
        const size_t S = (size_t)sm::sgm_ck_seg(p->num_disparities), H = (size_t)p->rows, W = (size_t)p->cols;
        size_t lines_x_segs = std::max(H * ((W + S - 1) / S), W * ((H + S - 1) / S));
        const bool diag = sm::sgm_ck_diag_ok(p->num_disparities, p->sgm_paths);
        if (diag) {   // the diagonal pair: W + H - 1 lines, slots strided by the longest diagonal
            const size_t SD = (size_t)sm::sgm_ck_diag_seg();
            lines_x_segs = std::max(lines_x_segs, (W + H - 1) * ((std::min(H, W) + SD - 1) / SD));
        }
        c->ck_pair = lines_x_segs * (size_t)p->num_disparities;
        if ((s = dalloc(c, &c->ck, cap * c->ck_pair))) return s;
        if (diag && (s = dalloc(c, &c->lx, cap * c->nvol + vpad))) return s;
    }
    if ((s = dalloc(c, &c->disp, cap * c->npix))) return s;
    if ((s = dalloc(c, &c->dummy, 64))) return s;
    if ((s = dalloc(c, &c->flags, cap * c->npix))) return s;
    if (p->optimization == SM_OPT_SO) {
        if ((s = dalloc(c, &c->so_trace, cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->so_cidx, cap * c->npix))) return s;
    }
    if ((p->do_refine && !owner) || p->optimization == SM_OPT_SO)
        if ((s = dalloc(c, &c->disp1, cap * c->npix))) return s;
    if (p->do_refine && !owner) {
        if ((s = dalloc(c, &c->flags1, cap * c->npix))) return s;
        if ((s = dalloc(c, &c->disp_tmp, cap * c->npix))) return s;
    }
    if ((s = dalloc(c, &c->px, 3 * cap * 2 * c->npix))) return s;
    if (uses_gf(*p) && p->gf_mode == SM_GF_XIMGPROC) {
        if ((s = dalloc(c, &c->gfc_rs, 4 * cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->gfc_ab, 4 * cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->gfc_img, cap * 9 * c->npix))) return s;
        if ((s = dalloc(c, &c->gfc_pix, cap * 9 * c->npix))) return s;
    } else if (uses_gf(*p)) {
        if ((s = dalloc(c, &c->gf_s, (c->acc ? 3 : 4) * cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->gf_planes, cap * 10 * c->npix))) return s;
        if ((s = dalloc(c, &c->gf_pix, cap * c->npix))) return s;
    }
    if (p->aggregation == SM_AGG_FIF) {
        if ((s = dalloc(c, &c->fif_s, (c->acc ? 1 : 2) * cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->fif_w, 2 * cap * c->npix))) return s;
    }
    if (p->aggregation == SM_AGG_AWS) {
        if ((s = dalloc(c, &c->aws_tab, (size_t)sm::AWS_GAM_N + sm::AWS_CB_N))) return s;
        HIP_TRY(c, hipMemcpy(c->aws_tab, aws_tables(), (sm::AWS_GAM_N + sm::AWS_CB_N) * sizeof(uint16_t), hipMemcpyHostToDevice));
        if ((s = dalloc(c, &c->aws_lab, cap * 2 * c->npix * 3))) return s;
        if ((s = dalloc(c, &c->aws_raw, (size_t)n_views(*p) * cap * c->nvol))) return s;
        // the bands are sized for radius 17 (sm_aws_config may set any smaller window later)
        const size_t smax = (size_t)(2 * sm::AWS_MAX_R + 1) * (2 * sm::AWS_MAX_R + 1);
        const size_t row_bytes = 2 * smax * p->cols * 4;
        // SM_AWS_BAND_BYTES: a smaller budget (tests: images of a few rows then span several bands)
        size_t budget = AWS_BAND_BYTES;
        if (const char* e = getenv("SM_AWS_BAND_BYTES")) budget = std::min<size_t>(budget, strtoull(e, nullptr, 10));
        const size_t fit = std::max<size_t>(1, budget / row_bytes);
        c->aws_band_rows = (int)std::min<size_t>({fit, cap * (size_t)p->rows, (size_t)32767});   // (2 x rows is a grid dimension)
    }
    if (p->aggregation == SM_AGG_BF)
        if ((s = dalloc(c, &c->bf_rs, cap * c->nvol))) return s;
    if (p->aggregation == SM_AGG_GFNL) {
        if ((s = dalloc(c, &c->gfnl_res, cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->gfnl_mask, cap * c->npix))) return s;
    }
    if (uses_nl(*p)) {
        const size_t ne = (size_t)p->rows * (p->cols - 1) + (size_t)(p->rows - 1) * p->cols;
        if ((s = dalloc(c, &c->nl_med, cap * c->npix * 3))) return s;
        if ((s = dalloc(c, &c->nl_ew, cap * ne))) return s;
        if ((s = dalloc(c, &c->nl_ints, 2 * cap * c->npix * 4))) return s;
        if ((s = dalloc(c, &c->nl_rec, 2 * (cap * c->npix + 2 * sm::NL_REC_PAD) * 4))) return s;
        HIP_TRY(c, hipMemset(c->nl_rec, 0, 2 * (cap * c->npix + 2 * sm::NL_REC_PAD) * 16));
        if ((s = dalloc(c, &c->nl_table, 256))) return s;
        if ((s = dalloc(c, &c->nl_val, cap * c->nvol))) return s;
        if ((s = dalloc(c, &c->nl_oup, cap * c->npix))) return s;
        if ((s = dalloc(c, &c->nl_ofin, cap * c->npix))) return s;
        if ((s = dalloc(c, &c->nl_walk, sm::nl_walk_scratch_bytes(p->rows, p->cols, cap)))) return s;
        if ((s = dalloc(c, &c->nl_offs, 2 * (sm::NL_LEVELS + 1) + 1))) return s;
        HIP_TRY(c, hipHostMalloc((void**)&c->nl_offs_h, (2 * (sm::NL_LEVELS + 1) + 1) * sizeof(int), hipHostMallocDefault));
        if ((s = dalloc(c, &c->nl_par, cap * c->npix))) return s;
        if ((s = dalloc(c, &c->nl_best, cap * c->npix))) return s;
        if ((s = dalloc(c, &c->nl_mst, sm::nl_mst_scratch_bytes(p->rows, p->cols, cap)))) return s;
        if ((s = dalloc(c, &c->nl_adj, cap * c->npix))) return s;
        // sm_run's pipelined front (one view, SGM): two sets of cost volume and penalty flags
        c->nl_pipe = p->aggregation == SM_AGG_NL && p->optimization == SM_OPT_SGM && !right_view(*p);
        if (c->nl_pipe) {
            if ((s = dalloc(c, &c->nl_vc, 2 * cap * c->nvol + vpad))) return s;
            if ((s = dalloc(c, &c->nl_fl, 2 * cap * c->npix))) return s;
        }
        double table[256];
        const double sg = p->nl_sigma < 0.01 ? 0.01 : p->nl_sigma;   // update_table (qx_tree_filter.cpp:23-24)
        for (int i = 0; i < 256; i++) table[i] = exp(-(double)i / (255 * sg));
        HIP_TRY(c, hipMemcpy(c->nl_table, table, 256 * sizeof(double), hipMemcpyHostToDevice));
    }
    {
        const bool plain = p->aggregation == SM_AGG_CBCA && p->cbca_iterations > 0 && p->optimization == SM_OPT_SGM;
        c->place_trials = p->placement_trials >= 0 ? p->placement_trials
                                                   : (plain && c->nvol * 4 >= ((size_t)1 << 28) ? 3 : 0);
        if (!(p->aggregation == SM_AGG_CBCA || p->aggregation == SM_AGG_NONE)) c->place_trials = 0;   // (GF / NL scratch not moved)
    }
    if (getenv("SM_TRACE_ALLOC"))   // diagnostics: where the large buffers landed
        fprintf(stderr, "[alloc] vm0 %p vm1 %p acc %p arms %p code %p px %p\n", (void*)c->vm0, (void*)c->vm1,
                (void*)c->acc, (void*)c->arms, (void*)c->code, (void*)c->px);
    build_luts(c);
    {
        // auto: the generic fused sweep wins where a pair's volume is large (full resolution:
        // v_norm + v_scan 12.2 -> 11.3 ms; 1080p 16.2 -> 16.0 ms) and loses at Teddy size (0.79 ->
        // 0.82 ms); the dedicated sweep at the reference's lag (NsV, D % 64 == 0) wins at every
        // size (Teddy x16: 0.765 -> 0.692 ms, profiles/r4b/ab_teddy.txt)
        const bool nsv = cbca_lag(*p) == 34 && p->num_disparities % 64 == 0;
        c->fuse_norm_scan = p->fuse_norm_scan == 1 || (p->fuse_norm_scan == -1 && (nsv || c->nvol * 4 >= ((size_t)1 << 28)));
        // auto = on: the fused sweep beat cost volume + H scan on all four bench workloads in
        // same-process A/Bs (profiles/fuse_cost_scan/ab_*.txt: full resolution 6.30 -> 4.32 ms,
        // 1080p 6.42 -> 5.06, KITTI 0.727 -> 0.548, Teddy x16 0.404 -> 0.334 ms), so there is no shape
        // rule; cost_scan_fused decides per view whether the configuration is eligible
        c->fuse_cost_scan = p->fuse_cost_scan != 0;
        if ((s = apply_schedule(c, p->num_streams, p->sub_batch))) return s;
        if ((s = aws_alloc_bands(c))) return s;
    }
    if ((s = dalloc(c, &c->luts, 2048))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->luts, c->lut_a, sizeof(c->lut_a), hipMemcpyHostToDevice, c->st));
    HIP_TRY(c, hipMemcpyAsync(c->luts + 1024, c->lut_b, sizeof(c->lut_b), hipMemcpyHostToDevice, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

// every stream of the context idle (its levels' work runs on them too)
static void drain(sm_ctx* c) {
    for (hipStream_t st : {c->nl_st, c->cst, c->xst[0], c->xst[1], c->xst[2], c->st})
        if (st) hipStreamSynchronize(st);
}

static void destroy_levels(sm_ctx* c) {
    for (sm_ctx* q : c->levels) {
        free_all(q);
        delete q;
    }
    c->levels.clear();
}

extern "C" {

sm_status sm_create(sm_ctx** out, const sm_params* p, int32_t hip_device) { return sm_create_ex(out, p, nullptr, hip_device); }

sm_status sm_create_ex(sm_ctx** out, const sm_params* p, const sm_create_opts* opts, int32_t hip_device) {
    return create_ctx(out, p, opts, hip_device, nullptr, 0);
}

sm_status sm_destroy(sm_ctx* c) {
    if (!c) return SM_OK;
    if (c->owner) return refuse_level(c);   // (its owner destroys it)
    hipSetDevice(c->device);
    if (c->pipe_live) join_all(c);
    drain(c);
    destroy_levels(c);
    free_all(c);
    delete c;
    return SM_OK;
}

const char* sm_last_error(const sm_ctx* c) { return c ? c->err.c_str() : "null context"; }

sm_status sm_set_images(sm_ctx* c, const uint8_t* lbgr, const uint8_t* rbgr, size_t cstride, const uint8_t* lgray,
                        const uint8_t* rgray, size_t gstride) {
    sm_status s = check(c);
    if (s) return s;
    if (!lbgr || !rbgr || !lgray || !rgray) return fail(c, SM_EINVAL, "null image pointer");
    if (cstride < (size_t)c->p.cols * 3 || gstride < (size_t)c->p.cols) return fail(c, SM_EINVAL, "row stride too small");
    return upload(c, 1, lbgr, rbgr, cstride, lgray, rgray, gstride);
}

sm_status sm_cost_calculate(sm_ctx* c) {
    sm_status s = check(c);
    if (s) return s;
    if (c->stage < 1) return fail(c, SM_ESTATE, "sm_cost_calculate before sm_set_images");
    const Group G = at(c, 0, c->n_loaded, c->st);
    if ((s = run_prep(c, G))) return s;
    if ((s = run_cost(c, 0, G))) return s;
    if (right_view(c->p) && (s = run_cost(c, 1, G))) return s;
    if (c->p.aggregation == SM_AGG_CBCA)
        for (int v = 0; v < n_views(c->p); v++)
            if ((s = run_cbca(c, v, false, 1.0f, G))) return s;
    if ((s = run_other_agg(c, G))) return s;
    c->stage = 2;
    return SM_OK;
}

sm_status sm_solve_all(sm_ctx* c, int32_t py_lev, float reg_lambda) {
    sm_status s = check(c);
    if (s) return s;
    if (c->stage != 2) return fail(c, SM_ESTATE, "sm_solve_all must follow sm_cost_calculate");
    if (py_lev != 1) return fail(c, SM_EINVAL, "PY_LVL > 1 needs every level's context: use sm_solve_all_pyr");
    const float m = 1 + reg_lambda;
    const float w = (float)(1. / (double)m);  // Mat::inv of the 1x1 regMat (cpp:2164)
    for (int v = 0; v < n_views(c->p); v++)   // img_n = Do_refine ? 2 : 1 (cpp:2178)
        if ((s = run_scale(c, v, w, at(c, 0, c->n_loaded, c->st)))) return s;
    c->stage = 3;
    return SM_OK;
}

// invWgt = row 0 of regMat.inv() (cpp:2147-2168): OpenCV's invert for a CV_32F matrix of order
// n <= 3 evaluates the adjugate over the determinant in double and rounds each entry to float;
// for n > 3 Mat::inv (DECOMP_LU) runs LUImpl<float> on a copy with the identity as right-hand
// side (lu_inv_row0; OpenCV's scalar loops, each product and sum rounded, pivot failure below
// 10 * FLT_EPSILON).
static bool lu_inv_row0(int L, float (*M)[sm::kMaxPyr], float* w) {
    float B[sm::kMaxPyr][sm::kMaxPyr];
    for (int i = 0; i < L; i++)
        for (int j = 0; j < L; j++) B[i][j] = i == j ? 1.f : 0.f;
    for (int i = 0; i < L; i++) {
        int k = i;
        for (int j = i + 1; j < L; j++)
            if (std::fabs(M[j][i]) > std::fabs(M[k][i])) k = j;
        if (std::fabs(M[k][i]) < FLT_EPSILON * 10) return false;
        if (k != i) {
            for (int j = i; j < L; j++) std::swap(M[i][j], M[k][j]);
            for (int j = 0; j < L; j++) std::swap(B[i][j], B[k][j]);
        }
        const float d = -1 / M[i][i];
        for (int j = i + 1; j < L; j++) {
            const float alpha = M[j][i] * d;
            for (int q = i + 1; q < L; q++) M[j][q] += alpha * M[i][q];
            for (int q = 0; q < L; q++) B[j][q] += alpha * B[i][q];
        }
    }
    for (int i = L - 1; i >= 0; i--)
        for (int j = 0; j < L; j++) {
            float s = B[i][j];
            for (int q = i + 1; q < L; q++) s -= M[i][q] * B[q][j];
            B[i][j] = s / M[i][i];
        }
    for (int j = 0; j < L; j++) w[j] = B[0][j];
    return true;
}

extern "C++" bool pyr_weights(int L, float lam, float* w) {
    float M[sm::kMaxPyr][sm::kMaxPyr] = {};
    for (int s = 0; s < L; s++) {
        if (s == 0) {
            M[s][s] = 1 + lam;
            if (L > 1) M[s][s + 1] = -lam;
        } else if (s == L - 1) {
            M[s][s] = 1 + lam;
            M[s][s - 1] = -lam;
        } else {
            M[s][s] = 1 + 2 * lam;
            M[s][s - 1] = -lam;
            M[s][s + 1] = -lam;
        }
    }
    if (L > 3) return lu_inv_row0(L, M, w);
    if (L == 1) {
        w[0] = (float)(1. / (double)M[0][0]);
        return true;
    }
    if (L == 2) {
        double d = (double)M[0][0] * M[1][1] - (double)M[0][1] * M[1][0];
        if (d == 0.) return false;
        d = 1. / d;
        w[0] = (float)(M[1][1] * d);
        w[1] = (float)(-M[0][1] * d);
        return true;
    }
    double d = M[0][0] * ((double)M[1][1] * M[2][2] - (double)M[1][2] * M[2][1]) -
               M[0][1] * ((double)M[1][0] * M[2][2] - (double)M[1][2] * M[2][0]) +
               M[0][2] * ((double)M[1][0] * M[2][1] - (double)M[1][1] * M[2][0]);
    if (d == 0.) return false;
    d = 1. / d;
    w[0] = (float)(((double)M[1][1] * M[2][2] - (double)M[1][2] * M[2][1]) * d);
    w[1] = (float)(((double)M[0][2] * M[2][1] - (double)M[0][1] * M[2][2]) * d);
    w[2] = (float)(((double)M[0][1] * M[1][2] - (double)M[0][2] * M[1][1]) * d);
    return true;
}

sm_status sm_solve_all_pyr(sm_ctx* const* levels, int32_t py_lvl, float reg_lambda) {
    if (!levels || !levels[0]) return SM_EINVAL;
    sm_ctx* c = levels[0];
    sm_status s = check(c);
    if (s) return s;
    if (py_lvl < 1 || py_lvl > sm::kMaxPyr) return fail(c, SM_EINVAL, "PY_LVL must be in [1, 8]");
    if (py_lvl == 1) return sm_solve_all(c, 1, reg_lambda);
    sm::PyrArgs a{};
    a.levels = py_lvl;
    a.n = c->n_loaded;
    for (int l = 0; l < py_lvl; l++) {
        sm_ctx* q = levels[l];
        if (!q) return fail(c, SM_EINVAL, "null level context");
        if (q->device != c->device) return fail(c, SM_EINVAL, "pyramid levels must share one device");
        if (q->stage != 2) return fail(c, SM_ESTATE, "every level needs sm_cost_calculate (and no SolveAll yet)");
        if (q->n_loaded != c->n_loaded) return fail(c, SM_EINVAL, "pyramid levels must hold the same number of pairs");
        if (n_views(q->p) < n_views(c->p)) return fail(c, SM_EINVAL, "coarser levels need do_refine like level 0");
        if (l > 0) {
            const sm_params& pp = levels[l - 1]->p;
            if (q->p.rows != (pp.rows + 1) / 2 || q->p.cols != (pp.cols + 1) / 2)
                return fail(c, SM_EINVAL, "level sizes must follow pyrDown: ((rows + 1) / 2, (cols + 1) / 2)");
            if (q->p.num_disparities < pp.num_disparities / 2 + 1)
                return fail(c, SM_EINVAL, "level num_disparities too small for curD = (curD + 1) / 2");
        }
        a.H[l] = q->p.rows;
        a.W[l] = q->p.cols;
        a.D[l] = q->p.num_disparities;
        if (l > 0) HIP_TRY(c, hipStreamSynchronize(q->st));   // coarse volumes complete
    }
    if (!pyr_weights(py_lvl, reg_lambda, a.w)) return fail(c, SM_EINVAL, "singular regularisation matrix");
    for (int v = 0; v < n_views(c->p); v++) {
        for (int l = 0; l < py_lvl; l++) a.vm[l] = v == 0 ? levels[l]->vm0 : levels[l]->vm1;
        const double bytes = (double)a.n * c->nvol * 8.0;
        if ((s = timed(c, c->st, v == 0 ? "solve_all_pyr" : "solve_all_pyr_r", bytes, [&] { sm::launch_solve_all_pyr(a, c->st); })))
            return s;
    }
    c->stage = 3;
    for (int l = 1; l < py_lvl; l++) levels[l]->stage = 3;
    return SM_OK;
}

sm_status sm_pyr_down(int32_t dev, const uint8_t* src, int32_t rows, int32_t cols, int32_t ch, uint8_t* dst) {
    if (!src || !dst || rows < 1 || cols < 1 || (ch != 1 && ch != 3)) return SM_EINVAL;
    if (hipSetDevice(dev) != hipSuccess) return SM_EHIP;
    const size_t in = (size_t)rows * cols * ch, out = (size_t)((rows + 1) / 2) * ((cols + 1) / 2) * ch;
    uint8_t *dsrc = nullptr, *ddst = nullptr;
    hipError_t e = hipMalloc((void**)&dsrc, in);
    if (e == hipSuccess) e = hipMalloc((void**)&ddst, out);
    if (e == hipSuccess) e = hipMemcpy(dsrc, src, in, hipMemcpyDefault);
    if (e == hipSuccess) {
        sm::launch_pyr_down(dsrc, ddst, rows, cols, ch, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(dst, ddst, out, hipMemcpyDefault);
    if (dsrc) hipFree(dsrc);
    if (ddst) hipFree(ddst);
    return e == hipSuccess ? SM_OK : SM_EHIP;
}

sm_status sm_pyr_down_f32(int32_t dev, const float* src, int32_t rows, int32_t cols, float* dst) {
    if (!src || !dst || rows < 1 || cols < 1) return SM_EINVAL;
    if (hipSetDevice(dev) != hipSuccess) return SM_EHIP;
    const size_t in = (size_t)rows * cols * 4, out = (size_t)((rows + 1) / 2) * ((cols + 1) / 2) * 4;
    float *dsrc = nullptr, *ddst = nullptr;
    hipError_t e = hipMalloc((void**)&dsrc, in);
    if (e == hipSuccess) e = hipMalloc((void**)&ddst, out);
    if (e == hipSuccess) e = hipMemcpy(dsrc, src, in, hipMemcpyDefault);
    if (e == hipSuccess) {
        sm::launch_pyr_down_f32(dsrc, ddst, rows, cols, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(dst, ddst, out, hipMemcpyDefault);
    if (dsrc) hipFree(dsrc);
    if (ddst) hipFree(ddst);
    return e == hipSuccess ? SM_OK : SM_EHIP;
}

sm_status sm_disp_optimize(sm_ctx* c, int16_t* disp_out) {
    sm_status s = check(c);
    if (s) return s;
    if (c->stage < 2 || c->stage > 3) return fail(c, SM_ESTATE, "sm_disp_optimize must follow sm_cost_calculate / sm_solve_all");
    if ((s = wait_copy(c))) return s;
    if ((s = eval_begin(c, c->n_loaded, true, false))) return s;
    for (int v = 0; v < opt_views(c->p); v++)   // num (cpp:1054, 1093, 1110)
        if ((s = run_optimize(c, v, at(c, 0, c->n_loaded, c->st)))) return s;
    c->stage = 4;
    c->rx_vol_ok = true;
    if (disp_out) return sm_download_disp(c, 1, disp_out);
    return SM_OK;
}

sm_status sm_refine(sm_ctx* c, int16_t* disp_out) {
    sm_status s = check(c);
    if (s) return s;
    if (!c->p.do_refine) return fail(c, SM_ESTATE, "sm_refine needs do_refine = 1 at sm_create (DP[1] is not computed otherwise)");
    if (c->stage != 4) return fail(c, SM_ESTATE, "sm_refine must follow sm_disp_optimize");
    if (refine_reads_volume(c) && c->p.optimization == SM_OPT_SGM && !c->p.keep_final_volume && !c->vt_on && !c->rx_vol_ok)
        return fail(c, SM_ESTATE, "sm_refine: do_pkr / do_subpixel / the discontinuity adjustment were switched on after sm_disp_optimize (SGM kept no path sum)");
    if ((s = wait_copy(c))) return s;
    if ((s = eval_begin(c, c->n_loaded, false, true))) return s;
    if ((s = run_refine(c, at(c, 0, c->n_loaded, c->st)))) return s;
    c->stage = 5;
    if (disp_out) return sm_download_disp(c, 1, disp_out);
    return SM_OK;
}

sm_status sm_get_disp(sm_ctx* c, int32_t view, int16_t* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst || view < 0 || view > 1) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 4) return fail(c, SM_ESTATE, "no disparity map yet");
    const int16_t* src = view == 0 ? c->disp : c->disp1;
    if (!src) return fail(c, SM_EINVAL, "DP[1] is only computed with do_refine = 1 or optimization so");
    return download_sync(c, dst, src, c->npix * 2);
}

sm_status sm_set_disp(sm_ctx* c, int32_t view, const int16_t* src) {
    sm_status s = check(c);
    if (s) return s;
    if (!src || view < 0 || view > 1) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 4) return fail(c, SM_ESTATE, "sm_set_disp must follow sm_disp_optimize");
    if ((s = wait_copy(c))) return s;
    int16_t* dst = view == 0 ? c->disp : c->disp1;
    if (!dst) return fail(c, SM_EINVAL, "DP[1] is only allocated with do_refine = 1 or optimization so");
    HIP_TRY(c, hipMemcpyAsync(dst, src, c->npix * 2, hipMemcpyHostToDevice, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    c->stage = 4;   // refine() may run (again) on the new maps
    return SM_OK;
}

sm_status sm_get_volume(sm_ctx* c, int32_t view, float* dst) {
    sm_status s = check_any(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (c->stage < 2) return fail(c, SM_ESTATE, "no volume yet");
    float* src = view == 0 ? c->vm0 : (view == 1 ? c->vm1 : nullptr);
    if (!src) return fail(c, SM_EINVAL, view == 1 ? "right view not computed (compute_right_view = 0)" : "bad view");
    if (c->stage >= 4 && !c->p.keep_final_volume && !c->vt_on && !(view == 0 && refine_reads_volume(c) && c->rx_vol_ok) &&
        c->p.optimization == SM_OPT_SGM)
        return fail(c, SM_ESTATE, "vm[view] after SGM is only kept with keep_final_volume = 1");
    return download_sync(c, dst, src, c->nvol * 4);
}

sm_status sm_set_volume(sm_ctx* c, int32_t view, const float* src) {
    sm_status s = check(c);
    if (s) return s;
    if (!src) return fail(c, SM_EINVAL, "null src");
    if (c->stage < 2) return fail(c, SM_ESTATE, "sm_set_volume must follow sm_cost_calculate");
    float* dst = view == 0 ? c->vm0 : (view == 1 ? c->vm1 : nullptr);
    if (!dst) return fail(c, SM_EINVAL, view == 1 ? "right view not computed (compute_right_view = 0)" : "bad view");
    HIP_TRY(c, hipMemcpyAsync(dst, src, c->nvol * 4, hipMemcpyHostToDevice, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    if (c->stage >= 4) c->stage = 3;   // dispOptimize may run (again) on the new volume
    return SM_OK;
}

sm_status sm_get_top_disp(sm_ctx* c, int32_t view, float* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst || view < 0 || view > 1) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 4 || !c->vt_tab || c->vt_ran_num[view] == 0 || c->vt_ran_num[view] != c->vt_num)
        return fail(c, SM_ESTATE, "no candidate table of this view yet (sm_vmtop_config, then sm_disp_optimize / sm_run)");
    const int M = c->vt_num;
    std::vector<float> tab(c->npix * M * 2);
    std::vector<int> cnt(c->npix);
    HIP_TRY(c, hipMemcpyAsync(tab.data(), c->vt_tab + (size_t)view * c->cap * c->npix * M, tab.size() * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->vt_cnt + (size_t)view * c->cap * c->npix, cnt.size() * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    memset(dst, 0, c->npix * (size_t)(M + 1) * 2 * sizeof(float));
    for (size_t i = 0; i < c->npix; i++) {
        float* o = dst + i * (size_t)(M + 1) * 2;
        const int n = cnt[i] < 0 ? 0 : (cnt[i] > M ? M : cnt[i]);
        memcpy(o, tab.data() + i * M * 2, (size_t)n * 2 * sizeof(float));
        o[(size_t)M * 2] = (float)cnt[i];
    }
    return SM_OK;
}

sm_status sm_get_arms(sm_ctx* c, int32_t view, uint16_t* dst) {
    sm_status s = check_any(c);
    if (s) return s;
    if (!dst || view < 0 || view > 1) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 2 || !needs_arms(c->p)) return fail(c, SM_ESTATE, "arms not computed");
    std::vector<uint32_t> tmp(c->npix * 2);
    if ((s = download_sync(c, tmp.data(), c->arms + (size_t)view * 2 * c->npix * 4, c->npix * 8))) return s;
    for (size_t i = 0; i < c->npix; i++) {
        dst[i * 4 + 0] = tmp[i] & 0xffff;
        dst[i * 4 + 1] = tmp[i] >> 16;
        dst[i * 4 + 2] = tmp[c->npix + i] & 0xffff;
        dst[i * 4 + 3] = tmp[c->npix + i] >> 16;
    }
    return SM_OK;
}

sm_status sm_get_census(sm_ctx* c, int32_t view, uint64_t* dst) {
    sm_status s = check_any(c);
    if (s) return s;
    if (!dst || view < 0 || view > 1) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 2 || !needs_census(c->p)) return fail(c, SM_ESTATE, "census not computed");
    return download_sync(c, dst, c->code + (size_t)view * c->npix, c->npix * 16);
}

int32_t sm_placement_trials_ms(sm_ctx* c, double* ms, int32_t max) {
    if (!c) return -1;
    const int32_t nt = (int32_t)c->place_ms.size();
    for (int32_t i = 0; ms && i < nt && i < max; i++) ms[i] = c->place_ms[i];
    return nt;
}

int32_t sm_placement_kept(const sm_ctx* c) { return c ? c->place_best : -1; }

// (a pipelined sm_run leaves its second group on a side stream: the main stream is made to wait
// for it first, so work ordered after the returned stream sees the whole call)
void* sm_stream(sm_ctx* c) {
    if (!c || check(c) != SM_OK) return nullptr;
    return (void*)c->st;
}

sm_status sm_profile_enable(sm_ctx* c, int32_t on) {
    if (sm_status r = refuse_level(c)) return r;
    c->prof = on != 0;
    return SM_OK;
}

static sm_status drain_profile(sm_ctx* c) {
    if (c->recs.empty()) return SM_OK;
    HIP_TRY(c, hipStreamSynchronize(c->st));
    for (auto& r : c->recs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
            c->kstat[r.kernel].launches++;
            c->kstat[r.kernel].total_ms += ms;
        }
        c->free_events.push_back(r.start);
        c->free_events.push_back(r.stop);
    }
    c->recs.clear();
    return SM_OK;
}

sm_status sm_profile_read(sm_ctx* c, int32_t max, char* names, int64_t* launches, double* total_ms,
                          double* bytes_per_launch, int32_t* count) {
    sm_status s = check(c);
    if (s) return s;
    if ((s = drain_profile(c))) return s;
    const int k = (int)c->knames.size();
    if (count) *count = k;
    for (int i = 0; i < k && i < max; i++) {
        if (names) {
            strncpy(names + (size_t)i * 48, c->knames[i].c_str(), 47);
            names[(size_t)i * 48 + 47] = 0;
        }
        if (launches) launches[i] = c->kstat[i].launches;
        if (total_ms) total_ms[i] = c->kstat[i].total_ms;
        if (bytes_per_launch) bytes_per_launch[i] = c->kstat[i].bytes;
    }
    return SM_OK;
}

sm_status sm_profile_reset(sm_ctx* c) {
    sm_status s = check(c);
    if (s) return s;
    if ((s = drain_profile(c))) return s;
    for (auto& st : c->kstat) st = ProfStat();
    return SM_OK;
}

sm_status sm_cal_err(const int16_t* DP, const float* DT, const uint8_t* mask, int32_t rows, int32_t cols, float thres,
                     float* pbm, float* rms) {
    if (!DP || !DT || !mask || !pbm || !rms || rows < 1 || cols < 1) return SM_EINVAL;
    int sumNum = 0, errorNumer = 0;
    float errorValueSum = 0;
    for (size_t i = 0; i < (size_t)rows * cols; i++) {
        if (mask[i] != 255) continue;
        sumNum++;
        if (DP[i] >= 0) {
            const float dif = fabsf(DT[i] - (float)DP[i]);
            errorValueSum = (float)((double)errorValueSum + pow((double)dif, 2));   // float += pow(float, int)
            if (dif > thres) errorNumer++;
        } else {
            errorNumer++;
            errorValueSum += 2;
        }
    }
    if (sumNum == 0) {   // the reference divides 0 / 0 here; report 0 instead of NaN
        *pbm = 0;
        *rms = 0;
        return SM_OK;
    }
    *pbm = (float)errorNumer / sumNum;
    *rms = sqrtf(errorValueSum / sumNum);
    return SM_OK;
}

float sm_expf_host(float x) { return sm::expf_host(x); }

// The aggregation-side *_config calls apply to every pyramid level: `one(context, level, dry)` is the call's
// per-context half; a dry pass over all levels checks the arguments (host code only) before the second pass
// changes anything, so a level that cannot take the setting fails the call, named, with every level unchanged.
extern "C++" {
template <typename F>
static sm_status on_levels(sm_ctx* c, F&& one) {
    sm_status s = refuse_level(c);
    if (s) return s;
    const int L = 1 + (int)c->levels.size();
    for (int dry = 1; dry >= 0; dry--) {
        if (!dry && L > 1) {   // the levels' buffers are used by work on the owner's streams
            if ((s = check(c))) return s;
            HIP_TRY(c, hipStreamSynchronize(c->st));
        }
        for (int l = 0; l < L; l++) {
            sm_ctx* q = l ? c->levels[l - 1] : c;
            if ((s = one(q, l, dry != 0))) {
                if (l) c->err = "pyramid level " + std::to_string(l) + ": " + q->err;
                return s;
            }
        }
    }
    return SM_OK;
}
}  // extern "C++"

static sm_status aws_config_one(sm_ctx* c, int32_t radius_v, int32_t radius_u, float gamma_c, bool dry) {
    // host state only (launches already queued carry their constants by value): no device call,
    // so the arguments are checked on a machine without a GPU too
    if (c->p.aggregation != SM_AGG_AWS) return fail(c, SM_EINVAL, "sm_aws_config: the context's aggregation is not SM_AGG_AWS");
    if (radius_v < 0 || radius_v > sm::AWS_MAX_R) return fail(c, SM_EINVAL, "radius_v must be in [0, 17]");
    if (radius_u < 0 || radius_u > sm::AWS_MAX_R) return fail(c, SM_EINVAL, "radius_u must be in [0, 17]");
    if (!(gamma_c > 0) || !std::isfinite(gamma_c)) return fail(c, SM_EINVAL, "gamma_c must be finite and > 0");
    if (dry) return SM_OK;
    c->aws_rv = radius_v;
    c->aws_ru = radius_u;
    c->aws_gamma = gamma_c;
    return SM_OK;
}

sm_status sm_aws_config(sm_ctx* c, int32_t radius_v, int32_t radius_u, float gamma_c) {
    return on_levels(c, [&](sm_ctx* q, int, bool dry) { return aws_config_one(q, radius_v, radius_u, gamma_c, dry); });
}

sm_status sm_so_config(sm_ctx* c, int32_t variant, float pn2, float pn3) {
    if (sm_status r = refuse_level(c)) return r;
    // host state only (a launch carries its constants by value): the arguments are checked before any device call,
    // so on a machine without a GPU too
    if (variant < SM_SO_L2R || variant > SM_SO_T2D) return fail(c, SM_EINVAL, "variant must be SM_SO_L2R, SM_SO_R2L or SM_SO_T2D (0, 1, 2)");
    auto pn_ok = [](float x) { return x == SM_SO_PN_DEFAULT || (std::isfinite(x) && x >= 0 && !std::signbit(x)); };
    if (!pn_ok(pn2)) return fail(c, SM_EINVAL, "pn2 must be SM_SO_PN_DEFAULT or finite and >= +0 (Pn2)");
    if (!pn_ok(pn3)) return fail(c, SM_EINVAL, "pn3 must be SM_SO_PN_DEFAULT or finite and >= +0 (Pn3)");
    const bool all_default = variant == SM_SO_L2R && pn2 == SM_SO_PN_DEFAULT && pn3 == SM_SO_PN_DEFAULT;
    if (c->p.optimization != SM_OPT_SO && !all_default)
        return fail(c, SM_EINVAL, "sm_so_config: the context's optimization is not SM_OPT_SO");
    // so: cpp:6305-6306; so_R2L: cpp:6716-6717; so_T2D: cpp:6607-6608
    const float d2 = variant == SM_SO_L2R ? 1.2f : 0.3f, d3 = variant == SM_SO_L2R ? 3.6f : 0.9f;
    c->so_variant = variant;
    c->so_pn2 = pn2 == SM_SO_PN_DEFAULT ? d2 : pn2;
    c->so_pn3 = pn3 == SM_SO_PN_DEFAULT ? d3 : pn3;
    return SM_OK;
}

sm_status sm_vmtop_config(sm_ctx* c, int32_t enable, int32_t method, int32_t num, float thres, int32_t ts, int32_t has_cir2,
                          int32_t cir3_color_limit) {
    if (sm_status r = refuse_level(c)) return r;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (method < 0 || method > 2) return fail(c, SM_EINVAL, "method must be 0, 1 or 2 (vmTop_method)");
    if (num < 1 || num > sm::VMTOP_MAX_NUM) return fail(c, SM_EINVAL, "num must be in [1, 8] (vmTop_Num)");
    if (!std::isfinite(thres)) return fail(c, SM_EINVAL, "thres must be finite (vmTop_thres)");
    if (enable && c->st) {   // a live context: size the tables for this num (first enable, or a larger num)
        if (!sm::vmtop_shape_ok(c->p.rows, c->p.cols, c->p.num_disparities, c->cap))
            return fail(c, SM_EINVAL, "sm_vmtop_config: rows * cols * batch_capacity too large");
        if (num > c->vt_alloc_num) {
            sm_status s = check(c);
            if (s) return s;
            HIP_TRY(c, hipStreamSynchronize(c->st));   // the old tables may still be read
            const size_t views = (size_t)opt_views(c->p), cap = (size_t)c->cap;
            dfree(c, c->vt_tab);
            c->vt_alloc_num = 0;
            if ((s = dalloc(c, &c->vt_tab, views * cap * c->npix * num))) return s;
            if (!c->vt_cnt && (s = dalloc(c, &c->vt_cnt, views * cap * c->npix))) return s;
            if (!c->vt_tcnt && (s = dalloc(c, &c->vt_tcnt, cap * ((size_t)c->p.cols + 2 * (size_t)c->p.rows)))) return s;
            c->vt_alloc_num = num;
        } else if (num != c->vt_num) {
            sm_status s = check(c);   // the table's stride changes: nothing queued may still write it
            if (s) return s;
            HIP_TRY(c, hipStreamSynchronize(c->st));
        }
    }
    if (num != c->vt_num) c->vt_ran_num[0] = c->vt_ran_num[1] = 0;
    c->vt_on = enable != 0 && c->st != nullptr;
    c->vt_method = method;
    c->vt_num = num;
    c->vt_thres = thres;
    c->vt_ts = ts;
    c->vt_cir2 = has_cir2 != 0;
    c->vt_color = cir3_color_limit != 0;
    return SM_OK;
}

static sm_status bf_config_one(sm_ctx* c, int32_t ksize_v, int32_t ksize_u, bool dry) {
    // host state only, like sm_aws_config
    if (c->p.aggregation != SM_AGG_BF) return fail(c, SM_EINVAL, "sm_bf_config: the context's aggregation is not SM_AGG_BF");
    if (ksize_v < 1 || ksize_v > sm::BF_MAX_K) return fail(c, SM_EINVAL, "ksize_v must be in [1, 32]");
    if (ksize_u < 1 || ksize_u > sm::BF_MAX_K) return fail(c, SM_EINVAL, "ksize_u must be in [1, 32]");
    if (c->p.rows < ksize_v / 2 + 1) return fail(c, SM_EINVAL, "ksize_v: rows must be >= ksize_v / 2 + 1 (one reflection)");
    if (c->p.cols < ksize_u / 2 + 1) return fail(c, SM_EINVAL, "ksize_u: cols must be >= ksize_u / 2 + 1 (one reflection)");
    if (dry) return SM_OK;
    c->bf_kv = ksize_v;
    c->bf_ku = ksize_u;
    return SM_OK;
}

sm_status sm_bf_config(sm_ctx* c, int32_t ksize_v, int32_t ksize_u) {
    return on_levels(c, [&](sm_ctx* q, int, bool dry) { return bf_config_one(q, ksize_v, ksize_u, dry); });
}

static sm_status gfnl_config_one(sm_ctx* c, float var_thresh, bool dry) {
    if (c->p.aggregation != SM_AGG_GFNL) return fail(c, SM_EINVAL, "sm_gfnl_config: the context's aggregation is not SM_AGG_GFNL");
    if (!std::isfinite(var_thresh)) return fail(c, SM_EINVAL, "var_thresh must be finite");
    if (dry) return SM_OK;
    c->gfnl_thresh = var_thresh;
    return SM_OK;
}

sm_status sm_gfnl_config(sm_ctx* c, float var_thresh) {
    return on_levels(c, [&](sm_ctx* q, int, bool dry) { return gfnl_config_one(q, var_thresh, dry); });
}

sm_status sm_get_gfnl_mask(sm_ctx* c, uint8_t* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (c->p.aggregation != SM_AGG_GFNL) return fail(c, SM_EINVAL, "sm_get_gfnl_mask: the context's aggregation is not SM_AGG_GFNL");
    if (c->stage < 2) return fail(c, SM_ESTATE, "no mask yet");
    return download_sync(c, dst, c->gfnl_mask, c->npix);
}

static sm_status dw_config_one(sm_ctx* c, int32_t enable, int32_t arm_l2, int32_t arm_l_out2, int32_t arm_c_thresh2,
                               int32_t arm_c_thresh_out2, float arm_len_thres, bool dry) {
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (c->p.aggregation != SM_AGG_CBCA)
        return fail(c, SM_EINVAL, "sm_cbca_double_config: the context's aggregation is not SM_AGG_CBCA");
    if (arm_l2 < 0) return fail(c, SM_EINVAL, "arm_l2 must be >= 0 (cbca_crossL[1])");
    if (arm_l_out2 < 0 || arm_l_out2 > 84) return fail(c, SM_EINVAL, "arm_l_out2 must be in [0, 84] (cbca_crossL_out[1])");
    if (arm_c_thresh2 < 0) return fail(c, SM_EINVAL, "arm_c_thresh2 must be >= 0 (cbca_cTresh[1])");
    if (arm_c_thresh_out2 < 0) return fail(c, SM_EINVAL, "arm_c_thresh_out2 must be >= 0 (cbca_cTresh_out[1])");
    if (!std::isfinite(arm_len_thres)) return fail(c, SM_EINVAL, "arm_len_thres must be finite (armLthres)");
    if (dry) return SM_OK;
    const bool on = enable != 0 && c->st != nullptr;
    if (c->st) {   // a live context: nothing queued may still use the old settings' buffers
        sm_status s = check_any(c);
        if (s) return s;
        const int lag2 = arm_l_out2 > c->p.arm_min_l ? arm_l_out2 : c->p.arm_min_l;
        if (on && (!c->vm2 || lag2 != c->arms2_lag)) {
            HIP_TRY(c, hipStreamSynchronize(c->st));
            c->dw_on = false;   // (stays off if an allocation below fails)
            const size_t cap = (size_t)c->cap;
            dfree(c, c->arms2_alloc);
            c->arms2 = nullptr;
            c->arms2_lag = -1;
            // the first arm set's layout, for this set's own lag
            if ((s = alloc_arm_planes(c, lag2, &c->arms2_alloc, &c->arms2, &c->arms2_bytes))) return s;
            c->arms2_lag = lag2;
            if (!c->vm2 && (s = dalloc(c, &c->vm2, cap * c->nvol + c->vtail))) return s;
            if (!c->dw_mask && (s = dalloc(c, &c->dw_mask, cap * c->npix))) return s;
        }
        // placement trials time one volume set against another; the second volume is not part of a set, so
        // a context that has had the double window on chooses no placement (the maps are the same either way)
        if (on) c->place_trials = 0;
    }
    c->dw_on = on;
    c->dw_ran = false;
    c->dw_l = arm_l2;
    c->dw_l_out = arm_l_out2;
    c->dw_ct = arm_c_thresh2;
    c->dw_ct_out = arm_c_thresh_out2;
    c->dw_isum = dw_int_threshold(arm_len_thres);
    c->dw_thres = arm_len_thres;
    return SM_OK;
}

sm_status sm_cbca_double_config(sm_ctx* c, int32_t enable, int32_t arm_l2, int32_t arm_l_out2, int32_t arm_c_thresh2,
                                int32_t arm_c_thresh_out2, float arm_len_thres) {
    // calArms divides window 1's arm limits by the level's scale too (cpp:5367-5371)
    return on_levels(c, [&](sm_ctx* q, int l, bool dry) {
        return dw_config_one(q, enable, arm_l2 >> l, arm_l_out2 >> l, arm_c_thresh2, arm_c_thresh_out2, arm_len_thres, dry);
    });
}

sm_status sm_get_cbca_dw_mask(sm_ctx* c, uint8_t* dst) {
    sm_status s = check_any(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (!c->dw_on || !c->dw_ran || c->stage < 2)
        return fail(c, SM_ESTATE, "no mask yet (sm_cbca_double_config, then sm_cost_calculate / sm_run)");
    return download_sync(c, dst, c->dw_mask, c->npix);
}

static sm_status intersect_config_one(sm_ctx* c, int32_t intersect, bool dry) {
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (c->p.aggregation != SM_AGG_CBCA)
        return fail(c, SM_EINVAL, "sm_cbca_intersect_config: the context's aggregation is not SM_AGG_CBCA");
    if (intersect != 0 && intersect != 1) return fail(c, SM_EINVAL, "intersect must be 0 or 1 (cbca_intersect)");
    if (dry) return SM_OK;
    const bool off = intersect == 0 && c->st != nullptr;
    if (c->st) {   // a live context: nothing queued may still run under the old setting
        sm_status s = check_any(c);
        if (s) return s;
        if (off && (!c->ni_tmp || !c->ni_area)) {
            HIP_TRY(c, hipStreamSynchronize(c->st));
            c->ni_on = false;   // (stays off if an allocation below fails)
            const size_t cap = (size_t)c->cap;
            if (!c->ni_tmp && (s = dalloc(c, &c->ni_tmp, cap * c->nvol))) return s;
            if (!c->ni_area && (s = dalloc(c, &c->ni_area, cap * 4 * c->npix))) return s;
        }
        // placement trials time one volume set against another; the ping-pong volume is not part of a set, so a
        // context that has had intersection off chooses no placement (the maps are the same either way)
        if (off) c->place_trials = 0;
    }
    c->ni_on = off;
    c->ni_ran = false;
    return SM_OK;
}

sm_status sm_cbca_intersect_config(sm_ctx* c, int32_t intersect) {
    return on_levels(c, [&](sm_ctx* q, int, bool dry) { return intersect_config_one(q, intersect, dry); });
}

sm_status sm_get_cbca_area(sm_ctx* c, int32_t view, int32_t* dst) {
    sm_status s = check_any(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (view < 0 || view >= n_views(c->p)) return fail(c, SM_EINVAL, "view must be 0, or 1 with do_refine");
    if (!c->ni_on || !c->ni_ran || c->stage < 2)
        return fail(c, SM_ESTATE, "no areas yet (sm_cbca_intersect_config(ctx, 0), then sm_cost_calculate / sm_run)");
    return download_sync(c, dst, c->ni_area + (size_t)view * 2 * c->npix, c->npix * sizeof(int32_t));
}

sm_status sm_refine_ext_config(sm_ctx* c, int32_t do_pkr, float pkr_ratio, int32_t disp_pkr, int32_t do_bg_ipol,
                               int32_t bg_ipl_depth, int32_t do_subpixel, int32_t se_mode) {
    if (sm_status r = refuse_level(c)) return r;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (!c->p.do_refine) return fail(c, SM_EINVAL, "sm_refine_ext_config: the context has do_refine = 0 (refine() never runs)");
    if (!std::isfinite(pkr_ratio)) return fail(c, SM_EINVAL, "pkr_ratio must be finite (ratio_PKR)");
    if (disp_pkr < -32768 || disp_pkr > -1) return fail(c, SM_EINVAL, "disp_pkr must be in [-32768, -1] (DISP_PKR)");
    if (bg_ipl_depth < 0 || bg_ipl_depth > 32767) return fail(c, SM_EINVAL, "bg_ipl_depth must be in [0, 32767] (bgIplDepth)");
    if (se_mode != SM_SE_REFERENCE && se_mode != SM_SE_FLOAT)
        return fail(c, SM_EINVAL, "se_mode must be SM_SE_REFERENCE (0) or SM_SE_FLOAT (1)");
    if (do_pkr && c->p.num_disparities < 2)
        return fail(c, SM_EINVAL, "do_pkr needs num_disparities >= 2 (calPKR's second search is undefined with one cost)");
    // with keep_final_volume k_so leaves the reference's accumulated volume in vm[0] (so_T2D runs on a clone there
    // and leaves the volume after SolveAll): what the reference's refine() reads
    if ((do_pkr || do_subpixel) && c->p.optimization == SM_OPT_SO && !c->p.keep_final_volume)
        return fail(c, SM_EINVAL, do_pkr ? "do_pkr: not with optimization so (the reference's so rewrites vm[0] in place)"
                                         : "do_subpixel: not with optimization so (the reference's so rewrites vm[0] in place)");
    if (c->st) {   // a live context
        if ((do_pkr || do_subpixel) && !sm::refine_ext_shape_ok(c->p.rows, c->p.cols, c->cap))
            return fail(c, SM_EINVAL, "sm_refine_ext_config: rows * cols * batch_capacity too large");
        sm_status s = check(c);
        if (s) return s;
        const size_t cap = (size_t)c->cap;
        if (do_pkr && !c->pkr_mask && (s = dalloc(c, &c->pkr_mask, cap * c->npix))) return s;
        if (do_subpixel && !c->se) {
            if ((s = dalloc(c, &c->se, cap * c->npix))) return s;
            if (!c->se_tmp && (s = dalloc(c, &c->se_tmp, cap * c->npix))) return s;
        }
    }
    const bool live = c->st != nullptr;
    const bool reads = live && (do_pkr || do_subpixel);
    // SGM keeps its path sum in vm[0] only while a stage reads it: one switched on after dispOptimize ran needs a
    // new sm_disp_optimize
    if (reads && !refine_reads_volume(c)) c->rx_vol_ok = false;
    c->rx_pkr = live && do_pkr;
    c->rx_bg = live && do_bg_ipol;
    c->rx_se = live && do_subpixel;
    c->rx_ratio = pkr_ratio;
    c->rx_disp_pkr = disp_pkr;
    c->rx_depth = bg_ipl_depth;
    c->rx_mode = se_mode;
    c->rx_pkr_ran = c->rx_se_ran = false;
    return SM_OK;
}

sm_status sm_get_pkr_mask(sm_ctx* c, uint8_t* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (!c->rx_pkr || !c->rx_pkr_ran || c->stage < 5)
        return fail(c, SM_ESTATE, "no mask yet (sm_refine_ext_config with do_pkr, then sm_refine / sm_run)");
    return download_sync(c, dst, c->pkr_mask, c->npix);
}

sm_status sm_download_subpixel(sm_ctx* c, int32_t n, float* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst || n < 1 || n > c->cap) return fail(c, SM_EINVAL, "bad arguments");
    if (!c->rx_se || !c->rx_se_ran || c->stage < 5)
        return fail(c, SM_ESTATE, "no sub-pixel map yet (sm_refine_ext_config with do_subpixel, then sm_refine / sm_run)");
    HIP_TRY(c, hipMemcpyAsync(dst, c->se, (size_t)n * c->npix * sizeof(float), hipMemcpyDefault, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

sm_status sm_get_subpixel(sm_ctx* c, float* dst) { return sm_download_subpixel(c, 1, dst); }

// the discontinuity adjustment's scratch, on the first call that needs it (batch_capacity pairs)
static sm_status da_alloc(sm_ctx* c) {
    const size_t cap = (size_t)c->cap;
    sm_status s;
    if (!c->da_u8 && (s = dalloc(c, &c->da_u8, cap * sm::DA_PLANES * c->npix))) return s;
    if (!c->da_mag && (s = dalloc(c, &c->da_mag, cap * c->npix))) return s;
    if (!c->da_lab && (s = dalloc(c, &c->da_lab, cap * c->npix))) return s;
    if (!c->da_hist && (s = dalloc(c, &c->da_hist, cap * 256))) return s;
    return SM_OK;
}

sm_status sm_refine_da_config(sm_ctx* c, int32_t on, int32_t canny_low, int32_t canny_high, int32_t blur_side,
                              int32_t blur_centre) {
    if (sm_status r = refuse_level(c)) return r;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (!c->p.do_refine) return fail(c, SM_EINVAL, "sm_refine_da_config: the context has do_refine = 0 (refine() never runs)");
    if (c->p.optimization == SM_OPT_SO && !c->p.keep_final_volume)   // (with it: see sm_refine_ext_config)
        return fail(c, SM_EINVAL, "sm_refine_da_config: not with optimization so (the reference's so rewrites vm[0] in place)");
    if (canny_low < 0 || canny_low > 32767) return fail(c, SM_EINVAL, "canny_low must be in [0, 32767]");
    if (canny_high < 0 || canny_high > 32767) return fail(c, SM_EINVAL, "canny_high must be in [0, 32767]");
    if (blur_side < 0) return fail(c, SM_EINVAL, "blur_side must be >= 0");
    if (blur_centre < 0) return fail(c, SM_EINVAL, "blur_centre must be >= 0");
    if (2 * (int64_t)blur_side + blur_centre > 256)
        return fail(c, SM_EINVAL, "blur_side, blur_centre: 2 * side + centre must be <= 256 (8.8 fixed point)");
    const bool live = c->st != nullptr;
    if (live && on) {
        if (!sm::refine_ext_shape_ok(c->p.rows, c->p.cols, c->cap))
            return fail(c, SM_EINVAL, "sm_refine_da_config: rows * cols * batch_capacity too large");
        sm_status s = check(c);
        if (s) return s;
        if ((s = da_alloc(c))) return s;
        // SGM keeps its path sum in vm[0] only while a stage reads it (see sm_refine_ext_config)
        if (!refine_reads_volume(c)) c->rx_vol_ok = false;
    }
    c->da_on = live && on;
    c->da_low = canny_low;
    c->da_high = canny_high;
    c->da_ks = blur_side;
    c->da_kc = blur_centre;
    c->da_ran = false;
    return SM_OK;
}

sm_status sm_get_da_edges(sm_ctx* c, uint8_t* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (!c->da_on || !c->da_ran || c->stage < 5)
        return fail(c, SM_ESTATE, "no edge map yet (sm_refine_da_config, then sm_refine / sm_run)");
    return download_sync(c, dst, c->da_u8 + (size_t)sm::DA_EDGE * c->npix, c->npix);
}

sm_status sm_refine_outlier_config(sm_ctx* c, int32_t classify, int32_t disp_mis, int32_t rv_combine, int32_t interpolate_type) {
    if (sm_status r = refuse_level(c)) return r;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (const char* why = outlier_config_error(c->p, classify, disp_mis, rv_combine, interpolate_type)) return fail(c, SM_EINVAL, why);
    const bool live = c->st != nullptr;
    if (live && (classify || rv_combine)) {
        sm_status s = check(c);
        if (s) return s;
        const size_t cap = (size_t)c->cap;
        if (classify && !c->oc_mask && (s = dalloc(c, &c->oc_mask, cap * c->npix))) return s;
        if (rv_combine && !c->oc_cand && (s = dalloc(c, &c->oc_cand, cap * c->npix))) return s;
        if (rv_combine && !c->oc_rowlast && (s = dalloc(c, &c->oc_rowlast, cap * (size_t)c->p.rows))) return s;
    }
    c->oc_classify = live && classify;
    c->oc_rv = live && rv_combine;
    c->oc_disp_mis = disp_mis;
    c->oc_type = interpolate_type;
    c->oc_ran = false;
    return SM_OK;
}

sm_status sm_get_lrc_mask(sm_ctx* c, uint8_t* dst) {
    // the argument and the state are checked before any device call, so on a machine without a GPU too
    if (!c) return SM_EINVAL;
    if (!dst) return fail(c, SM_EINVAL, "sm_get_lrc_mask: null dst");
    if (!c->oc_classify || !c->oc_ran || c->stage < 5)
        return fail(c, SM_ESTATE, "no mask yet (sm_refine_outlier_config with classify, then sm_refine / sm_run)");
    sm_status s = check(c);
    if (s) return s;
    return download_sync(c, dst, c->oc_mask, c->npix);
}

sm_status sm_da_run_image(sm_ctx* c, const uint8_t* src, int32_t first_stage, uint8_t* out_eq, uint8_t* out_blur,
                          uint8_t* out_edges) {
    sm_status s = check(c);
    if (s) return s;
    if (!src) return fail(c, SM_EINVAL, "null src");
    if (first_stage < 0 || first_stage > 2) return fail(c, SM_EINVAL, "first_stage must be 0 (equalise), 1 (blur) or 2 (Canny)");
    if (!sm::refine_ext_shape_ok(c->p.rows, c->p.cols, c->cap)) return fail(c, SM_EINVAL, "rows * cols * batch_capacity too large");
    if ((s = da_alloc(c))) return s;
    c->da_ran = false;   // pair 0's planes are this call's from here on
    uint8_t* planes = c->da_u8;
    HIP_TRY(c, hipMemcpyAsync(planes + (size_t)(first_stage == 2 ? sm::DA_BLUR : sm::DA_EQ) * c->npix, src, c->npix,
                              hipMemcpyHostToDevice, c->st));
    if ((s = run_da_image(c, at(c, 0, 1, c->st), first_stage, nullptr))) return s;
    if (out_eq && first_stage == 0) HIP_TRY(c, hipMemcpyAsync(out_eq, planes + (size_t)sm::DA_EQ * c->npix, c->npix, hipMemcpyDeviceToHost, c->st));
    if (out_blur && first_stage <= 1)
        HIP_TRY(c, hipMemcpyAsync(out_blur, planes + (size_t)sm::DA_BLUR * c->npix, c->npix, hipMemcpyDeviceToHost, c->st));
    if (out_edges) HIP_TRY(c, hipMemcpyAsync(out_edges, planes + (size_t)sm::DA_EDGE * c->npix, c->npix, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

sm_status sm_set_da_edges(sm_ctx* c, const uint8_t* edges) {
    sm_status s = check(c);
    if (s) return s;
    if (!edges) {
        c->da_user_on = false;
        return SM_OK;
    }
    if (!c->da_user && (s = dalloc(c, &c->da_user, c->npix))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->da_user, edges, c->npix, hipMemcpyHostToDevice, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    c->da_user_on = true;
    return SM_OK;
}

void sm_bgr2lab_host(const uint8_t* bgr, size_t npix, uint8_t* lab) {
    if (!bgr || !lab) return;
    const uint16_t* tab = aws_tables();
    for (size_t i = 0; i < npix; i++) sm::aws_lab_px(tab, bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], lab + 3 * i);
}

sm_status sm_get_aws_lab(sm_ctx* c, int32_t view, uint8_t* dst) {
    sm_status s = check(c);
    if (s) return s;
    if (!dst) return fail(c, SM_EINVAL, "null dst");
    if (c->p.aggregation != SM_AGG_AWS) return fail(c, SM_EINVAL, "sm_get_aws_lab: the context's aggregation is not SM_AGG_AWS");
    if (view != 0 && view != 1) return fail(c, SM_EINVAL, "bad view");
    if (c->stage < 2) return fail(c, SM_ESTATE, "no Lab plane yet");
    return download_sync(c, dst, c->aws_lab + (size_t)view * c->npix * 3, c->npix * 3);
}

sm_status sm_expf_device_range(sm_ctx* c, uint32_t first_bits, uint32_t n, float* out) {
    sm_status s = check(c);
    if (s) return s;
    if (!out) return fail(c, SM_EINVAL, "null out");
    float* dbuf = nullptr;
    if ((s = dalloc(c, &dbuf, n))) return s;
    sm::launch_expf_range(first_bits, n, dbuf, c->st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dbuf, (size_t)n * 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    dfree(c, dbuf);
    if (e != hipSuccess) return hip_fail(c, e, "sm_expf_device_range");
    return SM_OK;
}

sm_status sm_copy_ceiling(sm_ctx* c, uint64_t bytes, int32_t reps, double* best_gbs, double* median_gbs) {
    sm_status s = check(c);
    if (s) return s;
    if (!best_gbs || !median_gbs || reps < 1 || reps > 1000 || bytes < 16384) return fail(c, SM_EINVAL, "bad arguments");
    bytes = bytes / 16384 * 16384;
    char *src = nullptr, *dst = nullptr;
    if ((s = dalloc(c, &src, bytes))) return s;
    if ((s = dalloc(c, &dst, bytes))) {
        dfree(c, src);
        return s;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<double> gbs;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemsetAsync(src, 1, bytes, c->st);
    // grid sizes bracketing the volume sweeps' launch shapes; every (grid, repetition) is one sample
    for (int grid : {4096, 16384, 65536}) {
        for (int r = 0; r < reps + 1 && e == hipSuccess; r++) {
            if ((e = hipEventRecord(e0, c->st)) != hipSuccess) break;
            sm::launch_copy_x4(src, dst, bytes, grid, c->st);
            if ((e = hipGetLastError()) != hipSuccess) break;
            if ((e = hipEventRecord(e1, c->st)) != hipSuccess) break;
            if ((e = hipEventSynchronize(e1)) != hipSuccess) break;
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) break;
            if (r > 0 && ms > 0.f) gbs.push_back(2.0 * (double)bytes / (ms * 1e-3) / 1e9);   // read + write
        }
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    dfree(c, src);
    dfree(c, dst);
    if (e != hipSuccess) return hip_fail(c, e, "sm_copy_ceiling");
    if (gbs.empty()) return fail(c, SM_EHIP, "sm_copy_ceiling: no timing samples");
    std::sort(gbs.begin(), gbs.end());
    *best_gbs = gbs.back();
    *median_gbs = gbs[gbs.size() / 2];
    return SM_OK;
}

sm_status sm_div_area_check(sm_ctx* c, int32_t exp2, int32_t bmax, uint64_t* mismatches) {
    sm_status s = check(c);
    if (s) return s;
    if (!mismatches || bmax < 1 || bmax > 65535 || exp2 < -126 || exp2 > 126) return fail(c, SM_EINVAL, "bad arguments");
    unsigned long long* dbad = nullptr;
    if ((s = dalloc(c, &dbad, 1))) return s;
    hipError_t e = hipMemsetAsync(dbad, 0, sizeof(*dbad), c->st);
    if (e == hipSuccess) {
        sm::launch_div_check(exp2, bmax, dbad, c->st);
        e = hipGetLastError();
    }
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, dbad, sizeof(h), hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    dfree(c, dbad);
    if (e != hipSuccess) return hip_fail(c, e, "sm_div_area_check");
    *mismatches = h;
    return SM_OK;
}

// ---- the cross-scale pyramid inside sm_run ---------------------------------------------------

// level `l`'s parameters from level l - 1's (main_.cpp:138-148; calArms' scale, cpp:5367-5371): the image halves,
// rounding up; maxdisp / 2 + 1; the arm limits are level 0's divided by 2^l.  A level only builds and aggregates
// its volumes: optimization "", one stream, no placement trials.
static sm_params level_params(const sm_params& p0, const sm_params& prev, int l) {
    sm_params p = prev;
    p.rows = (prev.rows + 1) / 2;
    p.cols = (prev.cols + 1) / 2;
    p.num_disparities = (prev.num_disparities - 1) / 2 + 2;
    p.arm_l = p0.arm_l >> l;
    p.arm_l_out = p0.arm_l_out >> l;
    p.optimization = SM_OPT_WTA;
    p.placement_trials = 0;
    p.num_streams = 1;
    p.sub_batch = 0;
    return p;
}

extern "C++" sm_status pyr_sync_schedule(sm_ctx* c) {
    for (sm_ctx* q : c->levels) {
        q->nstreams = c->nstreams;   // (one AWS weight band per stream the owner's groups run on)
        sm_status s = aws_alloc_bands(q);
        if (s) return fail(c, s, "pyramid level " + std::to_string(q->level) + ": " + q->err);
    }
    return SM_OK;
}

sm_status sm_pyramid_config(sm_ctx* c, int32_t py_lvl) {
    sm_status s = refuse_level(c);
    if (s) return s;
    // the arguments are checked before any device call, so on a machine without a GPU too
    if (py_lvl < 1 || py_lvl > sm::kMaxPyr) return fail(c, SM_EINVAL, "PY_LVL must be in [1, 8]");
    std::vector<sm_params> lp(1, c->p);
    for (int l = 1; l < py_lvl; l++) {
        lp.push_back(level_params(c->p, lp[l - 1], l));
        std::string why;
        if (validate(lp[l], why, c->so_float_minima) == SM_OK && lp[l].aggregation == SM_AGG_BF &&
            (lp[l].rows < c->bf_kv / 2 + 1 || lp[l].cols < c->bf_ku / 2 + 1))
            why = "aggregation BF: the window (sm_bf_config) does not fit the image";
        if (!why.empty())
            return fail(c, SM_EINVAL, "PY_LVL " + std::to_string(py_lvl) + ": pyramid level " + std::to_string(l) + " (" +
                                          std::to_string(lp[l].rows) + " x " + std::to_string(lp[l].cols) + "): " + why);
    }
    if (!c->st) return SM_OK;   // (no live context: nothing to create)
    if ((s = check(c))) return s;
    if (py_lvl == 1 + (int)c->levels.size()) return SM_OK;
    drain(c);
    destroy_levels(c);
    if (const char* e = getenv("SM_PYR_AB")) {
        c->pyr_ab_old = strstr(e, "old_solve") != nullptr;
        c->pyr_ab_loop = strstr(e, "loop_down") != nullptr;
    }
    for (int l = 1; l < py_lvl && !s; l++) {
        sm_ctx* q = nullptr;
        sm_create_opts lo;   // a level is created under its owner's options
        sm_create_opts_default(&lo);
        lo.so_float_minima = c->so_float_minima;
        s = create_ctx(&q, &lp[l], &lo, c->device, c, l);
        if (q) c->levels.push_back(q);
        // the owner's aggregation-side settings (the *_config calls made before this one)
        if (!s && c->p.aggregation == SM_AGG_AWS) s = aws_config_one(q, c->aws_rv, c->aws_ru, c->aws_gamma, false);
        if (!s && c->p.aggregation == SM_AGG_BF) s = bf_config_one(q, c->bf_kv, c->bf_ku, false);
        if (!s && c->p.aggregation == SM_AGG_GFNL) s = gfnl_config_one(q, c->gfnl_thresh, false);
        if (!s && c->dw_on) s = dw_config_one(q, 1, c->dw_l >> l, c->dw_l_out >> l, c->dw_ct, c->dw_ct_out, c->dw_thres, false);
        if (!s && c->ni_on) s = intersect_config_one(q, 0, false);
        if (s) c->err = "pyramid level " + std::to_string(l) + ": " + (q ? q->err : std::string("out of host memory"));
    }
    if (!s) s = pyr_sync_schedule(c);
    if (s) {   // back to PY_LVL 1, with nothing kept
        const std::string why = c->err;
        destroy_levels(c);
        (void)hipGetLastError();
        c->err = why;
        return s;
    }
    return SM_OK;
}

sm_ctx* sm_pyramid_level(sm_ctx* c, int32_t level) {
    if (!c || c->owner || level < 0 || level > (int)c->levels.size()) return nullptr;
    return level == 0 ? c : c->levels[level - 1];
}

int32_t sm_pyramid_levels(const sm_ctx* c) { return c ? 1 + (int32_t)c->levels.size() : 0; }

}  // extern "C"
