// sm_run.cpp — the batch path: the stream schedule (apply_schedule, sm_set_schedule), sm_run's groups and
// pipeline, the volume placement trials, and the uploads and downloads that feed and drain it.
#include <stdio.h>
#include <stdlib.h>

#include <array>
#include <chrono>
#include <thread>

#include "sm_ctx.h"

// sm_params.num_streams / sub_batch -> the schedule sm_run follows (sm_create, sm_set_schedule).
// num_streams 0 (auto): two streams with CBCA at volumes >= 256 MiB per pair, where the next
// group's prep, cost and H scan share the CUs with this group's LDS-bound NORM_SCAN sweep
// (full resolution 37.8 -> 36.0 ms, 1080p x8 53.0 -> 50.3 ms, profiles/r4j; since the groups are
// pipelined across calls, round 5: KITTI x4 8.22 -> 7.58 ms, profiles/r5_final_wl; with the
// two-wave V sweep full resolution is as fast on one stream, 36.04 vs 35.99 ms, and KITTI still
// gains, 8.09 -> 7.58 ms, so the rule stays); and for batches of >= 8 smaller pairs with 4-path
// SGM and no refinement (Teddy x16 in two groups of 8: 2.48 -> 2.37 ms, profiles/r5_final3).
// Side streams are created on first use and kept.
sm_status apply_schedule(sm_ctx* c, int num_streams, int sub_batch) {
    const sm_params& p = c->p;
    if (sub_batch < 0 || num_streams < 0 || num_streams > 4)
        return fail(c, SM_EINVAL, "sub_batch >= 0 and num_streams in [0, 4] required");
    c->sub_batch = sub_batch;
    c->auto_groups = num_streams == 0 && p.aggregation == SM_AGG_CBCA && p.cbca_iterations > 0 &&
                     (c->nvol * 4 >= ((size_t)1 << 28) ||
                      (c->cap >= 8 && p.optimization == SM_OPT_SGM && p.sgm_paths == 4 && !p.do_refine));
    c->nstreams = c->auto_groups ? 2 : (num_streams < 1 ? 1 : num_streams);
    // the pipelined form of the two groups (sm_run): CBCA + SGM without refinement, where the
    // groups touch only their own pairs' buffers
    c->pipelined = c->auto_groups && p.optimization == SM_OPT_SGM && !p.do_refine;
    for (int i = 0; i + 1 < c->nstreams; i++)
        if (!c->xst[i]) HIP_TRY(c, hipStreamCreateWithFlags(&c->xst[i], hipStreamNonBlocking));
    return SM_OK;
}

// Queues the copies of pairs [b0, b1) of both views, colour and gray, on `st`.  dst rows: pair-major,
// view-interleaved; src: stacked images of p.rows rows each, cstride / gstride bytes per row
static sm_status copy_images(sm_ctx* c, int b0, int b1, const uint8_t* lbgr, const uint8_t* rbgr, size_t cstride,
                             const uint8_t* lgray, const uint8_t* rgray, size_t gstride, hipStream_t st) {
    const size_t H = c->p.rows, W = c->p.cols, crow = W * 3;
    for (int view = 0; view < 2; view++) {
        const uint8_t* src = view == 0 ? lbgr : rbgr;
        const uint8_t* gsrc = view == 0 ? lgray : rgray;
        for (int b = b0; b < b1; b++) {
            uint8_t* dst = c->bgr + ((size_t)b * 2 + view) * c->npix * 3;
            HIP_TRY(c, hipMemcpy2DAsync(dst, crow, src + (size_t)b * H * cstride, cstride, crow, H, hipMemcpyDefault, st));
            uint8_t* gdst = c->gray + ((size_t)b * 2 + view) * c->npix;
            HIP_TRY(c, hipMemcpy2DAsync(gdst, W, gsrc + (size_t)b * H * gstride, gstride, W, H, hipMemcpyDefault, st));
        }
    }
    return SM_OK;
}

sm_status upload(sm_ctx* c, int n, const uint8_t* lbgr, const uint8_t* rbgr, size_t cstride, const uint8_t* lgray,
                 const uint8_t* rgray, size_t gstride) {
    sm_status s = copy_images(c, 0, n, lbgr, rbgr, cstride, lgray, rgray, gstride, c->st);
    if (s) return s;
    HIP_TRY(c, hipStreamSynchronize(c->st));
    c->n_loaded = n;
    c->stage = 1;
    return SM_OK;
}

extern "C" {

sm_status sm_upload_batch(sm_ctx* c, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr, const uint8_t* lgray,
                          const uint8_t* rgray) {
    sm_status s = check(c);
    if (s) return s;
    if (n < 1 || n > c->cap) return fail(c, SM_EINVAL, "n must be in [1, batch_capacity]");
    if (!lbgr || !rbgr || !lgray || !rgray) return fail(c, SM_EINVAL, "null image pointer");
    return upload(c, n, lbgr, rbgr, (size_t)c->p.cols * 3, lgray, rgray, (size_t)c->p.cols);
}

static sm_status place_volumes(sm_ctx* c, int k, int n, float reg_lambda);

// what sm_run decides once per call
struct Schedule {
    float w;       // SolveAll's weight
    bool piped;    // the pipelined two-group form
    bool early;    // group k + 1 starts after group k's first CBCA sweep (else after its aggregation)
    bool start;    // the groups start from a joined state
    bool nl_pipe;  // prep, cost volume and trees on the NL front stream (run_nl)
    int levels;    // PY_LVL (sm_pyramid_config)
    float pw[sm::kMaxPyr];   // levels > 1: SolveAll's weight of every level (pyr_weights)
};

// The coarse levels of G's pairs, on G's stream (sm_pyramid_config; main_.cpp:138-156): every level's input
// images from the level above -- colour and gray, both views, filtered themselves -- in one launch per level,
// then prep, cost volume(s) and aggregation of levels PY_LVL - 1 .. 1 through the stage drivers, with the
// group's descriptor on the level's context.  The pyrDown launches come first: they are the coarse levels'
// only readers of level 0's input images, which the next call's asynchronous upload may overwrite once the
// group's in_ev is recorded (after level 0's cost volume or first sweep, later on this stream).
static sm_status run_coarse_levels(sm_ctx* c, const Group& G) {
    sm_status s = SM_OK;
    const int L = 1 + (int)c->levels.size();
    for (int l = 1; l < L && !s; l++) {
        sm_ctx* q = c->levels[l - 1];
        const sm_ctx* up = l == 1 ? c : c->levels[l - 2];
        const Group S = at(up, G.off, G.n, G.st, G.lane), Q = at(q, G.off, G.n, G.st, G.lane);
        const int H = up->p.rows, W = up->p.cols;
        const double bytes = (double)G.n * 2 * 4 * (up->npix + q->npix);
        s = timed(q, G.st, "pyr_down", bytes, [&] {
            if (c->pyr_ab_loop) {   // (A/B: the staged API's launch per image)
                for (int i = 0; i < 2 * G.n; i++) {
                    sm::launch_pyr_down(S.bgr + (size_t)i * up->npix * 3, Q.bgr + (size_t)i * q->npix * 3, H, W, 3, G.st);
                    sm::launch_pyr_down(S.gray + (size_t)i * up->npix, Q.gray + (size_t)i * q->npix, H, W, 1, G.st);
                }
            } else {
                sm::launch_pyr_down_batch(S.bgr, S.gray, Q.bgr, Q.gray, H, W, 2 * G.n, G.st);
            }
        });
    }
    for (int l = L - 1; l >= 1 && !s; l--) {
        sm_ctx* q = c->levels[l - 1];
        const Group Q = at(q, G.off, G.n, G.st, G.lane);
        if ((s = run_prep(q, Q))) break;
        if ((s = run_cost(q, 0, Q))) break;
        if (right_view(q->p) && (s = run_cost(q, 1, Q))) break;
        if (q->p.aggregation == SM_AGG_CBCA)
            for (int v = 0; v < n_views(q->p) && !s; v++) s = run_cbca(q, v, false, 1.0f, Q);
        if (!s) s = run_other_agg(q, Q);
    }
    if (s)
        for (sm_ctx* q : c->levels)
            if (!q->err.empty()) {
                c->err = "pyramid level " + std::to_string(q->level) + ": " + q->err;
                q->err.clear();
                break;
            }
    return s;
}

// Cross-scale SolveAll (cpp:2179-2203) of G's pairs into level 0's volume(s), on G's stream
static sm_status run_solve_all_pyr(sm_ctx* c, const Group& G, const Schedule& S) {
    sm::PyrArgs a{};
    a.levels = S.levels;
    a.n = G.n;
    for (int l = 0; l < S.levels; l++) {
        const sm_ctx* q = l ? c->levels[l - 1] : c;
        a.H[l] = q->p.rows;
        a.W[l] = q->p.cols;
        a.D[l] = q->p.num_disparities;
        a.w[l] = S.pw[l];
    }
    for (int v = 0; v < n_views(c->p); v++) {
        a.vm[0] = G.vm(v);
        for (int l = 1; l < S.levels; l++) {
            const sm_ctx* q = c->levels[l - 1];
            a.vm[l] = (v == 0 ? q->vm0 : q->vm1) + (size_t)G.off * q->nvol;
        }
        sm_status s = timed(c, G.st, Group::name("solve_all_pyr", v), (double)G.n * c->nvol * 8.0, [&] {
            if (c->pyr_ab_old) sm::launch_solve_all_pyr(a, G.st);   // (A/B: the staged API's kernel)
            else sm::launch_solve_all_pyr_batch(a, G.st);
        });
        if (s) return s;
    }
    return SM_OK;
}

// Group k of an sm_run: every stage of G's pairs on G's stream, with the events that tie it to the other
// groups, to the asynchronous map copy and to the next asynchronous upload.
static sm_status run_group(sm_ctx* c, Group G, int k, const Schedule& S) {
    const int ns = c->nstreams;
    sm_status s = SM_OK;
    if (ns > 1 && k > 0 && S.start) HIP_TRY(c, hipStreamWaitEvent(G.st, c->ev_stagger[(k - 1) % 8], 0));
    Group Go = G;   // what the optimiser reads
    const bool pyr = S.levels > 1;   // SolveAll is then the cross-scale pass below, not a weight fused into a last store
    if (pyr && (s = run_coarse_levels(c, G))) return s;
    const int set = c->nl_set;   // (NL: the record / table set this call's run_nl takes)
    if (S.nl_pipe) {
        if ((s = nl_open(c, G.st))) return s;
        const Group F = nl_front(c, G, set);
        if ((s = run_nl(c, G, true, S.w, &F))) return s;
        Go.flags = F.flags;   // the final volume is vm[0]; the penalty flags are the set's
    } else {
        if ((s = run_prep(c, G))) return s;
        if ((s = run_cost(c, 0, G))) return s;
        if (right_view(c->p) && (s = run_cost(c, 1, G))) return s;
        if ((s = run_other_agg(c, G, !pyr, S.w))) return s;   // SolveAll fused into the GF / NL output stores
    }
    // the group's input images are read by prep and the cost volume only (CBCA + SGM, no refinement:
    // the pipelined form): the next call's async upload may overwrite them once ev_in[k] is recorded --
    // here; or, where a fused first CBCA sweep reads the gray images and census codes itself, by run_cbca
    // after the last view's first sweep
    if (S.piped) {
        if ((s = use_event(c, c->ev_in[k]))) return s;
        if (cost_scan_fused(c, 0)) G.in_ev = c->ev_in[k];
        else HIP_TRY(c, hipEventRecord(c->ev_in[k], G.st));
    }
    if (ns > 1 && (s = use_event(c, c->ev_stagger[k % 8]))) return s;
    if (ns > 1 && S.early) G.stagger_ev = c->ev_stagger[k % 8];   // run_cbca records it after its first sweep
    for (int v = 0; v < n_views(c->p) && !S.nl_pipe; v++) {
        if (c->p.aggregation == SM_AGG_CBCA && cbca_iters(c) > 0)
            s = run_cbca(c, v, !pyr, S.w, G);   // SolveAll fused into the last pass
        else if (!pyr && !agg_scale_fused(c->p, v))
            s = run_scale(c, v, S.w, G);      // (GF, FIF, AWS, BF, GFNL and NL's vm[0]: fused above)
        if (s) return s;
    }
    if (pyr && (s = run_solve_all_pyr(c, G, S))) return s;
    // the maps are written from here on: an asynchronous copy of the previous run's maps
    // (sm_download_disp_async) must be done reading them
    // (a split copy: ev_copy covers pairs [0, copy_g) only; a group reaching past them -- the
    // second group, or any group of a different split or schedule -- waits for ev_copy2,
    // recorded after both copies)
    const bool past = c->copy_split && G.off + G.n > c->copy_g;
    if (c->copy_pending) HIP_TRY(c, hipStreamWaitEvent(G.st, past ? c->ev_copy2 : c->ev_copy, 0));
    if (ns > 1 && !S.early) HIP_TRY(c, hipEventRecord(c->ev_stagger[k % 8], G.st));   // the group's aggregation is done
    for (int v = 0; v < opt_views(c->p); v++)
        if ((s = run_optimize(c, v, Go))) return s;
    if (S.nl_pipe) HIP_TRY(c, hipEventRecord(c->nl_ev_opt[set], G.st));   // the NL set is released
    if (c->p.do_refine && (s = run_refine(c, G))) return s;
    return SM_OK;
}

sm_status sm_run(sm_ctx* c, int32_t n, float reg_lambda, int16_t* disp_out) {
    sm_status s = check_nojoin(c);   // (a pipelined run continues from the previous one's streams)
    if (s) return s;
    if (c->stage < 1) return fail(c, SM_ESTATE, "sm_run before images were uploaded");
    if (n < 1 || n > c->n_loaded) return fail(c, SM_EINVAL, "n must be in [1, pairs uploaded]");
    if (c->place_trials > 1) {   // the first run: choose the volume placement (place_volumes)
        const int k = c->place_trials;
        c->place_trials = 0;
        if ((s = join_all(c)) || (s = place_volumes(c, k, n, reg_lambda))) return s;
    }
    if ((s = eval_begin(c, n, true, c->p.do_refine != 0))) return s;   // (the error table: truth loaded, stage list fixed)
    const float m = 1 + reg_lambda;
    // Sub-batches: all stages of a group of pairs run back to back so that one pass's output is
    // still in the 256 MB Infinity Cache when the next pass reads it.  With SM_STREAMS = s > 1 the
    // groups alternate over s streams (group k on lane k % s: the main stream, then the side streams) and
    // group k + 1 starts once group k has finished its CBCA, so the LDS-bound aggregation sweeps of one
    // group share the CUs with the SGM paths of the previous one; the main stream joins every stream at
    // the end.
    const int g = group_size(c, n);
    const int ns = c->nstreams;
    // where group k + 1 starts: with CBCA after group k's first CBCA sweep (the next group's
    // prep, cost and first sweep then share the CUs with this group's LDS-bound NORM_SCAN
    // sweep: profiles/r4j, 1.5-5 % faster than starting after the whole CBCA), else after group
    // k's aggregation
    //
    // Pipelined (num_streams 0 with CBCA + SGM, two groups): group 0 on the main stream, group 1 on
    // the side stream, and the call returns WITHOUT joining them: the next call's group 0 follows
    // this call's group 0 on the main stream and its group 1 this call's group 1 on the side
    // stream, so group 1 keeps running about half a call behind group 0 -- its LDS- and
    // issue-bound CBCA sweeps (NsV: three waves per CU, one SIMD idle, 3 TB/s) beside group 0's SGM
    // passes, which use no LDS and stream HBM.  Two single-pair pipelines offset by half a call:
    // 36.1 -> 35.2 ms per two full-resolution pairs in the bench (profiles/r5l); the placement of an
    // instance's allocations moves both by up to 2 ms (tools/overlap_probe2.py).  Only
    // a pipeline start staggers group 1 (after group 0's CBCA); every other entry point joins
    // first (check -> join_all), and the asynchronous map copy waits for both groups.
    Schedule S;
    S.w = (float)(1. / (double)m);
    S.piped = c->pipelined && ns == 2 && n >= 2 && (n + g - 1) / g == 2;
    S.early = !S.piped && c->p.aggregation == SM_AGG_CBCA && cbca_iters(c) > 0;
    // (a different split of the pairs would let the groups of two calls share a pair: join first)
    if ((!S.piped || g != c->pipe_g) && (s = join_all(c))) return s;
    S.start = !(S.piped && c->pipe_live);
    S.levels = 1 + (int)c->levels.size();
    if (S.levels > 1 && !pyr_weights(S.levels, reg_lambda, S.pw)) return fail(c, SM_EINVAL, "singular regularisation matrix");
    S.nl_pipe = c->nl_pipe && g >= n && ns == 1 && S.levels == 1;
    if (ns > 1 && S.start) {   // the side streams start after everything queued so far on the main stream
        if ((s = use_event(c, c->ev_start))) return s;
        HIP_TRY(c, hipEventRecord(c->ev_start, c->st));
        for (int i = 0; i + 1 < ns; i++) HIP_TRY(c, hipStreamWaitEvent(c->xst[i], c->ev_start, 0));
    }
    for (int off = 0, k = 0; off < n && !s; off += g, k++) {
        const int lane = k % ns;
        s = run_group(c, at(c, off, std::min(g, n - off), lane ? c->xst[lane - 1] : c->st, lane), k, S);
    }
    if (S.piped && !s) {
        c->pipe_live = true;   // group 1 stays on the side stream (joined by the next other call)
        c->pipe_g = g;
    } else {   // the join runs on the error path too: nothing stays queued behind the main stream
        for (int i = 0; i + 1 < ns; i++) {
            const std::string why = c->err;
            const sm_status j = join_side(c, i);
            if (s) c->err = why;   // (the first failure is the one reported)
            else s = j;
        }
    }
    if (s) return s;
    c->stage = c->p.do_refine ? 5 : 4;
    c->rx_vol_ok = true;
    for (sm_ctx* q : c->levels) {   // (what the getters on sm_pyramid_level's contexts check)
        q->stage = 2;
        q->n_loaded = n;
    }
    if (disp_out) return sm_download_disp(c, n, disp_out);
    return SM_OK;
}

// Volume placement trials (sm_params.placement_trials).  One library, one process: the
// same kernels on different device allocations of the volumes run 5-8 % apart, stably per
// allocation -- with identical request counts (TCC_EA0_RDREQ / WRREQ) and no more translation
// misses (TCP_UTCL1_TRANSLATION_MISS ~1e3 of 4e8 requests), but more DRAM credit stalls
// (TCC_EA0_RDREQ_DRAM_CREDIT_STALL, TCC_TAG_STALL), i.e. the physical pages' spread over the HBM
// channels (profiles/r6g).  No allocation flag selects that, so the first sm_run holds k candidate
// sets of the large volumes at once (distinct pages), times the call's own pipeline on each (one
// warm-up, then the best of two) and keeps the fastest; the others are freed.  The maps are the
// same on every set; the trial runs' maps are overwritten by the real run that follows.
static sm_status place_volumes(sm_ctx* c, int k, int n, float reg_lambda) {
    float** slot[4] = {&c->vm0, &c->vm1, &c->acc, &c->ck};
    const size_t vol = c->cap * c->nvol + c->vtail;
    const size_t floats[4] = {vol, vol, vol, c->cap * c->ck_pair};
    std::vector<std::array<float*, 4>> sets(1);
    for (int i = 0; i < 4; i++) sets[0][i] = *slot[i];
    for (int t = 1; t < k; t++) {
        std::array<float*, 4> v{};
        const std::string err = c->err;
        bool ok = true;
        for (int i = 0; i < 4 && ok; i++)
            if (sets[0][i] && dalloc(c, &v[i], floats[i]) != SM_OK) ok = false;
        if (!ok) {   // (no room for another set: try the ones held, and report nothing)
            for (float*& q : v) dfree(c, q);
            (void)hipGetLastError();
            c->err = err;
            break;
        }
        sets.push_back(v);
    }
    if (sets.size() < 2) return SM_OK;
    const bool prof = c->prof;
    c->prof = false;
    sm_status s = SM_OK;
    size_t best = 0;
    double best_t = 1e30;
    c->place_ms.clear();
    for (size_t i = 0; i < sets.size() && !s; i++) {
        for (int j = 0; j < 4; j++) *slot[j] = sets[i][j];
        double tmin = 1e30;
        for (int r = 0; r < 3 && !s; r++) {   // (r = 0 touches the set's pages first)
            const auto t0 = std::chrono::steady_clock::now();
            s = sm_run(c, n, reg_lambda, nullptr);
            if (!s) s = sm_synchronize(c);
            const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (r > 0) tmin = std::min(tmin, t);
        }
        c->place_ms.push_back(tmin * 1e3);
        if (tmin < best_t) {
            best_t = tmin;
            best = i;
        }
    }
    c->prof = prof;
    for (size_t i = 0; i < sets.size(); i++)
        if (i != best)
            for (float*& q : sets[i]) dfree(c, q);
    for (int j = 0; j < 4; j++) *slot[j] = sets[best][j];
    c->place_best = (int)best;
    if (getenv("SM_TRACE_ALLOC")) {
        fprintf(stderr, "[place] %zu volume sets, kept %zu:", sets.size(), best);
        for (double t : c->place_ms) fprintf(stderr, " %.3f", t);
        fprintf(stderr, " ms\n");
    }
    return s;
}

sm_status sm_download_disp(sm_ctx* c, int32_t n, int16_t* disp_out) {
    sm_status s = check(c);
    if (s) return s;
    if (!disp_out || n < 1 || n > c->cap) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 4) return fail(c, SM_ESTATE, "no disparity map yet");
    HIP_TRY(c, hipMemcpyAsync(disp_out, c->disp, (size_t)n * c->npix * 2, hipMemcpyDefault, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
    return SM_OK;
}

sm_status sm_download_disp_async(sm_ctx* c, int32_t n, int16_t* disp_out) {
    sm_status s = check_nojoin(c);   // (keeps a pipelined run's groups apart)
    if (s) return s;
    if (!disp_out || n < 1 || n > c->cap) return fail(c, SM_EINVAL, "bad arguments");
    if (c->stage < 4) return fail(c, SM_ESTATE, "no disparity map yet");
    if (!c->cst) HIP_TRY(c, hipStreamCreateWithFlags(&c->cst, hipStreamNonBlocking));
    for (hipEvent_t* ev : {&c->ev_run, &c->ev_copy, &c->ev_copy2, &c->ev_side})
        if ((s = use_event(c, *ev))) return s;
    HIP_TRY(c, hipEventRecord(c->ev_run, c->st));
    HIP_TRY(c, hipStreamWaitEvent(c->cst, c->ev_run, 0));
    c->copy_split = c->pipe_live && n > c->pipe_g;
    c->copy_g = c->pipe_g;
    if (c->copy_split) {
        // a pipelined run: the first group's maps once the main stream is there, the second's once
        // the side stream is (waited for, not joined), so that the next run's group k waits for
        // its own maps' copy only
        const size_t g = (size_t)c->pipe_g;
        HIP_TRY(c, hipMemcpyAsync(disp_out, c->disp, g * c->npix * 2, hipMemcpyDefault, c->cst));
        HIP_TRY(c, hipEventRecord(c->ev_copy, c->cst));
        HIP_TRY(c, hipEventRecord(c->ev_side, c->xst[0]));
        HIP_TRY(c, hipStreamWaitEvent(c->cst, c->ev_side, 0));
        HIP_TRY(c, hipMemcpyAsync(disp_out + g * c->npix, c->disp + g * c->npix, ((size_t)n - g) * c->npix * 2,
                                  hipMemcpyDefault, c->cst));
        HIP_TRY(c, hipEventRecord(c->ev_copy2, c->cst));
    } else {
        if (c->pipe_live) {   // (n within the first group: its maps only)
            HIP_TRY(c, hipEventRecord(c->ev_side, c->xst[0]));
            HIP_TRY(c, hipStreamWaitEvent(c->cst, c->ev_side, 0));
        }
        HIP_TRY(c, hipMemcpyAsync(disp_out, c->disp, (size_t)n * c->npix * 2, hipMemcpyDefault, c->cst));
        HIP_TRY(c, hipEventRecord(c->ev_copy, c->cst));
    }
    c->copy_pending = true;
    // (one event after both copies on the copy stream: sm_download_wait's per-call marker)
    if ((s = use_event(c, c->ev_dl[c->dl_slot]))) return s;
    HIP_TRY(c, hipEventRecord(c->ev_dl[c->dl_slot], c->cst));
    c->dl_slot ^= 1;
    c->dl_count++;
    return SM_OK;
}

sm_status sm_download_wait(sm_ctx* c, int32_t back) {
    sm_status s = check_nojoin(c);   // (the pipeline stays live)
    if (s) return s;
    if (back < 0 || back > 1) return fail(c, SM_EINVAL, "back must be 0 (the last async download) or 1 (the one before)");
    if (c->dl_count <= back) return SM_OK;   // (no such download: nothing to wait for)
    hipEvent_t e = c->ev_dl[(c->dl_slot + 1 + back) & 1];
    if (e) HIP_TRY(c, hipEventSynchronize(e));
    return SM_OK;
}

// Asynchronous upload for a pipelined stream of calls (DistributedBatchRunner over hip_compute_fn):
// the copies are queued without joining a live pipeline or waiting on the host -- the next call's
// first group's pairs on the main stream (after that group's previous call), the second group's on
// the side stream (after the previous call's second group) -- so a call's inputs arrive while the
// previous call still runs.  The sources must stay unchanged until sm_upload_wait returns.
sm_status sm_upload_batch_async(sm_ctx* c, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr, const uint8_t* lgray,
                                const uint8_t* rgray) {
    sm_status s = check_nojoin(c);
    if (s) return s;
    if (n < 1 || n > c->cap) return fail(c, SM_EINVAL, "n must be in [1, batch_capacity]");
    if (!lbgr || !rbgr || !lgray || !rgray) return fail(c, SM_EINVAL, "null image pointer");
    // the split the next run will keep (group_size); any other shape joins first, as a synchronous
    // upload does
    const int g = group_size(c, n);
    const bool split = c->pipe_live && c->pipelined && g == c->pipe_g && (n + g - 1) / g == 2;
    if (!split && (s = join_all(c))) return s;
    for (int i = 0; i < 2; i++)
        if ((s = use_event(c, c->ev_up[i]))) return s;
    const size_t crow = (size_t)c->p.cols * 3, grow = (size_t)c->p.cols;
    auto copy = [&](int b0, int b1, hipStream_t st) { return copy_images(c, b0, b1, lbgr, rbgr, crow, lgray, rgray, grow, st); };
    // early: the copies go on their own stream as soon as each group's previous inputs are read
    // (ev_in, recorded after its cost volume -- after its first CBCA sweep where that sweep computes
    // the costs from the gray images itself, run_cbca), so they overlap that group's CBCA and SGM; the
    // group's next kernels wait for its copies (ev_up)
    const bool early = split && c->ev_in[0] && c->ev_in[1];
    const hipStream_t ust = nullptr;
    for (int grp = 0; early && grp < 2; grp++) {
        HIP_TRY(c, hipStreamWaitEvent(ust, c->ev_in[grp], 0));
        if ((s = copy(grp * g, std::min(n, (grp + 1) * g), ust))) return s;
        HIP_TRY(c, hipEventRecord(c->ev_up[grp], ust));
        HIP_TRY(c, hipStreamWaitEvent(grp == 0 ? c->st : c->xst[0], c->ev_up[grp], 0));
    }
    if (!early) {   // each group's pairs on the group's own stream
        if ((s = copy(0, split ? g : n, c->st))) return s;
        if (split && (s = copy(g, n, c->xst[0]))) return s;
        HIP_TRY(c, hipEventRecord(c->ev_up[0], c->st));
        if (split) HIP_TRY(c, hipEventRecord(c->ev_up[1], c->xst[0]));
    }
    c->up_split = split;
    c->n_loaded = n;
    c->stage = 1;
    return SM_OK;
}

sm_status sm_upload_wait(sm_ctx* c) {
    sm_status s = check_nojoin(c);
    if (s) return s;
    if (c->ev_up[0]) HIP_TRY(c, hipEventSynchronize(c->ev_up[0]));
    if (c->up_split && c->ev_up[1]) HIP_TRY(c, hipEventSynchronize(c->ev_up[1]));
    return SM_OK;
}

sm_status sm_run_batch(sm_ctx* c, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr, const uint8_t* lgray,
                       const uint8_t* rgray, float reg_lambda, int16_t* disp_out) {
    sm_status s = sm_upload_batch(c, n, lbgr, rbgr, lgray, rgray);
    if (s) return s;
    return sm_run(c, n, reg_lambda, disp_out);
}

sm_status sm_run_batch_multi(sm_ctx* const* ctxs, int32_t nctx, int32_t n, const uint8_t* lbgr, const uint8_t* rbgr,
                             const uint8_t* lgray, const uint8_t* rgray, float reg_lambda, int16_t* disp_out) {
    if (!ctxs || nctx < 1 || n < 1 || !lbgr || !rbgr || !lgray || !rgray || !disp_out) return SM_EINVAL;
    for (int i = 0; i < nctx; i++) {
        if (!ctxs[i]) return SM_EINVAL;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return fail(ctxs[i], SM_EINVAL, "sm_run_batch_multi: a context appears twice");
        const sm_params& a = ctxs[i]->p;
        const sm_params& b = ctxs[0]->p;
        if (a.rows != b.rows || a.cols != b.cols || a.num_disparities != b.num_disparities)
            return fail(ctxs[i], SM_EINVAL, "sm_run_batch_multi: contexts of different shapes");
    }
    // contiguous blocks of ceil(n / nctx) pairs: context i owns pairs [i * per, min(n, (i + 1) * per))
    const int per = (n + nctx - 1) / nctx;
    const size_t npix = (size_t)ctxs[0]->p.rows * ctxs[0]->p.cols;
    for (int i = 0; i < nctx; i++) {
        const int lo = std::min(n, i * per), cnt = std::min(n, lo + per) - lo;
        if (cnt > ctxs[i]->cap) return fail(ctxs[i], SM_EINVAL, "sm_run_batch_multi: block larger than batch_capacity");
    }
    std::vector<sm_status> st(nctx, SM_OK);
    auto work = [&](int i) {
        const int lo = std::min(n, i * per), cnt = std::min(n, lo + per) - lo;
        if (cnt <= 0) return;
        st[i] = sm_run_batch(ctxs[i], cnt, lbgr + lo * npix * 3, rbgr + lo * npix * 3, lgray + lo * npix,
                             rgray + lo * npix, reg_lambda, disp_out + lo * npix);
    };
    // one host thread per context (each context is used by one thread only, the C-ABI's rule)
    std::vector<std::thread> th;
    for (int i = 1; i < nctx; i++) th.emplace_back(work, i);
    work(0);
    for (auto& t : th) t.join();
    for (int i = 0; i < nctx; i++)
        if (st[i] != SM_OK) return st[i];
    return SM_OK;
}

sm_status sm_set_schedule(sm_ctx* c, int32_t num_streams, int32_t sub_batch) {
    sm_status s = check(c);
    if (s) return s;
    // (the previous sm_run joined its side streams into the main stream, so the next run's
    // groups are ordered after it whichever streams they use)
    if ((s = apply_schedule(c, num_streams, sub_batch))) return s;
    if ((s = aws_alloc_bands(c))) return s;
    if ((s = pyr_sync_schedule(c))) return s;
    c->p.num_streams = num_streams;
    c->p.sub_batch = sub_batch;
    return SM_OK;
}

sm_status sm_synchronize(sm_ctx* c) {
    sm_status s = check(c);
    if (s) return s;
    HIP_TRY(c, hipStreamSynchronize(c->st));
    if (c->cst) {
        HIP_TRY(c, hipStreamSynchronize(c->cst));
        c->copy_pending = false;
    }
    return SM_OK;
}

}  // extern "C"
