// sm_stages_agg.cpp — the drivers of the aggregations other than CBCA (GF, NL, FIF, AWS, BF, GFNL) and
// run_other_agg, which chooses among them and fuses SolveAll's scale into their last store.
#include <math.h>

#include <cmath>

#include "sm_ctx.h"

// guideFilter(0, vm) on one view (cpp:4492-4516): ximgproc form (the shipped build, sm_gf_cv.hip)
// or the MY_GUIDE form (sm_gf.hip), by sm_params.gf_mode
static sm_status run_gf(sm_ctx* c, int view, const Group& G, bool solve_all, float w) {
    const size_t off = G.off, cap = c->cap, nv = c->nvol;
    if (c->p.gf_mode == SM_GF_XIMGPROC) {
        sm::GfCvArgs a{};
        a.vm = G.vm(view);
        a.rs = G.slice(c->gfc_rs, nv);
        a.ab = G.slice(c->gfc_ab, nv);
        a.cap = c->cap;
        a.px = G.px + (size_t)view * c->npix;        // packed words of the view's image (run_prep)
        a.px_pair_stride = 2 * c->npix;
        a.img_rs = G.slice(c->gfc_img, 9 * c->npix);
        a.pix = G.slice(c->gfc_pix, 9 * c->npix);
        a.H = c->p.rows;
        a.W = c->p.cols;
        a.D = c->p.num_disparities;
        a.eps = c->p.gf_eps;
        a.solve_all = solve_all;
        a.scale = w;
        // R0: read p, write 4 doubles; C0: read 4 doubles, write 4 floats; R1: read 4 floats, write 4
        // doubles; C1: read 4 doubles, write q (the leaving rows / positions re-read from cache)
        const double bytes = (double)G.n * nv * (4 + 32 + 32 + 16 + 16 + 32 + 32 + 4);
        return timed(c, G.st, Group::name("gf", view), bytes, [&] { sm::launch_gf_cv(a, G.n, G.st); });
    }
    sm::GfArgs a{};
    a.vm = G.vm(view);
    float* s0 = c->acc ? c->acc : c->gf_s + 3 * cap * nv;
    a.s0 = s0 + off * nv;
    a.s1 = c->gf_s + (0 * cap + off) * nv;
    a.s2 = c->gf_s + (1 * cap + off) * nv;
    a.s3 = c->gf_s + (2 * cap + off) * nv;
    a.bgr = G.bgr + (size_t)view * c->npix * 3;   // I_c[view] (cpp:4502)
    a.bgr_pair_stride = 2 * c->npix * 3;
    a.px = G.px + (size_t)view * c->npix;        // packed words of the same image (run_prep)
    a.px_pair_stride = 2 * c->npix;
    a.planes = G.slice(c->gf_planes, 10 * c->npix);
    a.pix = G.slice(c->gf_pix, c->npix);
    a.H = c->p.rows;
    a.W = c->p.cols;
    a.D = c->p.num_disparities;
    a.eps = c->p.gf_eps;
    a.solve_all = solve_all;
    a.scale = w;
    // four volume sweeps, each reading and writing four channels (V0: reads one)
    const double bytes = (double)G.n * nv * (4 + 16 + 32 + 32 + 16 + 4);
    return timed(c, G.st, Group::name("gf", view), bytes, [&] { sm::launch_gf(a, G.n, G.st); });
}

// The NL front (median, edge weights, spanning trees, the tree walk) runs on its own stream: it
// reads only the colour images, which change only through upload() (which synchronises), so
// it need not wait for the work still queued on the group's stream -- with inputs resident across
// calls, this call's trees are built while the GPU finishes the previous call's filter and
// optimisation.  Records and path tables are double-buffered across calls; the walk waits
// only for the filter that last read the set it writes.
// nl_open creates that stream on first use, with the sets' events, recorded once on `st` (the
// stream of the group that runs NL first) so that the first waits find them complete.
// A pyramid level context takes its owner's front stream: the front's work space (spanning trees, tree walk) is
// one per context, and one stream orders the levels' and the groups' fronts as it orders the groups' alone.
sm_status nl_open(sm_ctx* c, hipStream_t st) {
    if (c->nl_st) return SM_OK;
    if (c->owner) {
        sm_status s = nl_open(c->owner, st);
        if (s) return fail(c, s, c->owner->err);
        c->nl_st = c->owner->nl_st;
    } else {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->nl_st, hipStreamNonBlocking));
    }
    for (hipEvent_t* ev : {c->nl_ev_set, c->nl_ev_opt})
        for (int i = 0; i < 2; i++) {
            sm_status s = use_event(c, ev[i]);
            if (s) return s;
            HIP_TRY(c, hipEventRecord(ev[i], st));
        }
    return SM_OK;
}

// The pipelined front's descriptor (sm_run with NL + SGM, after nl_open): G's pairs on nl_st, with the
// cost volume and penalty flags of record / table set `set`, which this call's prep and cost volume fill
Group nl_front(const sm_ctx* c, const Group& G, int set) {
    Group F = G;
    F.st = c->nl_st;
    F.vm0 = G.slice(c->nl_vc + (size_t)set * c->cap * c->nvol, c->nvol);
    F.flags = G.slice(c->nl_fl + (size_t)set * c->cap * c->npix, c->npix);
    return F;
}

// NL() on vm[0] (cpp:4892-4917): edge weights, spanning trees, the tree walk and the tree filter,
// all on the GPU (sm_nl.hip, sm_nl_mst.hip, sm_nl_walk.hip); the call takes record / table set c->nl_set
// `front`: nl_front(c, G, c->nl_set) -- the front then also runs the call's prep and cost volume
// `out`: where the filtered volume goes instead of vm[0] ("GFNL" keeps the raw costs for GF)
sm_status run_nl(sm_ctx* c, const Group& G, bool solve_all, float w, const Group* front, float* out) {
    const size_t np = c->npix;
    const int H = c->p.rows, W = c->p.cols, D = c->p.num_disparities;
    const size_t ne = (size_t)H * (W - 1) + (size_t)(H - 1) * W;
    const size_t slot = (size_t)c->cap * np;
    sm_status s = nl_open(c, G.st);
    if (s) return s;
    Group F = G;   // the front's launches (and their profiling events) go to nl_st
    F.st = c->nl_st;
    if (front) F = *front;
    if (c->owner) {   // a level's images are this call's pyrDown output, written on the group's stream
        if ((s = use_event(c, c->nl_ev_in))) return s;
        HIP_TRY(c, hipEventRecord(c->nl_ev_in, G.st));
        HIP_TRY(c, hipStreamWaitEvent(F.st, c->nl_ev_in, 0));
    }
    const int set = c->nl_set;
    c->nl_set ^= 1;
    int* I = c->nl_ints + (size_t)set * 4 * slot;
    int* rec_d = c->nl_rec + ((size_t)set * (slot + 2 * sm::NL_REC_PAD) + sm::NL_REC_PAD) * 4;
    constexpr int NOFF = 2 * (sm::NL_LEVELS + 1) + 1;
    if (front) {
        // this call's prep and cost volume, into the set's flags and cost volume: the set was
        // last read by the optimiser two calls back (its filter read the cost volume before)
        HIP_TRY(c, hipStreamWaitEvent(F.st, c->nl_ev_opt[set], 0));
        if ((s = run_prep(c, F))) return s;
        if ((s = run_cost(c, 0, F))) return s;
    }
    s = timed(c, F.st, "nl_edges", (double)G.n * np * 4, [&] {
        sm::launch_nl_edges(G.bgr, 2 * np * 3, G.slice(c->nl_med, np * 3), G.slice(c->nl_ew, ne), H, W, G.n, F.st);
    });
    if (s) return s;
    // the spanning trees' neighbour lists (Boruvka on the GPU, sm_nl_mst.hip); bytes = the edge
    // weights read once
    s = timed(c, F.st, "nl_mst", (double)G.n * ne, [&] {
        sm::launch_nl_mst(G.slice(c->nl_ew, ne), H, W, G.n, G.slice(c->nl_par, np), G.slice(c->nl_best, np),
                          c->nl_mst, G.slice(c->nl_adj, np), F.st);
    });
    if (s) return s;
    HIP_TRY(c, hipStreamWaitEvent(F.st, c->nl_ev_set[set], 0));
    // the tree walk (sm_nl_walk.hip); bytes = the records and path tables written
    s = timed(c, F.st, "nl_walk", (double)G.n * np * 32, [&] {
        sm::launch_nl_walk(G.slice(c->nl_adj, np), H, W, G.n, c->nl_walk, (int4*)rec_d, I, I + slot, I + 2 * slot,
                           I + 3 * slot, c->nl_offs, F.st);
    });
    if (s) return s;
    HIP_TRY(c, hipMemcpyAsync(c->nl_offs_h, c->nl_offs, NOFF * sizeof(int), hipMemcpyDeviceToHost, F.st));
    HIP_TRY(c, hipStreamSynchronize(F.st));   // the round offsets (the records are then in place)
    const int* up_off = c->nl_offs_h;
    const int* dn_off = c->nl_offs_h + sm::NL_LEVELS + 1;
    if (c->nl_offs_h[NOFF - 1] != 0)
        return fail(c, SM_EINVAL, "NL: spanning tree walk failed (flags " + std::to_string(c->nl_offs_h[NOFF - 1]) + ")");
    sm::NlArgs a{};
    a.chain_start = I;
    a.chain_len = I + slot;
    a.order_up = I + 2 * slot;
    a.order_down = I + 3 * slot;
    a.rec = (const int4*)rec_d;
    a.table = c->nl_table;
    a.val = c->nl_val;
    a.vm = out ? out : G.vm0;
    a.vc = F.vm0;
    a.oup = c->nl_oup;
    a.ofin = c->nl_ofin;
    a.nodes = (long)G.n * (long)np;
    a.W = W;
    a.solve_all = solve_all;
    a.scale = w;
    // the cost volume and the ones: up rounds, then down rounds; per voxel: cost in, up sum out;
    // up sum in, final out, float out (+ the light children's sums, about one per node)
    const double bytes = (double)G.n * c->nvol * (4 + 8 + 8 + 8 + 8 + 4);
    s = timed(c, G.st, "nl_filter", bytes, [&] {
        for (int r = 0; r < sm::NL_LEVELS; r++) sm::launch_nl_round(a, true, up_off[r], up_off[r + 1], D, G.st);
        for (int r = 0; r < sm::NL_LEVELS; r++) sm::launch_nl_round(a, false, dn_off[r], dn_off[r + 1], D, G.st);
    });
    if (s) return s;
    HIP_TRY(c, hipEventRecord(c->nl_ev_set[set], G.st));
    return SM_OK;
}

// FIF_Improve / FIF on one view (cpp:4707-4890, 4541-4705; sm_fif.hip): the view's weight planes,
// then H forward (vm -> c1), H backward (vm, c1 -> A), V forward (A -> T), V backward (A, T -> vm).
// c1 and T share one scratch volume (the SGM sum where there is one), A has its own; both are
// the group's own pairs' slices, so groups on different streams never share scratch.
static sm_status run_fif(sm_ctx* c, int view, const Group& G, bool solve_all, float w) {
    const sm_params& p = c->p;
    const size_t off = G.off, cap = c->cap, nv = c->nvol, np = c->npix;
    float* vm = G.vm(view);
    float* s0 = (c->acc ? c->acc : c->fif_s + cap * nv) + off * nv;   // c1, then T
    float* s1 = G.slice(c->fif_s, nv);                                  // A
    sm::FifArgs a{};
    a.bgr = G.bgr + (size_t)view * np * 3;   // I_c[view] (cpp:4718)
    a.bgr_pair_stride = 2 * np * 3;
    a.wh = G.slice(c->fif_w, np);
    a.wv = c->fif_w + (cap + off) * np;
    a.eps = p.fif_eps;
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.plain = p.fif_mode == SM_FIF_PLAIN;
    a.pn = p.fif_pn;
    a.scale = w;
    sm_status s = timed(c, G.st, Group::name("fif_weights", view), (double)G.n * np * (3 + 8), [&] { sm::launch_fif_weights(a, G.n, G.st); });
    if (s) return s;
    struct Pass { const char* name; const float* in; const float* fw; float* out; int vert, second; };
    const Pass passes[4] = {{"fif_h_fwd", vm, nullptr, s0, 0, 0},
                            {"fif_h_bwd", vm, s0, s1, 0, 1},
                            {"fif_v_fwd", s1, nullptr, s0, 1, 0},
                            {"fif_v_bwd", s1, s0, vm, 1, 1}};
    for (int i = 0; i < 4; i++) {
        const Pass& ps = passes[i];
        a.in = ps.in;
        a.fw = ps.fw;
        a.out = ps.out;
        a.vert = ps.vert;
        a.second = ps.second;
        a.solve_all = i == 3 && solve_all;   // SolveAll's 0 + w q in the last sweep's store
        // forward: read one volume, write one; backward: read two, write one (+ the weight plane)
        const double bytes = (double)G.n * nv * (ps.second ? 12.0 : 8.0) + (double)G.n * np * 4;
        if ((s = timed(c, G.st, Group::name(ps.name, view), bytes, [&] { sm::launch_fif_sweep(a, G.n, G.st); }))) return s;
    }
    return SM_OK;
}

// The 8-bit BGR2Lab tables (OpenCV's fixed-point path, restated: PARITY UNPINNED), gam | cb:
//   gam[i] = round(255 * 8 * g(i / 255)), g the inverse sRGB curve;  cb[i] = round(32768 * f(i / (255 * 8)))
const uint16_t* aws_tables() {
    static const std::vector<uint16_t> tab = [] {
        std::vector<uint16_t> t(sm::AWS_GAM_N + sm::AWS_CB_N);
        for (int i = 0; i < sm::AWS_GAM_N; i++) {
            const double x = i / 255.0;
            const double g = x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
            t[i] = (uint16_t)lrint(255.0 * 8.0 * g);
        }
        for (int i = 0; i < sm::AWS_CB_N; i++) {
            const double x = i / (255.0 * 8.0);
            const double f = x < 0.008856 ? 7.787 * x + 0.13793103448275862 : cbrt(x);
            t[sm::AWS_GAM_N + i] = (uint16_t)lrint(32768.0 * f);
        }
        return t;
    }();
    return tab.data();
}

// One band per stream of the schedule (sm_create, sm_set_schedule); a band is never freed or
// resized before sm_destroy.
sm_status aws_alloc_bands(sm_ctx* c) {
    if (c->p.aggregation != SM_AGG_AWS) return SM_OK;
    const size_t smax = (size_t)(2 * sm::AWS_MAX_R + 1) * (2 * sm::AWS_MAX_R + 1);
    const size_t row_floats = 2 * smax * c->p.cols;
    for (int i = 0; i < c->nstreams && i < 4; i++) {
        if (c->aws_band[i]) continue;
        // (+ 64 floats of slack past the last row)
        sm_status s = dalloc(c, &c->aws_band[i], (size_t)c->aws_band_rows * row_floats + 64);
        if (s) return s;
    }
    return SM_OK;
}

// AWS on every view of the group (cpp:5711-5792; sm_aws.hip): both images' Lab planes, a raw copy
// of each view's volume (the reference's vm_IB), then band by band the weights of both images and
// the aggregation of every view's rows of that band.  Lab planes and raw copies are the group's own
// pairs' slices and each stream has its own band, so groups on different streams share no scratch.
static sm_status run_aws(sm_ctx* c, const Group& G, bool solve_all, float w) {
    const sm_params& p = c->p;
    const size_t off = G.off, cap = c->cap, nv = c->nvol, np = c->npix;
    if (!c->aws_band[G.lane]) return fail(c, SM_ESTATE, "aggregation AWS: no weight band for this stream");
    sm::AwsArgs a{};
    a.tab = c->aws_tab;
    a.bgr = G.bgr;
    a.lab = G.slice(c->aws_lab, 2 * np * 3);
    a.wt = c->aws_band[G.lane];
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.rv = c->aws_rv;
    a.ru = c->aws_ru;
    a.gamma_c = c->aws_gamma;
    a.band_rows = c->aws_band_rows;
    a.solve_all = solve_all;
    a.scale = w;
    const int views = n_views(p);
    const double S = (double)(2 * a.rv + 1) * (2 * a.ru + 1);
    sm_status s = timed(c, G.st, "aws_lab", (double)G.n * 2 * np * 6, [&] { sm::launch_aws_lab(a, G.n, G.st); });
    if (s) return s;
    for (int v = 0; v < views; v++) {
        float* vm = G.vm(v);
        float* raw = c->aws_raw + ((size_t)v * cap + off) * nv;
        if ((s = timed(c, G.st, Group::name("aws_copy", v), (double)G.n * nv * 8, [&] {
                 hipMemcpyAsync(raw, vm, (size_t)G.n * nv * 4, hipMemcpyDeviceToDevice, G.st);
             })))
            return s;
    }
    const int rows = G.n * p.rows;
    for (int r0 = 0; r0 < rows; r0 += c->aws_band_rows) {
        a.r0 = r0;
        a.nr = std::min(c->aws_band_rows, rows - r0);
        if ((s = timed(c, G.st, "aws_weights", (double)a.nr * p.cols * S * 8, [&] { sm::launch_aws_weights(a, G.st); }))) return s;
        for (int v = 0; v < views; v++) {
            a.raw = c->aws_raw + ((size_t)v * cap + off) * nv;
            a.out = G.vm(v);
            a.lor = v;
            if ((s = timed(c, G.st, Group::name("aws_agg", v), (double)a.nr * p.cols * p.num_disparities * 8,
                           [&] { sm::launch_aws_agg(a, G.st); })))
                return s;
        }
    }
    return SM_OK;
}

// BF() (cpp:1023-1043; sm_bf.hip) on one view: the row sweep into the double row sums, the column
// sweep back into the volume.  The row sums are the group's own pairs' slice, shared by its views
// (they run one after the other on the group's stream).
static sm_status run_bf(sm_ctx* c, int view, const Group& G, bool solve_all, float w) {
    const sm_params& p = c->p;
    const size_t nv = c->nvol;
    sm::BfArgs a{};
    a.vm = G.vm(view);
    a.rs = G.slice(c->bf_rs, nv);
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.kv = c->bf_kv;
    a.ku = c->bf_ku;
    a.solve_all = solve_all;
    a.scale = w;
    if (p.rows < a.kv / 2 + 1 || p.cols < a.ku / 2 + 1) return fail(c, SM_ESTATE, "aggregation BF: the window does not fit the image");
    sm_status s = timed(c, G.st, Group::name("bf_rows", view), (double)G.n * nv * 12, [&] { sm::launch_bf_rows(a, G.n, G.st); });
    if (s) return s;
    return timed(c, G.st, Group::name("bf_cols", view), (double)G.n * nv * 12, [&] { sm::launch_bf_cols(a, G.n, G.st); });
}

// GFNL() (cpp:4421-4490): NL of the raw vm[0] into its own volume, guideFilter in place on every
// view (num = Do_refine ? 2 : 1, cpp:4499), then on vm[0] the blend under the left gray image's
// variance mask (sm_bf.hip).  SolveAll's scale goes into the blend's store (vm[0]) and into GF's
// last store (vm[1]).  All scratch is the group's own pairs' slices.
static sm_status run_gfnl(sm_ctx* c, const Group& G, bool solve_all, float w) {
    const sm_params& p = c->p;
    const size_t nv = c->nvol, np = c->npix;
    float* res = G.slice(c->gfnl_res, nv);
    sm_status s = run_nl(c, G, false, 1.f, nullptr, res);
    if (s) return s;
    if ((s = run_gf(c, 0, G, false, 1.f))) return s;
    if (n_views(p) == 2 && (s = run_gf(c, 1, G, solve_all, w))) return s;
    sm::GfnlArgs a{};
    a.gray = G.gray;   // I_g[0]
    a.gray_pair_stride = 2 * np;
    a.mask = G.slice(c->gfnl_mask, np);
    a.res = res;
    a.vm = G.vm0;
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.thresh = c->gfnl_thresh;
    a.solve_all = solve_all;
    a.scale = w;
    if ((s = timed(c, G.st, "gfnl_mask", (double)G.n * np * 2, [&] { sm::launch_gfnl_mask(a, G.n, G.st); }))) return s;
    return timed(c, G.st, "gfnl_blend", (double)G.n * nv * 12 + (double)G.n * np, [&] { sm::launch_gfnl_blend(a, G.n, G.st); });
}

// aggregation other than CBCA: GF, FIF and AWS on every view (num = Do_refine ? 2 : 1, cpp:4499, 4709-4711),
// NL on vm[0], BF on every view that exists (imgNum = Do_LRConsis ? 2 : 1, cpp:1025); SolveAll touches
// vm[1] only with Do_refine (cpp:2178)
sm_status run_other_agg(sm_ctx* c, const Group& G, bool solve_all, float w) {
    sm_status s = SM_OK;
    if (c->p.aggregation == SM_AGG_GF)
        for (int v = 0; v < n_views(c->p) && !s; v++) s = run_gf(c, v, G, solve_all, w);
    if (c->p.aggregation == SM_AGG_FIF)
        for (int v = 0; v < n_views(c->p) && !s; v++) s = run_fif(c, v, G, solve_all, w);
    if (c->p.aggregation == SM_AGG_AWS) s = run_aws(c, G, solve_all, w);
    if (c->p.aggregation == SM_AGG_NL) s = run_nl(c, G, solve_all, w);
    if (c->p.aggregation == SM_AGG_BF)
        for (int v = 0; v < (right_view(c->p) ? 2 : 1) && !s; v++) s = run_bf(c, v, G, solve_all && v < n_views(c->p), w);
    if (c->p.aggregation == SM_AGG_GFNL) s = run_gfnl(c, G, solve_all, w);
    return s;
}

// run_other_agg(.., solve_all = true, w) left SolveAll's weight in this view's volume: GF, FIF, AWS, BF and
// GFNL in every view SolveAll touches, NL in vm[0] only (sm_run scales every other view with run_scale)
bool agg_scale_fused(const sm_params& p, int view) {
    return p.aggregation == SM_AGG_GF || p.aggregation == SM_AGG_FIF || p.aggregation == SM_AGG_AWS ||
           p.aggregation == SM_AGG_BF || p.aggregation == SM_AGG_GFNL || (p.aggregation == SM_AGG_NL && view == 0);
}
