// sm_stages.cpp — the stage drivers of the default pipeline: each fills a kernel family's argument struct from
// the context and the group descriptor it is given and queues its launches on the group's stream (prep, cost
// volume, CBCA in its three forms, SolveAll's scale, dispOptimize with Do_vmTop, refine).  The other aggregations'
// drivers are in sm_stages_agg.cpp.
#include <math.h>

#include <cmath>

#include "sm_ctx.h"

// what both prep passes of run_prep share: the group's planes, the census window and window 0's arm settings
static sm::PrepArgs prep_args(const sm_ctx* c, const Group& G) {
    const sm_params& p = c->p;
    sm::PrepArgs a{};
    a.gray = G.gray;
    a.bgr = G.bgr;
    a.px = G.px;
    a.pxh = G.pxh;
    a.pxv = G.pxv;
    a.code = G.code;
    a.arms = G.arms;
    a.flags = G.flags;
    a.H = p.rows;
    a.W = p.cols;
    a.rv = p.census_rv;
    a.ru = p.census_ru;
    a.ring = p.census_ring;
    a.L = p.arm_l;
    a.L_out = p.arm_l_out;
    a.C_D = p.arm_c_thresh;
    a.C_D_out = p.arm_c_thresh_out;
    a.minL = p.arm_min_l;
    a.cor_thres = p.sgm_cor_dif_thres;
    return a;
}

sm_status run_prep(sm_ctx* c, const Group& G) {
    const sm_params& p = c->p;
    const bool census = needs_census(p), arms = needs_arms(p);
    const bool flags = p.optimization == SM_OPT_SGM;
    if (c->dw_on) {
        // window 1's arms first (calArms with cbca_crossL[1] .., cpp:4343), through the same arm kernels into
        // their own planes; the pass below then leaves the arm-walk planes as window 0 wrote them
        sm::PrepArgs a = prep_args(c, G);
        a.arms = G.slice(c->arms2, 2 * 2 * c->npix * 4);
        a.L = c->dw_l;
        a.L_out = c->dw_l_out;
        a.C_D = c->dw_ct;
        a.C_D_out = c->dw_ct_out;
        a.do_arms = 1;
        sm_status s = timed(c, G.st, "prep_dw", (double)G.n * 2 * c->npix * (3 + 8), [&] { sm::launch_prep(a, G.n, G.st); });
        if (s) return s;
    }
    {
        sm::PrepArgs a = prep_args(c, G);
        a.flags1 = flags && p.do_refine ? G.flags1 : nullptr;
        a.do_census = census;
        a.do_arms = arms;
        a.do_flags = flags;
        // the packed BGR plane's later readers: the GF image planes, so, refine's properIpol
        a.pack_px = uses_gf(p) || p.optimization == SM_OPT_SO || p.do_refine;
        return timed(c, G.st, "prep", (double)G.n * 2 * c->npix * (1 + 3 + (census ? 16 : 0) + (arms ? 8 : 0)) +
                                    (flags ? (double)G.n * c->npix * n_views(p) : 0),
                     [&] { sm::launch_prep(a, G.n, G.st); });
    }
}

// The view's cost volume is not written: its first CBCA H scan computes the costs itself
// (sm::launch_cbca_hsc, k_cost's select-free censusGrad elements with lamG == 1).  Only where CBCA
// runs on the view -- a right view that is only built keeps its cost volume.
bool cost_scan_fused(const sm_ctx* c, int view) {
    const sm_params& p = c->p;
    const int cw = (census_len(p) + 31) / 32;
    // (the double window runs the sweep once per arm set: the longer lag decides)
    const int lag = c->dw_on ? std::max(cbca_lag(p), cbca_lag2(c)) : cbca_lag(p);
    // (without arm intersection the costs come from the cost volume: the fused scan is the intersecting sweep)
    return c->fuse_cost_scan && !c->ni_on && p.aggregation == SM_AGG_CBCA && cbca_iters(c) > 0 && view < n_views(p) &&
           p.cost_method == SM_COST_CENSUS_GRAD && cw >= 3 && p.lam_g == 1.0f &&
           sm::cost_nosel_ok(p.grad_trunc, p.lam_g, (float)census_len(p)) &&
           sm::cbca_hsc_smem_bytes(lag, cw) <= 64 * 1024;
}

sm_status run_cost(sm_ctx* c, int view, const Group& G) {
    const sm_params& p = c->p;
    if (cost_scan_fused(c, view)) return SM_OK;
    sm::CostArgs a{};
    a.vm = G.vm(view);
    a.code = G.code;
    a.gray = G.gray;
    a.arms = G.arms;
    a.bgr = G.bgr;
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.view = view;
    a.nwords = (census_len(p) + 63) / 64;
    a.cwords = (census_len(p) + 31) / 32;
    a.census_default = (float)census_len(p) * 1.0f;
    a.grad_trunc = p.grad_trunc;
    a.grad_oor = (float)sqrt(pow((double)p.grad_trunc, 2) * 2);
    a.grad_adaptive = p.grad_adaptive;
    a.lam2 = p.lam_g;
    a.ad_trunc = p.ad_trunc_ad;
    a.ad_oor_exp = c->ad_oor_exp;
    a.lut = c->luts;
    if (cost_ext(p)) {
        // the literals of the reference's call sites: adGrad gen_ad_sd_vm(.., 0, 7), grad(.., 2) (cpp:60-62);
        // ADCensusGrad asdCal("AD", .., 255), grad(.., 500) (cpp:930-935); SD shares asdCal(.., 20) with AD
        if (p.cost_method == SM_COST_AD_GRAD) {
            a.ad_trunc = 7.0f;
            a.grad_trunc = 2.0f;
        } else if (p.cost_method == SM_COST_AD_CENSUS_GRAD) {
            a.ad_trunc = 255.0f;
            a.grad_trunc = 500.0f;
        }
        a.grad_oor = (float)sqrt(pow((double)a.grad_trunc, 2) * 2);
        const int m = p.cost_method;   // sm::SM_M_SD .. carry sm_cost_method's values
        return timed(c, G.st, view == 0 ? "cost_volume" : "cost_volume_right", (double)G.n * c->nvol * 4.0,
                     [&] { sm::launch_cost_ext(a, m, G.n, G.st); });
    }
    const int m = p.cost_method == SM_COST_CENSUS_GRAD ? sm::SM_M_CENSUS_GRAD
                  : p.cost_method == SM_COST_CENSUS    ? sm::SM_M_CENSUS
                  : p.cost_method == SM_COST_AD_CENSUS ? sm::SM_M_AD_CENSUS
                                                       : sm::SM_M_AD;
    return timed(c, G.st, view == 0 ? "cost_volume" : "cost_volume_right", (double)G.n * c->nvol * 4.0,
                 [&] { sm::launch_cost(a, m, G.n, G.st); });
}

// cbca_core with cbca_intersect == false (cpp:5585-5666) on a view: the arms of the view's own image, one area per
// pixel.  Each 1-D pass is a prefix kernel (in place) and a window kernel that writes the other volume of the
// ping-pong (the view's volume -> ni_tmp -> the view's volume), so every iteration ends in the view's volume;
// its second window kernel divides by the area and, in the last iteration of sm_run, applies SolveAll's weight
// (scaling an element commutes with nothing else after the division).  The areas ping-pong between the two
// planes the same way and end in plane 0.
static sm_status run_cbca_ni(sm_ctx* c, int view, bool fuse_scale, float w, const Group& G, int win) {
    const sm_params& p = c->p;
    const int N = cbca_iters(c);
    float* vol = win ? G.slice(c->vm2, c->nvol) : G.vm(view);
    float* tmp = G.slice(c->ni_tmp, c->nvol);
    sm::NiArgs a{};
    a.arms = (const uint32_t*)(win ? G.slice(c->arms2, 2 * 2 * c->npix * 4) : G.arms);
    a.area = G.slice(c->ni_area, 4 * c->npix);
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.view = view;
    a.scale = w;
    // algorithmic bytes: the prefix reads and writes the volume; the window reads every prefix position once
    // from memory (it is the head of one pixel and the tail of another) and writes the other volume
    const double bytes = (double)G.n * c->nvol * 8.0;
    const std::string sfx = Group::name("", view) + (win ? "_dw" : "") + "_ni";
    sm_status s;
    for (int k = 0; k < N; k++) {
        for (int pass = 0; pass < 2; pass++) {
            a.horiz = (k % 2 == 0) == (pass == 0) ? 1 : 0;   // H then V for even k, V then H for odd k
            a.src = pass == 0 ? vol : tmp;
            a.dst = pass == 0 ? tmp : vol;
            a.in_plane = pass;
            a.first = pass == 0;
            a.norm = pass == 1;
            a.apply_scale = fuse_scale && pass == 1 && k + 1 == N ? 1 : 0;
            const std::string dir = a.horiz ? "cbca_h_" : "cbca_v_";
            if ((s = timed(c, G.st, (dir + "prefix" + sfx).c_str(), bytes, [&] { sm::launch_ni_prefix(a, G.n, G.st); }))) return s;
            if ((s = timed(c, G.st, (dir + (a.norm ? "window_norm" : "window") + sfx).c_str(), bytes,
                           [&] { sm::launch_ni_window(a, G.n, G.st); })))
                return s;
            // the next group may start (as after the intersecting form's first sweep)
            if (!win && view == 0 && k == 0 && pass == 0 && G.stagger_ev) HIP_TRY(c, hipEventRecord(G.stagger_ev, G.st));
        }
    }
    c->ni_ran = true;
    return SM_OK;
}

// One cbca_core run on a view.  win 0: the view's volume with the window-0 arms (the only run without the
// double window).  win 1: the double window's large-window run, on the second volume with window 1's arms,
// lag and ring size; it records none of the group's events (the window-0 run that follows reads the same
// inputs last).
static sm_status run_cbca_core(sm_ctx* c, int view, bool fuse_scale, float w, const Group& G, int win) {
    // cbca_core (cpp:5585-5666): iteration k runs H then V for even k, V then H for odd k.
    // The last pass of iteration k and the first pass of iteration k+1 share a direction and
    // are fused into one CB_NORM_SCAN sweep, so N iterations take N + 1 sweeps.
    const sm_params& p = c->p;
    const int N = cbca_iters(c);
    if (N <= 0) return SM_OK;
    if (c->ni_on) return run_cbca_ni(c, view, fuse_scale, w, G, win);
    sm::CbcaArgs a{};
    a.vm = win ? G.slice(c->vm2, c->nvol) : G.vm(view);
    a.view = view;
    a.dummy = c->dummy;
    a.arms = (const uint32_t*)(win ? G.slice(c->arms2, 2 * 2 * c->npix * 4) : G.arms);
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.lag = win ? cbca_lag2(c) : cbca_lag(p);
    a.vm_end = (win ? c->vm2 : (view == 0 ? c->vm0 : c->vm1)) + (size_t)c->cap * c->nvol + c->vtail;   // incl. the tail pad
    a.arms_end = (const uint32_t*)(win ? c->arms2 + c->arms2_bytes : c->arms + c->arms_bytes);
    a.scale = w;
    a.apply_scale = 0;
    a.num_cu = c->num_cu;
    a.arm_pad_rows = 2 * a.lag;
    const double bytes = (double)G.n * c->nvol * 8.0;
    // profile names: "cbca_h_scan" etc. for vm[0], "cbca_h_scan_r" etc. for vm[1]; "_dw" for the large window
    auto nm = [&](const char* base) { return Group::name(base, view) + (win ? "_dw" : ""); };
    sm_status s;
    if (cost_scan_fused(c, view)) {   // the costs are computed in the sweep: it only writes the volume
        a.code = G.code;
        a.gray = G.gray;
        a.lut = c->luts;
        a.census_default = (float)census_len(p) * 1.0f;
        a.grad_trunc = p.grad_trunc;
        a.grad_adaptive = p.grad_adaptive;
        a.cwords = (census_len(p) + 31) / 32;
        // grad() built its adaptive weights from window 0's arms (cpp:630-633), before CBCA() made window 1's
        a.cost_arms = win ? (const uint32_t*)G.arms : nullptr;
        s = timed(c, G.st, nm("cbca_h_scan_cost"), (double)G.n * c->nvol * 4.0, [&] { sm::launch_cbca_hsc(a, G.n, G.st); });
    } else {
        s = timed(c, G.st, nm("cbca_h_scan"), bytes, [&] { sm::launch_cbca(a, true, sm::CB_SCAN, G.n, G.st); });
    }
    if (s) return s;
    // the last sweep that reads the group's input images
    if (!win && view == n_views(p) - 1 && G.in_ev) HIP_TRY(c, hipEventRecord(G.in_ev, G.st));
    // the next group may start: this group's next sweep is LDS- and issue-bound
    if (!win && view == 0 && G.stagger_ev) HIP_TRY(c, hipEventRecord(G.stagger_ev, G.st));
    for (int k = 0; k < N; k++) {
        const bool dir_h = (k % 2 == 1);  // direction of iteration k's second pass
        a.div_safe = cbca_div_safe(p, k) ? 1 : 0;   // this step's normalisation is iteration k's
        if (k + 1 < N && c->fuse_norm_scan) {
            s = timed(c, G.st, nm(dir_h ? "cbca_h_norm_scan" : "cbca_v_norm_scan"), bytes,
                      [&] { sm::launch_cbca(a, dir_h, sm::CB_NORM_SCAN, G.n, G.st); });
        } else if (k + 1 < N) {
            s = timed(c, G.st, nm(dir_h ? "cbca_h_norm" : "cbca_v_norm"), bytes,
                      [&] { sm::launch_cbca(a, dir_h, sm::CB_NORM, G.n, G.st); });
            if (s) return s;
            s = timed(c, G.st, nm(dir_h ? "cbca_h_scan" : "cbca_v_scan"), bytes,
                      [&] { sm::launch_cbca(a, dir_h, sm::CB_SCAN, G.n, G.st); });
        } else {
            a.apply_scale = fuse_scale ? 1 : 0;
            s = timed(c, G.st, nm(dir_h ? "cbca_h_norm" : "cbca_v_norm"), bytes,
                      [&] { sm::launch_cbca(a, dir_h, sm::CB_NORM, G.n, G.st); });
        }
        if (s) return s;
    }
    return SM_OK;
}

// CBCA() on one view (cpp:4333-4360).  With the double window: the large-window run on a second volume that
// starts from the same raw costs (its own fused first scan where the costs are computed in the sweep -- with
// window 0's arms for the gradient term's weights, as grad() computed them -- else one device copy of the raw
// volume), the window-0 run in place, then combine2Vm_4: the mask from the LEFT image's window-0 arms (made
// once, with view 0) and the selection.  SolveAll's weight is fused into the last normalising pass of both
// runs: every element of the composed volume is one of the two runs' elements, and scaling an element commutes
// with choosing it, so the result equals "compose, then scale" bit for bit.
sm_status run_cbca(sm_ctx* c, int view, bool fuse_scale, float w, const Group& G) {
    if (!c->dw_on) return run_cbca_core(c, view, fuse_scale, w, G, 0);
    const sm_params& p = c->p;
    sm_status s;
    if (!cost_scan_fused(c, view)) {
        const float* raw = G.vm(view);
        float* dst = G.slice(c->vm2, c->nvol);
        const size_t bytes = (size_t)G.n * c->nvol * 4;
        hipError_t e = hipSuccess;
        s = timed(c, G.st, Group::name("dw_copy_raw", view), 2.0 * bytes,
                  [&] { e = hipMemcpyAsync(dst, raw, bytes, hipMemcpyDeviceToDevice, G.st); });
        if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync (raw costs for the large window)");
        if (s) return s;
    }
    if ((s = run_cbca_core(c, view, fuse_scale, w, G, 1))) return s;
    if ((s = run_cbca_core(c, view, fuse_scale, w, G, 0))) return s;
    sm::DwArgs a{};
    a.arms = (const uint32_t*)G.arms;
    a.mask = c->dw_mask;
    a.vm = view == 0 ? c->vm0 : c->vm1;
    a.vm2 = c->vm2;
    a.pix0 = (size_t)G.off * c->npix;
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.isum = c->dw_isum;
    if (view == 0) {
        if ((s = timed(c, G.st, "dw_mask", (double)G.n * c->npix * 9.0, [&] { sm::launch_dw_mask(a, G.n, G.st); }))) return s;
        c->dw_ran = true;
    }
    // (algorithmic bytes: the mask; the volume traffic is 8 B per selected element, known only from the mask)
    return timed(c, G.st, Group::name("dw_select", view), (double)G.n * c->npix, [&] { sm::launch_dw_select(a, G.n, G.st); });
}

sm_status run_scale(sm_ctx* c, int view, float w, const Group& G) {
    return timed(c, G.st, Group::name("solve_all_scale", view), (double)G.n * c->nvol * 8.0,
                 [&] { sm::launch_scale(G.vm(view), (size_t)G.n * c->nvol, w, G.st); });
}

// Do_vmTop (cpp:1111-1121): selectTopCostFromVolumn on vm[view] as the optimiser left it, then
// genDispFromTopCostVm2 into DP[view]; I_c[0] is the colour image for both views
static sm_status run_vmtop(sm_ctx* c, int view, const Group& G, const float* vm, int16_t* disp) {
    const sm_params& p = c->p;
    const size_t T = (size_t)p.cols + 2 * (size_t)p.rows;
    sm::VmTopArgs a{};
    a.vm = vm;
    a.tab = G.slice(c->vt_tab + (size_t)view * c->cap * c->npix * c->vt_num, c->npix * c->vt_num);
    a.cnt = G.slice(c->vt_cnt + (size_t)view * c->cap * c->npix, c->npix);
    a.tcnt = G.slice(c->vt_tcnt, T);
    a.bgr = G.bgr;
    a.disp = disp;
    a.H = p.rows;
    a.W = p.cols;
    a.D = p.num_disparities;
    a.M = c->vt_num;
    a.n = G.n;
    a.thres = c->vt_thres;
    a.method = c->vt_method;
    a.ts = c->vt_ts;
    a.has_cir2 = c->vt_cir2;
    a.color_limit = c->vt_color;
    const double np = (double)G.n * c->npix, tab = 8.0 * a.M + 4;
    sm_status s = timed(c, G.st, Group::name("vmtop_select", view), (double)G.n * c->nvol * 4.0 + np * tab,
                        [&] { sm::launch_vmtop_select(a, G.st); });
    if (s) return s;
    c->vt_ran_num[view] = a.M;
    if (a.method == 0) {
        HIP_TRY(c, hipMemsetAsync(a.tcnt, 0, (size_t)G.n * T * sizeof(int), G.st));
        if ((s = timed(c, G.st, Group::name("vmtop_decide0_a", view), np * (9 * tab + 2),
                       [&] { sm::launch_vmtop_decide0_a(a, G.st); })))
            return s;
        for (int r = 0; r < sm::VMTOP_RELAX_ROUNDS; r++)
            if ((s = timed(c, G.st, Group::name("vmtop_decide0_w", view), np * 2, [&] { sm::launch_vmtop_decide0_w(a, G.st); })))
                return s;
        return timed(c, G.st, Group::name("vmtop_decide0_b", view), (double)G.n * T * 4 + np * 2,
                     [&] { sm::launch_vmtop_decide0_b(a, G.st); });
    }
    return timed(c, G.st, Group::name("vmtop_decide12", view), np * (tab + 2), [&] { sm::launch_vmtop_decide12(a, G.st); });
}

// dispOptimize (cpp:1046-1136) for one view: vm[0] with the left image's penalty flags
// (leftFirst = true) -> DP[0]; vm[1] with the right image's (leftFirst = false) -> DP[1].
sm_status run_optimize(sm_ctx* c, int view, const Group& G) {
    const sm_params& p = c->p;
    float* vm = G.vm(view);
    int16_t* disp = G.map(view);
    // Do_vmTop replaces gen_dispFromVm after "sgm" and "" (cpp:1108-1128); "so" never reaches it.  SGM then
    // writes its path sum into vm[view] (the keep_final_volume path) for the selection to read
    const bool vmtop = c->vt_on && p.optimization != SM_OPT_SO;
    // refine()'s calPKR and subpixelEnhancement read vm[0] as dispOptimize left it: the path sum (cpp:1380, 6152)
    const int keep_final = p.keep_final_volume || vmtop || (view == 0 && refine_reads_volume(c));
    if (p.optimization == SM_OPT_SGM) {
        static const int RV[8] = {+1, -1, 0, 0, +1, +1, -1, -1};  // cpp:6207
        static const int RU[8] = {0, 0, +1, -1, -1, +1, +1, -1};  // cpp:6208
        static const char* NAMES[8] = {"sgm_path0", "sgm_path1", "sgm_path2", "sgm_path3",
                                       "sgm_path4", "sgm_path5", "sgm_path6", "sgm_path7"};
        sm::SgmArgs a{};
        a.flags = G.penalty(view);
        a.dummy = c->dummy;
        a.vm = vm;
        a.acc = G.acc;
        a.bgr = G.bgr;
        a.disp = disp;
        a.H = p.rows;
        a.W = p.cols;
        a.D = p.num_disparities;
        a.p1 = p.sgm_p1;
        a.p2 = p.sgm_p2;
        a.cor_thres = p.sgm_cor_dif_thres;
        a.redu = p.sgm_redu_coeff;
        a.keep_final = keep_final;
        // the guided filter's output can be < 0.  FIF's cannot (so it stays false there, and "so"
        // applies too): with costs and weights >= +0 rounding is monotone, so c1, c2 >= vm, hence
        // fl(c1 + c2) >= vm and A = fl(fl(c1 + c2) - vm) >= +0; the vertical pass likewise
        // BF's are >= +0 while its sums are exact (bf_exact)
        a.signed_costs = uses_gf(p) || (p.aggregation == SM_AGG_BF && !bf_exact(p));
        int first = 0;   // first path left to the plain sweeps
        if (G.ck) {
            // checkpointed pairs (0, 1) and (2, 3): 4 + 8 + 4 + 8 B per element (+ 4 / S for
            // the checkpoints each way) instead of 8 + 12 + 12 + 8; with 8 paths the second
            // pair adds into the running sum (12 B) and paths 4 .. 7 follow as sweeps
            a.ck = G.ck;
            const double ckb = 4.0 / sm::sgm_ck_seg(p.num_disparities);
            const double nv = (double)G.n * c->nvol;
            const bool four = p.sgm_paths == 4;
            struct Pass { int path, mode; const char* name; double per; };
            const Pass passes[4] = {
                {0, sm::CK_A, "sgm_ck_a01", 4.0 + ckb},
                {0, sm::CK_B, "sgm_ck_b01", 8.0 + ckb},
                {2, sm::CK_A, "sgm_ck_a23", 4.0 + ckb},
                four ? Pass{2, sm::CK_B | sm::SGM_LAST, "sgm_last_wta", 8.0 + ckb + (keep_final ? 4.0 : 0)}
                     : Pass{2, sm::CK_B | sm::CK_MID, "sgm_ck_b23", 12.0 + ckb}};
            for (const Pass& ps : passes) {
                a.rv = RV[ps.path];
                a.ru = RU[ps.path];
                a.dir = ps.path;
                a.dir2 = ps.path + 1;
                const double bytes = nv * ps.per + ((ps.mode & sm::SGM_LAST) ? (double)G.n * c->npix * 2 : 0);
                const std::string name = Group::name(ps.name, view);
                sm_status s = timed(c, G.st, name.c_str(), bytes, [&] { sm::launch_sgm_ck(a, ps.mode, G.n, G.st); });
                if (s) return s;
            }
            first = 4;
            if (G.lx) {
                // 8 paths: the diagonal pair (4, 6) with L5 between them (sm_sgm.hip): pass A of
                // path 4, path 5 as an SGM_FIRST sweep storing L5, pass B of path 6 reading acc and
                // L5 (acc = ((acc + L4) + L5) + L6); path 7 follows as the last sweep
                const double ckd = 4.0 / sm::sgm_ck_diag_seg();
                a.rv = RV[4];
                a.ru = RU[4];
                a.dir = 4;
                a.dir2 = 6;
                sm_status s = timed(c, G.st, Group::name("sgm_ck_a46", view), nv * (4.0 + ckd),
                                    [&] { sm::launch_sgm_ck(a, sm::CK_A, G.n, G.st); });
                if (s) return s;
                sm::SgmArgs a5 = a;
                a5.rv = RV[5];
                a5.ru = RU[5];
                a5.dir = 5;
                a5.acc = G.lx;   // SGM_FIRST stores 0 + L5 == L5 (path costs are never -0)
                s = timed(c, G.st, Group::name("sgm_l5", view), nv * 8.0,
                          [&] { sm::launch_sgm_path(a5, sm::SGM_FIRST, G.n, G.st); });
                if (s) return s;
                a.lx = G.lx;
                s = timed(c, G.st, Group::name("sgm_ck_b46", view), nv * (16.0 + ckd),
                          [&] { sm::launch_sgm_ck(a, sm::CK_B | sm::CK_MID | sm::CK_X, G.n, G.st); });
                if (s) return s;
                first = 7;
            }
        }
        for (int i = first; i < p.sgm_paths; i++) {
            a.rv = RV[i];
            a.ru = RU[i];
            a.dir = i;
            int mode = (i == 0 ? sm::SGM_FIRST : 0) | (i == p.sgm_paths - 1 ? sm::SGM_LAST : 0);
            // algorithmic bytes per element: read C (+ read acc) (+ write acc | write final)
            double per = 4.0 + ((mode & sm::SGM_FIRST) ? 0 : 4.0) + ((mode & sm::SGM_LAST) ? (keep_final ? 4.0 : 0) : 4.0);
            double bytes = (double)G.n * c->nvol * per + ((mode & sm::SGM_LAST) ? (double)G.n * c->npix * 2 : 0);
            const std::string name = Group::name((mode & sm::SGM_LAST) ? "sgm_last_wta" : NAMES[i], view);
            sm_status s = timed(c, G.st, name.c_str(), bytes, [&] { sm::launch_sgm_path(a, mode, G.n, G.st); });
            if (s) return s;
        }
    } else if (p.optimization == SM_OPT_SO) {
        // so(vm[i], DP[i], I_c) reads I[0] — the left colours — for both views (cpp:1098, 6284)
        sm::SoArgs a{};
        a.vm = vm;
        a.trace = G.slice(c->so_trace, c->nvol);
        a.cidx = G.slice(c->so_cidx, c->npix);
        a.px = G.px;
        a.disp = disp;
        a.H = p.rows;
        a.W = p.cols;
        a.D = p.num_disparities;
        a.n = G.n;
        a.keep_final = p.keep_final_volume;
        a.pn2 = c->so_pn2;
        a.pn3 = c->so_pn3;
        a.float_minima = c->so_float_minima;
        // the call commented in at cpp:1096-1100 (sm_so_config)
        if (c->so_variant == SM_SO_T2D) {
            // so_T2D(vm_res, ..) runs on a clone (cpp:1095, 1097): vm[i] is read (4 B per element), never written
            a.keep_final = 0;
            const std::string name = Group::name("so_t2d", view);
            sm_status s = timed(c, G.st, name.c_str(), (double)G.n * c->nvol * 4.0, [&] { sm::launch_so_t2d(a, G.st); });
            if (s) return s;
        } else {
            a.r2l = c->so_variant == SM_SO_R2L;
            const std::string name = Group::name(a.r2l ? "so_r2l" : "so", view);
            sm_status s = timed(c, G.st, name.c_str(), (double)G.n * c->nvol * (4.0 + 1.0 + (p.keep_final_volume ? 4.0 : 0)),
                                [&] { sm::launch_so(a, G.st); });
            if (s) return s;
        }
    } else if (!vmtop) {
        const std::string name = Group::name("wta", view);
        sm_status s = timed(c, G.st, name.c_str(), (double)G.n * c->nvol * 4.0 + (double)G.n * c->npix * 2,
                            [&] { sm::launch_wta(vm, disp, G.n, p.rows, p.cols, p.num_disparities, G.st); });
        if (s) return s;
    }
    if (vmtop) {
        sm_status s = run_vmtop(c, view, G, vm, disp);
        if (s) return s;
    }
    if (c->ev_on && view == 0) {   // saveFromDisp<short, 0>(DP[0], "so" | name) (cpp:1102, 1131): the table's stage 0
        sm_status s = run_eval_stage(c, G, 0, disp);
        return s ? s : run_eval_final(c, G, 0, 1);
    }
    return SM_OK;
}

static sm::DaArgs da_args(sm_ctx* c, const Group& G) {
    sm::DaArgs a{};
    a.u8 = G.slice(c->da_u8, (size_t)sm::DA_PLANES * c->npix);
    a.mag = G.slice(c->da_mag, c->npix);
    a.lab = G.slice(c->da_lab, c->npix);
    a.hist = G.slice(c->da_hist, 256);
    a.H = c->p.rows;
    a.W = c->p.cols;
    a.n = G.n;
    a.low = std::min(c->da_low, c->da_high);   // Canny swaps thresholds given in the wrong order
    a.high = std::max(c->da_low, c->da_high);
    a.ks = c->da_ks;
    a.kc = c->da_kc;
    return a;
}

// discontinuityAdjust's image stages (cpp:6059-6064) for the group's pairs, entered at `first`: 0 equalizeHist (on
// `dp` as 8 bits, or with dp null on the image already in the DA_EQ plane), 1 GaussianBlur (on DA_EQ), 2 Canny (on
// DA_BLUR); the edge map ends in the DA_EDGE plane.  A fixed sequence of launches, nothing read back.
sm_status run_da_image(sm_ctx* c, const Group& G, int first, const int16_t* dp) {
    const sm::DaArgs a = da_args(c, G);
    const double np = (double)G.n * c->npix;
    sm_status s;
    if (first <= 0) {
        HIP_TRY(c, hipMemsetAsync(a.hist, 0, (size_t)G.n * 256 * sizeof(int), G.st));
        if ((s = timed(c, G.st, "refine_da_hist", np * (dp ? 3 : 1), [&] { sm::launch_da_hist(a, dp, G.st); }))) return s;
        if ((s = timed(c, G.st, "refine_da_equalize", np * 2, [&] { sm::launch_da_equalize(a, G.st); }))) return s;
    }
    if (first <= 1 && (s = timed(c, G.st, "refine_da_blur", np * 2, [&] { sm::launch_da_blur(a, G.st); }))) return s;
    if ((s = timed(c, G.st, "refine_da_sobel", np * 3, [&] { sm::launch_da_sobel(a, G.st); }))) return s;
    if ((s = timed(c, G.st, "refine_da_nms", np * (2 + 1 + 1 + 4), [&] { sm::launch_da_nms(a, G.st); }))) return s;
    if ((s = timed(c, G.st, "refine_da_link", np * (1 + 4), [&] { sm::launch_da_link(a, G.st); }))) return s;
    if ((s = timed(c, G.st, "refine_da_mark", np * 1, [&] { sm::launch_da_mark(a, G.st); }))) return s;
    return timed(c, G.st, "refine_da_edges", np * (1 + 4 + 1), [&] { sm::launch_da_edges(a, G.st); });
}

// refine(), non-USE_RECONCV branch (cpp:1347-1510), on DP[0] of n pairs: LR check (in place),
// region votes and proper interpolations (Jacobi, ping-pong with disp_tmp), 3x3 median.
sm_status run_refine(sm_ctx* c, const Group& G) {
    const sm_params& p = c->p;
    const int H = p.rows, W = p.cols;
    const double map = (double)G.n * c->npix * 2;
    const double np = (double)G.n * c->npix;
    sm_status s;
    // the error table (sm_eval_config): one entry wherever the reference calls saveFromDisp<short, 0> on DP[0],
    // in eval_stage_names' order; stage 0 is run_optimize's
    int es = 1;
    auto saved = [&](const int16_t* m) { return c->ev_on ? run_eval_stage(c, G, es++, m) : SM_OK; };
    if (c->oc_classify) {   // LRConsistencyCheck (cpp:2284-2335) in place of LRConsistencyCheck_normal (cpp:1364-1367)
        uint8_t* mask = G.slice(c->oc_mask, c->npix);
        // reads DP[0] and DP[1], writes the labels and the mask
        s = timed(c, G.st, "refine_lr_classify", np * (2 + 2 + 2 + 1), [&] {
            sm::launch_lr_classify(G.disp, G.disp1, mask, G.n, H, W, p.num_disparities, p.lr_max_diff, p.disp_occ,
                                   c->oc_disp_mis, G.st);
        });
        c->oc_ran = true;
    } else {
        s = timed(c, G.st, "refine_lr_check", 3 * map,
                  [&] { sm::launch_lr_check(G.disp, G.disp1, G.n, H, W, p.lr_max_diff, G.st); });
    }
    if (s || (s = saved(G.disp))) return s;   // "od" (cpp:1373)
    if (c->rx_pkr) {   // calPKR + signDp_UsingPKR (cpp:1378-1383) on vm[0] as dispOptimize left it
        sm::PkrArgs a{};
        a.vm = G.vm0;
        a.mask = G.slice(c->pkr_mask, c->npix);
        a.disp = G.disp;
        a.H = H;
        a.W = W;
        a.D = p.num_disparities;
        a.n = G.n;
        a.ratio = c->rx_ratio;
        a.disp_pkr = c->rx_disp_pkr;
        if ((s = timed(c, G.st, "refine_pkr", (double)G.n * c->nvol * 4.0 + np * 5, [&] { sm::launch_pkr(a, G.st); }))) return s;
        c->rx_pkr_ran = true;
        if ((s = saved(G.disp))) return s;   // "PKR" (cpp:1382)
    }
    int16_t* cur = G.disp;
    int16_t* nxt = G.disp_tmp;
    const uint32_t* arms = (const uint32_t*)G.arms;
    if (p.do_region_vote)
        for (int i = 0; i < p.region_vote_nums; i++) {
            if (c->oc_rv) {   // RV_combine_BG (cpp:7146-7216) in place of regionVote_my (cpp:1404-1408)
                sm::RvcArgs a{};
                a.src = cur;
                a.dst = nxt;
                const bool carry = c->oc_type >= 2;   // a hole of neither class takes the last classified hole's result
                a.cand = carry ? G.slice(c->oc_cand, c->npix) : nullptr;
                a.rowlast = carry ? G.slice(c->oc_rowlast, (size_t)H) : nullptr;
                a.arms = arms;
                a.H = H;
                a.W = W;
                a.D = p.num_disparities;
                a.n = G.n;
                a.rv_s = p.rv_s;
                a.rv_ratio = p.rv_ratio;
                a.depth = c->rx_depth;
                a.type = c->oc_type;
                a.disp_occ = p.disp_occ;
                a.disp_mis = c->oc_disp_mis;
                if ((s = timed(c, G.st, "refine_rv_combine", map * (carry ? 3 : 2), [&] { sm::launch_rv_combine(a, G.st); }))) return s;
                // k_rv_row_last reads the scratch map and writes a value per row; k_rv_carry reads the map, the scratch
                // map and the rows' values
                if (carry && (s = timed(c, G.st, "refine_rv_carry", 3 * map + 4.0 * G.n * H, [&] { sm::launch_rv_carry(a, G.st); })))
                    return s;
            } else if ((s = timed(c, G.st, "refine_region_vote", 2 * map, [&] {
                            sm::launch_region_vote(cur, nxt, arms, G.n, H, W, p.rv_s, p.rv_ratio, G.st);
                        }))) {
                return s;
            }
            std::swap(cur, nxt);
            if ((s = saved(cur))) return s;   // "RV<i>" (cpp:1420)
        }
    if (p.do_proper_ipol) {
        for (int i = 0; i < p.region_vote_nums; i++) {
            if ((s = timed(c, G.st, "refine_proper_ipol", 2 * map,
                           [&] { sm::launch_proper_ipol(cur, nxt, G.px, G.n, H, W, p.disp_occ, G.st); })))
                return s;
            std::swap(cur, nxt);
        }
        if ((s = saved(cur))) return s;   // "pi", once (cpp:1448)
    }
    if (c->rx_bg && c->rx_depth > 0) {   // BGIpol (cpp:1454-1465); a depth of 0 searches nothing
        sm::BgArgs a{};
        a.src = cur;
        a.r = nxt;
        a.H = H;
        a.W = W;
        a.n = G.n;
        a.depth = c->rx_depth;
        // k_bg_r reads the map and writes r; k_bg_scan reads both and writes the map
        if ((s = timed(c, G.st, "refine_bg_ipol", 4 * map, [&] { sm::launch_bg_ipol(a, G.st); }))) return s;
        std::swap(cur, nxt);
    }
    if (c->rx_bg && (s = saved(cur))) return s;   // "BG" (cpp:1459), also where depth 0 skipped the kernel
    if (c->da_on) {   // discontinuityAdjust(DP[0]) (cpp:1473-1476) on vm[0] as dispOptimize left it
        const sm::DaArgs a = da_args(c, G);
        if (c->da_user_on) {   // sm_set_da_edges: the supplied map for every pair
            for (int i = 0; i < G.n; i++)
                HIP_TRY(c, hipMemcpyAsync(a.u8 + ((size_t)i * sm::DA_PLANES + sm::DA_EDGE) * c->npix, c->da_user, c->npix,
                                          hipMemcpyDeviceToDevice, G.st));
        } else if ((s = run_da_image(c, G, 0, cur))) {
            return s;
        }
        // k_da_dir reads the map and the edge map's 3 x 3, writes the copy and the directions; k_da_adjust touches
        // the directions and, per pixel it can change, three map values and three costs
        if ((s = timed(c, G.st, "refine_da_dir", np * (2 + 1 + 2 + 1), [&] { sm::launch_da_dir(a, cur, nxt, G.st); }))) return s;
        if ((s = timed(c, G.st, "refine_da_adjust", np * 1,
                       [&] { sm::launch_da_adjust(a, cur, nxt, G.vm0, p.num_disparities, G.st); })))
            return s;
        std::swap(cur, nxt);
        c->da_ran = true;
        if ((s = saved(cur))) return s;   // "da" (cpp:1477)
    }
    if (c->rx_se) {   // subpixelEnhancement + medianBlur(SE, SE, 3) (cpp:1482-1495); DP[0] stays
        float* raw = G.slice(c->se_tmp, c->npix);
        float* out = G.slice(c->se, c->npix);
        const int keep = c->rx_mode == SM_SE_FLOAT;
        if ((s = timed(c, G.st, "refine_subpixel", np * (2 + 12 + 4), [&] {
                 sm::launch_subpixel(cur, G.vm0, raw, G.n, H, W, p.num_disparities, keep, G.st);
             })))
            return s;
        if ((s = timed(c, G.st, "refine_median3_f32", np * 8, [&] { sm::launch_median3_f32(raw, out, G.n, H, W, G.st); }))) return s;
        c->rx_se_ran = true;
    }
    if (p.do_last_median_blur) {
        if ((s = timed(c, G.st, "refine_median3", 2 * map, [&] { sm::launch_median3(cur, nxt, G.n, H, W, G.st); }))) return s;
        std::swap(cur, nxt);
        if ((s = saved(cur))) return s;   // "mb" (cpp:1501)
    }
    if (c->ev_on && (s = run_eval_final(c, G, 1, es - 1))) return s;
    if (cur != G.disp) HIP_TRY(c, hipMemcpyAsync(G.disp, cur, (size_t)map, hipMemcpyDeviceToDevice, G.st));
    return SM_OK;
}
