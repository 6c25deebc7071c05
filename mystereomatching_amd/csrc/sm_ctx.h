// sm_ctx.h — internal to the host side of libsm_hip.so (not installed): the context behind the C ABI's opaque
// sm_ctx and the helpers every host file uses -- error returns, the profiling bracket around a launch on a given
// stream, device memory and events through the context's registries, the group descriptor every stage driver takes
// (a group's buffer pointers, pairs, stream and lane), the entry checks -- and the declarations of what crosses the
// host files.  c->st is the context's main stream from sm_create to sm_destroy and nothing else: where a launch goes
// is the descriptor's business.  None of these names is exported (-fvisibility=hidden).
#pragma once
#include "../../include/sm_capi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "sm_eval_core.h"
#include "sm_kernels.h"

struct ProfRec {
    int kernel;
    hipEvent_t start, stop;
};

struct ProfStat {
    int64_t launches = 0;
    double total_ms = 0;
    double bytes = 0;  // algorithmic bytes per launch (last seen)
};

struct sm_ctx {
    sm_params p{};
    int device = 0;
    hipStream_t st = nullptr;   // the main stream (sm_create .. sm_destroy; never reassigned)
    std::string err;
    std::vector<void*> allocs;  // every device buffer the context owns (dalloc / dfree)
    std::vector<hipEvent_t> events;   // every untimed event the context owns (use_event)
    int cap = 1;
    size_t npix = 0, nvol = 0;
    size_t vtail = 0;           // floats of tail pad after each volume's cap * nvol
    uint8_t* bgr = nullptr;     // [cap][2][npix][3]
    uint8_t* gray = nullptr;    // [cap][2][npix]
    ulonglong2* code = nullptr; // [cap][2][npix]
    uint8_t* arms = nullptr;    // [cap][2 views][2 planes][npix] u32: (L | R<<16), (U | D<<16)
    uint8_t* arms_alloc = nullptr;  // arms - front pad of 2 * lag rows (CBCA V sweeps read there)
    size_t arms_bytes = 0;
    float* vm0 = nullptr;       // [cap][npix][D]
    float* vm1 = nullptr;       // [cap][npix][D] (right view, optional)
    float* acc = nullptr;       // [cap][npix][D]
    float* ck = nullptr;        // [cap][ck_pair]: checkpointed SGM path pairs (k_sgm_ck)
    size_t ck_pair = 0;         // floats per pair: lines x segments x D of the longer direction
    float* lx = nullptr;        // [cap][npix][D]: L5 between the diagonal pair (8 paths, sgm_ck_diag_ok)
    int16_t* disp = nullptr;    // [cap][npix] DP[0]
    int16_t* disp1 = nullptr;   // [cap][npix] DP[1] (do_refine)
    int16_t* disp_tmp = nullptr;// [cap][npix] refine ping-pong (do_refine)
    float* dummy = nullptr;     // 64 floats written by lanes past D
    uint8_t* flags = nullptr;   // [cap][npix] SGM colour-difference penalty bits, left image
    uint8_t* flags1 = nullptr;  // [cap][npix] same for the right image (do_refine)
    uint8_t* so_trace = nullptr;   // [cap][npix][D] "so" choice codes
    uint16_t* so_cidx = nullptr;   // [cap][npix] "so" row-minimum indices
    // which scan-line optimiser dispOptimize runs (sm_so_config; the call commented in at cpp:1096-1100)
    int so_variant = SM_SO_L2R;
    float so_pn2 = 1.2f, so_pn3 = 3.6f;   // the chosen function's Pn2 / Pn3 (so cpp:6305-6306)
    bool so_float_minima = false;         // sm_create_opts::so_float_minima: the optimisers' FM kernels (signed / NaN costs)
    uint32_t* px = nullptr;     // [cap][2][npix] packed BGR, then the pxh and pxv arm-walk planes (same shape)
    // aggregation "GF": three scratch volumes (the SGM sum is the fourth), image planes, per-pixel terms
    float* gf_s = nullptr;      // [3 (+1 without acc)][cap][nvol]
    float* gf_planes = nullptr; // [cap][10][npix]
    sm::GfPix* gf_pix = nullptr;// [cap][npix]
    // aggregation "GF", ximgproc form: row sums (4 double volumes), alpha / beta (4 float volumes),
    // image-plane row sums [cap][9][npix] doubles and per-pixel terms [cap][9][npix] floats
    double* gfc_rs = nullptr;
    float* gfc_ab = nullptr;
    double* gfc_img = nullptr;
    float* gfc_pix = nullptr;
    // aggregation "FIF": the scratch volume A (and c1 / T without the SGM sum to reuse), weight planes
    float* fif_s = nullptr;     // [1 (+1 without acc)][cap][nvol]
    float* fif_w = nullptr;     // [2][cap][npix] wh, wv of the view being filtered
    // aggregation "AWS": the window and gamma_c (sm_aws_config), the Lab tables and planes, the raw
    // copies of the aggregated volumes, and one weight band per stream a group can run on
    int aws_rv = sm::AWS_MAX_R, aws_ru = sm::AWS_MAX_R;
    float aws_gamma = 5.0f;
    uint16_t* aws_tab = nullptr;   // gam[256] | cb[3072]
    uint8_t* aws_lab = nullptr;    // [cap][2][npix][3]
    float* aws_raw = nullptr;      // [views][cap][nvol]
    float* aws_band[4] = {nullptr, nullptr, nullptr, nullptr};   // each [2][aws_band_rows][S][W]
    int aws_band_rows = 0;
    // aggregation "BF": the window (sm_bf_config) and the row sums between the two sweeps
    int bf_kv = 12, bf_ku = 12;
    double* bf_rs = nullptr;       // [cap][nvol]
    // aggregation "GFNL": the variance threshold (sm_gfnl_config), the NL result, arm_Mask
    float gfnl_thresh = 400.0f;
    float* gfnl_res = nullptr;     // [cap][nvol]
    uint8_t* gfnl_mask = nullptr;  // [cap][npix]
    // dispOptimize's Do_vmTop branch (sm_vmtop_config): the settings, the candidate tables and counts of every
    // view dispOptimize runs on, and method 0's pending-pixel counts per anti-diagonal
    bool vt_on = false;
    int vt_method = 0, vt_num = 2, vt_ts = 10, vt_cir2 = 1, vt_color = 0;
    float vt_thres = 1.09f;
    float2* vt_tab = nullptr;      // [views][cap][npix][vt_num] (disparity, cost)
    int* vt_cnt = nullptr;         // [views][cap][npix]
    int* vt_tcnt = nullptr;        // [cap][cols + 2 rows]
    int vt_alloc_num = 0;          // candidates per pixel the table is sized for
    int vt_ran_num[2] = {0, 0};    // vt_num of the last selection on each view (0: none), for sm_get_top_disp
    // CBCA()'s double-window branch (sm_cbca_double_config): window 1's arm settings and combine2Vm_4's
    // threshold, window 1's arm planes (laid out and padded like `arms`, for their own lag), the large-window
    // volume and arm_Mask.  One second volume serves both views: the views run one after the other on the
    // group's stream, and view 0's selection has read it before view 1's large-window run writes it.
    bool dw_on = false;
    int dw_l = 23, dw_l_out = 23, dw_ct = 30, dw_ct_out = 0;
    int dw_isum = 45;              // arm_Mask = sum of the nine arm maxima < dw_isum: armLthres' integer form (dw_int_threshold)
    float dw_thres = 5.0f;         // armLthres as given (a new pyramid level is configured from it)
    uint8_t* arms2 = nullptr;      // [cap][2 views][2 planes][npix] u32
    uint8_t* arms2_alloc = nullptr;
    size_t arms2_bytes = 0;
    int arms2_lag = -1;            // the lag arms2's pads are sized for
    float* vm2 = nullptr;          // [cap][npix][D] + the volumes' tail pad
    uint8_t* dw_mask = nullptr;    // [cap][npix]
    bool dw_ran = false;           // the mask holds the last sm_cost_calculate / sm_run's choice
    // cbca_core without arm intersection (sm_cbca_intersect_config(ctx, 0); sm_cbca_ni.hip): the other volume of
    // the passes' ping-pong (one serves both views and both windows: they run one after the other on the group's
    // stream) and the per-pixel areas
    bool ni_on = false;
    float* ni_tmp = nullptr;       // [cap][npix][D]
    int32_t* ni_area = nullptr;    // [cap][2 views][2 planes][npix]; an iteration leaves its areas in plane 0
    bool ni_ran = false;           // plane 0 holds the areas of the last sm_cost_calculate / sm_run's last iteration
    // refine()'s Do_calPKR, Do_bgIpol and Do_subpixelEnhancement stages (sm_refine_ext_config)
    bool rx_pkr = false, rx_bg = false, rx_se = false;
    float rx_ratio = 0.1f;         // ratio_PKR (cpp:4093)
    int rx_disp_pkr = -4 * 16;     // DISP_PKR (h:218)
    int rx_depth = 1000;           // bgIplDepth (h:311)
    int rx_mode = SM_SE_REFERENCE;
    uint8_t* pkr_mask = nullptr;   // [cap][npix] PKR_Err_Mask
    float* se = nullptr;           // [cap][npix] SE after its median
    float* se_tmp = nullptr;       // [cap][npix] SE before it (the median filters a copy)
    bool rx_pkr_ran = false, rx_se_ran = false;   // the last refine filled the mask / the float maps
    bool rx_vol_ok = true;         // no volume-reading stage was switched on since dispOptimize last ran
    // refine()'s Do_discontinuityAdjust stage (sm_refine_da_config; sm_refine_da.hip)
    bool da_on = false;
    int da_low = 20, da_high = 60; // Canny's thresholds (cpp:6064)
    int da_ks = 84, da_kc = 87;    // GaussianBlur(3 x 3, sigma 4) in 8.8 fixed point
    uint8_t* da_u8 = nullptr;      // [cap][DA_PLANES][npix]
    uint16_t* da_mag = nullptr;    // [cap][npix]
    int* da_lab = nullptr;         // [cap][npix]
    int* da_hist = nullptr;        // [cap][256]
    uint8_t* da_user = nullptr;    // [npix] sm_set_da_edges' map
    bool da_user_on = false;       // the next refine takes da_user for every pair instead of Canny's map
    bool da_ran = false;           // pair 0's DA_EDGE plane holds the last refine's edge map
    // refine()'s outlier classification (sm_refine_outlier_config; sm_refine_oc.hip)
    bool oc_classify = false;      // LRConsistencyCheck instead of LRConsistencyCheck_normal
    bool oc_rv = false;            // RV_combine_BG instead of regionVote_my
    int oc_disp_mis = -3 * 16;     // DISP_MIS (h:217)
    int oc_type = 0;               // interpolateType (h:310)
    uint8_t* oc_mask = nullptr;    // [cap][npix] LRC_Err_Mask
    int16_t* oc_cand = nullptr;    // [cap][npix] the classified holes' results of a round (types 2, 3)
    int16_t* oc_rowlast = nullptr; // [cap][rows] each row's last classified result
    bool oc_ran = false;           // the last refine filled the mask
    // the per-stage error table (sm_eval_config; sm_eval.hip, sm_eval_host.cpp): the settings, the uploaded truth,
    // the blocks' partial records, the table and (keep_maps) the stages' snapshots.  ev_smax = 7 + region_vote_nums
    // stages is the most a run can record, so the buffers never move once evaluation is on
    bool ev_on = false, ev_keep = false;
    sm::EvalThres ev_th{{1.0f, 0.f, 0.f, 0.f}, 1};
    float* ev_gt = nullptr;            // [cap][npix] DT
    uint8_t* ev_reg = nullptr;         // [cap][npix] bit r: I_mask[r] == 255
    sm_stage_err* ev_part = nullptr;   // [cap][ev_smax][3][ev_nblk]
    sm_stage_err* ev_table = nullptr;  // [cap][ev_smax][3]
    int16_t* ev_snap = nullptr;        // [ev_smax][ev_snap_stride]: [cap][npix] per stage
    size_t ev_snap_stride = 0;         // cap * npix rounded up to 8 elements (a stage keeps pair 0's alignment)
    size_t ev_nblk = 0;                // blocks per pair
    int ev_smax = 0;
    int ev_truth_n = 0;                // truth planes loaded (sm_upload_truth)
    std::vector<std::string> ev_names; // the stages the last run recorded
    std::vector<std::string> ev_preview;   // before any run: what the next sm_run would record (sm_eval_stage_name)
    int ev_n = 0;                      // the pairs it recorded
    bool ev_kept = false;              // it kept its maps
    // aggregation "NL" (and "GFNL"): median image, edge weights, spanning trees, the tree walk, filter values
    uint8_t* nl_med = nullptr;  // [cap][npix][3]
    uint8_t* nl_ew = nullptr;   // [cap][ne]
    int* nl_ints = nullptr;     // two sets of: chain_start, chain_len, order_up, order_down [cap][npix] each
    int* nl_rec = nullptr;      // two sets of path-node records (4 ints) [cap][npix], zero padding on both sides
    int* nl_par = nullptr;      // spanning-tree union-find parents [cap][npix] (sm_nl_mst.hip)
    unsigned long long* nl_best = nullptr;  // lightest edge key offered to each component [cap][npix]
    uint8_t* nl_mst = nullptr;              // spanning-tree work space (sm::nl_mst_scratch_bytes)
    uint32_t* nl_adj = nullptr;             // tree neighbour lists [cap][npix]
    uint8_t* nl_walk = nullptr;             // tree-walk work space (sm::nl_walk_scratch_bytes)
    int* nl_offs = nullptr;                 // round offsets + error flags (device)
    int* nl_offs_h = nullptr;               // the same, page-locked host copy
    int nl_set = 0;                         // record / table set the next run_nl takes (double-buffered)
    hipStream_t nl_st = nullptr;        // NL front (median, edge weights, spanning trees, tree walk)
    hipEvent_t nl_ev_set[2] = {nullptr, nullptr};   // the last filter reading each record / table set (group's stream)
    hipEvent_t nl_ev_in = nullptr;      // a pyramid level: the group's stream has written the level's images (run_nl)
    // pipelined NL front (sm_run with NL + SGM, one view): the call's prep and cost volume also run
    // on nl_st, into a cost volume and penalty flags of the call's set, so they overlap the
    // previous call's filter and SGM on the main stream
    bool nl_pipe = false;
    float* nl_vc = nullptr;                 // [2][cap][nvol] cost volumes (filter input)
    uint8_t* nl_fl = nullptr;               // [2][cap][npix] SGM penalty flags
    hipEvent_t nl_ev_opt[2] = {nullptr, nullptr};   // the last optimiser reading each set (main stream)
    double* nl_table = nullptr; // [256]
    double* nl_val = nullptr;   // [cap][nvol]
    double* nl_oup = nullptr;   // [cap][npix] the ones channel: up sums
    double* nl_ofin = nullptr;  // [cap][npix] final sums
    // the cross-scale pyramid inside sm_run (sm_pyramid_config): the contexts of levels 1 .. PY_LVL - 1, owned by
    // level 0's.  A level context is an ordinary context (sm_create's buffers for its own size, optimization "")
    // whose stages sm_run drives with the owner's groups, on the owner's streams; its launches are profiled in
    // the owner's table as name@level; nl_st is the owner's (borrowed).  Its own main stream serves the getters
    std::vector<sm_ctx*> levels;
    sm_ctx* owner = nullptr;    // set in a level context
    int level = 0;
    bool pyr_ab_old = false;    // A/B switches of tools/bench_pyramid.py (SM_PYR_AB, read by sm_pyramid_config): the
    bool pyr_ab_loop = false;   // staged SolveAll kernel / one pyrDown launch per image instead of the batch forms
    int n_loaded = 0;
    int stage = 0;              // 0 none, 1 images, 2 cost+agg, 3 solve_all, 4 optimized, 5 refined
    float lut_a[1024], lut_b[1024];
    float* luts = nullptr;      // device copy of lut_a | lut_b (per context: contexts on one device may differ)
    float ad_oor_exp = 0;
    bool fuse_norm_scan = false;
    bool fuse_cost_scan = false;   // eligible views run the first H scan with the costs computed in it (cost_scan_fused)
    int num_cu = 256;           // compute units of the device
    int sub_batch = 0;          // sm_params.sub_batch: run sm_run in groups of k pairs (0 = all)
    int nstreams = 1;           // sm_params.num_streams: groups alternate over s streams (see sm_run)
    bool auto_groups = false;   // num_streams = 0 chose two streams: sm_run splits n pairs into two groups
    bool pipelined = false;     // auto_groups with CBCA + SGM: the two groups run as a pipeline across calls
    bool pipe_live = false;     // the side stream still runs the second group of the last sm_run (not joined)
    int pipe_g = 0;             // pairs in the first group of the last pipelined sm_run
    hipEvent_t ev_copy2 = nullptr;   // async copy of a pipelined run's second group done (cst)
    bool copy_split = false;    // the pending async copy is two copies (ev_copy: group 0, ev_copy2: group 1)
    int copy_g = 0;             // with copy_split: pairs [0, copy_g) are ev_copy's, ev_copy2 covers all n
    hipEvent_t ev_dl[2] = {};   // the last two async downloads' copies done (cst), for sm_download_wait
    int dl_slot = 0;            // ev_dl slot of the next async download
    int dl_count = 0;
    hipEvent_t ev_up[2] = {};   // an async upload's copies done: main stream, side stream
    hipEvent_t ev_in[2] = {};   // a pipelined run's group k has read its input images: recorded after the cost
                                // volume, or (cost_scan_fused) after the last view's first CBCA sweep (Group::in_ev)
    // (an early async upload goes on the null stream: the runtime spreads streams round-robin over
    // GPU_MAX_HW_QUEUES (4) in-order hardware queues, and a fifth stream of the context shared one
    // with a group or the map copies, whose kernels / copies the upload then waited behind; the
    // null stream's queue carries nothing else on the hot path, and the context's streams are
    // non-blocking, so it implies no synchronisation with them)
    bool up_split = false;      // the async upload's second group went on the side stream
    hipStream_t xst[3] = {nullptr, nullptr, nullptr};  // extra streams when nstreams > 1
    hipStream_t cst = nullptr;  // copy stream of sm_download_disp_async
    hipEvent_t ev_run = nullptr, ev_copy = nullptr;     // run done (c->st) / async copy done (cst)
    bool copy_pending = false;  // an async copy may still read the maps
    int place_trials = 0;       // > 1: the first sm_run chooses among that many volume sets (place_volumes)
    std::vector<double> place_ms;   // the trials' pipeline times (sm_placement_trials_ms)
    int place_best = -1;
    // sm_run's schedule events
    hipEvent_t ev_start = nullptr;     // the main stream as the call found it: the side streams start after it
    hipEvent_t ev_stagger[8] = {};     // group k may be followed by group k + 1 (slot k % 8)
    hipEvent_t ev_join[3] = {};        // side stream i has finished its groups: the main stream waits (also join_all)
    hipEvent_t ev_side = nullptr;      // sm_download_disp_async: the side stream as the copy stream must find it
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> free_events;
    std::vector<std::string> knames;
    std::map<std::string, int> kidx;
    std::vector<ProfStat> kstat;
};

inline sm_status fail(sm_ctx* c, sm_status s, const std::string& msg) {
    if (c) c->err = msg;
    return s;
}

inline sm_status hip_fail(sm_ctx* c, hipError_t e, const char* where) {
    return fail(c, SM_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(c, expr)                                      \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail((c), e_, #expr); \
    } while (0)

// profiling's event pool and name table (sm_capi.cpp)
hipEvent_t get_event(sm_ctx* c);
int kernel_id(sm_ctx* c, const char* name, double bytes);

// Brackets one launch on stream `st` with events when profiling is on.  A pyramid level's launches go into its
// owner's table, as name@level.
template <typename F>
sm_status timed(sm_ctx* c, hipStream_t st, const char* name, double bytes, F&& launch) {
    ProfRec r{-1, nullptr, nullptr};
    sm_ctx* pc = c->owner ? c->owner : c;
    if (pc->prof) {
        r.kernel = c->owner ? kernel_id(pc, (std::string(name) + "@" + std::to_string(c->level)).c_str(), bytes)
                            : kernel_id(pc, name, bytes);
        r.start = get_event(pc);
        r.stop = get_event(pc);
        if (r.start) hipEventRecord(r.start, st);
    }
    launch();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(c, e, name);
    if (pc->prof && r.start && r.stop) {
        hipEventRecord(r.stop, st);
        pc->recs.push_back(r);
    }
    return SM_OK;
}
template <typename F>   // (a name built at the call: base + view / window suffix)
sm_status timed(sm_ctx* c, hipStream_t st, const std::string& name, double bytes, F&& launch) {
    return timed(c, st, name.c_str(), bytes, launch);
}

// Device memory goes through these two: dalloc records what it returns in c->allocs, dfree releases one
// buffer early and nulls the pointer, free_all (sm_destroy) releases whatever is still recorded.
template <typename T>
sm_status dalloc(sm_ctx* c, T** ptr, size_t count) {
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)ptr, count * sizeof(T));
    if (e != hipSuccess) {
        *ptr = nullptr;
        return fail(c, SM_ENOMEM, std::string("hipMalloc(") + std::to_string(count * sizeof(T)) + " B) failed: " + hipGetErrorString(e));
    }
    c->allocs.push_back(*ptr);
    return SM_OK;
}

template <typename T>
void dfree(sm_ctx* c, T*& ptr) {
    if (!ptr) return;
    hipFree(ptr);
    c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), (void*)ptr));
    ptr = nullptr;
}

// Events other than profiling's go through this: the first use creates the event (without timing) and records
// it in c->events; free_all (sm_destroy) destroys whatever is recorded there.
inline sm_status use_event(sm_ctx* c, hipEvent_t& ev) {
    if (ev) return SM_OK;
    HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->events.push_back(ev);
    return SM_OK;
}

// A group of pairs as a stage driver sees it: the device pointers of pair `off` onward (the kernels index pairs
// from their base pointers), how many pairs, and the stream the group's launches go to.
struct Group {
    uint8_t* bgr;
    uint8_t* gray;
    ulonglong2* code;
    uint8_t* arms;
    float* vm0;
    float* vm1;
    float* acc;
    float* ck;
    float* lx;
    int16_t* disp;
    int16_t* disp1;
    int16_t* disp_tmp;
    uint8_t* flags;
    uint8_t* flags1;
    uint32_t* px;
    uint32_t* pxh;
    uint32_t* pxv;
    int off, n;        // the first pair and the number of pairs
    hipStream_t st;
    int lane;          // 0: the main stream, i + 1: xst[i] (what exists once per stream is indexed by it: aws_band)
    // what run_cbca records for sm_run (null: nothing): after the last view's first sweep, the last reader of the
    // group's input images where that sweep computes the costs; after view 0's first sweep, where the next group starts
    hipEvent_t in_ev, stagger_ev;

    float* vm(int view) const { return view == 0 ? vm0 : vm1; }
    int16_t* map(int view) const { return view == 0 ? disp : disp1; }
    uint8_t* penalty(int view) const { return view == 0 ? flags : flags1; }
    // the group's slice of a per-pair scratch array of `stride` elements per pair
    template <typename T>
    T* slice(T* base, size_t stride) const {
        return base + (size_t)off * stride;
    }
    // a view's profile name: "gf" / "gf_r"
    static std::string name(const char* base, int view) { return std::string(base) + (view == 0 ? "" : "_r"); }
};

// Pairs [off, off + n) on stream `st` (lane: see Group; the reference-ordered entry points run on the main stream).
inline Group at(const sm_ctx* c, int off, int n, hipStream_t st, int lane = 0) {
    const size_t np = c->npix, nv = c->nvol;
    Group g{};
    g.off = off;
    g.n = n;
    g.st = st;
    g.lane = lane;
    g.bgr = g.slice(c->bgr, 2 * np * 3);
    g.gray = g.slice(c->gray, 2 * np);
    g.code = g.slice(c->code, 2 * np);
    g.arms = g.slice(c->arms, 2 * 2 * np * 4);
    g.vm0 = g.slice(c->vm0, nv);
    g.vm1 = c->vm1 ? g.slice(c->vm1, nv) : nullptr;
    g.acc = c->acc ? g.slice(c->acc, nv) : nullptr;
    g.ck = c->ck ? g.slice(c->ck, c->ck_pair) : nullptr;
    g.lx = c->lx ? g.slice(c->lx, nv) : nullptr;
    g.disp = g.slice(c->disp, np);
    g.disp1 = c->disp1 ? g.slice(c->disp1, np) : nullptr;
    g.disp_tmp = c->disp_tmp ? g.slice(c->disp_tmp, np) : nullptr;
    g.flags = g.slice(c->flags, np);
    g.flags1 = c->flags1 ? g.slice(c->flags1, np) : nullptr;
    g.px = g.slice(c->px, 2 * np);
    g.pxh = g.slice(c->px + (size_t)c->cap * 2 * np, 2 * np);
    g.pxv = g.slice(c->px + (size_t)2 * c->cap * 2 * np, 2 * np);
    return g;
}

// sm_run's group size for n pairs; an asynchronous upload splits its copies by the same figure
inline int group_size(const sm_ctx* c, int n) { return c->sub_batch > 0 ? c->sub_batch : (c->auto_groups ? (n + 1) / 2 : n); }

// the maps are about to be written: an asynchronous copy of the previous maps must be done
inline sm_status wait_copy(sm_ctx* c) {
    if (c->copy_pending) HIP_TRY(c, hipStreamWaitEvent(c->st, c->ev_copy, 0));
    if (c->copy_pending && c->copy_split) HIP_TRY(c, hipStreamWaitEvent(c->st, c->ev_copy2, 0));
    return SM_OK;
}

// A pyramid level context handed out by sm_pyramid_level takes the volume / arm / census / area / mask getters only.
inline sm_status refuse_level(sm_ctx* c) {
    if (!c) return SM_EINVAL;
    if (c->owner) return fail(c, SM_ESTATE, "a pyramid level context (sm_pyramid_level) takes only the getters; configure and run its owner");
    return SM_OK;
}

inline sm_status set_device(sm_ctx* c) {
    if (!c) return SM_EINVAL;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(c, e, "hipSetDevice");
    return SM_OK;
}

inline sm_status check_nojoin(sm_ctx* c) {
    sm_status s = refuse_level(c);
    return s ? s : set_device(c);
}

// Orders the main stream after everything queued on side stream i (one event).  A failed join drains the side
// stream on the host, so that its groups cannot race later work.
inline sm_status join_side(sm_ctx* c, int i) {
    sm_status s = use_event(c, c->ev_join[i]);
    hipError_t e = s ? hipSuccess : hipEventRecord(c->ev_join[i], c->xst[i]);
    if (!s && e == hipSuccess) e = hipStreamWaitEvent(c->st, c->ev_join[i], 0);
    if (e != hipSuccess) s = hip_fail(c, e, "stream join");
    if (s) hipStreamSynchronize(c->xst[i]);
    return s;
}

// A pipelined sm_run leaves its second group running on the side stream; every other entry point
// first orders the main stream after it, so that it sees (and may overwrite) the state of the whole call.
inline sm_status join_all(sm_ctx* c) {
    if (!c->pipe_live) return SM_OK;
    c->pipe_live = false;
    return join_side(c, 0);
}

inline sm_status check(sm_ctx* c) {
    sm_status s = check_nojoin(c);
    if (s) return s;
    return join_all(c);
}

// check() for the calls a level context takes too: the getters above, and the per-context halves of the
// aggregation-side *_config calls, which the owner's call runs on every level
inline sm_status check_any(sm_ctx* c) {
    sm_status s = set_device(c);
    if (s) return s;
    return join_all(c);
}

// ---- what crosses the host files -----------------------------------------------------------

// sm_validate.cpp
int census_len(const sm_params& p);
bool cost_ext(const sm_params& p);
bool needs_census(const sm_params& p);
bool needs_arms(const sm_params& p);
bool right_view(const sm_params& p);
int n_views(const sm_params& p);
int opt_views(const sm_params& p);
bool uses_gf(const sm_params& p);
bool uses_nl(const sm_params& p);
bool bf_exact(const sm_params& p);
int cbca_lag(const sm_params& p);
int cbca_lag2(const sm_ctx* c);
int cbca_iters(const sm_ctx* c);
bool refine_reads_volume(const sm_ctx* c);
const char* outlier_config_error(const sm_params& p, int classify, int disp_mis, int rv_combine, int interpolate_type);
int dw_int_threshold(float thres);
bool cbca_div_safe(const sm_params& p, int k);
// so_float_minima (sm_create_opts): "so" is then allowed after GF, GFNL and BF with inexact sums
sm_status validate(const sm_params& p, std::string& why, bool so_float_minima = false);
void build_luts(sm_ctx* c);

// sm_stages.cpp (all asynchronous on the group's stream)
sm_status run_prep(sm_ctx* c, const Group& G);
bool cost_scan_fused(const sm_ctx* c, int view);
sm_status run_cost(sm_ctx* c, int view, const Group& G);
sm_status run_cbca(sm_ctx* c, int view, bool fuse_scale, float w, const Group& G);
sm_status run_scale(sm_ctx* c, int view, float w, const Group& G);
sm_status run_optimize(sm_ctx* c, int view, const Group& G);
sm_status run_refine(sm_ctx* c, const Group& G);
sm_status run_da_image(sm_ctx* c, const Group& G, int first, const int16_t* dp);

// sm_eval_host.cpp: the error table's stage list and its launches on the group's stream
std::vector<std::string> eval_stage_names(const sm_ctx* c, bool stage0, bool refine);
sm_status eval_begin(sm_ctx* c, int n, bool stage0, bool refine);   // a run starts: checks the truth, fixes the list
sm_status run_eval_stage(sm_ctx* c, const Group& G, int stage, const int16_t* map);
sm_status run_eval_final(sm_ctx* c, const Group& G, int stage0, int nstages);

// sm_stages_agg.cpp
sm_status nl_open(sm_ctx* c, hipStream_t st);
Group nl_front(const sm_ctx* c, const Group& G, int set);
sm_status run_nl(sm_ctx* c, const Group& G, bool solve_all, float w, const Group* front = nullptr, float* out = nullptr);
sm_status run_other_agg(sm_ctx* c, const Group& G, bool solve_all = false, float w = 1.f);
bool agg_scale_fused(const sm_params& p, int view);
const uint16_t* aws_tables();
sm_status aws_alloc_bands(sm_ctx* c);

// sm_capi.cpp
bool pyr_weights(int L, float lam, float* w);     // row 0 of SolveAll's inverted matrix; false: singular
sm_status pyr_sync_schedule(sm_ctx* c);           // the levels follow the owner's stream count (per-lane scratch)

// sm_run.cpp
sm_status apply_schedule(sm_ctx* c, int num_streams, int sub_batch);
sm_status upload(sm_ctx* c, int n, const uint8_t* lbgr, const uint8_t* rbgr, size_t cstride, const uint8_t* lgray,
                 const uint8_t* rgray, size_t gstride);

