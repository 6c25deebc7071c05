// sm_kernels.h — internal launch interface between the C-ABI layer and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sm_capi.h"

namespace sm {

enum { SM_M_CENSUS_GRAD = 0, SM_M_CENSUS = 1, SM_M_AD_CENSUS = 2, SM_M_AD = 3 };
// the measures of k_cost_ext (sm_cost_ext.hip, launch_cost_ext); the values are sm_cost_method's (7 is reserved)
enum { SM_M_SD = 4, SM_M_BT = 5, SM_M_GRAD = 6, SM_M_TRUNC_AD = 8, SM_M_AD_GRAD = 9, SM_M_AD_CENSUS_GRAD = 10 };
enum { SGM_FIRST = 1, SGM_LAST = 2, SGM_KEEP = 4, SGM_SIGNED = 8 };  // KEEP: last path also writes the summed volume;
// SIGNED: costs may be negative (the guided filter's output), minima compare as floats
enum { CB_SCAN = 0, CB_NORM = 1, CB_NORM_SCAN = 2 };

struct PrepArgs {
    const uint8_t* gray;        // [n][2][H][W]
    const uint8_t* bgr;         // [n][2][H][W][3]
    uint32_t* px;               // [n][2][H][W] packed BGR (written by the pack pass)
    uint32_t* pxh;              // [n][2][H][W] arm-walk words, horizontal flags (k_pack_arms)
    uint32_t* pxv;              // [n][2][H][W] arm-walk words, vertical flags
    ulonglong2* code;           // [n][2][H][W]
    uint8_t* arms;              // [n][view][plane][H][W] u32: plane 0 = L | R<<16, plane 1 = U | D<<16
    uint8_t* flags;             // [n][H][W] left image
    uint8_t* flags1;            // [n][H][W] right image (nullptr: not needed)
    int H, W, rv, ru, ring;
    int L, L_out, C_D, C_D_out, minL, cor_thres;
    int do_census, do_arms, do_flags;
    int pack_px;                // the packed-BGR plane px is read later (GF, so, refine)
};

struct CostArgs {
    float* vm;                  // [n][H][W][D] destination (view's volume)
    int seg;                    // pixels of a row per block (set by launch_cost: <= the LDS capacity)
    const ulonglong2* code;     // [n][2][H][W]
    const uint8_t* gray;        // [n][2][H][W] (censusGrad: the gradients, grad_at)
    const uint8_t* arms;        // [n][view][plane][H][W] u32: plane 0 = L | R<<16, plane 1 = U | D<<16
    const uint8_t* bgr;         // [n][2][H][W][3]
    int H, W, D, view, nwords;
    int cwords;                 // 32-bit census words in use: ceil(bits / 32)
    float census_default;       // codeLength * truncRat (h:938)
    float grad_trunc, grad_oor; // 500, sqrt(2*500^2) (cpp:440)
    int grad_adaptive;
    float lam2;                 // lamG
    float ad_trunc;             // "AD" method truncation
    float ad_oor_exp;           // ADCensus: expf(-(trunc)/lamAD) for out-of-range pairs
    const float* lut;           // the context's exponent tables [2][1024]: expf(-x / lam) of the
                                // census (or AD-census census) term, then the ADCensus AD term
};

struct CbcaArgs {
    float* vm;                  // [n][H][W][D], in place
    float* dummy;               // 64 floats: private slots for lanes past D
    const uint32_t* arms;       // [n][view][plane][H][W]: plane 0 = L | R<<16, plane 1 = U | D<<16
    const float* vm_end;        // end of the volume allocation (reads past it return 0)
    const uint32_t* arms_end;   // end of the arm allocation (which has a 2 * lag row front pad)
    int H, W, D;
    int lag;                    // max arm length (the ring size is derived in sm_cbca.hip)
    int apply_scale;
    float scale;                // SolveAll weight (fused into the last normalising pass)
    int view;                   // 0: vm[0] (left reference), 1: vm[1] (right reference, Do_refine)
    int num_cu;                 // compute units of the device
    int arm_pad_rows;           // rows of front pad before the arm planes (2 lag; the allocation also
                                // has >= 2 lag + 64 rows of tail pad, and the volumes >= 8 rows)
    int div_safe;               // 1: every dividend of this launch's normalisation is 0 or >= 2^-110
                                // (proven by the host, cbca_div_safe): the area division needs no check
    // The first H scan that computes its censusGrad costs itself (launch_cbca_hsc): CostArgs'
    // inputs of the select-free elements with lamG == 1 (cost_nosel_ok, >= 3 census words)
    const ulonglong2* code;     // [n][2][H][W]
    const uint8_t* gray;        // [n][2][H][W]
    const float* lut;           // the context's exponent tables (CostArgs::lut)
    float census_default, grad_trunc;
    int grad_adaptive;
    int cwords;                 // 32-bit census words in use: 3 or 4
    const uint32_t* cost_arms;  // the arm planes the gradient term's adaptive weights read, where they are not
                                // `arms` (the double window's second run: grad() saw window 0's); nullptr: `arms`
};
constexpr int CBCA_VM_TAIL_ROWS = 8;   // volume tail pad in rows of W * D floats (fast V sweeps)

struct SgmArgs {
    float* vm;                  // [n][H][W][D] aggregated costs (also the final volume if keep_final)
    float* acc;                 // [n][H][W][D] running path sum
    float* dummy;               // 64 floats: store target of elements past D
    const uint8_t* bgr;         // [n][2][H][W][3] (left colour used for P1/P2 adaptivity)
    int16_t* disp;              // [n][H][W]
    const uint8_t* flags;       // [n][H][W] bit i: colour-difference penalty towards direction i
    int H, W, D, rv, ru, dir;
    float p1, p2;
    int cor_thres, redu, keep_final;
    int signed_costs;           // 1: C may be < 0 (aggregation GF): k_sgm with float minima
    int n;                      // pairs in the launch
    // checkpointed path pairs (k_sgm_ck): the second path of the pair is the first one reversed
    float* ck;                  // [n][lines][segments][D]: the first path's L at segment ends
    int dir2;                   // direction index of the pair's second path
    const float* lx;            // CK_X: [n][H][W][D] L of the path between the pair's two (8 paths: L5)
};

struct GfPix {                  // guided filter, p-independent terms of one pixel (sm_gf.hip)
    double cof[9];              // the nine cofactor expressions of guideFilterCore_matlab (cpp:5060-5078)
    double idet;                // 1 / DET
    float N;                    // BoxFilter(ones)
    float mI[3];                // mean_I[c], BGR
};

struct GfArgs {
    float* vm;                  // [n][H][W][D], filtered in place
    float *s0, *s1, *s2, *s3;   // four scratch volumes [n][H][W][D]
    const uint8_t* bgr;         // the view's colour image of pair 0 ([n][2][H][W][3] + view offset)
    size_t bgr_pair_stride;     // bytes between pairs
    const uint32_t* px;         // the same image as packed B | G << 8 | R << 16 words (prep's k_pack_bgr)
    size_t px_pair_stride;      // words between pairs
    float* planes;              // [n][10][H][W] scratch
    GfPix* pix;                 // [n][H][W]
    int H, W, D;
    float eps;
    int solve_all;              // 1: the output is SolveAll's `0 + w * q` (cpp:2189-2201), w = scale
    float scale;
};
void launch_gf(const GfArgs& a, int n, hipStream_t st);

struct GfCvArgs {               // guided filter, ximgproc form (sm_gf_cv.hip); pair-relative bases
    float* vm;                  // [n][H][W][D], filtered in place
    double* rs;                 // row sums: 4 channel planes, plane c at rs + c * cap * nvol
    float* ab;                  // alpha_0..2, beta: 4 planes, plane c at ab + c * cap * nvol
    int cap;                    // pairs per channel plane (the context's batch capacity)
    const uint32_t* px;         // the view's packed B | G << 8 | R << 16 words of pair 0
    size_t px_pair_stride;      // words between pairs
    double* img_rs;             // [n][9][H][W] image-plane row sums
    float* pix;                 // [n][9][H][W] mean_I (3), Sigma^-1 (6)
    int H, W, D;
    float eps;
    int solve_all;              // 1: the output is SolveAll's `0 + w * q` (cpp:2189-2201), w = scale
    float scale;
};
void launch_gf_cv(const GfCvArgs& a, int n, hipStream_t st);

// cv::boxFilter (normalised, BORDER_REFLECT_101, anchor k / 2) on a volume: aggregation "BF" (sm_bf.hip)
constexpr int BF_MAX_K = 32;    // the largest window side sm_bf_config accepts
struct BfArgs {                 // pair-relative bases
    float* vm;                  // [n][H][W][D], filtered in place (rows read it, cols write it)
    double* rs;                 // [n][H][W][D] row sums
    int H, W, D;
    int kv, ku;                 // window height and width, each in [1, BF_MAX_K]; H >= kv / 2 + 1, W >= ku / 2 + 1
    int solve_all;              // 1: the output is SolveAll's `0 + w * q` (cpp:2189-2201), w = scale
    float scale;
};
void launch_bf_rows(const BfArgs& a, int n, hipStream_t st);
void launch_bf_cols(const BfArgs& a, int n, hipStream_t st);

// aggregation "GFNL"'s variance mask and blend (sm_bf.hip); pair-relative bases
struct GfnlArgs {
    const uint8_t* gray;        // pair b's left gray image at gray + b * gray_pair_stride; H, W >= 10
    size_t gray_pair_stride;
    uint8_t* mask;              // [n][H][W] arm_Mask: 1 where the 19 x 19 variance is < thresh
    const float* res;           // [n][H][W][D] the NL result
    float* vm;                  // [n][H][W][D] the GF result on entry, the blend on return
    int H, W, D;
    float thresh;
    int solve_all;              // 1: the store is SolveAll's `0 + w * q`, w = scale
    float scale;
};
void launch_gfnl_mask(const GfnlArgs& a, int n, hipStream_t st);
void launch_gfnl_blend(const GfnlArgs& a, int n, hipStream_t st);

struct FifArgs {                // full-image guided filter "FIF" (sm_fif.hip); pair-relative bases
    // k_fif_weights: the view's colour image -> the weight planes
    const uint8_t* bgr;         // the view's colour image of pair 0
    size_t bgr_pair_stride;     // bytes between pairs
    float* wh;                  // [n][H][W] weight between (v, u) and (v, u + 1)
    float* wv;                  // [n][H][W] weight between (v, u) and (v + 1, u)
    float eps;                  // 0.08f (cpp:4713)
    // one sweep (launch_fif_sweep); wh (horizontal) / wv (vertical) are read
    const float* in;            // [n][H][W][D] the sweep's `add` volume: vm (horizontal) or A (vertical)
    const float* fw;            // backward sweeps: the forward sweep's result (c1 / T)
    float* out;                 // forward: c1 / T; backward: (fw + L) - in
    int H, W, D;
    int vert;                   // 0: lines are rows, 1: lines are columns
    int second;                 // 0: forward sweep, 1: backward sweep + combination
    int plain;                  // 1: FIF (cpp:4541-4705), 0: FIF_Improve (cpp:4707-4890)
    float pn;                   // Pn = 2 (cpp:4714)
    int solve_all;              // 1: a backward sweep's output is SolveAll's `0 + w * q` (cpp:2189-2201)
    float scale;
};
void launch_fif_weights(const FifArgs& a, int n, hipStream_t st);
void launch_fif_sweep(const FifArgs& a, int n, hipStream_t st);

// Adaptive support weights "AWS" (sm_aws.hip).
constexpr int AWS_MAX_R = 17;                       // W_V_AWS = W_U_AWS = 17 (cpp:5715), the largest radius
constexpr int AWS_GAM_N = 256, AWS_CB_N = 3072;     // the 8-bit BGR2Lab tables: [gam | cb], uint16 each

// One pixel of OpenCV's 8-bit BGR2Lab (fixed point; PARITY UNPINNED).  tab = gam[256] | cb[3072].
__host__ __device__ inline void aws_lab_px(const uint16_t* tab, int B, int G, int R, uint8_t* lab) {
    const uint16_t* cb = tab + AWS_GAM_N;
    const int b = tab[B], g = tab[G], r = tab[R];
    const int fx = cb[(r * 1777 + g * 1541 + b * 778 + 2048) >> 12];
    const int fy = cb[(r * 871 + g * 2929 + b * 296 + 2048) >> 12];
    const int fz = cb[(r * 73 + g * 448 + b * 3575 + 2048) >> 12];
    const int L = (296 * fy - 1336934 + 16384) >> 15;
    const int A = (500 * (fx - fy) + 128 * 32768 + 16384) >> 15;
    const int Bb = (200 * (fy - fz) + 128 * 32768 + 16384) >> 15;
    lab[0] = (uint8_t)(L < 0 ? 0 : L > 255 ? 255 : L);
    lab[1] = (uint8_t)(A < 0 ? 0 : A > 255 ? 255 : A);
    lab[2] = (uint8_t)(Bb < 0 ? 0 : Bb > 255 ? 255 : Bb);
}

struct AwsArgs {                // pair-relative bases; a "row unit" r is row r % H of pair r / H
    const uint16_t* tab;        // gam | cb
    const uint8_t* bgr;         // [n][2][H][W][3]
    uint8_t* lab;               // [n][2][H][W][3] (L, a, b) of both images
    float* wt;                  // the weight band: [2 images][band rows][S][W], row units r0 .. r0 + nr
    const float* raw;           // [n][H][W][D] the view's raw costs (the reference's vm_IB, unbordered)
    float* out;                 // [n][H][W][D] the view's volume (raw on entry: elements out of range stay)
    int H, W, D;
    int rv, ru;                 // window radii, each in [0, AWS_MAX_R]
    float gamma_c;
    int r0, nr;                 // the band's first row unit and its row count
    int band_rows;              // rows the band buffer holds per image (the image stride is band_rows * S * W)
    int lor;                    // the view (calvm_AWS<LOR>)
    int solve_all;              // 1: the store is SolveAll's `0 + w * q` (cpp:2189-2201), raw elements included
    float scale;
};
void launch_aws_lab(const AwsArgs& a, int n, hipStream_t st);
void launch_aws_weights(const AwsArgs& a, hipStream_t st);
void launch_aws_agg(const AwsArgs& a, hipStream_t st);

struct NlArgs {                 // non-local tree filter (sm_nl.hip); node ids = pair * H W + pixel
    const int4* rec;            // path nodes, each path bottom -> top: {x, meta, child weights, parent}
                                //   meta = nchild | (heavy + 1) << 3 | child directions << 6 (2 bits
                                //   each: +1, -1, +W, -W) | own edge weight << 16
    const int* chain_start;     // first record of each path
    const int* chain_len;
    const int* order_up;        // path indices sorted by up round
    const int* order_down;      // path indices sorted by down round
    const double* table;        // exp(-i / (255 sigma)), i = 0..255
    double* val;                // [nodes][D] up sums, then final values (in place)
    float* vm;                  // [nodes][D] normalised aggregated costs out
    const float* vc;            // [nodes][D] costs in (vm itself, or the pipelined front's volume)
    int solve_all;              // 1: vm out is SolveAll's `0 + w * v` (cpp:2189-2201), w = scale
    float scale;
    double* oup;                // [nodes] the ones volume's up sums (qx_tree_filter on ones)
    double* ofin;               // [nodes] its final sums: the normaliser fin(1)
    long nodes;                 // n H W
    int W;
};
constexpr int NL_REC_PAD = 64;  // zero records after the last path (blocked reads past a path's end)
constexpr int NL_LEVELS = 32;   // round tables of the GPU tree walk (light depth <= log2(H W) < 32)
// The tree walk on the GPU (sm_nl_walk.hip): from the neighbour words adj [n H W] of the spanning
// trees, the path records rec [n H W] (bottom -> top per path), chain_start / chain_len per path
// (indexed by the path top's preorder position), the paths of every up / down round (order_up,
// order_down) and offs [2 (NL_LEVELS + 1) + 1]: up round offsets, down round offsets, error flags.
size_t nl_walk_scratch_bytes(int H, int W, int n);
void launch_nl_walk(const uint32_t* adj, int H, int W, int n, uint8_t* scratch, int4* rec, int* chain_start, int* chain_len,
                    int* order_up, int* order_down, int* offs, hipStream_t st);
void launch_nl_edges(const uint8_t* bgr, size_t pair_stride, uint8_t* med, uint8_t* ew, int H, int W, int n, hipStream_t st);
void launch_nl_round(const NlArgs& a, bool up, int lo, int hi, int P, hipStream_t st);
// minimum spanning trees of n pairs' edge weights (sm_nl_mst.hip): par / best [n H W] and
// scratch [nl_mst_scratch_bytes] work space; adj [n H W] the neighbour words of
// nl_tree_from_lists (sm_nl_tree.h)
size_t nl_mst_scratch_bytes(int H, int W, int n);
void launch_nl_mst(const uint8_t* ew, int H, int W, int n, int* par, unsigned long long* best, uint8_t* scratch,
                   uint32_t* adj, hipStream_t st);

struct SoArgs {                 // scan-line optimisation "so" (sm_so.hip)
    float* vm;                  // [n][H][W][D] costs (accumulated in place when keep_final)
    uint8_t* trace;             // [n][H][W][D] choice codes
    uint16_t* cidx;             // [n][H][W] row-minimum index of the previous column
    const uint32_t* px;         // [n][2][H][W] packed BGR (view 0 = I_c[0] is used)
    int16_t* disp;              // [n][H][W]
    int H, W, D, n, keep_final;
    int r2l;                    // 0: so (left to right); 1: so_R2L (right to left).  launch_so only
    float pn2, pn3;             // the functions' Pn2 / Pn3 literals (so 1.2 / 3.6; so_R2L, so_T2D 0.3 / 0.9)
    int float_minima;           // 1: the FM instantiations (minima as the reference's C++ takes them: signed and NaN costs)
};

constexpr int kMaxPyr = 8;      // PY_LVL limit (sm_solve_all_pyr)
struct PyrArgs {                // SolveAll over PY_LVL pyramid levels (sm_pyramid.hip)
    float* vm[kMaxPyr];         // level s volume [n][H_s][W_s][D_s]; vm[0] is updated in place
    int H[kMaxPyr], W[kMaxPyr], D[kMaxPyr];
    float w[kMaxPyr];           // invWgt[s] = regInv(0, s)
    int levels, n;
};

void launch_cost(const CostArgs& a, int method, int n, hipStream_t st);
// methods SM_M_SD .. SM_M_AD_CENSUS_GRAD (sm_cost_ext.hip).  CostArgs as launch_cost reads them, with
// ad_trunc the measure's AD / SD truncation (SD: ad_trunc_ad; adGrad 7; ADCensusGrad 255) and
// grad_trunc / grad_oor its gradient truncation (grad: grad_trunc; adGrad 2; ADCensusGrad 500)
void launch_cost_ext(const CostArgs& a, int method, int n, hipStream_t st);
void launch_prep(const PrepArgs& a, int n, hipStream_t st);
size_t prep_smem_bytes(int rv, int ru, int L_out);
void launch_cbca(const CbcaArgs& a, bool horiz, int mode, int n, hipStream_t st);
// the first H scan (CB_SCAN) of a view whose cost volume was not written: costs computed in the sweep
void launch_cbca_hsc(const CbcaArgs& a, int n, hipStream_t st);
size_t cbca_hsc_smem_bytes(int lag, int cwords);   // its LDS per workgroup (static tables included)
bool cost_nosel_ok(float grad_trunc, float lam2, float census_default);   // the select-free cost elements apply
void launch_scale(float* vm, size_t n, float w, hipStream_t st);
void launch_sgm_path(const SgmArgs& a, int mode, int n, hipStream_t st);
// Checkpointed path pairs (sm_sgm.hip, k_sgm_ck): CK_A sweeps the pair's first path and keeps
// its L every sgm_ck_seg(D) steps; CK_B sweeps the second path, recomputing the first one's L
// segment by segment from those checkpoints, and writes L_first + L_second (CK_B), adds both to
// the running sum (CK_B | CK_MID, 8 paths) or adds them, takes the WTA and writes the map
// (CK_B | SGM_LAST [| SGM_KEEP]).
// CK_B | CK_MID | CK_X (8 paths, the diagonal pair (4, 6)): acc = ((acc + L4) + L5) + L6 with L5
// read from SgmArgs::lx (a path-5 sweep in SGM_FIRST mode stored it there).
enum { CK_A = 16, CK_B = 32, CK_MID = 64, CK_X = 128 };
bool sgm_ck_ok(int D, int paths);
int sgm_ck_seg(int D);
bool sgm_ck_diag_ok(int D, int paths);   // 8 paths: the diagonal pair (4, 6) checkpointed as well
int sgm_ck_diag_seg();
void launch_sgm_ck(const SgmArgs& a, int mode, int n, hipStream_t st);
void launch_wta(const float* vm, int16_t* disp, int n, int H, int W, int D, hipStream_t st);
void launch_expf_range(uint32_t first, uint32_t n, float* out, hipStream_t st);
void launch_copy_x4(const void* in, void* out, size_t bytes, int grid, hipStream_t st);   // bytes % 16384 == 0
void launch_div_check(int exp2, int bmax, unsigned long long* bad, hipStream_t st);
float expf_host(float x);
// refinement (sm_refine.hip)
void launch_lr_check(int16_t* d0, const int16_t* d1, int n, int H, int W, float maxdiff, hipStream_t st);
void launch_region_vote(const int16_t* src, int16_t* dst, const uint32_t* arms, int n, int H, int W, int rv_s,
                        float rv_ratio, hipStream_t st);
void launch_proper_ipol(const int16_t* src, int16_t* dst, const uint32_t* px, int n, int H, int W, int disp_occ,
                        hipStream_t st);
void launch_so(const SoArgs& a, hipStream_t st);
// so_T2D (sm_so_t2d.hip): the programme down the columns; reads vm, writes the map only (keep_final and r2l unused)
void launch_so_t2d(const SoArgs& a, hipStream_t st);
void launch_pyr_down(const uint8_t* src, uint8_t* dst, int rows, int cols, int ch, hipStream_t st);
void launch_pyr_down_f32(const float* src, float* dst, int rows, int cols, hipStream_t st);
void launch_solve_all_pyr(const PyrArgs& a, hipStream_t st);
// the batch path's forms (sm_run with a pyramid): pyrDown of a group's nimg = 2 n images, colour [nimg][rows][cols][3]
// and gray [nimg][rows][cols], in one launch; SolveAll with a 2 x 2 block of level-0 pixels per thread group
// (same sums as launch_solve_all_pyr, bit for bit)
void launch_pyr_down_batch(const uint8_t* src_bgr, const uint8_t* src_gray, uint8_t* dst_bgr, uint8_t* dst_gray, int rows,
                           int cols, int nimg, hipStream_t st);
void launch_solve_all_pyr_batch(const PyrArgs& a, hipStream_t st);
void launch_median3(const int16_t* src, int16_t* dst, int n, int H, int W, hipStream_t st);
int sgm_k_for(int D);

// dispOptimize's Do_vmTop branch (sm_vmtop.hip): candidate selection and the three decision methods
constexpr int VMTOP_MAX_NUM = 8;
struct VmTopArgs {
    const float* vm;            // [n][H][W][D] the volume dispOptimize would take the WTA of
    float2* tab;                // [n][H][W][M] (disparity, cost) of the kept candidates, sorted by (cost, d)
    int* cnt;                   // [n][H][W] candidates kept, 1 .. M
    int* tcnt;                  // [n][W + 2 H] method 0: case-2 pixels per t = u + 2 v (zeroed before decide0_a)
    const uint8_t* bgr;         // [n][2][H][W][3]; view 0 (I_c[0]) is read for both views
    int16_t* disp;              // [n][H][W]
    int H, W, D, M, n;
    float thres;                // vmTop_thres
    int method, ts, has_cir2, color_limit;
};
bool vmtop_shape_ok(int H, int W, int D, int n);
void launch_vmtop_select(const VmTopArgs& a, hipStream_t st);
void launch_vmtop_decide0_a(const VmTopArgs& a, hipStream_t st);   // writes -1 where case 2 is pending
constexpr int VMTOP_RELAX_ROUNDS = 6;                              // launches of decide0_w before decide0_b
void launch_vmtop_decide0_w(const VmTopArgs& a, hipStream_t st);   // pending pixels with no pending neighbour
void launch_vmtop_decide0_b(const VmTopArgs& a, hipStream_t st);
void launch_vmtop_decide12(const VmTopArgs& a, hipStream_t st);    // method 1 or 2

// CBCA()'s double-window branch (sm_cbca_dw.hip): combine2Vm_4's mask and selection
struct DwArgs {
    const uint32_t* arms;       // window-0 arm planes of the launch's first pair: [n][view][plane][H][W]
    uint8_t* mask;              // arm_Mask of every pair the context holds (allocation base): [cap][H][W]
    float* vm;                  // the view's volume, allocation base (16-byte aligned): [cap][H][W][D]
    const float* vm2;           // the large-window volume, allocation base: [cap][H][W][D]
    size_t pix0;                // first pixel of the launch: first pair * H * W
    int H, W, D;
    int isum;                   // arm_Mask = sum of the nine maxima < isum: armLthres (cpp:4297) in the integer
                                // form the host derives for it (dw_int_threshold, sm_validate.cpp)
};
void launch_dw_mask(const DwArgs& a, int n, hipStream_t st);     // H, W >= 2
void launch_dw_select(const DwArgs& a, int n, hipStream_t st);

// cbca_core without arm intersection (sm_cbca_ni.hip): one 1-D pass is launch_ni_prefix, then launch_ni_window
struct NiArgs {
    float* src;                 // the pass's input of the launch's first pair [n][H][W][D]: prefixed in place
    float* dst;                 // the pass's output (the other volume of the ping-pong), same shape
    const uint32_t* arms;       // the launch's first pair: [n][view][plane][H][W], plane 0 = L | R<<16, plane 1 = U | D<<16
    int32_t* area;              // the launch's first pair: [n][view][2][H][W]; the pass reads plane in_plane
                                // (prefixed in place) and writes the other one
    int H, W, D;
    int view;                   // 0: the left image's arms (vm[0]), 1: the right image's (vm[1])
    int horiz;                  // 1: lines are rows, 0: columns
    int in_plane;
    int first;                  // 1: the first pass of an iteration: the area going in is ones(h, w), not read
    int norm;                   // 1: the second pass: the window kernel divides by the area it computes
    int apply_scale;            // with norm: SolveAll's weight on the quotient
    float scale;
};
void launch_ni_prefix(const NiArgs& a, int n, hipStream_t st);
void launch_ni_window(const NiArgs& a, int n, hipStream_t st);   // H <= 65535 (sm_params' limit for rows)

// refine()'s Do_calPKR, Do_bgIpol and Do_subpixelEnhancement stages (sm_refine_ext.hip); pair-relative bases
struct PkrArgs {
    const float* vm;            // [n][H][W][D] vm[0] as dispOptimize left it
    uint8_t* mask;              // [n][H][W] PKR_Err_Mask
    int16_t* disp;              // [n][H][W] DP[0]: marked pixels >= 0 become disp_pkr
    int H, W, D, n;
    float ratio;                // ratio_PKR
    int disp_pkr;               // DISP_PKR
};
struct BgArgs {
    const int16_t* src;         // [n][H][W] the map before the stage
    int16_t* r;                 // [n][H][W] the right candidates, then the filled map
    int H, W, n;
    int depth;                  // bgIplDepth >= 1
};
bool refine_ext_shape_ok(int H, int W, int n);
void launch_pkr(const PkrArgs& a, hipStream_t st);                 // D >= 2
void launch_bg_ipol(const BgArgs& a, hipStream_t st);              // k_bg_r, then k_bg_scan
void launch_subpixel(const int16_t* dp, const float* vm, float* se, int n, int H, int W, int D, int keep_float,
                     hipStream_t st);
void launch_median3_f32(const float* src, float* dst, int n, int H, int W, hipStream_t st);

// refine()'s Do_discontinuityAdjust stage (sm_refine_da.hip); pair-relative bases.  The u8 scratch of a pair:
enum { DA_EQ = 0,      // DP[0] as 8 bits, equalised in place
       DA_BLUR = 1,    // after the Gaussian
       DA_EDGE = 2,    // Canny's edge map (0 / 255), or the one sm_set_da_edges supplied
       DA_CAND = 3,    // 0, 1 (candidate), 2 (candidate above the high threshold)
       DA_DIR = 4,     // the ordered pass's direction per pixel, 0xff where it changes nothing
       DA_FLAG = 5,    // 1 on the union-find root of a component that holds a strong candidate
       DA_PLANES = 6 };
struct DaArgs {
    uint8_t* u8;                // [n][DA_PLANES][H][W]
    uint16_t* mag;              // [n][H][W] |dx| + |dy| (12 bits) | NMS sector << 12
    int* lab;                   // [n][H][W] union-find parents, pair-local pixel indices (-1: no candidate)
    int* hist;                  // [n][256], zeroed before launch_da_hist
    int H, W, n;
    int low, high;              // Canny's thresholds, low <= high
    int ks, kc;                 // the Gaussian's side and centre taps (8.8 fixed point)
};
void launch_da_hist(const DaArgs& a, const int16_t* dp, hipStream_t st);   // dp null: the image already in DA_EQ
void launch_da_equalize(const DaArgs& a, hipStream_t st);
void launch_da_blur(const DaArgs& a, hipStream_t st);
void launch_da_sobel(const DaArgs& a, hipStream_t st);
void launch_da_nms(const DaArgs& a, hipStream_t st);
void launch_da_link(const DaArgs& a, hipStream_t st);
void launch_da_mark(const DaArgs& a, hipStream_t st);
void launch_da_edges(const DaArgs& a, hipStream_t st);
void launch_da_dir(const DaArgs& a, const int16_t* src, int16_t* dst, hipStream_t st);   // dst = src
void launch_da_adjust(const DaArgs& a, const int16_t* src, int16_t* dst, const float* vm, int D, hipStream_t st);

// refine()'s outlier classification (sm_refine_oc.hip); pair-relative bases
struct RvcArgs {
    const int16_t* src;         // [n][H][W] the map before the round
    int16_t* dst;               // [n][H][W] the copy the round fills
    int16_t* cand;              // [n][H][W] types 2, 3: the classified holes' results, -32768 elsewhere (else null)
    int16_t* rowlast;           // [n][H] types 2, 3: each row's last classified result, -32768 for none
    const uint32_t* arms;       // [n][view][plane][H][W]: the left image's arms are read
    int H, W, D, n;
    int rv_s;                   // validNum <= rv_s votes -1
    float rv_ratio;             // hist[most] / validNum > rv_ratio in float
    int depth;                  // bgIplDepth >= 0
    int type;                   // Parameters::interpolateType, 0 .. 3
    int disp_occ, disp_mis;
};
// LRConsistencyCheck, LOR = 0: d0 is labelled in place, mask gets 0 / 255
void launch_lr_classify(int16_t* d0, const int16_t* d1, uint8_t* mask, int n, int H, int W, int D, float maxdiff,
                        int disp_occ, int disp_mis, hipStream_t st);
void launch_rv_combine(const RvcArgs& a, hipStream_t st);          // D <= 1024 (sm_params' limit): 17 KiB of LDS
void launch_rv_carry(const RvcArgs& a, hipStream_t st);            // types 2, 3, after launch_rv_combine

// ---- the per-stage error table (sm_eval_config; sm_eval.hip, arithmetic and EvalArgs in sm_eval_core.h) ----
struct EvalArgs;
// one stage's maps of n pairs against the truth: partial records per (pair, stage, region, block)
void launch_eval_stage(const EvalArgs& a, int n, hipStream_t st);
// the partials of stages [stage0, stage0 + nstages) of n pairs summed into table[pair][stages_alloc][3]
void launch_eval_final(const sm_stage_err* part, sm_stage_err* table, size_t nblk, int stages_alloc, int stage0, int nstages,
                       int n, hipStream_t st);

}  // namespace sm
