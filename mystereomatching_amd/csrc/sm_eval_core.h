// sm_eval_core.h — the arithmetic of the per-stage error table (sm_eval_config), shared by the kernel (sm_eval.hip)
// and its restatement on the host (sm_eval_stage_host): the per-pixel terms, the fixed order of the sums, and the
// packing of the three region masks into one byte.  Plain C++ apart from the host/device marker: a stand-alone
// program (tests/cpp/eval_host_check.cpp) includes it without the HIP runtime.
//
// Order of sum_sq (and of the counts, where order does not matter), DESIGN 22:
//   block   EVAL_BLOCK_PIX = 256 threads x 8 consecutive pixels of one pair; block b covers [2048 b, 2048 (b + 1))
//   thread  t adds its pixels 2048 b + 8 t + j, j = 0 .. 7, in that order, from 0: per region whose bit is set the
//           term (double)dif * (double)dif with dif = fabsf(DT - (float)DP) for DP >= 0, the term 2.0 for DP < 0
//   wave    64 lanes: for off = 32, 16, .., 1: lane l < off takes a[l] + a[l + off]; lane 0 holds the wave's sum
//   block   ((w0 + w1) + w2) + w3 over its four waves: the block's partial record
//   final   64 lanes: lane l adds the partials of blocks l, l + 64, .. in that order, from 0; then the wave tree
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sm_capi.h"

#if defined(__HIPCC__)
#define SM_EVAL_HD __host__ __device__
#else
#define SM_EVAL_HD
#endif

namespace sm {

constexpr int EVAL_THREADS = 256;      // threads of a block
constexpr int EVAL_PER_THREAD = 8;     // consecutive pixels of a thread
constexpr int EVAL_BLOCK_PIX = EVAL_THREADS * EVAL_PER_THREAD;
constexpr int EVAL_WAVE = 64;
constexpr int EVAL_REGIONS = 3;        // I_mask's order: nonocc, all, disc
constexpr int EVAL_MAX_THRES = 4;

struct EvalThres {
    float t[EVAL_MAX_THRES];
    int n;
};

// k_eval_stage's arguments; the pointers are those of the group's first pair
struct EvalArgs {
    const int16_t* disp;   // [n][npix] the stage's maps
    const float* gt;       // [n][npix]
    const uint8_t* reg;    // [n][npix] packed region bytes
    int16_t* snap;         // [n][npix] this stage's snapshots (keep_maps), or null
    sm_stage_err* part;    // [n][stages][3][nblk] partial records
    size_t npix, nblk;
    size_t part_pair;      // records per pair: stages x 3 x nblk
    int stage;
    EvalThres th;
};

// one accumulator per region, in the table's layout
struct EvalAcc {
    sm_stage_err r[EVAL_REGIONS];
};

SM_EVAL_HD inline void eval_zero(EvalAcc& a) {
    for (int r = 0; r < EVAL_REGIONS; r++) {
        a.r[r].count = a.r[r].invalid = 0;
        for (int k = 0; k < EVAL_MAX_THRES; k++) a.r[r].bad[k] = 0;
        a.r[r].sum_sq = 0.0;
    }
}

SM_EVAL_HD inline void eval_add(sm_stage_err& a, const sm_stage_err& b) {
    a.count += b.count;
    a.invalid += b.invalid;
    for (int k = 0; k < EVAL_MAX_THRES; k++) a.bad[k] += b.bad[k];
    a.sum_sq = a.sum_sq + b.sum_sq;
}

// One pixel: disparity dp, truth dt, packed region byte m.  A pixel outside every region adds nothing (a region
// whose bit is clear receives +0.0, which changes no sum: the sums are never -0).
SM_EVAL_HD inline void eval_pixel(EvalAcc& a, int dp, float dt, uint32_t m, const EvalThres& th) {
    uint32_t bad[EVAL_MAX_THRES];
    uint32_t inv;
    double term;
    if (dp >= 0) {
        const float dif = fabsf(dt - (float)dp);
        term = (double)dif * (double)dif;   // pow(float, int) as the reference compiles it (sm_cal_err)
        inv = 0;
        for (int k = 0; k < EVAL_MAX_THRES; k++) bad[k] = (k < th.n && dif > th.t[k]) ? 1u : 0u;
    } else {
        term = 2.0;
        inv = 1;
        for (int k = 0; k < EVAL_MAX_THRES; k++) bad[k] = k < th.n ? 1u : 0u;
    }
    for (int r = 0; r < EVAL_REGIONS; r++) {
        const uint32_t in = (m >> r) & 1u;
        a.r[r].count += in;
        a.r[r].invalid += in & inv;
        for (int k = 0; k < EVAL_MAX_THRES; k++) a.r[r].bad[k] += in & bad[k];
        a.r[r].sum_sq = a.r[r].sum_sq + (in ? term : 0.0);
    }
}

inline size_t eval_blocks(size_t npix) { return (npix + EVAL_BLOCK_PIX - 1) / EVAL_BLOCK_PIX; }

// bit r of out[i] = (mask_r[i] == 255); a null mask is an absent region
inline void eval_pack_regions(size_t count, const uint8_t* nonocc, const uint8_t* all, const uint8_t* disc, uint8_t* out) {
    const uint8_t* m[EVAL_REGIONS] = {nonocc, all, disc};
    for (size_t i = 0; i < count; i++) {
        uint8_t b = 0;
        for (int r = 0; r < EVAL_REGIONS; r++)
            if (m[r] && m[r][i] == 255) b |= (uint8_t)(1u << r);
        out[i] = b;
    }
}

// a wave's tree over 64 accumulators of one region; the sum ends in a[0]
inline void eval_wave_tree_host(sm_stage_err* a) {
    for (int off = EVAL_WAVE / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++) eval_add(a[l], a[l + off]);
}

// The kernels' arithmetic for one map of npix pixels, in their order (see the head of this file).
inline void eval_stage_host(const int16_t* disp, const float* gt, const uint8_t* region, size_t npix, const EvalThres& th,
                            sm_stage_err out[EVAL_REGIONS]) {
    static_assert(sizeof(sm_stage_err) == 32, "sm_stage_err is 32 bytes");
    sm_stage_err lane[EVAL_REGIONS][EVAL_WAVE];   // the finaliser's lanes
    EvalAcc z;
    eval_zero(z);
    for (int r = 0; r < EVAL_REGIONS; r++)
        for (int l = 0; l < EVAL_WAVE; l++) lane[r][l] = z.r[r];
    const size_t nblk = eval_blocks(npix);
    sm_stage_err thr[EVAL_REGIONS][EVAL_THREADS];
    for (size_t b = 0; b < nblk; b++) {
        for (int t = 0; t < EVAL_THREADS; t++) {
            EvalAcc a;
            eval_zero(a);
            for (int j = 0; j < EVAL_PER_THREAD; j++) {
                const size_t i = b * EVAL_BLOCK_PIX + (size_t)t * EVAL_PER_THREAD + j;
                if (i < npix) eval_pixel(a, disp[i], gt[i], region[i], th);
            }
            for (int r = 0; r < EVAL_REGIONS; r++) thr[r][t] = a.r[r];
        }
        for (int r = 0; r < EVAL_REGIONS; r++) {
            for (int w = 0; w < EVAL_THREADS / EVAL_WAVE; w++) eval_wave_tree_host(&thr[r][w * EVAL_WAVE]);
            sm_stage_err p = thr[r][0];
            for (int w = 1; w < EVAL_THREADS / EVAL_WAVE; w++) eval_add(p, thr[r][w * EVAL_WAVE]);
            eval_add(lane[r][b % EVAL_WAVE], p);
        }
    }
    for (int r = 0; r < EVAL_REGIONS; r++) {
        eval_wave_tree_host(lane[r]);
        out[r] = lane[r][0];
    }
}

}  // namespace sm
