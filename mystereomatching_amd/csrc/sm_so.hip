// sm_so.hip — scan-line optimisation, optimization == "so" (stereoMatching.cpp:1091-1105, so()
// cpp:6272-6394): per row, a left-to-right dynamic programme over the disparities with a trace
// of every choice, then a right-to-left backtrack from the last column's minimum.
//
// Forward step at column u (u = 1 .. W-1), per disparity d, with prev = vm(u - 1) already updated:
//   Pn2 = 1.2f, Pn3 = 3.6f (SoArgs::pn2 / pn3), both halved when the mean channel |I(u) - I(u-1)| of I[0] exceeds 15
//   cost_min = prev[d]; candidates in this order, each taken only when strictly smaller:
//     prev[d-1] + Pn2 (d > 0), prev[d+1] + Pn2 (d < D-1), min_d' prev[d'] + Pn3 (first argmin)
//   vm(u)[d] += cost_min;  trace(u)[d] = the chosen disparity
// I[0] is the LEFT colour image for both views (dispOptimize passes I_c; so() reads I[0]).
//
// gfx950 mapping: one wave per (pair, row), lane l owns K consecutive disparities (registers);
// the row minimum is an unsigned-integer DPP reduction (every cost is >= +0, so bit patterns
// order like the floats; the FM instantiation, below, takes costs of either sign and NaN) plus a ballot for the
// first index; d +- 1 across lane edges come by DPP
// wave shifts.  Columns are prefetched a tile ahead.  The trace is stored as one byte per element
// (0: d, 1: d - 1, 2: d + 1, 3: the row minimum's index, kept per column), so the backtrack — a
// chain of W dependent reads, inherently sequential — reads one byte and one u16 per column.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"
#include "sm_so_step.h"

namespace sm {

namespace {

constexpr int SO_T = 8;   // columns per prefetch tile

// LT (LDS trace): the choice codes of a row live in LDS as two ballot masks per column and
// per lane slot j (bit l of mask 2j / 2j + 1 = bit 0 / 1 of the code of disparity l K + j), and
// the row-minimum indices as u16; the backtrack's W dependent reads then hit LDS instead of
// global memory (Teddy x16: the chain of ~450 dependent global loads per row dominated the
// kernel), and the byte-wise trace stores disappear.  Used when 4 rows' traces fit in 64 KB.
//
// R2L (so_R2L, cpp:6683-6826): the same programme run from column W - 1 down to column 0 with prev = vm(u + 1), the
// discontinuity between I(u) and I(u + 1), and the backtrack from column 0's first minimum towards W - 1.  The kernel
// counts steps s = 0 .. W - 1 of the scan; step s is column so_col<R2L>(W, s) = s (so) or W - 1 - s (so_R2L).  The trace of a
// line is private to its wave, so it is indexed by step in both directions; the volume, the colours and the map are
// indexed by column.  The penalties are arguments (so: 1.2 / 3.6, cpp:6305-6306; so_R2L: 0.3 / 0.9, cpp:6716-6717).
template <bool R2L>
__device__ __forceinline__ int so_col(int W, int s) {   // the column of step s of the scan
    return R2L ? W - 1 - s : s;
}

//
// FM (float minima; sm_create_opts::so_float_minima): every minimum is so_first_min (sm_so_step.h), the reference's
// own float loop, so the costs may have either sign and be NaN (GF, GFNL, inexact BF).  so_step needs nothing: each
// of its `<` is false when a side is NaN, so a NaN prev[d] gives cost_min = NaN, code 0 and nv = NaN, and a NaN
// c_min is never taken.  Padding lanes are skipped by so_first_min and never read as a neighbour (so_step's d > 0 /
// d < D - 1 guards).  With a +inf cost the reference's `FLT_MAX < +inf` selects d - 1 at d = 0 (d + 1 at d = D - 1)
// and its backtrack leaves the trace; here the backtrack's disparity is clamped to [0, D), so every access stays
// inside the line's own trace.  What the map holds on such a line is unspecified; other lines are independent.
template <int K, bool LT, bool R2L, bool FM>
__global__ __launch_bounds__(256) void k_so(const SoArgs a) {
    extern __shared__ __align__(16) uint64_t so_lds[];
    const int lane = threadIdx.x & 63;
    const int row_id = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int H = a.H, W = a.W, D = a.D;
    if (row_id >= a.n * H) return;   // whole waves only: no barrier follows
    const int b = row_id / H, v = row_id - b * H;
    const size_t npix = (size_t)H * W;
    const size_t pix0 = (size_t)b * npix + (size_t)v * W;
    float* vrow = a.vm + pix0 * D;                     // (u, d) at u * D + d
    uint8_t* trow = a.trace + pix0 * D;
    uint16_t* crow = a.cidx + pix0;
    // LT: this wave's trace masks [W][2K] u64, then its row-minimum indices [W] u16
    uint64_t* tl = so_lds + (size_t)(threadIdx.x >> 6) * so_lds_words(W, K);
    uint16_t* cl = (uint16_t*)(tl + (size_t)W * 2 * K);
    const uint32_t* prow = a.px + ((size_t)b * 2) * npix + (size_t)v * W;   // left view's packed BGR
    const int d0 = lane * K;
    bool valid[K];
#pragma unroll
    for (int j = 0; j < K; j++) valid[j] = d0 + j < D;
    float prev[K];
#pragma unroll
    for (int j = 0; j < K; j++) prev[j] = valid[j] ? vrow[(size_t)so_col<R2L>(W, 0) * D + d0 + j] : FLT_MAX;

    using Tile = float[SO_T][K];
    auto load_tile = [&](Tile& t, int u0) {
#pragma unroll
        for (int k = 0; k < SO_T; k++) {
            const int u = so_col<R2L>(W, min(u0 + k, W - 1));   // R2L: the tile runs downwards and clamps at column 0
#pragma unroll
            for (int j = 0; j < K; j++) t[k][j] = valid[j] ? vrow[(size_t)u * D + d0 + j] : 0.f;
        }
    };
    auto process = [&](const Tile& t, int u0) {
        // discontinuity flags of the tile's steps: lane k tests step u0 + k against its predecessor along the scan
        uint64_t disc;
        {
            const int u = u0 + lane;
            bool f = false;
            if (lane < SO_T && u < W) {
                f = so_is_disc(prow[so_col<R2L>(W, u)], prow[so_col<R2L>(W, u - 1)]);
            }
            disc = __ballot(f);
        }
#pragma unroll
        for (int k = 0; k < SO_T; k++) {
            const int u = u0 + k;
            if (u >= W) break;
            const bool dc = (disc >> k) & 1;
            // (a select of values: `dc ? pn2h : pn2` on the captured variables themselves is a select of their
            // addresses and keeps the whole closure in scratch memory)
            const float Pn2 = dc ? a.pn2 / 2 : a.pn2, Pn3 = dc ? a.pn3 / 2 : a.pn3;   // Pn /= 2 on a discontinuity
            // row minimum of prev and its first index (prev lanes past D hold FLT_MAX)
            float lm = prev[0];
            int li = d0;
#pragma unroll
            for (int j = 1; j < K; j++)
                if (prev[j] < lm) {
                    lm = prev[j];
                    li = d0 + j;
                }
            float wmin;
            int cidx;
            if (FM) {
                cidx = so_first_min<K>(prev, d0, D, wmin);
            } else {
                const uint32_t wm = wave_umin(__builtin_bit_cast(uint32_t, lm));
                const uint64_t hit = __ballot(__builtin_bit_cast(uint32_t, lm) == wm);
                cidx = __builtin_amdgcn_readlane(li, (int)__builtin_ctzll(hit));
                wmin = __builtin_bit_cast(float, wm);
            }
            float nv[K];
            so_step<K, false, LT>(prev, t[k], nv, wmin, Pn2, Pn3, d0, D, lane, tl + (size_t)u * 2 * K, trow + (size_t)u * D);
            if (lane == 0) {
                if (LT)
                    cl[u] = (uint16_t)cidx;
                else
                    crow[u] = (uint16_t)cidx;
            }
#pragma unroll
            for (int j = 0; j < K; j++) {
                prev[j] = valid[j] ? nv[j] : FLT_MAX;
                if (a.keep_final && valid[j]) vrow[(size_t)so_col<R2L>(W, u) * D + d0 + j] = nv[j];
            }
        }
    };
    Tile ta, tb;   // explicit ping-pong (no dynamically indexed register arrays)
    load_tile(ta, 1);
    for (int u0 = 1; u0 < W; u0 += 2 * SO_T) {
        if (u0 + SO_T < W) load_tile(tb, u0 + SO_T);
        process(ta, u0);
        if (u0 + SO_T >= W) break;
        if (u0 + 2 * SO_T < W) load_tile(ta, u0 + 2 * SO_T);
        process(tb, u0 + SO_T);
    }
    // backtrack: first minimum of the scan's last column, then one trace read per step
    int dmin;
    {
        float lm = prev[0];
        int li = d0;
#pragma unroll
        for (int j = 1; j < K; j++)
            if (prev[j] < lm) {
                lm = prev[j];
                li = d0 + j;
            }
        if (FM) {
            float wmin;
            dmin = so_first_min<K>(prev, d0, D, wmin);
        } else {
            const uint32_t wm = wave_umin(__builtin_bit_cast(uint32_t, lm));
            const uint64_t hit = __ballot(__builtin_bit_cast(uint32_t, lm) == wm);
            dmin = __builtin_amdgcn_readlane(li, (int)__builtin_ctzll(hit));
        }
    }
    __threadfence_block();   // this wave's trace stores are visible to its own loads
    int16_t* drow = a.disp + pix0;
    int outv = 0;            // lane (u & 63) of the current 64-column group holds disp[u]
    int u = W - 1;           // the step; its column is so_col<R2L>(W, u)
    outv = lane == (so_col<R2L>(W, u) & 63) ? dmin : outv;
    for (; u > 0; u--) {
        dmin = so_trace_next<K, LT>(dmin, tl + (size_t)u * 2 * K, trow + (size_t)u * D, LT ? cl[u] : crow[u]);
        if (FM) dmin = min(max(dmin, 0), D - 1);   // a +inf cost's trace may point outside [0, D) (see above)
        const int t = so_col<R2L>(W, u - 1);
        if (R2L) {   // columns rise: group t - 64 .. t - 1 is complete when column t opens the next one
            if ((t & 63) == 0) {
                const int g = t - 64;
                drow[g + lane] = (int16_t)outv;
            }
        } else if ((t & 63) == 63) {   // the group of columns t + 1 .. has been filled: flush it
            const int g = t + 1;
            if (g + lane < W) drow[g + lane] = (int16_t)outv;
        }
        outv = lane == (t & 63) ? dmin : outv;
    }
    if (R2L) {   // the last, possibly partial, group
        const int g = (W - 1) & ~63;
        if (g + lane < W) drow[g + lane] = (int16_t)outv;
    } else if (lane < W) {
        drow[lane] = (int16_t)outv;   // group 0 (columns 0 .. 63)
    }
}

}  // namespace

void launch_so(const SoArgs& a, hipStream_t st) {
    const int rows = a.n * a.H;
    dim3 grid((unsigned)((rows + 3) / 4));
    const int k = (a.D + 63) / 64;
    const int kk = k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)));
    const size_t shm = 4 * so_lds_words(a.W, kk) * 8;
    const bool lt = shm <= 64 * 1024;   // the row's trace in LDS when it fits, else in global memory
    const size_t sh = lt ? shm : 0;
#define SM_SO_LAUNCH_FM(KV, FMV)                                                                    \
    do {                                                                                            \
        if (a.r2l) {                                                                                \
            if (lt) hipLaunchKernelGGL((k_so<KV, true, true, FMV>), grid, dim3(256), sh, st, a);    \
            else hipLaunchKernelGGL((k_so<KV, false, true, FMV>), grid, dim3(256), 0, st, a);       \
        } else {                                                                                    \
            if (lt) hipLaunchKernelGGL((k_so<KV, true, false, FMV>), grid, dim3(256), sh, st, a);   \
            else hipLaunchKernelGGL((k_so<KV, false, false, FMV>), grid, dim3(256), 0, st, a);      \
        }                                                                                           \
    } while (0)
#define SM_SO_LAUNCH(KV)                                 \
    do {                                                 \
        if (a.float_minima) SM_SO_LAUNCH_FM(KV, true);   \
        else SM_SO_LAUNCH_FM(KV, false);                 \
    } while (0)
    if (kk == 1) SM_SO_LAUNCH(1);
    else if (kk == 2) SM_SO_LAUNCH(2);
    else if (kk == 4) SM_SO_LAUNCH(4);
    else if (kk == 8) SM_SO_LAUNCH(8);
    else SM_SO_LAUNCH(16);
#undef SM_SO_LAUNCH
#undef SM_SO_LAUNCH_FM
}

}  // namespace sm
