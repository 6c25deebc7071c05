// sm_so_t2d.hip — the scan-line optimiser run down the columns: so_T2D (stereoMatching.cpp:6580-6681), the call
// commented out at cpp:1097.  Per column u, a top-to-bottom dynamic programme over the disparities with a trace of
// every choice, then a bottom-to-top backtrack from the last row's minimum.
//
// Forward step at row v (v = 1 .. H-1), per disparity d, with prev = vm(v - 1, u) already updated:
//   Pn2 = 0.3f, Pn3 = 0.9f (SoArgs::pn2 / pn3; cpp:6607-6608), both halved when the mean channel
//   |I(v, u) - I(v-1, u)| of I[0] exceeds 15 (float sum; sum /= 3; cpp:6592-6600)
//   c_min = min_d' prev[d'] (first argmin, strict <) + Pn3
//   cost_min = prev[d]; candidates in this order, each taken only when strictly smaller:
//     prev[d-1] + Pn2 (d > 0), prev[d+1] + Pn2 (d < D-1), c_min
//   vm(v, u)[d] += (cost_min - c_min)   (cpp:6644: one rounded difference, then one rounded sum)
//   trace(v, u)[d] = the chosen disparity
// The addend is <= 0, so the accumulated costs go negative even on costs >= +0: every minimum here is a float
// minimum (v_min_f32 and float compares: -0 == +0, first index on ties), never one on bit patterns.  Costs are
// finite, as for so: lanes past D hold FLT_MAX and never win against a real cost, and no NaN is ordered (the FM
// instantiation, below, takes NaN too).
// The last-row minimum is `if (c_min > vP[d])` (cpp:6659, first index); the backtrack follows
// trace(v, u)[disp(v, u)] upwards (cpp:6667-6679).  The reference's backtrack sits inside its column loop; its last
// execution, after every column's forward pass, is the result, and that is what this kernel computes.
// The reference runs on a clone (vm_res, cpp:1095): vm[view] is only read here, nothing is stored to it.
// I[0] is the LEFT colour image for both views, as for so.
//
// gfx950 mapping: one wave per (pair, column), lane l owns K consecutive disparities in registers, as in k_so.  A
// step reads D contiguous floats at a stride of W D floats; the four waves of a block own adjacent columns, so a
// block's step reads one contiguous span of 4 D floats.  Rows are prefetched a tile ahead.  The trace is k_so's:
// two ballot masks per row and lane slot in LDS while four columns' masks fit in 64 KB, else byte codes in the
// so_trace / so_cidx buffers, where column u of pair b owns bytes [(b H W + u H) D, (b H W + (u + 1) H) D) — inside
// the pair's own [H][W][D] slice, so a group's slice of the buffers holds its pairs.
// The map's stores are 2-byte stores W apart (one per row and column): 2 B against the 4 D B read for the same pixel,
// issued 64 rows at a time off the dependent chain of the backtrack.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"
#include "sm_so_step.h"

namespace sm {

namespace {

constexpr int T2D_T = 8;   // rows per prefetch tile

// first index of the minimum of the wave's K-per-lane values of either sign (strict <, so the first of equal
// values, -0 == +0); lanes past D hold FLT_MAX.  `wm` receives the minimum, wave-uniform.
template <int K>
__device__ __forceinline__ int t2d_argmin(const float (&p)[K], int d0, float& wm) {
    float lm = p[0];
    int li = d0;
#pragma unroll
    for (int j = 1; j < K; j++)
        if (p[j] < lm) {
            lm = p[j];
            li = d0 + j;
        }
    // v_min_f32 may return either zero when -0 meets +0, per lane; one lane's value is taken for all.
    // Finite costs are a precondition the ballot depends on: a NaN minimum equals no lane's value, hit would be 0 and
    // the lane index 64 (k_so's compare of bit patterns always has a hit).  A default sm_create keeps it: it refuses
    // "so" after the aggregations whose costs may be signed or NaN (GF, GFNL, inexact BF).  Contexts created with
    // so_float_minima = 1 lift those refusals and run the FM instantiation below, which never comes here.
    wm = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave_min(lm))));
    const uint64_t hit = __ballot(lm == wm);
    return __builtin_amdgcn_readlane(li, (int)__builtin_ctzll(hit));
}

// FM (float minima; sm_create_opts::so_float_minima): every minimum is so_first_min (sm_so_step.h), defined for NaN
// too, and the backtrack's disparity is clamped to [0, D) as in k_so (a +inf cost; the column's map is unspecified).
template <int K, bool LT, bool FM>
__global__ __launch_bounds__(256) void k_so_t2d(const SoArgs a) {
    extern __shared__ __align__(16) uint64_t t2d_lds[];
    const int lane = threadIdx.x & 63;
    const int col_id = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int H = a.H, W = a.W, D = a.D;
    if (col_id >= a.n * W) return;   // whole waves only: no barrier follows
    const int b = col_id / W, u = col_id - b * W;
    const size_t npix = (size_t)H * W;
    const size_t vstride = (size_t)W * D;                               // floats between rows of a column
    const float* vcol = a.vm + ((size_t)b * npix + u) * D;             // (v, d) at v * vstride + d
    uint8_t* tcol = a.trace + ((size_t)b * npix + (size_t)u * H) * D;   // (v, d) at v * D + d
    uint16_t* ccol = a.cidx + (size_t)b * npix + (size_t)u * H;
    // LT: this wave's trace masks [H][2K] u64, then its row-minimum indices [H] u16
    uint64_t* tl = t2d_lds + (size_t)(threadIdx.x >> 6) * so_lds_words(H, K);
    uint16_t* cl = (uint16_t*)(tl + (size_t)H * 2 * K);
    const uint32_t* pcol = a.px + ((size_t)b * 2) * npix + u;           // left view's packed BGR, row v at v * W
    const int d0 = lane * K;
    bool valid[K];
#pragma unroll
    for (int j = 0; j < K; j++) valid[j] = d0 + j < D;
    float prev[K];
#pragma unroll
    for (int j = 0; j < K; j++) prev[j] = valid[j] ? vcol[d0 + j] : FLT_MAX;

    using Tile = float[T2D_T][K];
    auto load_tile = [&](Tile& t, int v0) {
#pragma unroll
        for (int k = 0; k < T2D_T; k++) {
            const int v = min(v0 + k, H - 1);
#pragma unroll
            for (int j = 0; j < K; j++) t[k][j] = valid[j] ? vcol[(size_t)v * vstride + d0 + j] : 0.f;
        }
    };
    auto process = [&](const Tile& t, int v0) {
        // discontinuity flags of the tile's rows: lane k tests row v0 + k against the row above
        uint64_t disc;
        {
            const int v = v0 + lane;
            bool f = false;
            if (lane < T2D_T && v < H) {
                f = so_is_disc(pcol[(size_t)v * W], pcol[(size_t)(v - 1) * W]);
            }
            disc = __ballot(f);
        }
#pragma unroll
        for (int k = 0; k < T2D_T; k++) {
            const int v = v0 + k;
            if (v >= H) break;
            const bool dc = (disc >> k) & 1;
            // (a select of values: `dc ? pn2h : pn2` on the captured variables themselves is a select of their
            // addresses and keeps the whole closure in scratch memory)
            const float Pn2 = dc ? a.pn2 / 2 : a.pn2, Pn3 = dc ? a.pn3 / 2 : a.pn3;   // Pn /= 2 on a discontinuity
            float wm;
            const int cidx = FM ? so_first_min<K>(prev, d0, D, wm) : t2d_argmin<K>(prev, d0, wm);
            float nv[K];
            so_step<K, true, LT>(prev, t[k], nv, wm, Pn2, Pn3, d0, D, lane, tl + (size_t)v * 2 * K, tcol + (size_t)v * D);
            if (lane == 0) {
                if (LT)
                    cl[v] = (uint16_t)cidx;
                else
                    ccol[v] = (uint16_t)cidx;
            }
#pragma unroll
            for (int j = 0; j < K; j++) prev[j] = valid[j] ? nv[j] : FLT_MAX;
        }
    };
    Tile ta, tb;   // explicit ping-pong (no dynamically indexed register arrays)
    load_tile(ta, 1);
    for (int v0 = 1; v0 < H; v0 += 2 * T2D_T) {
        if (v0 + T2D_T < H) load_tile(tb, v0 + T2D_T);
        process(ta, v0);
        if (v0 + T2D_T >= H) break;
        if (v0 + 2 * T2D_T < H) load_tile(ta, v0 + 2 * T2D_T);
        process(tb, v0 + T2D_T);
    }
    // backtrack: first minimum of the last row, then one trace read per row
    float wm;
    int dmin = FM ? so_first_min<K>(prev, d0, D, wm) : t2d_argmin<K>(prev, d0, wm);
    __threadfence_block();   // this wave's trace stores are visible to its own loads
    int16_t* dcol = a.disp + (size_t)b * npix + u;   // row v at v * W
    int outv = 0;            // lane (v & 63) of the current 64-row group holds disp(v, u)
    int v = H - 1;
    outv = lane == (v & 63) ? dmin : outv;
    for (; v > 0; v--) {
        dmin = so_trace_next<K, LT>(dmin, tl + (size_t)v * 2 * K, tcol + (size_t)v * D, LT ? cl[v] : ccol[v]);
        if (FM) dmin = min(max(dmin, 0), D - 1);
        const int t = v - 1;
        if ((t & 63) == 63) {   // the group of rows t + 1 .. has been filled: flush it
            const int g = t + 1;
            if (g + lane < H) dcol[(size_t)(g + lane) * W] = (int16_t)outv;
        }
        outv = lane == (t & 63) ? dmin : outv;
    }
    if (lane < H) dcol[(size_t)lane * W] = (int16_t)outv;   // group 0 (rows 0 .. 63)
}

}  // namespace

void launch_so_t2d(const SoArgs& a, hipStream_t st) {
    const int cols = a.n * a.W;
    dim3 grid((unsigned)((cols + 3) / 4));
    const int k = (a.D + 63) / 64;
    const int kk = k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)));
    const size_t shm = 4 * so_lds_words(a.H, kk) * 8;
    const bool lt = shm <= 64 * 1024;   // the columns' traces in LDS when they fit, else in global memory
#define SM_T2D_LAUNCH_FM(KV, FMV)                                                             \
    do {                                                                                      \
        if (lt) hipLaunchKernelGGL((k_so_t2d<KV, true, FMV>), grid, dim3(256), shm, st, a);   \
        else hipLaunchKernelGGL((k_so_t2d<KV, false, FMV>), grid, dim3(256), 0, st, a);       \
    } while (0)
#define SM_T2D_LAUNCH(KV)                                 \
    do {                                                  \
        if (a.float_minima) SM_T2D_LAUNCH_FM(KV, true);   \
        else SM_T2D_LAUNCH_FM(KV, false);                 \
    } while (0)
    if (kk == 1) SM_T2D_LAUNCH(1);
    else if (kk == 2) SM_T2D_LAUNCH(2);
    else if (kk == 4) SM_T2D_LAUNCH(4);
    else if (kk == 8) SM_T2D_LAUNCH(8);
    else SM_T2D_LAUNCH(16);
#undef SM_T2D_LAUNCH
#undef SM_T2D_LAUNCH_FM
}

}  // namespace sm
