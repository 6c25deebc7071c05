// sm_box_sweep.h — OpenCV's normalised box filter on f32 as its generic FilterEngine runs it
// (RowSum<float, double>, then ColumnSum<double, float>), once, for every kernel that needs it:
// "BF" (sm_bf.hip: BORDER_REFLECT_101, any window) and the shipped "GF" (sm_gf_cv.hip:
// BORDER_REFLECT, 19 x 19).  Window k, anchor k / 2 (an even window is not centred: 12 covers the
// offsets -6 .. +5), r = the border policy, along a line of n elements:
//
//   RS(x)  = running sum in double: the first k reflected values in(r(x - k/2 + j)), j = 0 .. k - 1,
//            added left to right, then s += (double)in(r(x + k - k/2)) - (double)in(r(x - k/2))
//   out(y) = (float)(s0 * scale),  s0 = SUM + RS(r(y + k - 1 - k/2)),  SUM = s0 - RS(r(y - k/2)),
//            SUM starting as RS(r(i - k/2)), i = 0 .. k - 2, added in that order
//
// Every operation is the reference's, in its order.  No product feeds a sum here, so nothing in
// this header leans on the library's -ffp-contract=off; what fetch, store and emit compute does.
//
// gfx950 mapping: the sweeps below are per lane.  The volume kernels run them with one wave per
// (pair, line, 64-disparity chunk) and lane = disparity (line_block), the image-plane kernels
// with one thread per line; `fetch` and `store` / `emit` do the addressing.  Loop bounds depend
// on n and k alone, so they are wave-uniform.
#pragma once
#include <hip/hip_runtime.h>

#include "sm_device.h"

namespace sm {

// OpenCV borderInterpolate() where one reflection suffices: the window may reach at most n
// elements past either end with Reflect (BORDER_REFLECT), n - 1 with Reflect101
// (BORDER_REFLECT_101).  The host checks it (sm_create, sm_bf_config).  sm_device.h's looping
// reflect101 serves the callers that may reflect more than once.
struct Reflect {
    static __device__ __forceinline__ int at(int p, int n) { return p < 0 ? -p - 1 : (p >= n ? 2 * n - 1 - p : p); }
};
struct Reflect101 {
    static __device__ __forceinline__ int at(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }
};

// What a 64-lane block of a line sweep over [pair][line][D] works on: block = (pair, line,
// 64-disparity chunk) behind xcd_swizzle, lane = disparity.  Lanes past D are not live and
// read disparity dd = D - 1.
struct LineBlock {
    int pair, line, chunk, d, dd;
    bool live;
};
__device__ __forceinline__ LineBlock line_block(int lines, int D) {
    const int nchunks = (D + 63) >> 6;
    const int blk = xcd_swizzle(blockIdx.x, gridDim.x);
    LineBlock b;
    b.pair = blk / (lines * nchunks);
    const int lc = blk - b.pair * lines * nchunks;
    b.line = lc / nchunks;
    b.chunk = lc - b.line * nchunks;
    b.d = b.chunk * 64 + (int)threadIdx.x;
    b.live = b.d < D;
    b.dd = b.live ? b.d : D - 1;
    return b;
}

// RowSum over a line of n elements with C channels: fetch(u, x) reads element u's inputs into
// float x[C], store(u, S) takes its running sums, const double S[C].  K > 0: the window, known
// at compile time; K == 0: k_runtime.  Ext position i (element r(i - k/2)) enters the sums; from i = k
// on, position i - k leaves.  It is read again, not kept: it was loaded k positions earlier (an
// L1 / L2 hit).  Two tiles of T positions are in flight.
template <int C, class Border, int T, int K, class Fetch, class Store>
__device__ __forceinline__ void box_row_sweep(int n, int k_runtime, Fetch fetch, Store store) {
    const int k = K > 0 ? K : k_runtime, a = k / 2;
    const int L = n + k - 1;   // ext positions
    struct Tile {
        float in[T][C], out[T][C];
    };
    auto load = [&](Tile& t, int i0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = min(i0 + s, L - 1);
            fetch(Border::at(i - a, n), t.in[s]);
            fetch(Border::at(max(i - k, 0) - a, n), t.out[s]);
        }
    };
    double S[C];
#pragma unroll
    for (int c = 0; c < C; c++) S[c] = 0;
    auto process = [&](const Tile& t, int i0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = i0 + s;
            if (i >= L) break;
            if (i < k) {
#pragma unroll
                for (int c = 0; c < C; c++) S[c] += (double)t.in[s][c];
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const double dlt = (double)t.in[s][c] - (double)t.out[s][c];
                    S[c] += dlt;
                }
            }
            if (i >= k - 1) store(i - (k - 1), S);
        }
    };
    Tile ta, tb;
    load(ta, 0);
    for (int i0 = 0; i0 < L; i0 += 2 * T) {
        load(tb, i0 + T);
        process(ta, i0);
        if (i0 + T >= L) break;
        load(ta, i0 + 2 * T);
        process(tb, i0 + T);
    }
}

// ColumnSum down a line of n rows, ring form (window K at compile time): fetch(row, x) reads a
// row's row sums into double x[C], emit(y, mean) takes output y's box means, const float
// mean[C] = (float)(s0 * scale).  The row sum leaving at output y (ext row y) entered at output
// y - (K - 1), or is one of the K - 1 rows SUM starts from: a register ring of K - 1 rows, slot
// y mod (K - 1), so every row sum is read once.  The entering rows are fetched PF outputs
// ahead; PF divides K - 1, so the prefetch slots repeat with the ring and every index is static.
template <int C, class Border, int K, int PF, class Fetch, class Emit>
__device__ __forceinline__ void box_col_sweep_ring(int n, double scale, Fetch fetch, Emit emit) {
    constexpr int RK = K - 1, a = K / 2;
    static_assert(K > 1 && RK % PF == 0, "prefetch slots repeat with the ring");
    double SUM[C], ring[RK][C], nx[PF][C];
#pragma unroll
    for (int i = 0; i < RK; i++) fetch(Border::at(i - a, n), ring[i]);
#pragma unroll
    for (int c = 0; c < C; c++) SUM[c] = 0;
#pragma unroll
    for (int i = 0; i < RK; i++)
#pragma unroll
        for (int c = 0; c < C; c++) SUM[c] += ring[i][c];
    auto enter = [&](int y, double (&x)[C]) { fetch(Border::at(min(y, n - 1) + RK - a, n), x); };
#pragma unroll
    for (int j = 0; j < PF; j++) enter(j, nx[j]);
    for (int y0 = 0; y0 < n; y0 += RK) {
#pragma unroll
        for (int s = 0; s < RK; s++) {
            const int y = y0 + s;
            if (y >= n) return;   // (not `break`: no ring state to carry out of the unrolled loop)
            double s0[C];
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double sp = nx[s % PF][c];
                s0[c] = SUM[c] + sp;
                SUM[c] = s0[c] - ring[s][c];
                ring[s][c] = sp;
            }
            enter(y + PF, nx[s % PF]);
            float mean[C];
#pragma unroll
            for (int c = 0; c < C; c++) mean[c] = (float)(s0[c] * scale);
            emit(y, mean);
        }
    }
}

// ColumnSum, tiled form for a window kv known at run time: the leaving row is read again.  Two
// tiles of T outputs are in flight.  fetch and emit as for the ring form.
template <int C, class Border, int T, class Fetch, class Emit>
__device__ __forceinline__ void box_col_sweep_tiled(int n, int kv, double scale, Fetch fetch, Emit emit) {
    const int a = kv / 2;
    double SUM[C];
#pragma unroll
    for (int c = 0; c < C; c++) SUM[c] = 0;
    for (int i = 0; i < kv - 1; i++) {
        double x[C];
        fetch(Border::at(i - a, n), x);
#pragma unroll
        for (int c = 0; c < C; c++) SUM[c] += x[c];
    }
    struct Tile {
        double enter[T][C], leave[T][C];
    };
    auto load = [&](Tile& t, int y0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int y = min(y0 + s, n - 1);
            fetch(Border::at(y + kv - 1 - a, n), t.enter[s]);
            fetch(Border::at(y - a, n), t.leave[s]);
        }
    };
    auto process = [&](const Tile& t, int y0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int y = y0 + s;
            if (y >= n) break;
            float mean[C];
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double s0 = SUM[c] + t.enter[s][c];
                mean[c] = (float)(s0 * scale);
                SUM[c] = s0 - t.leave[s][c];
            }
            emit(y, mean);
        }
    };
    Tile ta, tb;
    load(ta, 0);
    for (int y0 = 0; y0 < n; y0 += 2 * T) {
        load(tb, y0 + T);
        process(ta, y0);
        if (y0 + T >= n) break;
        load(ta, y0 + 2 * T);
        process(tb, y0 + T);
    }
}

}  // namespace sm
