// sm_bf.hip — OpenCV's normalised cv::boxFilter on f32 with BORDER_REFLECT_101, an arbitrary window
// kv x ku (each in [1, 32]) and the default anchor k / 2, as two aggregations use it:
//
//   "BF"   (BF(), stereoMatching.cpp:1023-1043): boxFilter(vm[i], vm[i], -1, Size(12, 12)) on every
//          view's whole volume, in place;
//   "GFNL" (GFNL(), cpp:4421-4490): var = box19(I I) - box19(I) box19(I) of the left gray image,
//          arm_Mask = var < 400, and vm[0] = mask ? NL : (float)(0.5 NL + 0.5 GF).
//
// The filter itself, its border policy and its gfx950 mapping are sm_box_sweep.h's (shared with
// the "GF" sweeps of sm_gf_cv.hip); here it runs with one channel and Reflect101:
//   k_bf_rows  p -> RS (one double volume), runtime ku
//   k_bf_cols  RS -> vm [+ SolveAll's 0 + w q].  At the reference's kv = 12 the ring form, the
//              whole ring prefetched; any other kv the tiled form.
// 4 + 8 + 8 + 4 = 24 B per element.
//
// The variance plane is two 19 x 19 filters of integers <= 255^2: their sums are exact (below
// 2^25, in uint32 here as in the reference's doubles), so the order of the taps is free and one
// thread per pixel sums the window directly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_box_sweep.h"
#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

namespace {

constexpr int BF_T = 4;        // positions per prefetched tile (two tiles in flight)
constexpr int BF_RING_KV = 12; // the reference's window height: the column sweep's ring form

// one wave per (pair, row, chunk)
__global__ __launch_bounds__(64) void k_bf_rows(const BfArgs a) {
    const LineBlock B = line_block(a.H, a.D);
    const int W = a.W, D = a.D;
    const size_t row0 = (((size_t)B.pair * a.H + B.line) * W) * D;   // element (b, y, 0, 0)
    const float* __restrict__ vm = a.vm + row0 + B.dd;
    double* __restrict__ rs = a.rs + row0 + B.d;
    box_row_sweep<1, Reflect101, BF_T, 0>(
        W, a.ku, [&](int u, float (&x)[1]) { x[0] = vm[(size_t)u * D]; },
        [&](int u, const double (&S)[1]) {
            if (B.live) rs[(size_t)u * D] = S[0];
        });
}

// one wave per (pair, column, chunk).  KV > 0: the window height, known at compile time (ring
// form); KV == 0: a.kv (tiled form)
template <int KV>
__global__ __launch_bounds__(64) void k_bf_cols(const BfArgs a) {
    const LineBlock B = line_block(a.W, a.D);
    const int H = a.H;
    const int kv = KV > 0 ? KV : a.kv;
    const size_t col0 = (((size_t)B.pair * H) * a.W + B.line) * a.D;   // element (b, 0, u, 0)
    const size_t rstep = (size_t)a.W * a.D;
    const double* __restrict__ rs = a.rs + col0 + B.dd;
    float* __restrict__ vm = a.vm + col0 + B.d;
    const double scale = 1. / (double)(kv * a.ku);
    auto fetch = [&](int y, double (&x)[1]) { x[0] = rs[(size_t)y * rstep]; };
    auto emit = [&](int y, const float (&m)[1]) {
        const float q = solve_all_store(m[0], a.solve_all, a.scale);
        if (B.live) vm[(size_t)y * rstep] = q;
    };
    if constexpr (KV > 1)
        box_col_sweep_ring<1, Reflect101, KV, KV - 1>(H, scale, fetch, emit);
    else
        box_col_sweep_tiled<1, Reflect101, BF_T>(H, kv, scale, fetch, emit);
}

constexpr int GFNL_R = 9, GFNL_K = 2 * GFNL_R + 1;   // the variance plane's window (cpp:4454-4455)

// one thread per pixel: arm_Mask = box19(I I) - box19(I)^2 < thresh on the pair's left gray image
__global__ __launch_bounds__(256) void k_gfnl_mask(const uint8_t* __restrict__ gray, size_t gray_pair_stride,
                                                   uint8_t* __restrict__ mask, int H, int W, int n, float thresh) {
    const size_t npix = (size_t)H * W;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix * n) return;
    const size_t b = t / npix, i = t - b * npix;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const uint8_t* g = gray + b * gray_pair_stride;
    uint32_t s1 = 0, s2 = 0;   // <= 361 * 255^2 < 2^25: exact, as the reference's double sums are
    for (int dy = 0; dy < GFNL_K; dy++) {
        const uint8_t* row = g + (size_t)Reflect101::at(y - GFNL_R + dy, H) * W;
#pragma unroll
        for (int dx = 0; dx < GFNL_K; dx++) {
            const uint32_t v = row[Reflect101::at(x - GFNL_R + dx, W)];
            s1 += v;
            s2 += v * v;
        }
    }
    const double scale = 1. / (GFNL_K * GFNL_K);
    const float m = (float)((double)s1 * scale), m2 = (float)((double)s2 * scale);
    const float mm = m * m;
    const float var = m2 - mm;
    mask[t] = var < thresh ? 1 : 0;
}

__device__ __forceinline__ float gfnl_blend1(float r, float g, bool m, int solve_all, float scale) {
    // `0.5 * res + 0.5 * vm` with double literals: one rounding to double, one to float
    const float v = m ? r : (float)(0.5 * (double)r + 0.5 * (double)g);
    return solve_all_store(v, solve_all, scale);
}

// V elements per thread (V = 4 needs D % 4 == 0: the four share a pixel)
template <int V>
__global__ __launch_bounds__(256) void k_gfnl_blend(const GfnlArgs a, size_t nelem) {
    const size_t t = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (t >= nelem) return;
    const bool m = a.mask[t / (size_t)a.D] != 0;
    if constexpr (V == 4) {
        const float4 r = *(const float4*)(a.res + t), g = *(const float4*)(a.vm + t);
        float4 o;
        o.x = gfnl_blend1(r.x, g.x, m, a.solve_all, a.scale);
        o.y = gfnl_blend1(r.y, g.y, m, a.solve_all, a.scale);
        o.z = gfnl_blend1(r.z, g.z, m, a.solve_all, a.scale);
        o.w = gfnl_blend1(r.w, g.w, m, a.solve_all, a.scale);
        *(float4*)(a.vm + t) = o;
    } else {
        a.vm[t] = gfnl_blend1(a.res[t], a.vm[t], m, a.solve_all, a.scale);
    }
}

}  // namespace

void launch_bf_rows(const BfArgs& a, int n, hipStream_t st) {
    const int nchunks = (a.D + 63) / 64;
    hipLaunchKernelGGL(k_bf_rows, dim3(a.H * nchunks * n), dim3(64), 0, st, a);
}

void launch_bf_cols(const BfArgs& a, int n, hipStream_t st) {
    const int nchunks = (a.D + 63) / 64;
    const dim3 grid(a.W * nchunks * n);
    if (a.kv == BF_RING_KV)
        hipLaunchKernelGGL(k_bf_cols<BF_RING_KV>, grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(k_bf_cols<0>, grid, dim3(64), 0, st, a);
}

void launch_gfnl_mask(const GfnlArgs& a, int n, hipStream_t st) {
    const size_t tp = (size_t)n * a.H * a.W;
    hipLaunchKernelGGL(k_gfnl_mask, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, st, a.gray, a.gray_pair_stride,
                       a.mask, a.H, a.W, n, a.thresh);
}

void launch_gfnl_blend(const GfnlArgs& a, int n, hipStream_t st) {
    const size_t nelem = (size_t)n * a.H * a.W * a.D;
    if (a.D % 4 == 0)
        hipLaunchKernelGGL(k_gfnl_blend<4>, dim3((unsigned)((nelem / 4 + 255) / 256)), dim3(256), 0, st, a, nelem);
    else
        hipLaunchKernelGGL(k_gfnl_blend<1>, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, st, a, nelem);
}

}  // namespace sm
