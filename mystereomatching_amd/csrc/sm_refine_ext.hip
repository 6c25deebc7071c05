// sm_refine_ext.hip — three more stages of refine() (stereoMatching.cpp:1347-1510), off by default
// (sm_refine_ext_config): the peak-ratio check (Do_calPKR: calPKR + signDp_UsingPKR, cpp:4087-4140), the
// background fill (Do_bgIpol: BGIpol + backgroundInterpolateCore, cpp:7323-7338, 7011-7043) and the sub-pixel
// map (Do_subpixelEnhancement: subpixelEnhancement + medianBlur(SE, SE, 3), cpp:6138-6167, 1482-1495).
// A translation unit of its own; it shares sm_refine.hip's pixel mapping (sm_refine_map.h).
//
// k_pkr          the one volume pass.  16 lanes (one DPP row) serve a pixel: each keeps the two smallest of the
//                costs it reads (lane l the disparities 64 c + 4 l .. + 3 of every chunk c with 16-byte loads
//                when D % 4 == 0, else d = 16 c + l, both contiguous over the row), the pairs are merged with
//                four DPP steps inside the row, lane 0 writes the mask byte and marks DP[0].  Any D >= 2.
// k_bg_r         BGIpol's right search on the input map: one wave per (pair, row) walks the row right to left in
//                64-column chunks; r(u) is the nearest valid value in (u, u + depth] or -1.
// k_bg_scan      BGIpol's in-place walk as a first-order recurrence: the same wave layout, left to
//                right, an inclusive scan of (constant | min-with-constant) maps per chunk and one carried value.
// k_subpixel     three gathered costs per pixel, both forms of the result.
// k_median3_f32  k_median3's network on floats.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "sm_device.h"
#include "sm_kernels.h"
#include "sm_refine_map.h"

namespace sm {

namespace {

// the two smallest of a multiset, (a0 <= a1): merge with another such pair.  No NaN reaches here.
__device__ __forceinline__ void pkr_merge(float& a0, float& a1, float b0, float b1) {
    const float lo = fminf(a0, b0), hi = fmaxf(a0, b0);
    a1 = fminf(hi, fminf(a1, b1));
    a0 = lo;
}

// calPKR's scan is `vmP[d] < min` from min = FLT_MAX: a NaN, +inf or FLT_MAX never becomes a minimum
__device__ __forceinline__ void pkr_take(float& m0, float& m1, float x) {
    const bool t0 = x < m0, t1 = x < m1;
    m1 = t0 ? m0 : (t1 ? x : m1);
    m0 = t0 ? x : m0;
}

template <int CTRL>
__device__ __forceinline__ void pkr_step(float& m0, float& m1) {
    const float o0 = dpp_f<CTRL>(m0), o1 = dpp_f<CTRL>(m1);
    pkr_merge(m0, m1, o0, o1);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_pkr(PkrArgs a, long total) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long pix = gid >> 4;
    const int l = threadIdx.x & 15;
    const bool live = pix < total;
    const int D = a.D;
    const float* p = a.vm + (size_t)(live ? pix : 0) * D;
    float m0 = FLT_MAX, m1 = FLT_MAX;
    if (live) {
        if (VEC) {   // D % 4 == 0 and a 16-byte aligned volume: d + 3 < D
#pragma unroll 2
            for (int d = 4 * l; d < D; d += 64) {
                const float4 t = *reinterpret_cast<const float4*>(p + d);
                pkr_take(m0, m1, t.x);
                pkr_take(m0, m1, t.y);
                pkr_take(m0, m1, t.z);
                pkr_take(m0, m1, t.w);
            }
        } else {
#pragma unroll 4
            for (int d = l; d < D; d += 16) pkr_take(m0, m1, p[d]);
        }
    }
    // every lane of the wave takes part (dead groups carry FLT_MAX pairs)
    pkr_step<DPP_QUAD_1032>(m0, m1);
    pkr_step<DPP_QUAD_2301>(m0, m1);
    pkr_step<DPP_ROW_HALF_MIRROR>(m0, m1);
    pkr_step<DPP_ROW_MIRROR>(m0, m1);
    if (live && l == 0) {
        // The two values decide, not their slots -- but for the sign of a zero: with c0 < 0 and c1 == 0 the ratio is
        // +inf or -inf by it, and the reference's c1 is the first zero in d order (its strict `<` keeps it).  Rare,
        // so this lane rescans the pixel.  (Every other ratio is the same for either zero: a zero c0 under c1 > 0
        // gives 1, two zeros give NaN.)
        if (m1 == 0.0f && m0 < 0.0f)
            for (int d = 0; d < D; d++) {
                const float x = p[d];
                if (x == 0.0f) {
                    m1 = x;
                    break;
                }
            }
        // (cost[1] - cost[0]) / cost[1] < ratio_PKR in float (cpp:4118); 0 / 0 = NaN compares false
        const float num = m1 - m0;
        const float q = num / m1;
        const bool bad = q < a.ratio;
        a.mask[pix] = bad ? 1 : 0;
        if (bad && a.disp[pix] >= 0) a.disp[pix] = (int16_t)a.disp_pkr;   // signDp_UsingPKR (cpp:4136)
    }
}

constexpr int BG_NONE = 0x7fffffff;   // "no candidate" of BGIpol's recurrence: min' treats it as +infinity

// rows of n pairs, one wave each; returns false past the last row
__device__ __forceinline__ bool bg_row(const BgArgs& a, size_t& base) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    base = (size_t)row * a.W;
    return row < (long)a.n * a.H;
}

__global__ __launch_bounds__(256) void k_bg_r(BgArgs a) {
    size_t base;
    if (!bg_row(a, base)) return;   // wave-uniform
    const int lane = threadIdx.x & 63, W = a.W;
    const int16_t* src = a.src + base;
    int16_t* r = a.r + base;
    int cpos = -1, cval = 0;   // the nearest valid pixel right of the chunk (cpos < 0: none)
    for (int c0 = (W - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
        const int u = c0 + lane;
        const int v = u < W ? (int)src[u] : -1;
        const unsigned long long m = __ballot(v >= 0);
        const unsigned long long above = lane == 63 ? 0ull : m & (~0ull << (lane + 1));
        const int j = above ? __ffsll((long long)above) - 1 : 0;
        const int vj = __shfl(v, j, 64);   // every lane takes part
        const int pos = above ? c0 + j : cpos;
        const int val = above ? vj : cval;
        if (u < W) r[u] = (int16_t)((pos >= 0 && pos - u <= a.depth) ? val : -1);
        if (m) {   // wave-uniform
            const int j0 = __ffsll((long long)m) - 1;
            cpos = c0 + j0;
            cval = __shfl(v, j0, 64);
        }
    }
}

// y(u) = valid ? old(u) : min'(r(u), y(u - 1)) with y(-1) = none; new(u) = y(u) unless it is none (then old(u)).
// A pixel's map of y(u - 1) is the constant k (valid) or x -> min(k, x) (hole; k = r(u) or none).  With
// f = (cf, kf) applied first and g = (cg, kg) second, g o f = (cg | cf, cg ? kg : min(kg, kf)).
__global__ __launch_bounds__(256) void k_bg_scan(BgArgs a) {
    size_t base;
    if (!bg_row(a, base)) return;
    const int lane = threadIdx.x & 63, W = a.W;
    const int16_t* src = a.src + base;
    int16_t* r = a.r + base;   // read as r(u), rewritten as new(u) by the same lane
    int carry = BG_NONE;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int u = c0 + lane;
        const bool in = u < W;
        const int old = in ? (int)src[u] : -1;
        const int ru = in ? (int)r[u] : -1;
        int cf = old >= 0 ? 1 : 0;                              // lanes past W: the identity min(none, x)
        int k = old >= 0 ? old : (ru >= 0 ? ru : BG_NONE);
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int pc = __shfl_up(cf, s, 64), pk = __shfl_up(k, s, 64);
            if (lane >= s) {
                k = cf ? k : min(k, pk);
                cf |= pc;
            }
        }
        const int y = cf ? k : min(k, carry);
        if (in) r[u] = (int16_t)(y == BG_NONE ? old : y);
        carry = __shfl(y, 63, 64);
    }
}

// subpixelEnhancement (cpp:6138-6167).  SM_SE_REFERENCE: `disp -= diff` on a short (cpp:6161) converts
// fl((float)d - diff) back to short, truncating toward zero; SM_SE_FLOAT keeps the float.
__global__ __launch_bounds__(256) void k_subpixel(const int16_t* __restrict__ dp, const float* __restrict__ vm,
                                                  float* __restrict__ se, int H, int W, int D, int keep_float) {
    const Pix p = pixel_of(H, W);
    if (!p.ok) return;
    const size_t o = ((size_t)p.b * H + p.v) * W + p.u;
    const int d = dp[o];
    float out = (float)d;
    if (d > 0 && d < D - 1) {
        const float* c = vm + o * D + d;
        const float cost = c[0], cp = c[1], cm = c[-1];
        const float two_c = 2 * cost;
        const float sum = cp + cm;
        const float inner = sum - two_c;
        const float denom = 2 * inner;
        if (denom != 0) {
            const float num = cp - cm;
            const float diff = num / denom;
            if (diff > -1 && diff < 1) {
                const float f = (float)d - diff;
                out = keep_float ? f : (float)(int16_t)f;
            }
        }
    }
    se[o] = out;
}

__device__ __forceinline__ void cswap_f(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

// cv::medianBlur(SE, SE, 3) (cpp:1490) on CV_32F: k_median3's network; the map holds no NaN
__global__ __launch_bounds__(256) void k_median3_f32(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
    const Pix p = pixel_of(H, W);
    if (!p.ok) return;
    const size_t npix = (size_t)H * W;
    const float* s = src + (size_t)p.b * npix;
    const int r0 = max(p.v - 1, 0) * W, r1 = p.v * W, r2 = min(p.v + 1, H - 1) * W;
    const int c0 = max(p.u - 1, 0), c1 = p.u, c2 = min(p.u + 1, W - 1);
    float x0 = s[r0 + c0], x1 = s[r0 + c1], x2 = s[r0 + c2];
    float x3 = s[r1 + c0], x4 = s[r1 + c1], x5 = s[r1 + c2];
    float x6 = s[r2 + c0], x7 = s[r2 + c1], x8 = s[r2 + c2];
    cswap_f(x1, x2); cswap_f(x4, x5); cswap_f(x7, x8);
    cswap_f(x0, x1); cswap_f(x3, x4); cswap_f(x6, x7);
    cswap_f(x1, x2); cswap_f(x4, x5); cswap_f(x7, x8);
    cswap_f(x0, x3); cswap_f(x5, x8); cswap_f(x4, x7);
    cswap_f(x3, x6); cswap_f(x1, x4); cswap_f(x2, x5);
    cswap_f(x4, x7); cswap_f(x4, x2); cswap_f(x6, x4);
    cswap_f(x4, x2);
    dst[(size_t)p.b * npix + (size_t)p.v * W + p.u] = x4;
}

}  // namespace

bool refine_ext_shape_ok(int H, int W, int n) {
    const double px = (double)H * W * n;
    return px * 16 / 256 < 2147483647.0 && px < 2147483647.0 * 16;
}

void launch_pkr(const PkrArgs& a, hipStream_t st) {
    const long total = (long)a.n * a.H * a.W;
    const dim3 grid((unsigned)((total * 16 + 255) / 256));
    if (a.D % 4 == 0 && ((uintptr_t)a.vm & 15) == 0) hipLaunchKernelGGL(k_pkr<true>, grid, dim3(256), 0, st, a, total);
    else hipLaunchKernelGGL(k_pkr<false>, grid, dim3(256), 0, st, a, total);
}

void launch_bg_ipol(const BgArgs& a, hipStream_t st) {
    const long rows = (long)a.n * a.H;
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(k_bg_r, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_bg_scan, grid, dim3(256), 0, st, a);
}

void launch_subpixel(const int16_t* dp, const float* vm, float* se, int n, int H, int W, int D, int keep_float,
                     hipStream_t st) {
    hipLaunchKernelGGL(k_subpixel, grid_of(n, H, W), dim3(256), 0, st, dp, vm, se, H, W, D, keep_float);
}

void launch_median3_f32(const float* src, float* dst, int n, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(k_median3_f32, grid_of(n, H, W), dim3(256), 0, st, src, dst, H, W);
}

}  // namespace sm
