// sm_bf.hip — OpenCV's normalised cv::boxFilter on f32 with BORDER_REFLECT_101, an arbitrary window
// kv x ku (each in [1, 32]) and the default anchor k / 2, as two aggregations use it:
//
//   "BF"   (BF(), stereoMatching.cpp:1023-1043): boxFilter(vm[i], vm[i], -1, Size(12, 12)) on every
//          view's whole volume, in place;
//   "GFNL" (GFNL(), cpp:4421-4490): var = box19(I I) - box19(I) box19(I) of the left gray image,
//          arm_Mask = var < 400, and vm[0] = mask ? NL : (float)(0.5 NL + 0.5 GF).
//
// The filter (generic RowSum<float, double> + ColumnSum<double, float>), anchors av = kv / 2,
// au = ku / 2, r = REFLECT_101 (p < 0 -> -p; p >= n -> 2n - 2 - p; one reflection suffices for
// n >= k / 2 + 1):
//   RS(y, x)  = running row sum in double: the first ku reflected values x - au .. x - au + ku - 1,
//               then s += (double)src[r(x + ku - au)] - (double)src[r(x - au)]
//   out(y, x) = (float)(s0 * 1 / (kv ku)),  s0 = SUM + RS(r(y + kv - 1 - av)),  SUM = s0 - RS(r(y - av)),
//               SUM starting as the sum of RS(r(i - av)), i < kv - 1
// An even window is therefore not centred: 12 covers the offsets -6 .. +5.
//
// gfx950 mapping (volume): two line sweeps over [H][W][D] with lane = disparity and one wave per
// (line, 64-disparity chunk), like the "GF" sweeps (sm_gf_cv.hip):
//   k_bf_rows  p -> RS (one double volume); the element leaving the window is read again (it was
//              loaded ku positions earlier: an L1 / L2 hit)
//   k_bf_cols  RS -> vm [+ SolveAll's 0 + w q].  At the reference's kv = 12 the window's row sums
//              sit in a register ring of kv - 1 rows, so every RS element is read once; any other
//              kv reads the leaving row again.
// 4 + 8 + 8 + 4 = 24 B per element.  Every operation is the reference's, in its order
// (-ffp-contract=off).
//
// The variance plane is two 19 x 19 filters of integers <= 255^2: their sums are exact (below
// 2^25, in uint32 here as in the reference's doubles), so the order of the taps is free and one
// thread per pixel sums the window directly.
// A translation unit of its own (it shares no code with the guided filter).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

namespace {

constexpr int BF_T = 4;        // positions per prefetched tile (two tiles in flight)
constexpr int BF_RING_KV = 12; // the reference's window height: the column sweep's ring form

// OpenCV borderInterpolate(BORDER_REFLECT_101) where one reflection suffices
__device__ __forceinline__ int bf_r101(int p, int len) { return p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p); }

// one wave per (pair, row, chunk)
__global__ __launch_bounds__(64) void k_bf_rows(const BfArgs a) {
    constexpr int T = BF_T;
    const int lane = threadIdx.x;
    const int nchunks = (a.D + 63) >> 6;
    const int blk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int b = blk / (a.H * nchunks);
    const int lc = blk - b * a.H * nchunks;
    const int y = lc / nchunks, chunk = lc - y * nchunks;
    const int d = chunk * 64 + lane;
    const bool live = d < a.D;
    const int dd = live ? d : a.D - 1;
    const int W = a.W, D = a.D, ku = a.ku, au = ku / 2;
    const size_t row0 = (((size_t)b * a.H + y) * W) * D + dd;   // element (b, y, 0, dd)
    const float* __restrict__ vm = a.vm;
    double* __restrict__ rs = a.rs;
    const int L = W + ku - 1;   // ext positions: position i is column r101(i - au)

    struct Tile {
        float in[T], out[T];
    };
    auto load = [&](Tile& t, int i0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = min(i0 + s, L - 1);
            t.in[s] = vm[row0 + (size_t)bf_r101(i - au, W) * D];
            t.out[s] = vm[row0 + (size_t)bf_r101(max(i - ku, 0) - au, W) * D];
        }
    };
    double S = 0;
    auto process = [&](const Tile& t, int i0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = i0 + s;
            if (i >= L) break;   // wave-uniform
            if (i < ku)
                S += (double)t.in[s];
            else
                S += (double)t.in[s] - (double)t.out[s];
            if (i >= ku - 1 && live) rs[row0 - dd + d + (size_t)(i - (ku - 1)) * D] = S;
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

// one wave per (pair, column, chunk).  KV > 0: the window height, known at compile time (ring
// form); KV == 0: a.kv (the leaving row is read again)
template <int KV>
__global__ __launch_bounds__(64) void k_bf_cols(const BfArgs a) {
    constexpr int T = BF_T;
    const int lane = threadIdx.x;
    const int nchunks = (a.D + 63) >> 6;
    const int blk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int b = blk / (a.W * nchunks);
    const int lc = blk - b * a.W * nchunks;
    const int u = lc / nchunks, chunk = lc - u * nchunks;
    const int d = chunk * 64 + lane;
    const bool live = d < a.D;
    const int dd = live ? d : a.D - 1;
    const int H = a.H, W = a.W, D = a.D;
    const int kv = KV > 0 ? KV : a.kv, av = kv / 2;
    const size_t col0 = (((size_t)b * H) * W + u) * D + dd;   // element (b, 0, u, dd)
    const size_t rstep = (size_t)W * D;
    const double* __restrict__ rs = a.rs;
    float* __restrict__ vm = a.vm;
    const double scale = 1. / (double)(kv * a.ku);
    auto emit = [&](int y, double s0) {
        float q = (float)(s0 * scale);
        if (a.solve_all) {   // SolveAll fused (sm_run): its `sum = 0; sum += w * v`
            float sum = 0.f;
            sum += a.scale * q;
            q = sum;
        }
        if (live) vm[col0 - dd + d + (size_t)y * rstep] = q;
    };
    double SUM = 0;
    if constexpr (KV > 1) {
        // The row sum leaving at output y (ext row y) entered at output y - (kv - 1), or is one of
        // the kv - 1 rows SUM starts from: a ring of kv - 1 rows, slot y mod (kv - 1).
        constexpr int RK = KV - 1;
        double ring[RK], nx[RK];
#pragma unroll
        for (int i = 0; i < RK; i++) ring[i] = rs[col0 + (size_t)bf_r101(i - av, H) * rstep];
#pragma unroll
        for (int i = 0; i < RK; i++) SUM += ring[i];
        auto fetch = [&](int y) { return rs[col0 + (size_t)bf_r101(min(y, H - 1) + RK - av, H) * rstep]; };
#pragma unroll
        for (int k = 0; k < RK; k++) nx[k] = fetch(k);
        for (int y0 = 0; y0 < H; y0 += RK) {
#pragma unroll
            for (int s = 0; s < RK; s++) {
                const int y = y0 + s;
                if (y >= H) break;   // wave-uniform
                const double sp = nx[s];
                const double s0 = SUM + sp;
                SUM = s0 - ring[s];
                ring[s] = sp;
                nx[s] = fetch(y + RK);
                emit(y, s0);
            }
        }
    } else {
        for (int i = 0; i < kv - 1; i++) SUM += rs[col0 + (size_t)bf_r101(i - av, H) * rstep];
        struct Tile {
            double sp[T], sm[T];
        };
        auto load = [&](Tile& t, int y0) {
#pragma unroll
            for (int s = 0; s < T; s++) {
                const int y = min(y0 + s, H - 1);
                t.sp[s] = rs[col0 + (size_t)bf_r101(y + kv - 1 - av, H) * rstep];
                t.sm[s] = rs[col0 + (size_t)bf_r101(y - av, H) * rstep];
            }
        };
        auto process = [&](const Tile& t, int y0) {
#pragma unroll
            for (int s = 0; s < T; s++) {
                const int y = y0 + s;
                if (y >= H) break;   // wave-uniform
                const double s0 = SUM + t.sp[s];
                SUM = s0 - t.sm[s];
                emit(y, s0);
            }
        };
        Tile ta, tb;
        load(ta, 0);
        for (int y0 = 0; y0 < H; y0 += 2 * T) {
            load(tb, y0 + T);
            process(ta, y0);
            if (y0 + T >= H) break;
            load(ta, y0 + 2 * T);
            process(tb, y0 + T);
        }
    }
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
        const uint8_t* row = g + (size_t)bf_r101(y - GFNL_R + dy, H) * W;
#pragma unroll
        for (int dx = 0; dx < GFNL_K; dx++) {
            const uint32_t v = row[bf_r101(x - GFNL_R + dx, W)];
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
    float v = m ? r : (float)(0.5 * (double)r + 0.5 * (double)g);
    if (solve_all) {   // SolveAll fused (sm_run): its `sum = 0; sum += w * v`
        float sum = 0.f;
        sum += scale * v;
        v = sum;
    }
    return v;
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
