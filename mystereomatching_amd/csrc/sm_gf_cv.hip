// sm_gf_cv.hip — aggregation "GF" in the form the reference's shipped build runs:
// cv::ximgproc::guidedFilter(I_c[i] as float, vm[i], vm[i], gf_r[0] = 9, gf_eps[0] = 1e-4)
// (stereoMatching.cpp:4513, `//#define MY_GUIDE` at h:38; constants h:297-298).  The restated
// algorithm (oracle/sm_oracle_agg.c, smo_guided_filter_cv) is He et al.'s colour guided filter in
// the structure of ximgproc's GuidedFilterImpl, every mean an OpenCV normalised box filter with
// BORDER_REFLECT, 19 x 19 (sm_box_sweep.h: the filter, shared with "BF"):
//
//   Sigma        = box(I_i I_j) - mean_I_i mean_I_j (+ eps on the diagonal), inverted by cofactors
//   alpha_c      = sum_k Sigma^-1(c, k) (box(p I_k) - mean_p mean_I_k),  beta = mean_p - alpha . mean_I
//   q            = box(beta) + sum_c box(alpha_c) I_c
//
// gfx950 mapping.  The p-independent terms (mean_I and Sigma^-1 per pixel, 9 floats) come from
// nine image planes, row-summed by one thread per row (k_gfcv_img_rows), column-summed by one
// thread per plane and column (k_gfcv_img_cols), Sigma inverted per pixel (k_gfcv_pix).  The
// volume work is four of the header's line sweeps over [H][W][D], each carrying four channels:
//   R0: row sums of (p, p B, p G, p R)          -> RS (four double volumes)
//   C0: column sums -> mean_p, cov, alpha, beta -> AB (four float volumes)
//   R1: row sums of (alpha_0..2, beta)           -> RS
//   C1: column sums -> q                         -> vm  [+ SolveAll's 0 + w q]
// The double intermediates are what OpenCV's FilterEngine keeps between its row and column
// filters; a row chain (RowSum's running update) can only run sequentially along the whole row,
// so the row sums round-trip HBM.  The float products and sums around the box means are the
// restatement's, in its order (-ffp-contract=off: no fused multiply-adds), so the volume is
// bit-exact to the oracle.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_box_sweep.h"
#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

namespace {

constexpr int GC_R = 9;              // gf_r[0] (h:297)
constexpr int GC_K = 2 * GC_R + 1;   // box size
#ifndef SM_GFCV_PF
#define SM_GFCV_PF 3     // rows of row sums prefetched ahead by the column sweeps (divides 18)
#endif
#ifndef SM_GFCV_T
#define SM_GFCV_T 4   // positions per prefetched tile of the row sweeps (two tiles in flight)
#endif

// image planes 0..8: B, G, R, BB, BG, BR, GG, GR, RR (float products of the float guide)
__device__ __forceinline__ float gc_plane(uint32_t w, int k) {
    const float b = (float)(w & 0xffu), g = (float)((w >> 8) & 0xffu), r = (float)((w >> 16) & 0xffu);
    switch (k) {
        case 0: return b;
        case 1: return g;
        case 2: return r;
        case 3: return b * b;
        case 4: return b * g;
        case 5: return b * r;
        case 6: return g * g;
        case 7: return g * r;
        default: return r * r;
    }
}

// one thread per (pair, plane, row): the plane's row sums into rs
__global__ __launch_bounds__(256) void k_gfcv_img_rows(const uint32_t* __restrict__ px, size_t px_pair_stride,
                                                       double* __restrict__ rs, int H, int W, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 9 * H) return;
    const int y = t % H, k = (t / H) % 9, b = t / (9 * H);
    const uint32_t* row = px + (size_t)b * px_pair_stride + (size_t)y * W;
    double* out = rs + (((size_t)b * 9 + k) * H + y) * W;
    box_row_sweep<1, Reflect, SM_GFCV_T, GC_K>(
        W, GC_K, [&](int u, float (&x)[1]) { x[0] = gc_plane(row[u], k); }, [&](int u, const double (&S)[1]) { out[u] = S[0]; });
}

// one thread per (pair, plane, column): the plane's box means into pix[b][k] (planes 3..8 are
// replaced by Sigma^-1 in k_gfcv_pix).  The tiled column form (a column walk is a chain of
// dependent adds: the next rows' sums are loaded while the current ones are added).
__global__ __launch_bounds__(256) void k_gfcv_img_cols(const double* __restrict__ rs, float* __restrict__ pix, int H, int W,
                                                       int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 9 * W) return;
    const int x = t % W, k = (t / W) % 9, b = t / (9 * W);
    const size_t npix = (size_t)H * W;
    const double* base = rs + ((size_t)b * 9 + k) * npix + x;
    float* out = pix + ((size_t)b * 9 + k) * npix + x;
    box_col_sweep_tiled<1, Reflect, SM_GFCV_T>(
        H, GC_K, 1. / (GC_K * GC_K), [&](int y, double (&v)[1]) { v[0] = base[(size_t)y * W]; },
        [&](int y, const float (&m)[1]) { out[(size_t)y * W] = m[0]; });
}

// per pixel: Sigma = box(I_i I_j) - m_i m_j (+ eps on the diagonal) and its inverse by the
// restatement's float cofactors / det, written over the box(I_i I_j) planes 3..8 as the entries
// 00, 01, 02, 11, 12, 22 (planes 0..2 keep mean_I)
__global__ __launch_bounds__(256) void k_gfcv_pix(float* __restrict__ pix, int H, int W, int n, float eps) {
    const size_t npix = (size_t)H * W;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npix * n) return;
    const size_t b = t / npix, i = t - b * npix;
    float* pl = pix + b * 9 * npix + i;
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = pl[k * npix];
    float a[6];
    {
        const int I0[6] = {0, 0, 0, 1, 1, 2}, I1[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int v = 0; v < 6; v++) {
            const float mm = m[I0[v]] * m[I1[v]];
            a[v] = m[3 + v] - mm;
            if (I0[v] == I1[v]) a[v] = a[v] + eps;
        }
    }
    const float a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    float b00 = a11 * a22, b01 = a02 * a12, b02 = a01 * a12, b11 = a00 * a22, b12 = a01 * a02, b22 = a00 * a11;
    float mm;
    mm = a12 * a12; b00 = b00 - mm;
    mm = a01 * a22; b01 = b01 - mm;
    mm = a02 * a11; b02 = b02 - mm;
    mm = a02 * a02; b11 = b11 - mm;
    mm = a00 * a12; b12 = b12 - mm;
    mm = a01 * a01; b22 = b22 - mm;
    float det = a00 * b00;
    mm = a01 * b01; det = det + mm;
    mm = a02 * b02; det = det + mm;
    pl[3 * npix] = b00 / det;
    pl[4 * npix] = b01 / det;
    pl[5 * npix] = b02 / det;
    pl[6 * npix] = b11 / det;
    pl[7 * npix] = b12 / det;
    pl[8 * npix] = b22 / det;
}

// ---------------------------------------------------------------------------------------------
// Row sweep: one wave per (pair, row, chunk), lane = disparity.  MODE 0 reads p (vm) and the
// guide, MODE 1 reads alpha_0..2, beta (AB).
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(64) void k_gfcv_rows(const GfCvArgs a) {
    const LineBlock B = line_block(a.H, a.D);
    const int W = a.W, D = a.D;
    const size_t npix = (size_t)a.H * W;
    const size_t nvol = npix * D;
    const size_t row0 = ((size_t)B.pair * npix + (size_t)B.line * W) * D;   // element (b, y, 0, 0)
    const uint32_t* gw = a.px + (size_t)B.pair * a.px_pair_stride + (size_t)B.line * W;
    const float* vm = a.vm + row0 + B.dd;
    const float* ab = a.ab + row0 + B.dd;
    double* rs = a.rs + row0 + B.d;
    const size_t plane = (size_t)a.cap * nvol;   // elements between the channel planes of RS and AB

    box_row_sweep<4, Reflect, SM_GFCV_T, GC_K>(
        W, GC_K,
        [&](int u, float (&x)[4]) {
            const size_t e = (size_t)u * D;
            if (MODE == 0) {
                const float p = vm[e];
                const uint32_t w = gw[u];
                x[0] = p;
                x[1] = p * (float)(w & 0xffu);             // mul(src, guideCn[0]) (covSrcGuide)
                x[2] = p * (float)((w >> 8) & 0xffu);
                x[3] = p * (float)((w >> 16) & 0xffu);
            } else {
#pragma unroll
                for (int c = 0; c < 4; c++) x[c] = ab[c * plane + e];
            }
        },
        [&](int u, const double (&S)[4]) {
            if (!B.live) return;
#pragma unroll
            for (int c = 0; c < 4; c++) rs[c * plane + (size_t)u * D] = S[c];
        });
}

// ---------------------------------------------------------------------------------------------
// Column sweep: one wave per (pair, column, chunk), lane = disparity.
// MODE 0: mean_p, box(p I_c) -> cov, alpha, beta -> AB.  MODE 1: box(alpha), box(beta) -> q -> vm.
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(64) void k_gfcv_cols(const GfCvArgs a) {
    const LineBlock B = line_block(a.W, a.D);
    const int H = a.H, W = a.W, D = a.D;
    const size_t npix = (size_t)H * W;
    const size_t nvol = npix * D;
    const size_t col0 = ((size_t)B.pair * npix + B.line) * D;   // element (b, 0, u, 0)
    const size_t rstep = (size_t)W * D;
    const double* rs = a.rs + col0 + B.dd;
    float* ab = a.ab + col0 + B.d;
    float* vm = a.vm + col0 + B.d;
    const size_t plane = (size_t)a.cap * nvol;   // elements between the channel planes of RS and AB
    const float* pix = a.pix + (size_t)B.pair * 9 * npix + B.line;
    const uint32_t* gw = a.px + (size_t)B.pair * a.px_pair_stride + B.line;

    // output row y from the box means m (MODE 0: alpha, beta -> AB; MODE 1: q -> vm)
    auto emit = [&](int y, const float (&m)[4]) {
        const size_t po = (size_t)y * W;
        const size_t e = (size_t)y * rstep;
        if (MODE == 0) {
            const float mI[3] = {pix[0 * npix + po], pix[1 * npix + po], pix[2 * npix + po]};
            const float iv[6] = {pix[3 * npix + po], pix[4 * npix + po], pix[5 * npix + po],
                                 pix[6 * npix + po], pix[7 * npix + po], pix[8 * npix + po]};
            const float mP = m[0];
            float cov[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float mm = mP * mI[c];
                cov[c] = m[1 + c] - mm;
            }
            // inverse entry (g, k): 00 01 02 / 01 11 12 / 02 12 22
            const int IX[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            float al[3];
#pragma unroll
            for (int g = 0; g < 3; g++) {
                float acc = iv[IX[g][0]] * cov[0];
#pragma unroll
                for (int k = 1; k < 3; k++) {
                    const float mm = iv[IX[g][k]] * cov[k];
                    acc = acc + mm;
                }
                al[g] = acc;
            }
            float be = mP;
#pragma unroll
            for (int g = 0; g < 3; g++) {
                const float mm = al[g] * mI[g];
                be = be - mm;
            }
            if (B.live) {
                ab[0 * plane + e] = al[0];
                ab[1 * plane + e] = al[1];
                ab[2 * plane + e] = al[2];
                ab[3 * plane + e] = be;
            }
        } else {
            const uint32_t w = gw[po];
            const float I[3] = {(float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu)};
            float q = m[3];   // box(beta)
#pragma unroll
            for (int g = 0; g < 3; g++) {
                const float mm = m[g] * I[g];
                q = q + mm;
            }
            q = solve_all_store(q, a.solve_all, a.scale);
            if (B.live) vm[e] = q;
        }
    };
    // The ring form: the tiled form (tools/experiments/gfcv_cols_tiled.patch) read the leaving row
    // a second time 18 rows later, past L2.
    box_col_sweep_ring<4, Reflect, GC_K, SM_GFCV_PF>(
        H, 1. / (GC_K * GC_K),
        [&](int y, double (&x)[4]) {
#pragma unroll
            for (int c = 0; c < 4; c++) x[c] = rs[c * plane + (size_t)y * rstep];
        },
        emit);
}

}  // namespace

size_t gfcv_img_scratch_doubles(int H, int W, int n) { return (size_t)n * 9 * H * W; }

void launch_gf_cv(const GfCvArgs& a, int n, hipStream_t st) {
    {
        const int tr = n * 9 * a.H;
        hipLaunchKernelGGL(k_gfcv_img_rows, dim3((tr + 255) / 256), dim3(256), 0, st, a.px, a.px_pair_stride, a.img_rs, a.H,
                           a.W, n);
        const int tc = n * 9 * a.W;
        hipLaunchKernelGGL(k_gfcv_img_cols, dim3((tc + 255) / 256), dim3(256), 0, st, a.img_rs, a.pix, a.H, a.W, n);
        const size_t tp = (size_t)n * a.H * a.W;
        hipLaunchKernelGGL(k_gfcv_pix, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, st, a.pix, a.H, a.W, n, a.eps);
    }
    const int nchunks = (a.D + 63) / 64;
    hipLaunchKernelGGL(k_gfcv_rows<0>, dim3(a.H * nchunks * n), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_gfcv_cols<0>, dim3(a.W * nchunks * n), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_gfcv_rows<1>, dim3(a.H * nchunks * n), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_gfcv_cols<1>, dim3(a.W * nchunks * n), dim3(64), 0, st, a);
}

}  // namespace sm
