// sm_pyramid.hip — the cross-scale pyramid of main_.cpp:131-158 (PY_LEV > 1).
//
//   pyrDown   cv::pyrDown on the u8 colour / gray inputs (main_.cpp:145-148): 5x5 binomial
//             1-4-6-4-1 filter, BORDER_REFLECT_101, (sum + 128) >> 8, every second row / column.
//   SolveAll  (stereoMatching.cpp:2142-2208) for PY_LVL levels: level 0's volume becomes
//             sum_s invWgt[s] * vm_s(y >> s, x >> s, d_s), d_s = (d_{s-1} + 1) / 2, summed in level
//             order from 0.f (the host computes invWgt with OpenCV's small-matrix invert).
// Both are bandwidth-trivial next to the per-level cost / CBCA passes: pyrDown touches each input
// byte ~2x (cached), SolveAll reads level 0 (4 B / element) plus the coarse levels (1/8, 1/64 of
// that, mostly from L2) and writes level 0 once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

namespace {

// one destination element (pixel x channel) of cv::pyrDown; the 5 x 5 integer sum is exact, so any summation
// order equals OpenCV's separable row-then-column evaluation
__device__ __forceinline__ uint8_t pyr_down_elem(const uint8_t* __restrict__ src, int rows, int cols, int ch, size_t i) {
    const int dc = (cols + 1) / 2;
    const int c = (int)(i % ch);
    const size_t px = i / ch;
    const int x = (int)(px % dc), y = (int)(px / dc);
    const int k[5] = {1, 4, 6, 4, 1};
    int cx[5];
#pragma unroll
    for (int j = 0; j < 5; j++) cx[j] = reflect101(2 * x + j - 2, cols);
    int sum = 0;
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + r - 2, rows) * cols * ch + c;
        int rs = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) rs += k[j] * (int)row[(size_t)cx[j] * ch];
        sum += k[r] * rs;
    }
    return (uint8_t)((sum + 128) >> 8);
}

// one thread per destination pixel x channel
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows,
                                                  int cols, int ch) {
    const int dr = (rows + 1) / 2, dc = (cols + 1) / 2;
    const size_t total = (size_t)dr * dc * ch;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = pyr_down_elem(src, rows, cols, ch, i);
}

// the same for a group's images in one launch: blockIdx.z chooses the colour (0) or the gray (1) images,
// blockIdx.y strides over the nimg images of that kind, blockIdx.x over an image's elements
__global__ __launch_bounds__(256) void k_pyr_down_batch(const uint8_t* __restrict__ src_bgr, const uint8_t* __restrict__ src_gray,
                                                        uint8_t* __restrict__ dst_bgr, uint8_t* __restrict__ dst_gray,
                                                        int rows, int cols, int nimg) {
    const int ch = blockIdx.z == 0 ? 3 : 1;
    const uint8_t* src = blockIdx.z == 0 ? src_bgr : src_gray;
    uint8_t* dst = blockIdx.z == 0 ? dst_bgr : dst_gray;
    const int dr = (rows + 1) / 2, dc = (cols + 1) / 2;
    const size_t total = (size_t)dr * dc * ch, in = (size_t)rows * cols * ch;
    for (int img = blockIdx.y; img < nimg; img += gridDim.y)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
            dst[(size_t)img * total + i] = pyr_down_elem(src + (size_t)img * in, rows, cols, ch, i);
}

// cv::pyrDown on a 1-channel f32 image (main_.cpp:149: the ground truth DT goes down the pyramid
// with the inputs).  OpenCV's scalar pyrDown_ (FltCast<float, 8>) order, restated: the row pass
// r = s0*6 + (s-1 + s+1)*4 + s-2 + s+2 (left to right), the column pass the same over the five row
// sums, then * (1/256) (exact: a power of two).  OpenCV's SIMD rows may fuse multiply-adds, so the
// last bit is unpinned; only the evaluator reads DT, never the disparity path.
__global__ __launch_bounds__(256) void k_pyr_down_f32(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                      int cols) {
    const int dr = (rows + 1) / 2, dc = (cols + 1) / 2;
    const size_t total = (size_t)dr * dc;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % dc), y = (int)(i / dc);
        int cx[5];
#pragma unroll
        for (int j = 0; j < 5; j++) cx[j] = reflect101(2 * x + j - 2, cols);
        float r[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const float* row = src + (size_t)reflect101(2 * y + k - 2, rows) * cols;
            r[k] = row[cx[2]] * 6.f + (row[cx[1]] + row[cx[3]]) * 4.f + row[cx[0]] + row[cx[4]];
        }
        dst[i] = (r[2] * 6.f + (r[1] + r[3]) * 4.f + r[0] + r[4]) * (1.f / 256.f);
    }
}

// one wave per level-0 pixel (grid-stride), lanes over disparities; levels read in order
__global__ __launch_bounds__(256) void k_solve_all_pyr(const PyrArgs a) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    const int H0 = a.H[0], W0 = a.W[0], D0 = a.D[0];
    const size_t npix0 = (size_t)H0 * W0;
    const size_t total = npix0 * (size_t)a.n;
    for (size_t q = wave; q < total; q += nwaves) {
        const size_t b = q / npix0, p = q - b * npix0;
        const int y = (int)(p / W0), x = (int)(p - (size_t)y * W0);
        for (int d = lane; d < D0; d += 64) {
            int cy = y, cx = x, cd = d;
            float sum = 0.f;
            for (int s = 0; s < a.levels; s++) {
                const size_t npix = (size_t)a.H[s] * a.W[s];
                const float cur = a.vm[s][(b * npix + (size_t)cy * a.W[s] + cx) * a.D[s] + cd];
                sum += a.w[s] * cur;
                cy >>= 1;
                cx >>= 1;
                cd = (cd + 1) >> 1;
            }
            a.vm[0][(b * npix0 + p) * D0 + d] = sum;
        }
    }
}

// The batch path's SolveAll: blockIdx = (tile of column pairs, row pair, pair of the batch), so no index is
// divided out per element.  A thread group of `tpp` lanes owns a 2 x 2 block of level-0 pixels -- they share
// every coarser level's pixel, which is read once -- and strides over the disparities in units of four
// (VEC: 16-byte loads and stores; needs D_0 % 4 == 0 and 16-byte aligned volumes) or one.  Four consecutive fine
// disparities 4u .. 4u + 3 map to at most three coarse ones per level (then two).  The four pixels' loads are
// independent and in flight together.  Sums as in k_solve_all_pyr: 0.f + w_0 c_0, then one rounded product and
// one rounded sum per level, in level order.
template <bool VEC>
__global__ __launch_bounds__(256) void k_solve_all_pyr_batch(const PyrArgs a, int tpp, int xstep) {
    constexpr int E = VEC ? 4 : 1;
    const int H0 = a.H[0], W0 = a.W[0], D0 = a.D[0];
    const int U = D0 / E;
    const int u0 = threadIdx.x % tpp, xo = threadIdx.x / tpp;
    const int xp = blockIdx.x * xstep + xo, yp = blockIdx.y;
    if (xo >= xstep || 2 * xp >= W0) return;
    const size_t npix0 = (size_t)H0 * W0;
    const bool has_x1 = 2 * xp + 1 < W0, has_y1 = 2 * yp + 1 < H0;
    const bool ok[4] = {true, has_x1, has_y1, has_x1 && has_y1};
    for (int b = blockIdx.z; b < a.n; b += gridDim.z) {
        float* p0 = a.vm[0] + ((size_t)b * npix0 + (size_t)(2 * yp) * W0 + 2 * xp) * D0;
        float* pix[4] = {p0, p0 + D0, p0 + (size_t)W0 * D0, p0 + (size_t)W0 * D0 + D0};
        for (int u = u0; u < U; u += tpp) {
            const int d = u * E;
            float v[4][4];   // [pixel][disparity of the unit]; the first E are used
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if constexpr (VEC) {
                    const float4 t = ok[q] ? *reinterpret_cast<const float4*>(pix[q] + d) : make_float4(0.f, 0.f, 0.f, 0.f);
                    v[q][0] = t.x;
                    v[q][1] = t.y;
                    v[q][2] = t.z;
                    v[q][3] = t.w;
                } else {
                    v[q][0] = ok[q] ? pix[q][d] : 0.f;
                }
            }
            const float w0 = a.w[0];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int j = 0; j < E; j++) v[q][j] = 0.f + w0 * v[q][j];
            int cd[E];
#pragma unroll
            for (int j = 0; j < E; j++) cd[j] = d + j;
            for (int s = 1; s < a.levels; s++) {
                const int Ws = a.W[s], Ds = a.D[s];
                const float* c = a.vm[s] + (((size_t)b * a.H[s] + (size_t)(yp >> (s - 1))) * Ws + (size_t)(xp >> (s - 1))) * Ds;
#pragma unroll
                for (int j = 0; j < E; j++) cd[j] = (cd[j] + 1) >> 1;
                const int c0 = cd[0], span = cd[E - 1] - c0;   // span <= 2
                const float f0 = c[c0];
                const float f1 = span >= 1 ? c[c0 + 1] : f0;
                const float f2 = span >= 2 ? c[c0 + 2] : f0;
                const float ws = a.w[s];
#pragma unroll
                for (int j = 0; j < E; j++) {
                    const int k = cd[j] - c0;
                    const float t = ws * (k == 0 ? f0 : (k == 1 ? f1 : f2));
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q][j] += t;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!ok[q]) continue;
                if constexpr (VEC)
                    *reinterpret_cast<float4*>(pix[q] + d) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
                else
                    pix[q][d] = v[q][0];
            }
        }
    }
}

}  // namespace

void launch_pyr_down(const uint8_t* src, uint8_t* dst, int rows, int cols, int ch, hipStream_t st) {
    const size_t total = (size_t)((rows + 1) / 2) * ((cols + 1) / 2) * ch;
    size_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_pyr_down, dim3((unsigned)blocks), dim3(256), 0, st, src, dst, rows, cols, ch);
}

void launch_pyr_down_f32(const float* src, float* dst, int rows, int cols, hipStream_t st) {
    const size_t total = (size_t)((rows + 1) / 2) * ((cols + 1) / 2);
    size_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_pyr_down_f32, dim3((unsigned)blocks), dim3(256), 0, st, src, dst, rows, cols);
}

void launch_solve_all_pyr(const PyrArgs& a, hipStream_t st) {
    const size_t waves = (size_t)a.H[0] * a.W[0] * a.n;
    size_t blocks = (waves + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_solve_all_pyr, dim3((unsigned)blocks), dim3(256), 0, st, a);
}

void launch_pyr_down_batch(const uint8_t* src_bgr, const uint8_t* src_gray, uint8_t* dst_bgr, uint8_t* dst_gray, int rows,
                           int cols, int nimg, hipStream_t st) {
    if (nimg < 1) return;
    const size_t total = (size_t)((rows + 1) / 2) * ((cols + 1) / 2) * 3;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_pyr_down_batch, dim3((unsigned)blocks, (unsigned)std::min(nimg, 32768), 2), dim3(256), 0, st, src_bgr,
                       src_gray, dst_bgr, dst_gray, rows, cols, nimg);
}

void launch_solve_all_pyr_batch(const PyrArgs& a, hipStream_t st) {
    if (a.n < 1) return;
    const bool vec = a.D[0] % 4 == 0 && ((uintptr_t)a.vm[0] & 15) == 0;
    const int U = vec ? a.D[0] / 4 : a.D[0];
    const int tpp = std::min(U, 256), xstep = 256 / tpp;
    const int Wp = (a.W[0] + 1) / 2, Hp = (a.H[0] + 1) / 2;
    const dim3 grid((unsigned)((Wp + xstep - 1) / xstep), (unsigned)Hp, (unsigned)std::min(a.n, 32768));
    if (vec) hipLaunchKernelGGL(k_solve_all_pyr_batch<true>, grid, dim3(256), 0, st, a, tpp, xstep);
    else hipLaunchKernelGGL(k_solve_all_pyr_batch<false>, grid, dim3(256), 0, st, a, tpp, xstep);
}

}  // namespace sm
