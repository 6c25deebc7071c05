// sm_cbca_dw.hip — CBCA()'s double-window branch (Parameters::cbca_double_win, cpp:4337-4357): the volume is
// aggregated twice, with the arms of window 1 (into a second volume) and of window 0 (in place), and
// combine2Vm_4 (cpp:4273-4331) gives every pixel whose neighbourhood has only short window-0 arms the
// large-window costs.  The two aggregations are the sweeps above with a second arm set; this file holds the
// mask and the selection.  The sweeps are sm_cbca.hip's; this file is a translation unit of its own.
//
// k_dw_mask    arm_Lst(v, u) = the longest of the four window-0 arms of the LEFT image (HVL[0], cpp:4287),
//              cv::boxFilter 3 x 3 (normalised, BORDER_REFLECT_101, double sums, (float)(sum * (1.0 / 9))),
//              arm_Mask = filtered < armLthres.  Arm lengths are integers, so the nine-term sum is exact in
//              any order, and the float form is non-decreasing in it: the host turns the threshold into
//              the integer isum with `filtered < thres  <=>  sum < isum` for every sum the arm kernel can
//              produce (dw_int_threshold, sm_validate.cpp; 45 for the reference's 5).  One thread per pixel,
//              one byte out; reads 2 planes x 9 taps (8 B per pixel from HBM, the rest from L2).
// k_dw_select  vm[view](v, u, :) = vm2[view](v, u, :) where the mask is set (`x * 0 + y * 1` on finite
//              costs: a copy).  A thread owns one 16-byte piece of one pixel's D floats and returns after
//              its mask byte when the pixel keeps vm, so the volume traffic is 8 B per selected element
//              and none for the others; the mask costs 1 B per pixel (the D / 4 threads of a pixel read
//              the same byte: one request per wave or fewer).  D % 4 == 0: every piece is an aligned
//              dwordx4.  Else a pixel's floats start at any dword: the pieces are the aligned dwordx4s
//              inside [p D, p D + D) plus a scalar head and a scalar tail of up to three floats each.
#include <hip/hip_runtime.h>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

__device__ __forceinline__ int dw_arm_max(const uint32_t* __restrict__ p0, const uint32_t* __restrict__ p1, size_t i) {
    const uint32_t h = p0[i], v = p1[i];
    return (int)max(max(h & 0xffffu, h >> 16), max(v & 0xffffu, v >> 16));
}

__global__ __launch_bounds__(256) void k_dw_mask(const DwArgs a) {
    const int u = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y, b = blockIdx.z;
    if (u >= a.W) return;
    const size_t npix = (size_t)a.H * a.W;
    // view 0's planes of pair b (counted from the launch's first pair): [b][view][plane][npix]
    const uint32_t* p0 = a.arms + (size_t)b * 4 * npix;
    const uint32_t* p1 = p0 + npix;
    int sum = 0;
#pragma unroll
    for (int dv = -1; dv <= 1; dv++) {
        const int vv = v + dv;
        const size_t row = (size_t)((unsigned)vv < (unsigned)a.H ? vv : reflect101(vv, a.H)) * a.W;
#pragma unroll
        for (int du = -1; du <= 1; du++) {
            const int uu = u + du;
            sum += dw_arm_max(p0, p1, row + ((unsigned)uu < (unsigned)a.W ? uu : reflect101(uu, a.W)));
        }
    }
    a.mask[a.pix0 + (size_t)b * npix + (size_t)v * a.W + u] = sum < a.isum ? 1 : 0;
}

// D % 4 == 0: q = D / 4 pieces per pixel; piece i of the launch is floats [4 i, 4 i + 4) after pixel pix0
__global__ __launch_bounds__(256) void k_dw_select(const DwArgs a, size_t pieces, int q) {
    const float4* __restrict__ src = (const float4*)a.vm2 + a.pix0 * (unsigned)q;
    float4* __restrict__ dst = (float4*)a.vm + a.pix0 * (unsigned)q;
    const uint8_t* __restrict__ mask = a.mask + a.pix0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (size_t)gridDim.x * 256) {
        if (!mask[i / (unsigned)q]) continue;
        dst[i] = src[i];
    }
}

// any D: K = D / 4 + 2 pieces per pixel: piece 0 the scalar head, 1 .. D / 4 the aligned dwordx4s, K - 1 the tail.
// Element indices count from the allocations' bases (16-byte aligned), so index % 4 == 0 means aligned.
__global__ __launch_bounds__(256) void k_dw_select_tail(const DwArgs a, size_t pieces, int K) {
    const float* __restrict__ src = a.vm2;
    float* __restrict__ dst = a.vm;
    const size_t D = (size_t)a.D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (size_t)gridDim.x * 256) {
        const size_t lp = i / (unsigned)K, pix = a.pix0 + lp;
        if (!a.mask[pix]) continue;
        const int k = (int)(i - lp * (unsigned)K);
        const size_t s = pix * D, e = s + D;
        const size_t a0 = (s + 3) & ~(size_t)3;                     // first aligned float at or after s
        const size_t e4 = e & ~(size_t)3, a1 = e4 > a0 ? e4 : a0;   // end of the aligned run
        if (k == 0) {
            for (size_t j = s; j < a0 && j < e; j++) dst[j] = src[j];
        } else if (k == K - 1) {
            for (size_t j = a1; j < e; j++) dst[j] = src[j];
        } else {
            const size_t j = a0 + (size_t)(k - 1) * 4;
            if (j + 4 <= a1) *(float4*)(dst + j) = *(const float4*)(src + j);
        }
    }
}

void launch_dw_mask(const DwArgs& a, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_dw_mask, dim3((a.W + 255) / 256, a.H, n), dim3(256), 0, st, a);
}

void launch_dw_select(const DwArgs& a, int n, hipStream_t st) {
    const size_t npix = (size_t)n * a.H * a.W;
    const bool vec = a.D % 4 == 0;
    const int K = vec ? a.D / 4 : a.D / 4 + 2;
    const size_t pieces = npix * (size_t)K;
    size_t blocks = (pieces + 255) / 256;
    if (blocks > (1u << 20)) blocks = 1u << 20;
    if (blocks == 0) return;
    if (vec) hipLaunchKernelGGL(k_dw_select, dim3((unsigned)blocks), dim3(256), 0, st, a, pieces, K);
    else hipLaunchKernelGGL(k_dw_select_tail, dim3((unsigned)blocks), dim3(256), 0, st, a, pieces, K);
}

}  // namespace sm
