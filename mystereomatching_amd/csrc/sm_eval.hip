// sm_eval.hip — the per-stage error table (sm_eval_config): calErr (stereoMatching.h:1748-1825) for the three
// regions at once, at every place the reference calls saveFromDisp<short, 0> (cpp:588-601), on the maps of a group's
// pairs while a stage has just written them.  The arithmetic and its order are sm_eval_core.h's; sm_eval_stage_host
// restates both on the host.
//
// k_eval_stage  grid [blocks of a pair][pairs of the group], 256 threads x 8 consecutive pixels.  A pair starts at
//               pair * npix elements, so for odd npix neither the int16 map, the float truth nor the region bytes
//               are 16-byte aligned.  A block that lies wholly inside its pair and whose four pointers are aligned
//               (block-uniform) takes the direct path: one 16-byte load of the map, two of the truth, one 8-byte load
//               of the region bytes per thread, and with keep_maps one 16-byte store of the snapshot.  Every other
//               block -- a misaligned pair, and the tail block of any pair -- stages its pixels through LDS with
//               element-wise loads that consecutive lanes coalesce (and stores the snapshot the same way), bounds
//               checked per element; pixels past the pair enter as "in no region".  Both paths hand every thread the
//               same eight pixels, so the sums do not depend on the path.  Lane -> wave by shuffles (a fixed tree),
//               wave -> block through LDS in wave order; one 32-byte record per (pair, stage, region, block), plain
//               stores.  No atomics of any kind.
// k_eval_final  one wave per (region, stage, pair): lane l adds the partial records of blocks l, l + 64, .. in that
//               order, then the same tree; lane 0 stores the table entry.
// The decomposition into blocks depends on npix alone: the table is the same for every grouping of the pairs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_eval_core.h"
#include "sm_kernels.h"

namespace sm {

namespace {

typedef short short8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void wave_tree(sm_stage_err& a) {
#pragma unroll
    for (int off = EVAL_WAVE / 2; off >= 1; off >>= 1) {
        sm_stage_err o;
        o.count = __shfl_down(a.count, off, EVAL_WAVE);
        o.invalid = __shfl_down(a.invalid, off, EVAL_WAVE);
#pragma unroll
        for (int k = 0; k < EVAL_MAX_THRES; k++) o.bad[k] = __shfl_down(a.bad[k], off, EVAL_WAVE);
        o.sum_sq = __shfl_down(a.sum_sq, off, EVAL_WAVE);
        eval_add(a, o);   // lanes >= off add what no later step reads
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_stage(EvalArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t s_d[EVAL_BLOCK_PIX];
    __shared__ __attribute__((aligned(16))) float s_g[EVAL_BLOCK_PIX];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[EVAL_BLOCK_PIX];
    __shared__ sm_stage_err s_w[EVAL_REGIONS][EVAL_THREADS / EVAL_WAVE];
    const int t = threadIdx.x;
    const size_t b = blockIdx.x, pair = blockIdx.y;
    const size_t first = b * EVAL_BLOCK_PIX;            // < npix: the grid has eval_blocks(npix) blocks per pair
    const size_t left = a.npix - first;
    const int16_t* d = a.disp + pair * a.npix + first;
    const float* g = a.gt + pair * a.npix + first;
    const uint8_t* rg = a.reg + pair * a.npix + first;
    int16_t* sn = a.snap ? a.snap + pair * a.npix + first : nullptr;
    const bool direct = left >= (size_t)EVAL_BLOCK_PIX && (((uintptr_t)d | (uintptr_t)g | (uintptr_t)sn) & 15) == 0 &&
                        ((uintptr_t)rg & 7) == 0;
    short8 dv;
    float4 g0, g1;
    uint2 rv;
    if (direct) {
        dv = *reinterpret_cast<const short8*>(d + t * EVAL_PER_THREAD);
        g0 = *reinterpret_cast<const float4*>(g + t * EVAL_PER_THREAD);
        g1 = *reinterpret_cast<const float4*>(g + t * EVAL_PER_THREAD + 4);
        rv = *reinterpret_cast<const uint2*>(rg + t * EVAL_PER_THREAD);
        if (sn) *reinterpret_cast<short8*>(sn + t * EVAL_PER_THREAD) = dv;
    } else {
        const int cnt = left < (size_t)EVAL_BLOCK_PIX ? (int)left : EVAL_BLOCK_PIX;
        for (int i = t; i < EVAL_BLOCK_PIX; i += EVAL_THREADS) {
            const bool in = i < cnt;
            const int16_t v = in ? d[i] : (int16_t)0;
            s_d[i] = v;
            s_g[i] = in ? g[i] : 0.f;
            s_r[i] = in ? rg[i] : (uint8_t)0;
            if (in && sn) sn[i] = v;
        }
        __syncthreads();
        dv = *reinterpret_cast<const short8*>(s_d + t * EVAL_PER_THREAD);
        g0 = *reinterpret_cast<const float4*>(s_g + t * EVAL_PER_THREAD);
        g1 = *reinterpret_cast<const float4*>(s_g + t * EVAL_PER_THREAD + 4);
        rv = *reinterpret_cast<const uint2*>(s_r + t * EVAL_PER_THREAD);
    }
    const float gv[EVAL_PER_THREAD] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    EvalAcc acc;
    eval_zero(acc);
#pragma unroll
    for (int j = 0; j < EVAL_PER_THREAD; j++) {
        const uint32_t m = ((j < 4 ? rv.x : rv.y) >> (8 * (j & 3))) & 0xffu;
        eval_pixel(acc, (int)dv[j], gv[j], m, a.th);
    }
    const int lane = t & (EVAL_WAVE - 1), wave = t / EVAL_WAVE;
#pragma unroll
    for (int r = 0; r < EVAL_REGIONS; r++) {
        wave_tree(acc.r[r]);
        if (lane == 0) s_w[r][wave] = acc.r[r];
    }
    __syncthreads();
    if (t < EVAL_REGIONS) {
        sm_stage_err p = s_w[t][0];
        for (int w = 1; w < EVAL_THREADS / EVAL_WAVE; w++) eval_add(p, s_w[t][w]);
        a.part[pair * a.part_pair + ((size_t)a.stage * EVAL_REGIONS + t) * a.nblk + b] = p;
    }
}

__global__ __launch_bounds__(EVAL_WAVE) void k_eval_final(const sm_stage_err* __restrict__ part, sm_stage_err* __restrict__ table,
                                                          size_t nblk, int stages_alloc, int stage0) {
    const int r = blockIdx.x, stage = stage0 + blockIdx.y, lane = threadIdx.x;
    const size_t pair = blockIdx.z;
    const size_t slot = (pair * stages_alloc + stage) * EVAL_REGIONS + r;
    const sm_stage_err* p = part + slot * nblk;
    EvalAcc z;
    eval_zero(z);
    sm_stage_err acc = z.r[0];
    for (size_t b = lane; b < nblk; b += EVAL_WAVE) eval_add(acc, p[b]);
    wave_tree(acc);
    if (lane == 0) table[slot] = acc;
}

}  // namespace

void launch_eval_stage(const EvalArgs& a, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_stage, dim3((unsigned)a.nblk, (unsigned)n), dim3(EVAL_THREADS), 0, st, a);
}

void launch_eval_final(const sm_stage_err* part, sm_stage_err* table, size_t nblk, int stages_alloc, int stage0, int nstages,
                       int n, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_final, dim3(EVAL_REGIONS, (unsigned)nstages, (unsigned)n), dim3(EVAL_WAVE), 0, st, part, table,
                       nblk, stages_alloc, stage0);
}

}  // namespace sm
