// sm_cost_elem.h — the censusGrad cost element and its staged inputs, shared by the cost-volume
// kernel (k_cost, sm_kernels.hip) and the first CBCA H scan that computes the costs itself
// (k_cbca_hsc, sm_cbca.hip): both compile the code below, so their volumes agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"

namespace sm {

// Select-free gradient elements (NOSEL = censusGrad with >= 3 census words and OORZ): an
// out-of-range candidate's staged record carries gx = gy = COST_OOR_GRAD and a census count bias
// of icd, so the element's own arithmetic yields the reference's out-of-range value without a
// select: min(|f - S|, T) per axis (T = grad_trunc, 500) makes G >= 0.999 min(T, S - 255) (the
// host enables the path only when that, over lamG, lies below -17.5, so e1 rounds away exactly as
// it does for the reference's 707.1068), and popc + icd >= icd
// picks LUT entry icd (the LUT holds 2 - expf(-C / lamCen) and is clamped at icd, so no min
// is needed either).  The exponential's input is clamped at -100 instead of selecting 0 below
// -17.5: expf_glibc_core is exact down to -103.9, and every value below 2^-25 leaves
// fl(t - e) == t.  Saves the range test, three selects and a min per element.
constexpr int LUT_T_N = 260;   // >= 128 census bits + icd (<= 128) + 1
// The out-of-range sentinel gradient (NOSEL): |f - S| for a real gradient f in [-255, 255] lies in
// [S - 255, S + 255] = [295, 805]; with the truncation min(., T) the element's G is then >= 0.999
// min(T, 295) (the host's NOSEL test, cost_nosel_ok in sm_kernels.hip), and unclamped (FAST below) G <= 677.5.
constexpr float COST_OOR_GRAD = 550.0f;
// FAST elements (NOSEL, lamG == 1, adaptive weights, T >= 382.5, focus pixel off the image border): the gradient
// images are 0.5 (I[+1] - I[-1]) inside the image and full differences on its border rows and
// columns (calGrad, cpp:271-350), so an interior focus pixel has |gx|, |gy| <= 127.5 and a
// candidate in the same row |gx| <= 255, |gy| <= 127.5: |dx| <= 382.5 <= T and |dy| <= 255, the
// truncation is the identity, and wa |dx| == |fl(wa dx)| (wa, wb > 0; round-to-nearest is
// symmetric), so G = |fl(wa dx)| + |fl(wb dy)| takes one packed subtract, one packed multiply and
// one add with both operands' abs modifiers.  With wa + wb = 1 (up to 2^-24), G <= 382.5 for real
// candidates and <= 677.5 for the sentinel (unit weights could reach 1355), so -G >= -700 keeps expf_glibc_core's exponent field from wrapping without the -100
// clamp (below -103.9 the core returns a double < 2^-149 that rounds to 0 or the least
// subnormal, which fl(t - e) absorbs like the reference's exact value).  The census count
// starts from the record's bias word and accumulates through three v_bcnt_u32_b32 (one chain).

// The LDS copy of the 2^(i/32) table sits in static LDS (a link-time address), so
// its byte offset (ki % 32) * 8 is one SDWA shift with a byte-0 destination select
// ((ki << 3) & 0xff) and the table's address goes into the ds_read's offset field.
struct LdsExpTab {
    const uint64_t* p;
};
__device__ __forceinline__ uint64_t exp_tab_at(const LdsExpTab& t, uint64_t ki) {
    uint32_t off;
    asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD"
        : "=v"(off) : "v"((uint32_t)ki));
    return *(const uint64_t*)((const char*)t.p + off);
}
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// One select-free element.  Focus pixel: census words c0 .. c3 (CW of them in use), gradient
// (fx, fy), weights (wa, wb).  Candidate: staged census words r0 (CW == 3: r0.w is not a census
// word), gradient words gw, count bias pc (icd for out-of-range candidates, else 0).  luta: the
// clamped 2 - e0 table (LUT_T_N entries), etab: the LDS copy of the 2^(i/32) table.
template <int CW, bool LAM1, bool FAST>
__device__ __forceinline__ float cost_elem_nosel(const uint4 r0, const uint2 gw, uint32_t pc, uint32_t c0, uint32_t c1,
                                                 uint32_t c2, uint32_t c3, float fx, float fy, float wa, float wb,
                                                 float grad_trunc, float lam2, const float* luta, const uint64_t* etab) {
    static_assert(CW == 3 || CW == 4, "select-free elements need >= 3 census words");
    typedef float f2 __attribute__((ext_vector_type(2)));
    pc = bcnt_acc(c0 ^ r0.x, pc);
    pc = bcnt_acc(c1 ^ r0.y, pc);
    pc = bcnt_acc(c2 ^ r0.z, pc);
    if (CW == 4) pc = bcnt_acc(c3 ^ r0.w, pc);
    const f2 dv = f2{fx, fy} - f2{__uint_as_float(gw.x), __uint_as_float(gw.y)};
    float g;
    if constexpr (FAST) {
        const f2 tv = f2{wa, wb} * dv;
        g = fabsf(tv.x) + fabsf(tv.y);
    } else {
        const f2 tv = f2{wa, wb} * f2{fminf(fabsf(dv.x), grad_trunc), fminf(fabsf(dv.y), grad_trunc)};
        g = tv.x + tv.y;
    }
    // (-fminf(g, 100) == fmaxf(-g, -100): both paths end in a negated conversion)
    const float xg = LAM1 ? (FAST ? -g : -fminf(g, 100.0f)) : fmaxf(-g / lam2, -100.0f);
    const float t = luta[pc];                       // fl(2 - expf(-min(pc, icd) / lamCen))
    const float ex = expf_glibc_core(xg, LdsExpTab{etab});
    return t - ex;
}

// x / y gradients of gray image G at (v, u) (calGrad, cpp:271-350): central differences inside,
// one-sided ones on the border rows and columns.  The four bytes are fetched first (grad_fetch;
// (v, u) inside the image) so that a caller can issue the loads ahead of their use.
struct GradRaw {
    uint32_t xp, xm, yp, ym;   // row[min(u + 1, W - 1)], row[max(u - 1, 0)], and the same along v (one register each)
};
__device__ __forceinline__ GradRaw grad_fetch(const uint8_t* G, int v, int u, int H, int W) {
    const uint8_t* row = G + (size_t)v * W;
    GradRaw r;
    r.xp = row[min(u + 1, W - 1)];
    r.xm = row[max(u - 1, 0)];
    r.yp = G[(size_t)min(v + 1, H - 1) * W + u];
    r.ym = G[(size_t)max(v - 1, 0) * W + u];
    return r;
}
// (a border difference is exact as it stands, half an interior one too: the products below are
// the reference's values, and a one-pixel axis gives 0)
__device__ __forceinline__ float2 grad_finish(const GradRaw r, int v, int u, int H, int W) {
    // (bytes convert exactly and their difference is exact: (float)a - (float)b == (float)(a - b))
    const float gxv = ((u == 0 || u == W - 1) ? 1.0f : 0.5f) * ((float)r.xp - (float)r.xm);
    const float gyv = ((v == 0 || v == H - 1) ? 1.0f : 0.5f) * ((float)r.yp - (float)r.ym);
    return make_float2(gxv, gyv);
}

// adaptive gradient weights of a focus pixel from its arm-pair words (calgradvm, cpp:388-455)
__device__ __forceinline__ float2 cost_grad_weights(uint32_t ph, uint32_t pv) {
    float sH = (float)min(ph & 0xffffu, ph >> 16);
    float sV = (float)min(pv & 0xffffu, pv >> 16);
    if (sH == 0) sH = 1;
    if (sV == 0) sV = 1;
    const float wa = sH / (sH + sV);
    return make_float2(wa, 1.0f - wa);
}

}  // namespace sm
