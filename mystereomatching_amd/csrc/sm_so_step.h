// sm_so_step.h — what the scan-line optimiser kernels share (k_so in sm_so.hip: so and so_R2L; k_so_t2d in
// sm_so_t2d.hip: so_T2D): one step of the dynamic programme for a lane's K consecutive disparities, the two trace
// stores and the trace read of the backtrack.  The kernels differ in the scan (rows or columns, its direction and
// strides), in the minimum they hand in (bit patterns for costs >= +0, floats for so_T2D's signed costs, or
// so_first_min below: the reference's own loop, for costs of either sign and NaN) and in the addend (cost_min, or
// so_T2D's cost_min - c_min).
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"

namespace sm {

// LDS trace of one line (a row, or a column for so_T2D) of `steps` steps, per wave, in u64 words: two ballot masks
// per step and lane slot j (bit l of mask 2j / 2j + 1 = bit 0 / 1 of the code of disparity l K + j), then the
// steps' minimum indices as u16
__host__ __device__ inline size_t so_lds_words(int steps, int K) {
    return (size_t)steps * 2 * K + ((size_t)steps * 2 + 7) / 8;
}

__device__ __forceinline__ float so_shr1_f(float v) {   // lane l <- lane l - 1 (lane 0 <- FLT_MAX)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0x7f7fffff, __builtin_bit_cast(int, v),
                                                                 DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ float so_shl1_f(float v) {   // lane l <- lane l + 1 (lane 63 <- FLT_MAX)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0x7f7fffff, __builtin_bit_cast(int, v),
                                                                 DPP_WAVE_SHL1, 0xF, 0xF, false));
}

// The reference's first minimum of a line's D costs, as its C++ takes it (cpp:6354-6363, 6396-6406):
//   m = c[0], i = 0;  for d = 1 .. D-1: if (c[d] < m) { m = c[d]; i = d; }
// for costs of either sign, +-0 and NaN: -0 == +0 (the first of equal values wins whatever its sign bit), a NaN at
// index 0 is sticky (every later compare is false: the result is (NaN, 0)), a NaN at any other index never wins.
// Lane l holds p = c[d0 .. d0 + K); disparities >= D (padding) never win, whatever the real costs are.  Returns i and
// sets wm = m (wave-uniform: c[i] itself, read from the lane that holds it).
// In the lane, the loop's own compares, skipping NaN (a NaN running value is replaced by whatever follows, so it
// stays NaN only while every value was).  Across lanes, an unsigned minimum of one order-preserving key per lane:
// floats map to keys monotonically (-0 first folded onto +0, so the two zeros share a key and the lower lane wins
// the tie), NaN and padding to the largest key, the sticky NaN of lane 0 to key 0, below -inf's.  The integer
// minimum always equals some lane's key, so the ballot is never empty; v_min_f32, which drops NaN and may return
// either zero, is not used.  (If every key is the largest, c[0] is NaN and held key 0: impossible.)
template <int K>
__device__ __forceinline__ int so_first_min(const float (&p)[K], int d0, int D, float& wm) {
    float lm = p[0];
    int li = d0;
#pragma unroll
    for (int j = 1; j < K; j++) {
        const bool take = d0 + j < D && (p[j] < lm || lm != lm);
        lm = take ? p[j] : lm;
        li = take ? d0 + j : li;
    }
    const bool sticky = d0 == 0 && p[0] != p[0];
    if (sticky) {
        lm = p[0];
        li = 0;
    }
    uint32_t b = __builtin_bit_cast(uint32_t, lm);
    b = (b << 1) == 0 ? 0u : b;                                           // -0 -> +0
    uint32_t key = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);      // negative: all bits flipped; else the sign bit set
    if (lm != lm || d0 >= D) key = 0xffffffffu;
    if (sticky) key = 0u;
    const uint32_t km = wave_umin(key);
    const int src = (int)__builtin_ctzll(__ballot(key == km));
    wm = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lm), src));
    return __builtin_amdgcn_readlane(li, src);
}

// L_isDisc of two packed BGR pixels: float sum = 0; sum += abs(IP[c] - IP_pre[c]); sum /= 3; sum > 15 (cpp:6285-6296)
__device__ __forceinline__ bool so_is_disc(uint32_t x, uint32_t y) {
    float sum = 0.f;
    sum += abs((int)(x & 0xff) - (int)(y & 0xff));
    sum += abs((int)((x >> 8) & 0xff) - (int)((y >> 8) & 0xff));
    sum += abs((int)((x >> 16) & 0xff) - (int)((y >> 16) & 0xff));
    sum /= 3;
    return sum > 15;
}

// One step for the lane's disparities d0 .. d0 + K - 1 (cpp:6305-6334): prev the predecessor's accumulated costs
// (lanes past D hold FLT_MAX), cur this pixel's costs, wmin the wave-uniform minimum of prev.  Candidates in the
// reference's order, each taken only when strictly smaller: prev[d], prev[d-1] + Pn2 (d > 0), prev[d+1] + Pn2
// (d < D-1), c_min = wmin + Pn3.  nv = cur + cost_min, or with NORM cur + (cost_min - c_min) (so_T2D, cpp:6644: one
// rounded difference, then one rounded sum).  The choice codes (0: d, 1: d - 1, 2: d + 1, 3: the minimum's index) go
// to the step's LDS masks tl [2K] (LT) or to its byte codes tb [D] in global memory.
template <int K, bool NORM, bool LT>
__device__ __forceinline__ void so_step(const float (&prev)[K], const float (&cur)[K], float (&nv)[K], float wmin, float Pn2,
                                        float Pn3, int d0, int D, int lane, uint64_t* tl, uint8_t* tb) {
    const float c_min = wmin + Pn3;
    const float left = so_shr1_f(prev[K - 1]);    // prev[d0 - 1]
    const float right = so_shl1_f(prev[0]);       // prev[d0 + K]
    uint32_t codes = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int d = d0 + j;
        const float pm = j > 0 ? prev[j - 1] : left;
        const float pp = j < K - 1 ? prev[j + 1] : right;
        const float c_minus = d > 0 ? pm + Pn2 : FLT_MAX;
        const float c_plus = d < D - 1 ? pp + Pn2 : FLT_MAX;
        float cost_min = prev[j];
        uint32_t code = 0;
        if (c_minus < cost_min) {
            cost_min = c_minus;
            code = 1;
        }
        if (c_plus < cost_min) {
            cost_min = c_plus;
            code = 2;
        }
        if (c_min < cost_min) {
            cost_min = c_min;
            code = 3;
        }
        if (NORM) {
            const float add = cost_min - c_min;   // <= 0
            nv[j] = cur[j] + add;
        } else {
            nv[j] = cur[j] + cost_min;
        }
        if (LT) {
            const uint64_t b0 = __ballot(code & 1u), b1 = __ballot(code & 2u);
            if (lane == 0) {
                tl[2 * j] = b0;
                tl[2 * j + 1] = b1;
            }
            continue;
        }
        codes |= code << (8 * (j & 3));
        if ((j & 3) == 3 || j == K - 1) {   // flush the codes of disparities base .. j
            const int base = j & ~3;
            uint8_t* tp = tb + d0 + base;
            if (j - base == 3 && (D & 3) == 0 && d0 + base + 3 < D) {
                *(uint32_t*)tp = codes;      // 4-byte aligned: a step's codes start at a multiple of D, D % 4 == 0 and (d0 + base) % 4 == 0
            } else {
#pragma unroll
                for (int q = 0; q <= (j & 3); q++)
                    if (d0 + base + q < D) tp[q] = (uint8_t)(codes >> (8 * q));
            }
            codes = 0;
        }
    }
}

// The backtrack's step: the disparity that the trace of one step (tl / tb as in so_step, ci its minimum index)
// holds for dmin.  LT: uniform LDS reads of the two masks of dmin's slot.
template <int K, bool LT>
__device__ __forceinline__ int so_trace_next(int dmin, const uint64_t* tl, const uint8_t* tb, int ci) {
    int code;
    if (LT) {
        const int l = dmin / K, j = dmin - l * K;
        const uint64_t m0 = tl[2 * j], m1 = tl[2 * j + 1];
        code = (int)((m0 >> l) & 1u) | (int)(((m1 >> l) & 1u) << 1);
    } else {
        code = tb[dmin];
    }
    return code == 0 ? dmin : (code == 1 ? dmin - 1 : (code == 2 ? dmin + 1 : ci));
}

}  // namespace sm
