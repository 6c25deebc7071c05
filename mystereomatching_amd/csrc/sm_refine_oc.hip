// sm_refine_oc.hip — refine()'s outlier classification (stereoMatching.cpp:1347-1510), off by default
// (sm_refine_outlier_config): the classifying LR check (LRConsistencyCheck, LOR = 0, cpp:2284-2335, the commented
// alternative at cpp:1367) and the vote with a real ratio (RV_combine_BG, cpp:7146-7216, the commented alternative
// at cpp:1408, with cal_histogram_for_HV cpp:6830-6862 and backgroundInterpolateCore cpp:6964-7043).
// A translation unit of its own; it shares sm_refine.hip's pixel mapping (sm_refine_map.h).
//
// k_lr_classify  one thread per pixel.  A failed pixel u is a mismatch when some d' in [0, min(D, u + 1)) has
//                DP1(u - d') == d'; with x = u - d' that is "some x has 0 <= DP1(x) < D and x + DP1(x) == u", so
//                a wave scatters the flags of the columns [ub - D + 1, ub + 63] into the 64 LDS slots of its row
//                segment (plain stores of 1: idempotent) and every failed pixel looks its own slot up: O(W + D)
//                reads per row segment instead of O(D) per failed pixel.
// k_rv_combine   a block compacts the holes of its 64 x 4 tile into an LDS list (as k_proper_ipol does); one wave
//                serves one hole.  The vote: the four 16-lane rows of the wave take four region rows at a time,
//                counts go into the wave's LDS histogram of D 32-bit bins (the lanes that agree with the first
//                counted lane are added as one popcount, the rest with LDS atomics), the argmax breaks ties on
//                the lowest disparity.  The background value: the wave walks the hole's row right, then left, 64
//                columns per step, up to bgIplDepth.  LDS: 1 KiB list + 16 B + 4 x D x 4 B (5.0 KiB at D = 256,
//                17 KiB at the largest D): LDS allows the 8 blocks of 256 a CU can hold, so it never limits occupancy.
// k_rv_row_last, k_rv_carry   interpolateType 2 / 3 leave a hole that is neither DISP_OCC nor DISP_MIS with the
//                result of the last classified hole before it in raster order (the reference's `dp_` outlives
//                both loops, cpp:7158).  k_rv_combine writes the classified holes' results into a scratch map
//                (OC_NONE elsewhere); one wave per row finds the last of its row, then one wave per row takes
//                the nearest earlier row's last as its carry-in and walks the row left to right, 64 columns per
//                step: a max-scan over flagged indices, two fixed launches, nothing read back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"
#include "sm_refine_map.h"

namespace sm {

namespace {

constexpr int OC_NONE = -32768;   // the scratch map / row table: no classified hole here

__global__ __launch_bounds__(256) void k_lr_classify(int16_t* __restrict__ d0, const int16_t* __restrict__ d1,
                                                     uint8_t* __restrict__ mask, int H, int W, int D, float maxdiff,
                                                     int disp_occ, int disp_mis) {
    __shared__ int flag[TX * TY];   // a wave's 64 slots: the columns of its row segment
    const Pix p = pixel_of(H, W);
    const int lane = threadIdx.x & (TX - 1), wbase = threadIdx.x - lane;
    const int ub = p.u - lane;      // first column of the tile
    const bool rowok = p.v < H;     // wave-uniform
    const size_t row = rowok ? ((size_t)p.b * H + p.v) * W : 0;
    flag[threadIdx.x] = 0;
    __syncthreads();
    for (int x0 = max(ub - (D - 1), 0); x0 < ub + TX; x0 += TX) {   // block-uniform
        const int x = x0 + lane;
        if (rowok && x < W) {
            const int e = d1[row + x];
            const int t = x + e - ub;
            if (e >= 0 && e < D && t >= 0 && t < TX) flag[wbase + t] = 1;
        }
    }
    __syncthreads();
    if (!p.ok) return;
    const int d = d0[row + p.u];
    const bool bad = d < 0 || p.u - d < 0 || (float)abs(d - (int)d1[row + p.u - d]) > maxdiff;
    mask[row + p.u] = bad ? 255 : 0;
    if (bad) d0[row + p.u] = (int16_t)(flag[threadIdx.x] ? disp_mis : disp_occ);
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// cal_histogram_for_HV for the hole (v, u) by one wave (all 64 lanes enter; v, u wave-uniform).  hist: D bins.
__device__ __forceinline__ int vote_hv(const RvcArgs& a, const int16_t* dp, const uint32_t* lr, const uint32_t* ud,
                                       int v, int u, int* hist, int lane) {
    const int W = a.W, D = a.D;
    for (int d = lane; d < D; d += 64) hist[d] = 0;
    // the clear before any lane's add: one wave's LDS operations complete in order; the fence and the wave barrier
    // keep the compiler from moving an access across and state the intent
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint32_t av = ud[(size_t)v * W + u];
    const int v0 = max(v - (int)(av & 0xffff), 0), v1 = min(v + (int)(av >> 16), a.H - 1);
    const int sub = lane >> 4, l16 = lane & 15;
    int cnt = 0;
    for (int vb = v0; vb <= v1; vb += 4) {
        const int vn = vb + sub;
        const bool rowok = vn <= v1;
        const uint32_t h = rowok ? lr[(size_t)vn * W + u] : 0u;
        const int u0 = max(u - (int)(h & 0xffff), 0), u1 = min(u + (int)(h >> 16), W - 1);
        const int len = rowok ? u1 - u0 + 1 : 0;
        const int maxlen = max(max(__shfl(len, 0, 64), __shfl(len, 16, 64)), max(__shfl(len, 32, 64), __shfl(len, 48, 64)));
        const int16_t* row = dp + (size_t)(rowok ? vn : v) * W;
        for (int i0 = 0; i0 < maxlen; i0 += 16) {   // wave-uniform
            const int un = u0 + i0 + l16;
            const int q = (rowok && un <= u1) ? (int)row[un] : -1;
            cnt += q >= 0 ? 1 : 0;
            const bool inb = q >= 0 && q < D;   // a value >= D counts in validNum and in no bin
            const unsigned long long m = __ballot(inb);
            if (m) {
                const int lead = __ffsll((long long)m) - 1;
                const int qv = __shfl(q, lead, 64);
                const unsigned long long same = __ballot(inb && q == qv);
                if (lane == lead) atomicAdd(&hist[qv], (int)__popcll(same));
                else if (inb && q != qv) atomicAdd(&hist[q], 1);
            }
        }
    }
    const int valid = wave_sum(cnt);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's own adds before its reads
    __builtin_amdgcn_wave_barrier();
    int bc = -1, bd = 0;
    for (int d = lane; d < D; d += 64) {
        const int c = hist[d];
        if (c > bc) {
            bc = c;
            bd = d;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int oc = __shfl_xor(bc, m, 64), od = __shfl_xor(bd, m, 64);
        if (oc > bc || (oc == bc && od < bd)) {
            bc = oc;
            bd = od;
        }
    }
    if (valid <= a.rv_s) return -1;
    const float ratio = (float)bc / (float)valid;   // float division, strict compare (cpp:6860-6861)
    return ratio > a.rv_ratio ? bd : -1;
}

// backgroundInterpolateCore for the hole (v, u) by one wave: the nearest value >= 0 in (u, u + depth] and in
// [u - depth, u), the smaller of those found or -1
__device__ __forceinline__ int fill_bg(const RvcArgs& a, const int16_t* row, int u, int lane) {
    const int W = a.W, depth = a.depth;
    int rgt = -1, lft = -1;
    for (int c0 = u + 1; c0 < W && c0 - u <= depth; c0 += 64) {   // wave-uniform
        const int x = c0 + lane;
        const int q = (x < W && x - u <= depth) ? (int)row[x] : -1;
        const unsigned long long m = __ballot(q >= 0);
        if (m) {
            rgt = __shfl(q, __ffsll((long long)m) - 1, 64);
            break;
        }
    }
    for (int c0 = u - 1; c0 >= 0 && u - c0 <= depth; c0 -= 64) {
        const int x = c0 - lane;
        const int q = (x >= 0 && u - x <= depth) ? (int)row[x] : -1;
        const unsigned long long m = __ballot(q >= 0);
        if (m) {
            lft = __shfl(q, __ffsll((long long)m) - 1, 64);
            break;
        }
    }
    if (rgt < 0) return lft;
    if (lft < 0) return rgt;
    return min(rgt, lft);
}

__global__ __launch_bounds__(256) void k_rv_combine(RvcArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* holes = reinterpret_cast<uint32_t*>(smem);               // TX * TY entries
    int* nholes = reinterpret_cast<int*>(smem + TX * TY * 4);          // 16 bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* hist = reinterpret_cast<int*>(smem + TX * TY * 4 + 16) + (size_t)wave * a.D;
    const int H = a.H, W = a.W;
    const Pix p = pixel_of(H, W);
    const size_t npix = (size_t)H * W;
    const int16_t* dp = a.src + (size_t)p.b * npix;
    int16_t* out = a.dst + (size_t)p.b * npix;
    int16_t* cand = a.cand ? a.cand + (size_t)p.b * npix : nullptr;
    if (threadIdx.x == 0) *nholes = 0;
    __syncthreads();
    if (p.ok) {
        const size_t o = (size_t)p.v * W + p.u;
        const int cur = dp[o];
        if (cur >= 0) {
            out[o] = (int16_t)cur;
            if (cand) cand[o] = (int16_t)OC_NONE;
        } else {
            holes[atomicAdd(nholes, 1)] = (uint32_t)threadIdx.x;
        }
    }
    __syncthreads();
    const int n = *nholes;
    const uint32_t* lr = a.arms + (size_t)p.b * 4 * npix;   // [b][view 0][plane 0] = L | R << 16
    const uint32_t* ud = lr + npix;                          // plane 1 = U | D << 16
    const int u_org = p.u - (int)(threadIdx.x & (TX - 1)), v_org = p.v - (int)(threadIdx.x / TX);
    for (int base = 0; base < n; base += 4) {
        const int hi = __builtin_amdgcn_readfirstlane(base + wave);
        if (hi >= n) continue;   // wave-uniform; the waves share nothing from here on
        const int t = __builtin_amdgcn_readfirstlane((int)holes[hi]);
        const int u = u_org + (t & (TX - 1)), v = v_org + t / TX;
        const size_t o = (size_t)v * W + u;
        const int cur = __builtin_amdgcn_readfirstlane((int)dp[o]);
        const bool occ = cur == a.disp_occ, mis = cur == a.disp_mis;
        const int type = a.type;
        const bool assigned = type < 2 || occ || mis;
        const bool need_rv = type == 0 || (type >= 2 && mis) || (type == 3 && occ);
        const bool need_bg = type == 1 || (type >= 2 && occ);
        int rv = -1, bg = -1;
        if (need_rv) rv = vote_hv(a, dp, lr, ud, v, u, hist, lane);
        if (need_bg) bg = fill_bg(a, dp + (size_t)v * W, u, lane);
        // type 3 on an occlusion: the smaller of the two when both exist, else the one that does (cpp:7193-7200)
        const int res = (need_rv && need_bg) ? ((rv >= 0 && bg >= 0) ? min(rv, bg) : max(rv, bg)) : (need_rv ? rv : bg);
        if (lane == 0) {
            out[o] = (int16_t)((assigned && res >= 0) ? res : cur);
            if (cand) cand[o] = (int16_t)(assigned ? res : OC_NONE);
        }
    }
}

// rows of n pairs, one wave each; false past the last row
__device__ __forceinline__ bool oc_row(int n, int H, long& row) {
    row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    return row < (long)n * H;
}

__global__ __launch_bounds__(256) void k_rv_row_last(RvcArgs a) {
    long r;
    if (!oc_row(a.n, a.H, r)) return;   // wave-uniform
    const int lane = threadIdx.x & 63, W = a.W;
    const int16_t* cand = a.cand + (size_t)r * W;
    int last = OC_NONE;
    for (int c0 = (W - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
        const int x = c0 + lane;
        const int cv = x < W ? (int)cand[x] : OC_NONE;
        const unsigned long long m = __ballot(cv != OC_NONE);
        if (m) {
            last = __shfl(cv, 63 - __clzll((long long)m), 64);
            break;
        }
    }
    if (lane == 0) a.rowlast[r] = (int16_t)last;
}

__global__ __launch_bounds__(256) void k_rv_carry(RvcArgs a) {
    long r;
    if (!oc_row(a.n, a.H, r)) return;
    const int lane = threadIdx.x & 63, W = a.W, H = a.H;
    const int b = (int)(r / H), v = (int)(r - (long)b * H);
    const int16_t* rl = a.rowlast + (size_t)b * H;   // the carry never leaves the pair
    int carry = -1;                                   // dp_'s initial value (cpp:7158)
    for (int c0 = v - 1; c0 >= 0; c0 -= 64) {
        const int i = c0 - lane;
        const int val = i >= 0 ? (int)rl[i] : OC_NONE;
        const unsigned long long m = __ballot(val != OC_NONE);
        if (m) {
            carry = __shfl(val, __ffsll((long long)m) - 1, 64);
            break;
        }
    }
    const int16_t* src = a.src + (size_t)r * W;
    const int16_t* cand = a.cand + (size_t)r * W;
    int16_t* dst = a.dst + (size_t)r * W;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int x = c0 + lane;
        const bool in = x < W;
        const int cv = in ? (int)cand[x] : OC_NONE;
        const int s = in ? (int)src[x] : 0;
        const unsigned long long m = __ballot(cv != OC_NONE);
        const unsigned long long below = lane == 63 ? m : m & ((1ull << (lane + 1)) - 1);
        const int j = below ? 63 - __clzll((long long)below) : 0;
        const int vj = __shfl(cv, j, 64);   // every lane takes part
        const int val = below ? vj : carry;
        if (in && s < 0 && s != a.disp_occ && s != a.disp_mis && val >= 0) dst[x] = (int16_t)val;
        if (m) carry = __shfl(cv, 63 - __clzll((long long)m), 64);
    }
}

}  // namespace

void launch_lr_classify(int16_t* d0, const int16_t* d1, uint8_t* mask, int n, int H, int W, int D, float maxdiff,
                        int disp_occ, int disp_mis, hipStream_t st) {
    hipLaunchKernelGGL(k_lr_classify, grid_of(n, H, W), dim3(256), 0, st, d0, d1, mask, H, W, D, maxdiff, disp_occ, disp_mis);
}

void launch_rv_combine(const RvcArgs& a, hipStream_t st) {
    const size_t lds = (size_t)TX * TY * 4 + 16 + (size_t)4 * a.D * sizeof(int);
    hipLaunchKernelGGL(k_rv_combine, grid_of(a.n, a.H, a.W), dim3(256), lds, st, a);
}

void launch_rv_carry(const RvcArgs& a, hipStream_t st) {
    const long rows = (long)a.n * a.H;
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(k_rv_row_last, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_rv_carry, grid, dim3(256), 0, st, a);
}

}  // namespace sm
