// sm_fif.hip — aggregation "FIF": the full-image guided filter's four weighted sweeps.
//
// Reference: FIF_Improve (stereoMatching.cpp:4707-4890, what costCalculate calls for "FIF") and
// the plain form FIF (cpp:4541-4705).  Per view, with the guide If = u8 * (float)(1 / 255.0)
// (OpenCV's 8u -> 32f convertTo: PARITY UNPINNED), eps = 0.08f, Pn = 2, BIG = FLT_MAX:
//   s = (float)((double)dB^2 + (double)dG^2 + (double)dR^2)   (std::pow(float, int) is double)
//   wh(v, u) = expf(-s / (eps * eps)) between (v, u) and (v, u + 1); wv between (v, u) and (v + 1, u)
//   step(prev, add, w)[d] = add[d] + min(min(d > 0 ? prev[d-1] + Pn : BIG,
//                                            d < D-1 ? prev[d+1] + Pn : BIG), prev[d]) * w
//   (plain form: add[d] + prev[d] * w)
//   c1[u] = step(c1[u-1], vm[u], wh[u-1]),  c1[0] = vm[0]      (per row, left to right)
//   c2[u] = step(c2[u+1], vm[u], wh[u]),    c2[W-1] = vm[W-1]  (right to left)
//   A = (c1 + c2) - vm
//   T[v] = step(T[v-1], A[v], wv[v-1]),     T[0] = A[0]        (per column, downwards)
//   Bt[v] = step(Bt[v+1], A[v], wv[v]),     Bt[H-1] = A[H-1]   (upwards)
//   vm = (T + Bt) - A
// Every operation is rounded on its own (-ffp-contract=off), as in the reference's scalar loops.
//
// gfx950 mapping.  The recurrence is the SGM path recurrence without the path minimum, and the
// sweeps are laid out like k_sgm / k_sgm_rows (sm_sgm.hip): a wave walks a scan line with the
// previous pixel of each step in its own registers, lane l of the line holding disparities
// [l K, l K + K); the d +/- 1 neighbours cross lanes with one DPP shift each way (FLT_MAX at the
// line's ends), no LDS.  D <= 64: four lines per wave, one DPP row of 16 lanes per line, so a
// step of a wave still moves up to 4 x 256 B per volume; larger D: one line per wave.  Lanes past
// D load a clamped address, carry BIG and never store.  The next T steps of every input volume
// and of the line's weights are prefetched into registers, two tiles in flight; D % 4 == 0 with
// K % 4 == 0 moves each lane's disparities as dwordx4.
// Four launches per view: H forward (vm -> c1), H backward (vm, c1 -> A), V forward (A -> T),
// V backward (A, T -> vm, times SolveAll's weight when fused): 8 + 12 + 8 + 12 = 40 B per element
// and two scratch volumes (c1 and T share one).
// A translation unit of its own; only the wave-per-line layout is sm_sgm.hip's.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

__constant__ uint64_t c_exp_tab_fif[32] = SM_EXPF_TABLE;

// wh / wv planes of n pairs' guide images; the last column of wh and the last row of wv are
// never read (written as 0)
__global__ __launch_bounds__(256) void k_fif_weights(const FifArgs a) {
    __shared__ float tab[256];   // convertTo(CV_32F, 1 / 255.0): (float)u8 * (float)(1 / 255.0)
    tab[threadIdx.x] = (float)threadIdx.x * (float)(1 / 255.0);
    __syncthreads();
    const size_t npix = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int b = blockIdx.y;
    const int v = (int)(i / a.W), u = (int)(i - (size_t)v * a.W);
    const uint8_t* img = a.bgr + (size_t)b * a.bgr_pair_stride;
    const uint8_t* p = img + i * 3;
    const float ee = a.eps * a.eps;
    auto wgt = [&](const uint8_t* q) {   // q: the next pixel (u + 1 or v + 1)
        const float d0 = tab[q[0]] - tab[p[0]];
        const float d1 = tab[q[1]] - tab[p[1]];
        const float d2 = tab[q[2]] - tab[p[2]];
        const double sd = (double)d0 * (double)d0 + (double)d1 * (double)d1 + (double)d2 * (double)d2;
        const float s = (float)sd;
        return expf_glibc(-s / ee, c_exp_tab_fif);
    };
    a.wh[(size_t)b * npix + i] = u + 1 < a.W ? wgt(p + 3) : 0.f;
    a.wv[(size_t)b * npix + i] = v + 1 < a.H ? wgt(p + (size_t)a.W * 3) : 0.f;
}

enum : int { FIF_ROW_SHL1 = 0x101, FIF_ROW_SHR1 = 0x111 };

// lane l <- lane l - 1 (SHR) / l + 1 (SHL) of its line; FLT_MAX at the line's ends
template <int LPW, bool RIGHT>
__device__ __forceinline__ float fif_shift(float v) {
    constexpr int CTRL = LPW == 1 ? (RIGHT ? DPP_WAVE_SHR1 : DPP_WAVE_SHL1) : (RIGHT ? FIF_ROW_SHR1 : FIF_ROW_SHL1);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, FLT_MAX), __builtin_bit_cast(int, v),
                                                                 CTRL, 0xF, 0xF, false));
}

template <int K, int T, bool SECOND>
struct FifTile {
    float a[T][K];                    // the sweep's `add` volume (vm / A)
    float f[SECOND ? T : 1][K];       // backward sweeps: the forward sweep's result (c1 / T)
    float w[T];                       // the line's weight of each step
};

// One sweep.  LPW lines per wave (1 or 4), K disparities per lane, VEC: dwordx4 accesses
// (D % 4 == 0, K % 4 == 0), PLAIN: the form without the d +/- 1 minimum, SECOND: the backward
// sweep, which also combines (fw + L) - add into its output.
template <int K, int LPW, bool VEC, bool PLAIN, bool SECOND, int T>
__global__ __launch_bounds__(256) void k_fif_sweep(const FifArgs a) {
    constexpr int KV = VEC ? K / 4 : 1;
    const int wave = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    const int H = a.H, W = a.W, D = a.D;
    const int b = blockIdx.y;
    const bool vert = a.vert != 0;
    const int nl = vert ? W : H, steps = vert ? H : W;
    const int line0 = wave * LPW;
    if (line0 >= nl) return;   // wave-uniform
    const int sub = LPW == 1 ? 0 : lane >> 4, li = LPW == 1 ? lane : lane & 15;
    const bool line_ok = line0 + sub < nl;
    const int line = line_ok ? line0 + sub : nl - 1;   // lines past the last one repeat it and never store
    const size_t npix = (size_t)H * W;
    // step j of the line is pixel p0 + j * pstep: forward sweeps start at the first pixel of the
    // line, backward sweeps at its last
    const long pstep = (vert ? (long)W : 1L) * (SECOND ? -1 : 1);
    const size_t p0 = vert ? (size_t)(SECOND ? H - 1 : 0) * W + line : (size_t)line * W + (SECOND ? W - 1 : 0);
    const long vstep = pstep * D;
    const float* ibase = a.in + ((size_t)b * npix + p0) * D;
    const float* fbase = SECOND ? a.fw + ((size_t)b * npix + p0) * D : nullptr;
    float* obase = a.out + ((size_t)b * npix + p0) * D;
    const float* wbase = (vert ? a.wv : a.wh) + (size_t)b * npix + p0;
    const int d0 = li * K;
    int ld[K];        // load column, clamped to a valid one
    bool val[K];      // element inside D
    bool has_up[K];   // d + 1 inside D
    int ldc[KV];
    bool cval[KV];
#pragma unroll
    for (int k = 0; k < K; k++) {
        val[k] = d0 + k < D;
        has_up[k] = d0 + k < D - 1;
        ld[k] = val[k] ? d0 + k : D - 1;
    }
#pragma unroll
    for (int c = 0; c < KV; c++) {
        cval[c] = d0 + 4 * c < D;                  // VEC: D % 4 == 0, a chunk is inside D or past it
        ldc[c] = cval[c] ? d0 + 4 * c : D - 4;
    }
    const float pn = a.pn;

    auto clampj = [&](int j) { return j < 0 ? 0 : (j < steps ? j : steps - 1); };
    auto load = [&](FifTile<K, T, SECOND>& t, int j0) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const long off = (long)clampj(j0 + s) * vstep;
            if (VEC) {
#pragma unroll
                for (int c = 0; c < KV; c++) {
                    const float4 v = ld_stream4(ibase + off + ldc[c]);
                    t.a[s][4 * c + 0] = v.x;
                    t.a[s][4 * c + 1] = v.y;
                    t.a[s][4 * c + 2] = v.z;
                    t.a[s][4 * c + 3] = v.w;
                    if (SECOND) {
                        const float4 q = ld_stream4(fbase + off + ldc[c]);
                        t.f[s][4 * c + 0] = q.x;
                        t.f[s][4 * c + 1] = q.y;
                        t.f[s][4 * c + 2] = q.z;
                        t.f[s][4 * c + 3] = q.w;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    t.a[s][k] = ld_stream(ibase + off + ld[k]);
                    if (SECOND) t.f[s][k] = ld_stream(fbase + off + ld[k]);
                }
            }
            // the weight between step j and step j - 1 sits at the lower pixel of the two: the
            // previous one of a forward sweep, this one of a backward sweep (step 0 uses none)
            t.w[s] = wbase[(long)clampj(SECOND ? j0 + s : j0 + s - 1) * pstep];
        }
    };

    float Lp[K];
#pragma unroll
    for (int k = 0; k < K; k++) Lp[k] = FLT_MAX;

    auto step = [&](const FifTile<K, T, SECOND>& t, int s, int j) {
        float L[K];
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < K; k++) L[k] = t.a[s][k];
        } else {
            const float w = t.w[s];
            if (PLAIN) {
#pragma unroll
                for (int k = 0; k < K; k++) L[k] = t.a[s][k] + Lp[k] * w;
            } else {
                float P[K];
#pragma unroll
                for (int k = 0; k < K; k++) P[k] = Lp[k] + pn;
                const float left = fif_shift<LPW, true>(P[K - 1]);
                const float right = fif_shift<LPW, false>(P[0]);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const float lo = (k == 0) ? (li > 0 ? left : FLT_MAX) : P[k - 1];
                    const float up = has_up[k] ? ((k == K - 1) ? right : P[k + 1]) : FLT_MAX;
                    const float m = fminf(fminf(lo, up), Lp[k]);
                    L[k] = t.a[s][k] + m * w;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) L[k] = val[k] ? L[k] : FLT_MAX;   // lanes past D take part as BIG
        float o[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (SECOND) {
                o[k] = solve_all_store((t.f[s][k] + L[k]) - t.a[s][k], a.solve_all, a.scale);
            } else {
                o[k] = L[k];
            }
        }
        float* dst = obase + (long)j * vstep;
        if (VEC) {
#pragma unroll
            for (int c = 0; c < KV; c++)
                if (line_ok && cval[c])
                    st_stream4(dst + d0 + 4 * c, make_float4(o[4 * c + 0], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]));
        } else {
#pragma unroll
            for (int k = 0; k < K; k++)
                if (line_ok && val[k]) st_stream(dst + d0 + k, o[k]);
        }
#pragma unroll
        for (int k = 0; k < K; k++) Lp[k] = L[k];
    };

    auto process = [&](const FifTile<K, T, SECOND>& t, int j0) {
#pragma unroll
        for (int s = 0; s < T; s++)
            if (j0 + s < steps) step(t, s, j0 + s);   // wave-uniform
    };

    FifTile<K, T, SECOND> ta, tb;
    load(ta, 0);
    for (int j0 = 0; j0 < steps; j0 += 2 * T) {
        load(tb, j0 + T);
        process(ta, j0);
        load(ta, j0 + 2 * T);
        process(tb, j0 + T);
    }
}

template <int K, int LPW, bool VEC, bool PLAIN>
static void launch_fif_kp(const FifArgs& a, int n, hipStream_t st) {
    constexpr int T = K <= 2 ? 16 : 32 / K;
    const int nl = a.vert ? a.W : a.H;
    const int waves = (nl + LPW - 1) / LPW;
    dim3 grid((waves + 3) / 4, n);
    if (a.second)
        hipLaunchKernelGGL((k_fif_sweep<K, LPW, VEC, PLAIN, true, T>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_fif_sweep<K, LPW, VEC, PLAIN, false, T>), grid, dim3(256), 0, st, a);
}

template <int K, int LPW, bool VEC>
static void launch_fif_k(const FifArgs& a, int n, hipStream_t st) {
    if (a.plain)
        launch_fif_kp<K, LPW, VEC, true>(a, n, st);
    else
        launch_fif_kp<K, LPW, VEC, false>(a, n, st);
}

template <int K, int LPW>
static void launch_fif_v(const FifArgs& a, int n, hipStream_t st) {
    if (K % 4 == 0 && a.D % 4 == 0)
        launch_fif_k<K, LPW, (K % 4 == 0)>(a, n, st);
    else
        launch_fif_k<K, LPW, false>(a, n, st);
}

void launch_fif_weights(const FifArgs& a, int n, hipStream_t st) {
    const size_t npix = (size_t)a.H * a.W;
    dim3 grid((unsigned)((npix + 255) / 256), n);
    hipLaunchKernelGGL(k_fif_weights, grid, dim3(256), 0, st, a);
}

// D <= 64: four lines per wave (a DPP row of 16 lanes each), else one; K = disparities per lane
void launch_fif_sweep(const FifArgs& a, int n, hipStream_t st) {
    const int D = a.D;
    // (horizontal sweeps at D = 64 with one row per wave and one disparity per lane instead:
    // 0.281 vs 0.286-0.296 ms forward, 0.384-0.404 vs 0.393-0.418 ms backward at Teddy x16, inside
    // the run-to-run spread, so there is one layout per D)
    if (D <= 16) launch_fif_v<1, 4>(a, n, st);
    else if (D <= 32) launch_fif_v<2, 4>(a, n, st);
    else if (D <= 64) launch_fif_v<4, 4>(a, n, st);
    else if (D <= 128) launch_fif_v<2, 1>(a, n, st);
    else if (D <= 256) launch_fif_v<4, 1>(a, n, st);
    else if (D <= 512) launch_fif_v<8, 1>(a, n, st);
    else launch_fif_v<16, 1>(a, n, st);
}

}  // namespace sm
