// sm_cost_ext.hip — the cost measures beyond k_cost's four: "SD", "BT", "grad",
// "TruncAD", "adGrad" and "ADCensusGrad" of costCalculate (cpp:954-987).  A translation unit of its
// own; the per-element cost terms it shares with k_cost are sm_cost_elem.h's.
//
// k_cost_ext<M> has k_cost's block shape: one row segment of np focus pixels x D.  The moving
// pixels [u0 - (D - 1), u0 + np) (view 1: [u0, u0 + np + D - 1)) are staged in LDS once per block,
// as planes that hold only what measure M reads; each wave then takes one focus pixel at a time
// (its values are wave-uniform; two pixels per trip for D <= 64), its lanes run over d, and the D floats of a pixel go out as
// coalesced non-temporal buffer stores.  Positions outside the image are staged as zeros and the
// reference's out-of-range value is selected afterwards.
//   SD / AD   gen_ad_sd_vm (cpp:2468-2509)       TruncAD  gen_truncAD_vm (cpp:2511-2548)
//   BT        calNeiMaxMin (cpp:197-227), calCostForBT (cpp:142-195), gray images
//   grad      calgradvm (cpp:388-455)            adGrad   gen_vm_from2vm_fixWgt (cpp:3767-3796)
//   ADCensusGrad  gen_vm_from3vm_exp (cpp:3592-3652, the live line cpp:3640)
// Every float op is written in the reference's order and the file is compiled with
// -ffp-contract=off: ADCensusGrad's two fp64 products and their sum stay three roundings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_cost_elem.h"
#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

namespace {

__constant__ uint64_t c_ext_exp_tab[32] = SM_EXPF_TABLE;

// pixels of a row segment per block: k_cost's values (SM_COST_P_ONE / SM_COST_P_MULTI)
constexpr int EXT_P_ONE = 240, EXT_P_MULTI = 192;
__host__ __device__ constexpr int ext_p(bool one) { return one ? EXT_P_ONE : EXT_P_MULTI; }
constexpr int EXT_STORE_AUX = 2;   // slc = non-temporal, as k_cost's stores (SM_COST_STORE_AUX)

template <int M>
struct ExtNeeds {
    static constexpr bool BGR = M == SM_M_SD || M == SM_M_TRUNC_AD || M == SM_M_AD_GRAD || M == SM_M_AD_CENSUS_GRAD;
    static constexpr bool BT = M == SM_M_BT;
    static constexpr bool GRAD = M == SM_M_GRAD || M == SM_M_AD_GRAD || M == SM_M_AD_CENSUS_GRAD;
    static constexpr bool CEN = M == SM_M_AD_CENSUS_GRAD;
    // bytes per moving pixel and per focus pixel
    static constexpr int MOV = (BGR ? 4 : 0) + (BT ? 12 : 0) + (GRAD ? 8 : 0) + (CEN ? 16 : 0);
    static constexpr int FOC = (BGR ? 4 : 0) + (BT ? 12 : 0) + (GRAD ? 16 : 0) + (CEN ? 16 : 0);
};

// sum over B, G, R of |x_c - y_c| (POW = 1) or its square (POW = 2) for packed pixels
template <int POW>
__device__ __forceinline__ int bgr_dist(uint32_t x, uint32_t y) {
    const int d0 = abs((int)(x & 0xff) - (int)(y & 0xff));
    const int d1 = abs((int)((x >> 8) & 0xff) - (int)((y >> 8) & 0xff));
    const int d2 = abs((int)(x >> 16) - (int)(y >> 16));
    return POW == 1 ? d0 + d1 + d2 : d0 * d0 + d1 * d1 + d2 * d2;
}

// calgradvm's element (cpp:430-440): a min(|dx|, T) + (1 - a) min(|dy|, T)
__device__ __forceinline__ float grad_elem(float fx, float fy, float mx, float my, float wa, float wb, float T) {
    const float dx = fminf(fabsf(fx - mx), T);
    const float dy = fminf(fabsf(fy - my), T);
    const float t1 = wa * dx;
    const float t2 = wb * dy;
    return t1 + t2;
}

// AD with truncation T of the packed pixels x, y: min(fl(sum / 3), T), or T itself out of range.  The
// division runs on the zero record of an out-of-range candidate too and is discarded: the element
// loop stays branch-free (the barrier keeps the compiler from branching around the division).
__device__ __forceinline__ float ad_elem(uint32_t x, uint32_t y, bool oor, float T) {
    float ad = fminf((float)bgr_dist<1>(x, y) / 3.0f, T);
    asm volatile("" : "+v"(ad));
    return oor ? T : ad;
}

// expf_glibc for x <= 0 without a branch: the core is valid down to glibc's underflow bound, below
// which the result is 0 (sm_device.h); the bound itself is the core's smallest valid input
__device__ __forceinline__ float expf_neg(float x, const uint64_t* etab) {
    const float lo = -0x1.9fe368p6f;
    const float e = expf_glibc_core(fmaxf(x, lo), LdsExpTab{etab});
    return x < lo ? 0.0f : e;
}

template <int M, bool ONE>
__global__ __launch_bounds__(256) void k_cost_ext(const CostArgs a) {
    typedef ExtNeeds<M> N;
    extern __shared__ __align__(16) unsigned char xs_raw[];
    __shared__ uint64_t etab[32];                   // the 2^(i/32) table of the device expf
    constexpr int P = ext_p(ONE);
    const int D = a.D, W = a.W, H = a.H;
    const int nbx = (W + a.seg - 1) / a.seg;
    const int blk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int bx = blk % nbx, rest = blk / nbx;
    const int v = rest % H, b = rest / H;
    const int u0 = bx * a.seg;
    const int np = min(a.seg, W - u0);              // <= P
    const int nm = np + D - 1;                      // moving pixels needed
    const int nmc = P + D - 1;                      // the planes' capacity
    const int sgn = a.view == 0 ? 1 : -1;           // moving position = u - sgn * d
    const int mbase = a.view == 0 ? u0 - (D - 1) : u0;
    const size_t npix = (size_t)H * W;
    const int fview = a.view, mview = 1 - a.view;
    const size_t fimg = ((size_t)b * 2 + fview) * npix, mimg = ((size_t)b * 2 + mview) * npix;
    const size_t frow = fimg + (size_t)v * W, mrow = mimg + (size_t)v * W;
    // LDS planes: the 16-byte census records first, then 4-byte planes
    unsigned char* sp = xs_raw;
    auto carve = [&](bool on, int bytes) {
        unsigned char* r = sp;
        if (on) sp += bytes;
        return r;
    };
    uint4* mcode = (uint4*)carve(N::CEN, 16 * nmc);
    uint4* fcode = (uint4*)carve(N::CEN, 16 * P);
    uint32_t* mpx = (uint32_t*)carve(N::BGR, 4 * nmc);
    uint32_t* fpx = (uint32_t*)carve(N::BGR, 4 * P);
    float* mgray = (float*)carve(N::BT, 4 * nmc);   // BT: the gray value and its neighbour range
    float* mlo = (float*)carve(N::BT, 4 * nmc);
    float* mhi = (float*)carve(N::BT, 4 * nmc);
    float* fgray = (float*)carve(N::BT, 4 * P);
    float* flo = (float*)carve(N::BT, 4 * P);
    float* fhi = (float*)carve(N::BT, 4 * P);
    float* mgx = (float*)carve(N::GRAD, 4 * nmc);
    float* mgy = (float*)carve(N::GRAD, 4 * nmc);
    float* fgx = (float*)carve(N::GRAD, 4 * P);
    float* fgy = (float*)carve(N::GRAD, 4 * P);
    float* fwa = (float*)carve(N::GRAD, 4 * P);     // adaptive weight a (1 if off)
    float* fwb = (float*)carve(N::GRAD, 4 * P);     // 1 - a (1 if off)
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if (N::CEN && tid < 32) etab[tid] = c_ext_exp_tab[tid];

    // one pixel's staged values; (lo, hi): min / max of I(q), (I(q - 1) + I(q)) / 2 and
    // (I(q + 1) + I(q)) / 2, the image's edge columns without the missing neighbour (exact halves)
    auto stage = [&](size_t img, size_t row, int q, uint4* code, uint32_t* px, float* gray, float* lo, float* hi, float* gx,
                     float* gy, int i) {
        const bool in = q >= 0 && q < W;
        if (N::CEN) {
            uint4 c = make_uint4(0, 0, 0, 0);
            if (in) {
                const ulonglong2 w = a.code[row + q];
                c = make_uint4((uint32_t)w.x, (uint32_t)(w.x >> 32), (uint32_t)w.y, (uint32_t)(w.y >> 32));
            }
            code[i] = c;
        }
        if (N::BGR) {
            uint32_t x = 0;
            if (in) {
                const uint8_t* p = a.bgr + (row + q) * 3;
                x = p[0] | (p[1] << 8) | (p[2] << 16);
            }
            px[i] = x;
        }
        if (N::BT) {
            float g = 0.f, l = 0.f, h = 0.f;
            if (in) {
                const uint8_t* r = a.gray + row;
                g = (float)r[q];
                const float il = q > 0 ? 0.5f * ((float)r[q - 1] + g) : g;
                const float ir = q < W - 1 ? 0.5f * ((float)r[q + 1] + g) : g;
                l = fminf(g, fminf(il, ir));
                h = fmaxf(g, fmaxf(il, ir));
            }
            gray[i] = g;
            lo[i] = l;
            hi[i] = h;
        }
        if (N::GRAD) {
            float2 gr = make_float2(0.f, 0.f);
            if (in) gr = grad_finish(grad_fetch(a.gray + img, v, q, H, W), v, q, H, W);
            gx[i] = gr.x;
            gy[i] = gr.y;
        }
    };
    for (int i = tid; i < np; i += 256) {
        const int u = u0 + i;
        stage(fimg, frow, u, fcode, fpx, fgray, flo, fhi, fgx, fgy, i);
        if (N::GRAD) {
            float wa = 1.f, wb = 1.f;
            if (a.grad_adaptive) {
                const uint32_t* planes = (const uint32_t*)a.arms + ((size_t)b * 2 + fview) * 2 * npix + (size_t)v * W + u;
                const float2 wg = cost_grad_weights(planes[0], planes[npix]);
                wa = wg.x;
                wb = wg.y;
            }
            fwa[i] = wa;
            fwb[i] = wb;
        }
    }
    for (int i = tid; i < nm; i += 256) stage(mimg, mrow, mbase + i, mcode, mpx, mgray, mlo, mhi, mgx, mgy, i);
    __syncthreads();

    const int lane = threadIdx.x;
    if (ONE && lane >= D) return;                   // D <= 64: one disparity per lane; no barrier follows
    const float* out = a.vm + ((size_t)b * npix + (size_t)v * W + u0) * D;
    const __amdgpu_buffer_rsrc_t ro = buf_rsrc(out, np * D * 4);
    const int wy = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const float adT = a.ad_trunc, gT = a.grad_trunc, gO = a.grad_oor, cd = a.census_default;
    auto pixel = [&](int pl) {
        const int u = u0 + pl;
        // the focus pixel's values (wave-uniform)
        uint4 cf = make_uint4(0, 0, 0, 0);
        uint32_t fc = 0;
        float fg = 0.f, fl = 0.f, fh = 0.f, fx = 0.f, fy = 0.f, wa = 0.f, wb = 0.f;
        if (N::CEN) cf = fcode[pl];
        if (N::BGR) fc = fpx[pl];
        if (N::BT) {
            fg = fgray[pl];
            fl = flo[pl];
            fh = fhi[pl];
        }
        if (N::GRAD) {
            fx = fgx[pl];
            fy = fgy[pl];
            wa = fwa[pl];
            wb = fwb[pl];
        }
        auto elem = [&](int d, int q) {             // disparity d, moving position q = u - sgn * d
            const int mi = q - mbase;               // in [0, nm): view 0 pl + D - 1 - d, view 1 pl + d
            const bool oor = (unsigned)q >= (unsigned)W;
            float res;
            if constexpr (M == SM_M_SD) {
                // the squares' partial sums are exact integers <= 195075 in the reference's float too
                float sd = fminf((float)bgr_dist<2>(fc, mpx[mi]) / 3.0f, adT);
                asm volatile("" : "+v"(sd));              // keep the element loop branch-free
                res = oor ? adT : sd;
            } else if constexpr (M == SM_M_TRUNC_AD) {
                res = oor ? 60.0f : (float)min(bgr_dist<1>(fc, mpx[mi]), 60);
            } else if constexpr (M == SM_M_BT) {
                const float mg = mgray[mi];
                const float v0 = fmaxf(0.0f, fmaxf(mlo[mi] - fg, fg - mhi[mi]));   // focus value against the moving range
                const float v1 = fmaxf(0.0f, fmaxf(fl - mg, mg - fh));             // moving value against the focus range
                res = oor ? 20.0f : fminf(fminf(v0, v1), 20.0f);
            } else if constexpr (M == SM_M_GRAD) {
                const float g = grad_elem(fx, fy, mgx[mi], mgy[mi], wa, wb, gT);
                res = oor ? gO : g;
            } else if constexpr (M == SM_M_AD_GRAD) {
                const float ad = ad_elem(fc, mpx[mi], oor, adT);
                const float g0 = grad_elem(fx, fy, mgx[mi], mgy[mi], wa, wb, gT);
                const float g = oor ? gO : g0;
                const float w0 = (float)0.11, w1 = (float)(1 - 0.11);
                const float t0 = ad * w0;
                const float t1 = g * w1;
                res = t0 + t1;
            } else {   // SM_M_AD_CENSUS_GRAD
                const float ad = ad_elem(fc, mpx[mi], oor, adT);
                const uint4 cm = mcode[mi];
                const int pc = __popc(cf.x ^ cm.x) + __popc(cf.y ^ cm.y) + __popc(cf.z ^ cm.z) + __popc(cf.w ^ cm.w);
                const float cen = oor ? cd : fminf((float)pc, cd);
                const float g0 = grad_elem(fx, fy, mgx[mi], mgy[mi], wa, wb, gT);
                const float g = oor ? gO : g0;
                const double h0 = 0.5 * (double)ad;
                const double h1 = 0.5 * (double)cen;
                const float m = (float)(h0 + h1);
                const float e0 = 1.0f - expf_neg(-m, etab);
                const float e1 = 1.0f - expf_neg(-g / 2.0f, etab);
                const double p0 = 0.7 * (double)e0;
                const double p1 = 0.3 * (double)e1;
                res = (float)(p0 + p1);
            }
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, res), ro, d * 4, pl * D * 4, EXT_STORE_AUX);
        };
        int q = u - sgn * lane;
        if constexpr (ONE) {
            elem(lane, q);                          // lane < D <= 64
        } else {
            for (int d = lane; d < D; d += 64, q -= sgn * 64) elem(d, q);
        }
    };
    int pl = wy;
    if constexpr (ONE) {
        // D <= 64: one element per lane and pixel leaves the LDS latency exposed, so pixels pl and
        // pl + 4 go per trip (two independent elements per lane), as in k_cost
        for (; pl + 4 < np; pl += 8) {
            pixel(pl);
            pixel(pl + 4);
        }
    }
    for (; pl < np; pl += 4) pixel(pl);
}

template <int M>
size_t ext_smem_bytes(int D) {
    const int P = ext_p(D <= 64);
    return (size_t)ExtNeeds<M>::MOV * (P + D - 1) + (size_t)ExtNeeds<M>::FOC * P;   // (+ the static table)
}

template <int M>
void launch_ext_m(const CostArgs& a, dim3 grid, hipStream_t st) {
    const size_t shm = ext_smem_bytes<M>(a.D);
    if (a.D <= 64)
        hipLaunchKernelGGL((k_cost_ext<M, true>), grid, dim3(64, 4), shm, st, a);
    else
        hipLaunchKernelGGL((k_cost_ext<M, false>), grid, dim3(64, 4), shm, st, a);
}

}  // namespace

void launch_cost_ext(const CostArgs& a0, int method, int n, hipStream_t st) {
    // equal segments of at most ext_p pixels, as launch_cost
    CostArgs a = a0;
    const int P = ext_p(a.D <= 64);
    const int nb = (a.W + P - 1) / P;
    a.seg = (a.W + nb - 1) / nb;
    const dim3 grid((unsigned)(nb * a.H * n));
    switch (method) {
        case SM_M_SD: launch_ext_m<SM_M_SD>(a, grid, st); break;
        case SM_M_BT: launch_ext_m<SM_M_BT>(a, grid, st); break;
        case SM_M_GRAD: launch_ext_m<SM_M_GRAD>(a, grid, st); break;
        case SM_M_TRUNC_AD: launch_ext_m<SM_M_TRUNC_AD>(a, grid, st); break;
        case SM_M_AD_GRAD: launch_ext_m<SM_M_AD_GRAD>(a, grid, st); break;
        default: launch_ext_m<SM_M_AD_CENSUS_GRAD>(a, grid, st); break;
    }
}

}  // namespace sm
