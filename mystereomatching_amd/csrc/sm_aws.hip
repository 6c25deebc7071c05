// sm_aws.hip — aggregation "AWS": adaptive support weights (Yoon and Kweon) over a
// (2 rv + 1) x (2 ru + 1) window, 35 x 35 in the reference.
//
// Reference: AWS(), the branch without JBF_STANDARD (stereoMatching.cpp:5711-5792), with
// genWeight_AWS / calW4_AWS / calvm_AWS (stereoMatching.h:1305-1350, 1472-1493, 1533-1548).
//   Lab[i] = BGR2Lab(I_c[i]) on u8 (OpenCV's fixed-point path, aws_lab_px: PARITY UNPINNED),
//            bordered with REFLECT_101 (the conversion is per pixel, so the border commutes)
//   wt[i](p)[tap] = expf(-dif / gamma_c),  dif = (float)sqrt((double)s),
//            s = (float)((double)(dL dL) * 0.153787 + (double)(da da) + (double)(db db))
//   vm[LOR](v, u)[d], with u1 = u + d LOR and u2 = u - d (1 - LOR); u1 >= W or u2 < 0: unchanged;
//   else, over the taps in raster order (dv outer, du inner), every operation rounded to f32:
//            ele = wt[0](v, u1)[tap] * wt[1](v, u2)[tap];  denom += ele;
//            numer += ele * vm_raw(refl(v + dv), refl(u + du))[d];      vm = numer / denom
//
// gfx950 mapping.
//   k_aws_lab      both images' Lab planes, once per call;
//   k_aws_weights  the weights of a band of image rows, both images, [image][row][tap][u] (u minor),
//                  into a band buffer of fixed size (a whole image's weights would be H W S 4 B:
//                  0.83 GB per Teddy view); both views of the band's rows read the same band;
//   k_aws_agg      one block = one image row, 32 adjacent u, 64 adjacent d: four waves of 8 u each,
//                  lanes along d.  Per dv the block stages in LDS the raw strip (32 + 2 ru) x 64, the
//                  per-lane weights (the other image's, at u -/+ d: 95 pixels x nu taps) and the
//                  lane-uniform weights (this view's image at u: 32 x nu); all of a thread's staging
//                  loads (up to 40 buffer loads) are issued before the first is used.  A lane slides
//                  its 8 u along du with the strip values in a rotating register window (one LDS
//                  read per 8 taps); each tap reads the two weights from LDS (one conflict-free, one
//                  broadcast) and does mul, add, mul, add, separately rounded (-ffp-contract=off),
//                  which the compiler packs two u at a time (v_pk_mul_f32 / v_pk_add_f32).
//                  76 VGPRs, 35.2 KB LDS, no scratch: four blocks (16 waves) per CU.
// A translation unit of its own (it shares no code with the guided filter).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

__constant__ uint64_t c_exp_tab_aws[32] = SM_EXPF_TABLE;

constexpr int AWS_TUW = 8;                      // adjacent u per lane
constexpr int AWS_TUB = 4 * AWS_TUW;            // u per block (four waves)
constexpr int AWS_NU = 2 * AWS_MAX_R + 1;       // taps per window row at the largest radius
constexpr int AWS_COLS = AWS_TUB + 2 * AWS_MAX_R;   // strip columns
constexpr int AWS_NP = AWS_TUB + 63;            // pixels of the per-lane weights a block reads
constexpr int AWS_WO_LD = 96, AWS_WU_LD = 36;   // LDS row strides

__global__ __launch_bounds__(256) void k_aws_lab(const AwsArgs a, size_t npx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const uint8_t* p = a.bgr + i * 3;
    aws_lab_px(a.tab, p[0], p[1], p[2], a.lab + i * 3);
}

// grid: (ceil(S W / 256), band rows, 2 images)
__global__ __launch_bounds__(256) void k_aws_weights(const AwsArgs a) {
    const int H = a.H, W = a.W, nu = 2 * a.ru + 1, S = (2 * a.rv + 1) * nu;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;   // S W <= 1225 * 65535 fits
    if (t >= (uint32_t)S * W) return;
    const int tap = (int)(t / (uint32_t)W), u = (int)(t - (uint32_t)tap * W);
    const int dv = tap / nu - a.rv, du = tap % nu - a.ru;
    const int r = a.r0 + blockIdx.y, b = r / H, v = r - b * H, img = blockIdx.z;
    const uint8_t* lab = a.lab + (size_t)(b * 2 + img) * H * W * 3;
    const uint8_t* p = lab + ((size_t)v * W + u) * 3;
    const uint8_t* q = lab + ((size_t)reflect101(v + dv, H) * W + reflect101(u + du, W)) * 3;
    const float d0 = (float)p[0] - (float)q[0];
    const float d1 = (float)p[1] - (float)q[1];
    const float d2 = (float)p[2] - (float)q[2];
    const float s = (float)((double)(d0 * d0) * 0.153787 + (double)(d1 * d1) + (double)(d2 * d2));
    // (float)sqrt((double)s): over every reachable s the correctly rounded f32 root is the same float
    const float dif = __builtin_sqrtf(s);
    const float w = expf_glibc((-dif) / a.gamma_c, c_exp_tab_aws);
    a.wt[((size_t)img * a.band_rows + blockIdx.y) * S * W + t] = w;
}

// One window column of the 8 u a lane holds: the lane-uniform weights (an LDS broadcast) and the
// per-lane weights from LDS, the strip values from the rotating register window.  K = du % 8.
template <int K>
__device__ __forceinline__ void aws_du(const float* wuw, const float* wow, const float* vsw, int du,
                                       float (&rg)[AWS_TUW], float (&num)[AWS_TUW], float (&den)[AWS_TUW]) {
    rg[(K + AWS_TUW - 1) % AWS_TUW] = vsw[(du + AWS_TUW - 1) * 64];
#pragma unroll
    for (int j = 0; j < AWS_TUW; j++) {
        const float ele = wuw[j * AWS_WU_LD + du] * wow[du * AWS_WO_LD + j];
        den[j] = den[j] + ele;
        num[j] = num[j] + ele * rg[(K + j) % AWS_TUW];
    }
}

// grid: (ceil(W / 32) * ceil(D / 64), band rows)
__global__ __launch_bounds__(256) void k_aws_agg(const AwsArgs a) {
    __shared__ float vs[AWS_COLS * 64];          // raw strip: [column][d]
    __shared__ float wo[AWS_NU * AWS_WO_LD];     // per-lane weights: [du][pixel - pbase]
    __shared__ float wu[AWS_TUB * AWS_WU_LD];    // lane-uniform weights: [u - u0][du]
    __shared__ uint32_t cofs[AWS_COLS];          // byte offset of each strip column in a volume row
    const int H = a.H, W = a.W, D = a.D, rv = a.rv, ru = a.ru, lor = a.lor;
    const int nv = 2 * rv + 1, nu = 2 * ru + 1;
    const int nchunk = (D + 63) >> 6;
    const int tile = blockIdx.x / nchunk, chunk = blockIdx.x - tile * nchunk;
    const int u0 = tile * AWS_TUB, d0 = chunk * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = tid >> 6;
    const int r = a.r0 + blockIdx.y, b = r / H, v = r - b * H;
    const int d = d0 + lane;
    const float* __restrict__ raw = a.raw + (size_t)b * H * W * D;
    float* __restrict__ out = a.out + (size_t)b * H * W * D;
    const size_t S = (size_t)nv * nu;
    // the view's own image gives the lane-uniform weight (at u), the other image the per-lane one
    // (view 0: the right image at u - d; view 1: the left image at u + d)
    const float* __restrict__ wt_u = a.wt + ((size_t)lor * a.band_rows + blockIdx.y) * S * W;
    const float* __restrict__ wt_o = a.wt + ((size_t)(1 - lor) * a.band_rows + blockIdx.y) * S * W;
    const int pbase = lor ? u0 + d0 : u0 - d0 - 63;
    const int ibase = (lor ? lane : 63 - lane) + wv * AWS_TUW;
    const int ncols = AWS_TUB + 2 * ru;

    // does any element of the block aggregate?  (block-uniform)
    const int umax = min(u0 + AWS_TUB, W) - 1;
    const bool any = lor ? u0 + d0 < W : umax - d0 >= 0;

    float num[AWS_TUW], den[AWS_TUW];
#pragma unroll
    for (int j = 0; j < AWS_TUW; j++) num[j] = den[j] = 0.f;

    if (any) {
        // staging roles: a thread stages d = d0 + lane of every fourth strip column, and pixel
        // pbase + (tid & 127) of every second du
        const bool d_ok = d < D;
        const int sp = pbase + (tid & 127);
        const bool sp_ok = (tid & 127) < AWS_NP && sp >= 0 && sp < W;
        constexpr int NSV = (AWS_COLS + 3) / 4, NSW = (AWS_NU + 1) / 2;
        // buffer loads with per-lane byte offsets; an offset >= 2^31 makes a lane's load return 0.
        // The strip's reflected columns do not depend on dv: their byte offsets sit in LDS.
        for (int c = tid; c < ncols; c += 256) cofs[c] = (uint32_t)(reflect101(u0 - ru + c, W) * D) * 4u;
        __syncthreads();
        const uint32_t vo_d = d_ok ? (uint32_t)d * 4u : 0x80000000u;
        const uint32_t vo_p = sp_ok ? (uint32_t)sp * 4u : 0x80000000u;
        const int tw0 = tid >> 7, tc0 = tid >> 6;
        // the lane-uniform weights: pixel u0 + (tid & 31) of every eighth du
        constexpr int NSU = (AWS_NU + 7) / 8;
        const int su = u0 + (tid & 31);
        float tv[NSV], tw[NSW], tu[NSU];
        auto fetch = [&](int dvi) {
            // The offsets and predicates below do not depend on dv; computed from a value the
            // compiler cannot see through, they are redone per dv (a dozen VALU operations)
            // instead of living in 40 VGPRs and 80 SGPRs across the tap loops.
            int z = 0;
            asm volatile("" : "+v"(z));
            const auto rr = buf_rsrc(raw + (size_t)reflect101(v + dvi - rv, H) * W * D, W * D * 4);
#pragma unroll
            for (int i = 0; i < NSV; i++) {
                const int c = tc0 + 4 * i + z;
                tv[i] = buf_ld(rr, c < ncols ? vo_d + cofs[min(c, ncols - 1)] : 0x80000000u, 0);
            }
            const auto rw = buf_rsrc(wt_o + (size_t)dvi * nu * W, nu * W * 4);
#pragma unroll
            for (int i = 0; i < NSW; i++) {
                const int t = tw0 + 2 * i + z;
                tw[i] = buf_ld(rw, t < nu ? vo_p + (uint32_t)(t * W) * 4u : 0x80000000u, 0);
            }
            const auto ru_ = buf_rsrc(wt_u + (size_t)dvi * nu * W, nu * W * 4);
#pragma unroll
            for (int i = 0; i < NSU; i++) {
                const int t = (tid >> 5) + 8 * i + z;
                tu[i] = buf_ld(ru_, t < nu && su < W ? (uint32_t)(t * W + su) * 4u : 0x80000000u, 0);
            }
        };
        const float* wuw = wu + wv * AWS_TUW * AWS_WU_LD;
        const float* vsw = vs + wv * AWS_TUW * 64 + lane;
        const float* wow = wo + ibase;
        for (int dvi = 0; dvi < nv; dvi++) {
            fetch(dvi);        // all of the row's loads are in flight before the first is used
            __syncthreads();   // the previous dv's reads are done
#pragma unroll
            for (int i = 0; i < NSV; i++)
                if (wv + 4 * i < AWS_COLS) vs[(wv + 4 * i) * 64 + lane] = tv[i];
            if ((tid & 127) < AWS_WO_LD) {
#pragma unroll
                for (int i = 0; i < NSW; i++)
                    if ((tid >> 7) + 2 * i < AWS_NU) wo[((tid >> 7) + 2 * i) * AWS_WO_LD + (tid & 127)] = tw[i];
            }
#pragma unroll
            for (int i = 0; i < NSU; i++)
                if ((tid >> 5) + 8 * i < AWS_WU_LD) wu[(tid & 31) * AWS_WU_LD + (tid >> 5) + 8 * i] = tu[i];
            __syncthreads();
            float rg[AWS_TUW];   // strip column c of the wave's window lives in rg[c % 8]
#pragma unroll
            for (int j = 0; j < AWS_TUW - 1; j++) rg[j] = vsw[j * 64];
            for (int du0 = 0; du0 < nu; du0 += AWS_TUW) {
                if (du0 + 0 < nu) aws_du<0>(wuw, wow, vsw, du0 + 0, rg, num, den);   // (wave-uniform tests)
                if (du0 + 1 < nu) aws_du<1>(wuw, wow, vsw, du0 + 1, rg, num, den);
                if (du0 + 2 < nu) aws_du<2>(wuw, wow, vsw, du0 + 2, rg, num, den);
                if (du0 + 3 < nu) aws_du<3>(wuw, wow, vsw, du0 + 3, rg, num, den);
                if (du0 + 4 < nu) aws_du<4>(wuw, wow, vsw, du0 + 4, rg, num, den);
                if (du0 + 5 < nu) aws_du<5>(wuw, wow, vsw, du0 + 5, rg, num, den);
                if (du0 + 6 < nu) aws_du<6>(wuw, wow, vsw, du0 + 6, rg, num, den);
                if (du0 + 7 < nu) aws_du<7>(wuw, wow, vsw, du0 + 7, rg, num, den);
            }
        }
    }
    if (d >= D) return;
#pragma unroll
    for (int j = 0; j < AWS_TUW; j++) {
        const int u = u0 + wv * AWS_TUW + j;
        if (u >= W) break;
        const bool ok = lor ? u + d < W : u - d >= 0;
        const size_t e = ((size_t)v * W + u) * D + d;
        if (!ok && !a.solve_all) continue;   // `out` holds the raw cost already
        out[e] = solve_all_store(ok ? num[j] / den[j] : raw[e], a.solve_all, a.scale);
    }
}

void launch_aws_lab(const AwsArgs& a, int n, hipStream_t st) {
    const size_t npx = (size_t)n * 2 * a.H * a.W;
    hipLaunchKernelGGL(k_aws_lab, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, a, npx);
}

void launch_aws_weights(const AwsArgs& a, hipStream_t st) {
    const size_t SW = (size_t)(2 * a.rv + 1) * (2 * a.ru + 1) * a.W;
    hipLaunchKernelGGL(k_aws_weights, dim3((unsigned)((SW + 255) / 256), a.nr, 2), dim3(256), 0, st, a);
}

void launch_aws_agg(const AwsArgs& a, hipStream_t st) {
    const unsigned tiles = (a.W + AWS_TUB - 1) / AWS_TUB, chunks = (a.D + 63) / 64;
    hipLaunchKernelGGL(k_aws_agg, dim3(tiles * chunks, a.nr), dim3(256), 0, st, a);
}

}  // namespace sm
