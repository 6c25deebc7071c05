// sm_vmtop.hip — dispOptimize's Do_vmTop branch (stereoMatching.cpp:1108-1128): instead of the plain WTA every
// pixel keeps the vmTop_Num cheapest disparities within a factor vmTop_thres of its minimum
// (selectTopCostFromVolumn, h:2405-2461) and chooses among them from its neighbours' candidates
// (genDispFromTopCostVm2, cpp:1514-1885).  A translation unit of its own, beside "so" (sm_so.hip) and WTA.
//
// k_vmtop_select   the hot path: one read of the volume.  A group of 16 lanes (one DPP row) holds one pixel's
//                  D costs in registers, lane l the disparities 64 c + 4 l .. + 3 of every 64-chunk c (one
//                  16-byte load per chunk when D % 4 == 0), so a wave carries four pixels.  Round k takes the
//                  (cost, d) lexicographic minimum -- the reference's strict `>` scan: the lowest d wins a tie
//                  -- with four DPP steps inside the row, masks the winner to FLT_MAX and keeps it while
//                  cost < firstV * thres (round 0 always).  Positions past D hold FLT_MAX at d >= D, which
//                  loses every tie against a masked disparity, as the reference's rescan of a masked volume.
//                  Lane k keeps candidate k; the table is [pixel][M] (d, cost) pairs plus a count per pixel.
// k_vmtop_decide0_a  method 0, one thread per pixel: row 0, column 0 and single-candidate pixels (case 1) and
//                  the pixels whose cost-keyed container is not empty (case 3), which read only the tables of
//                  the pixel and its 8 neighbours.  Pixels with an empty container (case 2) read four map
//                  values that are outputs: they are marked pending (-1) and counted per t = u + 2 v.
// k_vmtop_decide0_w  a relaxation round over all pixels: pending pixels whose four neighbours are not pending
//                  (any more).  Launched VMTOP_RELAX_ROUNDS times: pending pixels sit in clusters, short chains
//                  end here.
// k_vmtop_decide0_b  the rest in the reference's raster dependency: (v, u) reads (v, u - 1), (v - 1, u - 1),
//                  (v - 1, u) and (v - 1, u + 1), all of a smaller t.  One workgroup per pair walks the t that
//                  still hold pending pixels in order with a workgroup barrier between them; nothing waits on
//                  another workgroup, every loop is bounded by H and W.
// k_vmtop_decide12 methods 1 and 2: sequential along a row (dP[u - 1]), one thread per row.
#include "sm_kernels.h"
#include "sm_device.h"

#include <cfloat>

namespace sm {

namespace {

constexpr int VT_M = VMTOP_MAX_NUM;

__device__ __forceinline__ bool vt_less(float c0, int d0, float c1, int d1) { return c0 < c1 || (c0 == c1 && d0 < d1); }

template <int CTRL>
__device__ __forceinline__ void vt_step(float& c, int& d) {
    const float oc = dpp_f<CTRL>(c);
    const int od = dpp_i<CTRL>(d);
    const bool take = vt_less(oc, od, c, d);
    c = take ? oc : c;
    d = take ? od : d;
}

// NCH: 64-disparity chunks per pixel (D <= 64 NCH); VEC: D % 4 == 0, 16-byte loads
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void k_vmtop_select(VmTopArgs a, long total) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long pix = gid >> 4;
    const int l = threadIdx.x & 15;
    const bool live = pix < total;
    const int D = a.D;
    const float* p = a.vm + (size_t)(live ? pix : 0) * D;
    float c[NCH][4];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        const int d0 = ch * 64 + 4 * l;
        if (VEC) {
            float4 t = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX);
            if (live && d0 < D) t = *reinterpret_cast<const float4*>(p + d0);   // D % 4 == 0: d0 + 3 < D
            c[ch][0] = t.x;
            c[ch][1] = t.y;
            c[ch][2] = t.z;
            c[ch][3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) c[ch][j] = (live && d0 + j < D) ? p[d0 + j] : FLT_MAX;
        }
    }
    const int M = a.M;
    float firstV = 0.f, myd = 0.f, myc = 0.f;
    int kept = 0;
    bool alive = true;
    for (int k = 0; k < M; k++) {   // uniform over the wave: the DPP steps read every lane
        float bc = c[0][0];
        int bd = 4 * l;
#pragma unroll
        for (int ch = 0; ch < NCH; ch++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (ch == 0 && j == 0) continue;
                const bool take = c[ch][j] < bc;   // ascending d inside a lane: strict, the lowest d stays
                bc = take ? c[ch][j] : bc;
                bd = take ? ch * 64 + 4 * l + j : bd;
            }
        vt_step<DPP_QUAD_1032>(bc, bd);
        vt_step<DPP_QUAD_2301>(bc, bd);
        vt_step<DPP_ROW_HALF_MIRROR>(bc, bd);
        vt_step<DPP_ROW_MIRROR>(bc, bd);   // every lane of the row: the pixel's minimum
        if (k == 0) firstV = bc;
        alive = alive && (k == 0 || bc < firstV * a.thres);   // the loop breaks at the first failure
        if (alive) {
            kept++;
            if (l == k) {
                myd = (float)bd;
                myc = bc;
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ch++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (ch * 64 + 4 * l + j == bd) c[ch][j] = FLT_MAX;
        }
    }
    if (live) {
        if (l < kept) a.tab[(size_t)pix * M + l] = make_float2(myd, myc);
        if (l == 0) a.cnt[pix] = kept;
    }
}

struct VtCand {
    float d[VT_M], c[VT_M];
    int n;
};

__device__ __forceinline__ void vt_load(const VmTopArgs& a, size_t p, VtCand& t) {
    t.n = a.cnt[p];
#pragma unroll
    for (int k = 0; k < VT_M; k++) {
        float2 e = make_float2(-1.f, 0.f);
        if (k < t.n) e = a.tab[p * a.M + k];
        t.d[k] = e.x;
        t.c[k] = e.y;
    }
}

__global__ __launch_bounds__(256) void k_vmtop_decide0_a(VmTopArgs a) {
    const int H = a.H, W = a.W;
    const size_t npix = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix * a.n) return;
    const int b = (int)(p / npix);
    const int r = (int)(p - (size_t)b * npix);
    const int v = r / W, u = r - v * W;
    VtCand t;
    vt_load(a, p, t);
    if (u == 0 || v == 0 || t.n <= 1) {   // case 1
        a.disp[p] = (int16_t)t.d[0];
        return;
    }
    // dispCost_container is a std::map keyed by COST whose insert does not overwrite: of candidates with equal
    // cost the first one inserted stays.  Inserts run over the pairs i < j with |d_i - d_j| < ts, (c_i, d_i)
    // then (c_j, d_j) (without vmTop_hasCir2: every candidate in order); tm is a candidate's first insert.
    bool inc[VT_M];
    int tm[VT_M];
#pragma unroll
    for (int x = 0; x < VT_M; x++) {
        inc[x] = false;
        tm[x] = 0x7fffffff;
        if (x < t.n) {
            if (!a.has_cir2) {
                inc[x] = true;
                tm[x] = x;
            } else {
#pragma unroll
                for (int y = 0; y < VT_M; y++) {
                    if (y == x || y >= t.n) continue;
                    if (abs((int)t.d[x] - (int)t.d[y]) < a.ts) {
                        const int i = x < y ? x : y, j = x < y ? y : x;
                        const int when = 2 * (i * VT_M + j) + (x == j ? 1 : 0);
                        inc[x] = true;
                        tm[x] = when < tm[x] ? when : tm[x];
                    }
                }
            }
        }
    }
    bool sv[VT_M];
    bool any = false;
#pragma unroll
    for (int x = 0; x < VT_M; x++) {
        sv[x] = inc[x];
#pragma unroll
        for (int y = 0; y < VT_M; y++)
            if (y != x && inc[y] && t.c[y] == t.c[x] && tm[y] < tm[x]) sv[x] = false;
        any = any || sv[x];
    }
    if (!any) {   // case 2: needs output values; k_vmtop_decide0_b
        a.disp[p] = -1;
        atomicAdd(&a.tcnt[(size_t)b * (W + 2 * H) + u + 2 * v], 1);
        return;
    }
    // case 3
    int num[VT_M];
    float cs[VT_M];
#pragma unroll
    for (int x = 0; x < VT_M; x++) {
        num[x] = 1;
        cs[x] = 0.f + t.c[x];
    }
    const uint8_t* img = a.bgr + (size_t)b * 2 * npix * 3;   // I_c[0] for both views
    const uint8_t* tar = img + (size_t)r * 3;
    for (int i = 0; i < 8; i++) {   // l, u, r, d, lu, rd, ru, ld
        const int dv = i == 1 || i == 4 || i == 6 ? -1 : (i == 3 || i == 5 || i == 7 ? 1 : 0);
        const int du = i == 0 || i == 4 || i == 7 ? -1 : (i == 2 || i == 5 || i == 6 ? 1 : 0);
        const int v_ = v + dv, u_ = u + du;
        if (v_ < 0 || v_ >= H || u_ < 0 || u_ >= W) continue;
        if (a.color_limit) {   // judgeColorDif(tarP, neiP, 10, 3)
            const uint8_t* nei = img + ((size_t)v_ * W + u_) * 3;
            bool ok = true;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) ok = ok && abs((int)tar[ch] - (int)nei[ch]) <= 10;
            if (!ok) continue;
        }
        const size_t q = (size_t)b * npix + (size_t)v_ * W + u_;
        const int nn = a.cnt[q];
        for (int y = 0; y < VT_M; y++) {
            if (y >= nn) break;
            const float2 e = a.tab[q * a.M + y];
#pragma unroll
            for (int x = 0; x < VT_M; x++)
                if (sv[x] && t.d[x] == e.x) {
                    num[x]++;
                    cs[x] += e.y;
                }
        }
    }
    // over the disparities ascending: the larger num, on equal num the strictly smaller cost sum
    int bn = -1;
    float bcs = FLT_MAX, bdv = 0.f;
#pragma unroll
    for (int x = 0; x < VT_M; x++) {
        if (!sv[x]) continue;
        const bool better = num[x] > bn || (num[x] == bn && (cs[x] < bcs || (cs[x] == bcs && t.d[x] < bdv)));
        if (bn < 0 || better) {
            bn = num[x];
            bcs = cs[x];
            bdv = t.d[x];
        }
    }
    a.disp[p] = (int16_t)bdv;
}

// case 2 of pixel r = v W + u (u, v >= 1) of one pair's map `disp`, whose four neighbours are final
__device__ __forceinline__ int16_t vt_case2(const VmTopArgs& a, size_t gp, const int16_t* disp, size_t r, int u, int W) {
    // the count and all M table slots at once (slots past the count are allocated, their contents unused): no
    // load waits for another, which is what the ordered pass's step time is made of
    VtCand c;
    c.n = a.cnt[gp];
#pragma unroll
    for (int k = 0; k < VT_M; k++) {
        float2 e = make_float2(-1.f, 0.f);
        if (k < a.M) e = a.tab[gp * a.M + k];
        c.d[k] = e.x;
        c.c[k] = e.y;
    }
    const int pre1 = disp[r - 1], pre2 = disp[r - W], lt = disp[r - W - 1];
    const int rt = u != W - 1 ? disp[r - W + 1] : 10000;
    int m1 = 0x7fffffff, m2 = m1, m3 = m1, m4 = m1, e1 = -1, e2 = -1, e3 = -1, e4 = -1;
#pragma unroll
    for (int k = 0; k < VT_M; k++) {
        if (k >= c.n) continue;
        const int dd = (int)c.d[k];
        const int f1 = abs(dd - pre1), f2 = abs(dd - pre2), f3 = abs(dd - rt), f4 = abs(dd - lt);
        if (f1 < m1) { m1 = f1; e1 = dd; }
        if (f2 < m2) { m2 = f2; e2 = dd; }
        if (f3 < m3) { m3 = f3; e3 = dd; }
        if (f4 < m4) { m4 = f4; e4 = dd; }
    }
    const int m = min(min(m3, m4), min(m1, m2));
    const int e = m == m4 ? e4 : (m == m1 ? e1 : (m == m2 ? e2 : e3));
    return (int16_t)(m < 1000 ? e : (int)c.d[0]);
}

// One relaxation round, a thread per pixel: a pending pixel whose four neighbours are not pending is resolved
// now.  A value read here is -1 or final (a pixel's value is a function of its neighbours' final values and is
// written once), so a neighbour resolved by another thread of the same launch is either used or waited for:
// the map does not depend on that.  Pending pixels sit in clusters, so a few rounds leave the ordered pass
// (k_vmtop_decide0_b) only the long chains.
__global__ __launch_bounds__(256) void k_vmtop_decide0_w(VmTopArgs a) {
    const int H = a.H, W = a.W;
    const size_t npix = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix * a.n) return;
    if (a.disp[p] != -1) return;
    const int b = (int)(p / npix);
    const size_t r = p - (size_t)b * npix;
    const int v = (int)(r / W), u = (int)(r - (size_t)v * W);   // pending: u, v >= 1
    const int16_t* disp = a.disp + (size_t)b * npix;
    if (disp[r - 1] == -1 || disp[r - W] == -1 || disp[r - W - 1] == -1 || (u != W - 1 && disp[r - W + 1] == -1)) return;
    a.disp[p] = vt_case2(a, p, disp, r, u, W);
    atomicSub(&a.tcnt[(size_t)b * (W + 2 * H) + u + 2 * v], 1);
}

constexpr int VT_CHUNK = 1024;

__global__ __launch_bounds__(256) void k_vmtop_decide0_b(VmTopArgs a) {
    const int H = a.H, W = a.W;
    const size_t npix = (size_t)H * W;
    const int b = blockIdx.x;
    const int T = W + 2 * H;
    const int* tc = a.tcnt + (size_t)b * T;
    int16_t* disp = a.disp + (size_t)b * npix;
    __shared__ unsigned long long nz[VT_CHUNK / 64];   // bit i of word w: t0 + 64 w + i still has pending pixels
    const int wave = threadIdx.x >> 6;
    for (int t0 = 0; t0 < T; t0 += VT_CHUNK) {
        for (int it = 0; it < VT_CHUNK / 256; it++) {
            const int i = it * 256 + (int)threadIdx.x;
            const unsigned long long m = __ballot(t0 + i < T && tc[t0 + i] != 0);
            if ((threadIdx.x & 63) == 0) nz[it * 4 + wave] = m;
        }
        __syncthreads();
        for (int w = 0; w < VT_CHUNK / 64; w++) {
            unsigned long long m = nz[w];   // uniform over the workgroup
            for (int k = 0; k < 64 && m != 0; k++) {
                const int t = t0 + w * 64 + __builtin_ctzll(m);
                m &= m - 1;
                // u = t - 2 v in [1, W - 1], v in [1, H - 1]
                int vlo = (t - (W - 1) + 1) >> 1;
                vlo = vlo < 1 ? 1 : vlo;
                int vhi = (t - 1) >> 1;
                vhi = vhi > H - 1 ? H - 1 : vhi;
                for (int v = vlo + (int)threadIdx.x; v <= vhi; v += 256) {
                    const int u = t - 2 * v;
                    const size_t r = (size_t)v * W + u;
                    // (loads first, for every pixel of the anti-diagonal: one memory round trip per t)
                    const int16_t cur = disp[r];
                    const int16_t val = vt_case2(a, (size_t)b * npix + r, disp, r, u, W);
                    if (cur == -1) disp[r] = val;
                }
                __syncthreads();   // this t's outputs are visible to the workgroup before the next t reads them
            }
        }
        __syncthreads();   // everyone has left the chunk before nz is overwritten
    }
}

__global__ __launch_bounds__(64) void k_vmtop_decide12(VmTopArgs a) {
    const int H = a.H, W = a.W;
    const size_t npix = (size_t)H * W;
    const long row = (long)blockIdx.x * 64 + threadIdx.x;
    if (row >= (long)a.n * H) return;
    const int b = (int)(row / H);
    const size_t p0 = (size_t)row * W;   // == b npix + v W
    const uint8_t* img = a.bgr + (size_t)b * 2 * npix * 3 + (p0 - (size_t)b * npix) * 3;
    int pre = 0;
    for (int u = 0; u < W; u++) {
        VtCand c;
        vt_load(a, p0 + u, c);
        int out = (int)c.d[0];
        if (u != 0 && c.n != 1) {
            int d0 = -1, d1 = -1, m0 = a.method == 1 ? 10000 : 1000000, m1 = 1000000;
#pragma unroll
            for (int k = 0; k < VT_M; k++) {
                if (k >= c.n) continue;
                const int s = (int)fabsf(c.d[k] - (float)pre);
                if (s < 2 && s < m0) {
                    m0 = s;
                    d0 = (int)c.d[k];
                }
            }
            if (a.method == 1) {
                out = d0 == -1 ? (int)c.d[0] : d0;
            } else {
                if (u < W - 1) {
                    const float aft = a.tab[(p0 + u + 1) * a.M].x;
#pragma unroll
                    for (int k = 0; k < VT_M; k++) {
                        if (k >= c.n) continue;
                        const int s = (int)fabsf(c.d[k] - aft);
                        if (s < 2 && s < m1) {
                            m1 = s;
                            d1 = (int)c.d[k];
                        }
                    }
                }
                if (d0 != -1 && d1 == -1) {
                    out = d0;
                } else if (d0 == -1 && d1 != -1) {
                    out = d1;
                } else if (d0 != -1 && d1 != -1) {   // 1 <= u < W - 1 here
                    const uint8_t* cp = img + (size_t)u * 3;
                    int cpre = 0, caft = 0;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        cpre += abs((int)cp[ch] - (int)cp[ch - 3]);
                        caft += abs((int)cp[ch] - (int)cp[ch + 3]);
                    }
                    out = cpre <= caft ? d0 : d1;
                }
            }
        }
        a.disp[p0 + u] = (int16_t)out;
        pre = (int16_t)out;
    }
}

template <bool VEC>
void select_nch(const VmTopArgs& a, long total, dim3 grid, hipStream_t st) {
    const int nch = (a.D + 63) / 64;
    if (nch <= 1) hipLaunchKernelGGL((k_vmtop_select<1, VEC>), grid, dim3(256), 0, st, a, total);
    else if (nch <= 2) hipLaunchKernelGGL((k_vmtop_select<2, VEC>), grid, dim3(256), 0, st, a, total);
    else if (nch <= 4) hipLaunchKernelGGL((k_vmtop_select<4, VEC>), grid, dim3(256), 0, st, a, total);
    else if (nch <= 8) hipLaunchKernelGGL((k_vmtop_select<8, VEC>), grid, dim3(256), 0, st, a, total);
    else hipLaunchKernelGGL((k_vmtop_select<16, VEC>), grid, dim3(256), 0, st, a, total);
}

}  // namespace

bool vmtop_shape_ok(int H, int W, int D, int n) {
    const double px = (double)H * W * n;
    return D >= 1 && D <= 1024 && px * 16 / 256 < 2147483647.0 && (double)n * H < 2147483647.0 * 64;
}

void launch_vmtop_select(const VmTopArgs& a, hipStream_t st) {
    const long total = (long)a.n * a.H * a.W;
    const dim3 grid((unsigned)((total * 16 + 255) / 256));
    // 16-byte loads need every pixel's costs 16-byte aligned
    if (a.D % 4 == 0 && ((uintptr_t)a.vm & 15) == 0) select_nch<true>(a, total, grid, st);
    else select_nch<false>(a, total, grid, st);
}

void launch_vmtop_decide0_a(const VmTopArgs& a, hipStream_t st) {
    const long total = (long)a.n * a.H * a.W;
    hipLaunchKernelGGL(k_vmtop_decide0_a, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

void launch_vmtop_decide0_w(const VmTopArgs& a, hipStream_t st) {
    const long total = (long)a.n * a.H * a.W;
    hipLaunchKernelGGL(k_vmtop_decide0_w, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

void launch_vmtop_decide0_b(const VmTopArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_vmtop_decide0_b, dim3((unsigned)a.n), dim3(256), 0, st, a);
}

void launch_vmtop_decide12(const VmTopArgs& a, hipStream_t st) {
    const long rows = (long)a.n * a.H;
    hipLaunchKernelGGL(k_vmtop_decide12, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, a);
}

}  // namespace sm
