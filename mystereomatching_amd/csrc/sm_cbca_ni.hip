// sm_cbca_ni.hip — cbca_core without arm intersection (Parameters::cbca_intersect == false, cpp:5585-5666): the
// cross-based aggregation of Zhang et al.  The support region of a pixel comes from the view's own image's arms
// (HVL[LOR]) and is the same for every disparity, so one integer area per pixel replaces one per volume element.
// A translation unit of its own: it shares no kernel with the intersecting sweeps of sm_cbca.hip.
//
// One 1-D pass (gen1DCumu cpp:3896-3926, then cal1DCost h:1643-1715) is two kernels, the plain form:
//
// k_ni_prefix  S(x) = S(x - 1) + vm(x) along the pass axis, in place, f32, in scan order; the same prefix of
//              the int32 area plane.  A "line" is a row (H pass: positions D floats apart) or a pair's whole
//              image of columns (V pass: positions W D floats apart); a thread owns VEC consecutive floats
//              of the line's cross-section and walks the positions, NI_TILE positions loaded ahead of the
//              NI_TILE being summed and stored.  The thread that owns a pixel's disparity 0 carries the
//              pixel's area as well (first pass of an iteration: the input is ones(h, w), cpp:5606, and is
//              not read).  8 B per element (read, write).
// k_ni_window  out(p, d) = inner ? S(x + head, d) - S(x - tail - 1, d) : S(x + head, d) with (tail, head) the
//              pixel's own arm pair of the pass direction and inner = x - tail - 1 >= 0, the same for all d;
//              area_out likewise in integers.  One thread per VEC floats of a pixel, fully parallel; it
//              writes the OTHER volume (a pass never reads its own outputs).  The second pass of an
//              iteration also divides (genfinalVm_cbca cpp:3969-3992: (float)area, one IEEE f32 division)
//              and, in the last iteration of sm_run, applies SolveAll's weight.  12 B per element requested
//              (two reads, one write); every S position is the head of one pixel and the tail of another,
//              so 8 B per element from HBM, the rest from L2.
//
// VEC = 4 (16-byte accesses) where D % 4 == 0, else 1.  x + head never passes the line's end (the arm kernel
// stops at the image border); the kernels clamp it all the same, so no arm word can make them read outside
// the volume.
#include <hip/hip_runtime.h>

#include "sm_device.h"
#include "sm_kernels.h"

namespace sm {

constexpr int NI_TILE = 8;

template <int V>
struct ni_vec {
    float x[V];
};
template <int V>
__device__ __forceinline__ ni_vec<V> ni_load(const float* p) {
    ni_vec<V> r;
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        r.x[0] = t.x, r.x[1] = t.y, r.x[2] = t.z, r.x[3] = t.w;
    } else {
        r.x[0] = *p;
    }
    return r;
}
template <int V>
__device__ __forceinline__ void ni_store(float* p, const ni_vec<V>& r) {
    if constexpr (V == 4) *(float4*)p = make_float4(r.x[0], r.x[1], r.x[2], r.x[3]);
    else *p = r.x[0];
}

// total = lines * EV threads, EV = (floats of a line's cross-section) / V
template <int V>
__global__ __launch_bounds__(256) void k_ni_prefix(const NiArgs a, size_t total, int EV) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t line = t / (unsigned)EV;
    const int e = (int)(t - line * (unsigned)EV) * V;
    const int L = a.horiz ? a.W : a.H;
    const size_t stride = a.horiz ? (size_t)a.D : (size_t)a.W * a.D;
    float* __restrict__ p = a.src + line * (size_t)L * stride + e;
    // the thread of a pixel's disparity 0 also sums the pixel's area: H pass line = (pair, row), the row's pixels
    // one apart; V pass line = pair, column e / D, the column's pixels W apart
    const bool has_area = e % a.D == 0;
    const size_t npix = (size_t)a.H * a.W;
    int32_t* __restrict__ q = nullptr;
    size_t qs = 1;
    if (has_area) {
        if (a.horiz) {
            const size_t pair = line / (unsigned)a.H, v = line - pair * (unsigned)a.H;
            q = a.area + (pair * 4 + (size_t)a.view * 2 + a.in_plane) * npix + v * a.W;
        } else {
            q = a.area + (line * 4 + (size_t)a.view * 2 + a.in_plane) * npix + e / a.D;
            qs = (size_t)a.W;
        }
    }
    const bool load_area = has_area && !a.first;
    ni_vec<V> s;
#pragma unroll
    for (int k = 0; k < V; k++) s.x[k] = -0.0f;   // -0 + x == x for every x: S(0) = vm(0)
    int32_t sa = 0;
    ni_vec<V> cur[NI_TILE], nxt[NI_TILE];
    int32_t ca[NI_TILE], na[NI_TILE];
#pragma unroll
    for (int i = 0; i < NI_TILE; i++) ca[i] = na[i] = 1;
    int x0 = 0;
    if (L >= NI_TILE) {
#pragma unroll
        for (int i = 0; i < NI_TILE; i++) cur[i] = ni_load<V>(p + (size_t)i * stride);
        if (load_area) {
#pragma unroll
            for (int i = 0; i < NI_TILE; i++) ca[i] = q[(size_t)i * qs];
        }
    }
    for (; x0 + NI_TILE <= L; x0 += NI_TILE) {
        const bool more = x0 + 2 * NI_TILE <= L;
        if (more) {
#pragma unroll
            for (int i = 0; i < NI_TILE; i++) nxt[i] = ni_load<V>(p + (size_t)(x0 + NI_TILE + i) * stride);
            if (load_area) {
#pragma unroll
                for (int i = 0; i < NI_TILE; i++) na[i] = q[(size_t)(x0 + NI_TILE + i) * qs];
            }
        }
#pragma unroll
        for (int i = 0; i < NI_TILE; i++) {
#pragma unroll
            for (int k = 0; k < V; k++) s.x[k] += cur[i].x[k];
            ni_store<V>(p + (size_t)(x0 + i) * stride, s);
        }
        if (has_area) {
#pragma unroll
            for (int i = 0; i < NI_TILE; i++) {
                sa += ca[i];
                q[(size_t)(x0 + i) * qs] = sa;
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < NI_TILE; i++) {
                cur[i] = nxt[i];
                ca[i] = na[i];
            }
        }
    }
    for (int x = x0; x < L; x++) {
        const ni_vec<V> c = ni_load<V>(p + (size_t)x * stride);
#pragma unroll
        for (int k = 0; k < V; k++) s.x[k] += c.x[k];
        ni_store<V>(p + (size_t)x * stride, s);
        if (has_area) {
            sa += load_area ? q[(size_t)x * qs] : 1;
            q[(size_t)x * qs] = sa;
        }
    }
}

// grid (ceil(W DV / 256), H, n), DV = D / V: thread t of a row is pixel u = t / DV, floats [V (t % DV), + V)
template <int V>
__global__ __launch_bounds__(256) void k_ni_window(const NiArgs a, int DV) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const int u = (int)(t / (unsigned)DV), v = blockIdx.y;
    if (u >= a.W) return;
    const int d = (int)(t - (unsigned)u * (unsigned)DV) * V;
    const size_t npix = (size_t)a.H * a.W, pair = blockIdx.z;
    const size_t p = (size_t)v * a.W + u, pix = pair * npix + p;
    const int L = a.horiz ? a.W : a.H;
    const int ps = a.horiz ? 1 : a.W;   // pixels between two positions of a line
    const uint32_t w = a.arms[((pair * 2 + a.view) * 2 + (a.horiz ? 0 : 1)) * npix + p];
    const int tail = (int)(w & 0xffffu), head = (int)(w >> 16);
    const int x = a.horiz ? u : v;
    const int hi = min(x + head, L - 1), pt = x - tail - 1;
    const bool inner = pt >= 0;
    const size_t oh = (size_t)(hi - x) * ps;               // pixels from p to the head position (hi >= x)
    const size_t ol = inner ? (size_t)(x - pt) * ps : 0;   // pixels from the tail position to p (read where inner)
    const int32_t* __restrict__ ain = a.area + (pair * 4 + (size_t)a.view * 2 + a.in_plane) * npix;
    int32_t ao = ain[p + oh];
    ni_vec<V> r = ni_load<V>(a.src + (pix + oh) * a.D + d);
    if (inner) {
        ao -= ain[p - ol];
        const ni_vec<V> lo = ni_load<V>(a.src + (pix - ol) * a.D + d);
#pragma unroll
        for (int k = 0; k < V; k++) r.x[k] -= lo.x[k];
    }
    if (d == 0) a.area[(pair * 4 + (size_t)a.view * 2 + (a.in_plane ^ 1)) * npix + p] = ao;
    if (a.norm) {
        const float fa = (float)ao;
#pragma unroll
        for (int k = 0; k < V; k++) {
            const float qv = r.x[k] / fa;
            r.x[k] = a.apply_scale ? a.scale * qv : qv;
        }
    }
    ni_store<V>(a.dst + pix * a.D + d, r);
}

void launch_ni_prefix(const NiArgs& a, int n, hipStream_t st) {
    const int V = a.D % 4 == 0 ? 4 : 1;
    const size_t lines = a.horiz ? (size_t)n * a.H : (size_t)n;
    const size_t ev = (a.horiz ? (size_t)a.D : (size_t)a.W * a.D) / V;
    const size_t total = lines * ev;
    if (total == 0) return;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (V == 4) hipLaunchKernelGGL(k_ni_prefix<4>, dim3(blocks), dim3(256), 0, st, a, total, (int)ev);
    else hipLaunchKernelGGL(k_ni_prefix<1>, dim3(blocks), dim3(256), 0, st, a, total, (int)ev);
}

void launch_ni_window(const NiArgs& a, int n, hipStream_t st) {
    const int V = a.D % 4 == 0 ? 4 : 1;
    const int DV = a.D / V;
    if (n <= 0 || a.H <= 0 || a.W <= 0 || DV <= 0) return;
    const size_t npix = (size_t)a.H * a.W;
    for (int n0 = 0; n0 < n; n0 += 65535) {   // (grid.z holds at most 65535 pairs)
        NiArgs b = a;
        b.src += (size_t)n0 * npix * a.D;
        b.dst += (size_t)n0 * npix * a.D;
        b.arms += (size_t)n0 * 4 * npix;
        b.area += (size_t)n0 * 4 * npix;
        const dim3 grid((unsigned)(((size_t)a.W * DV + 255) / 256), (unsigned)a.H, (unsigned)(n - n0 < 65535 ? n - n0 : 65535));
        if (V == 4) hipLaunchKernelGGL(k_ni_window<4>, grid, dim3(256), 0, st, b, DV);
        else hipLaunchKernelGGL(k_ni_window<1>, grid, dim3(256), 0, st, b, DV);
    }
}

}  // namespace sm
