// sm_refine_da.hip — refine()'s discontinuity adjustment (Do_discontinuityAdjust: discontinuityAdjust,
// stereoMatching.cpp:6057-6136), off by default (sm_refine_da_config).  The three OpenCV calls of the stage
// (equalizeHist, GaussianBlur, Canny on an 8-bit image) are restated in integers ("unpinned").
// A translation unit of its own; it shares sm_refine.hip's pixel mapping (sm_refine_map.h): one thread per pixel,
// a block never straddles two pairs.
//
// k_da_hist      DP[0] -> u8 (clamp to [0, 255]) and the pair's 256-bin histogram: LDS counts per block, one
//                global integer atomic per non-empty bin and block.
// k_da_equalize  every block rebuilds the pair's LUT from the histogram (an inclusive scan in LDS) and maps its tile.
// k_da_blur      3 x 3 Gaussian in 8.8 fixed point, both passes in one kernel (nine cached bytes per pixel).
// k_da_sobel     dx, dy (BORDER_REPLICATE) -> L1 magnitude (<= 2040) and the NMS sector, packed in 16 bits.
// k_da_nms       candidates (m > low, non-maximum suppression) in classes 0 / weak 1 / strong 2; labels start as
//                the pixel's own index, the root flags as 0.
// k_da_link      hysteresis as connected components of the candidate mask: lock-free union-find, every candidate
//                links to its left and three upper candidate neighbours with atomicMin on the larger root.  The
//                trees differ from run to run, the components do not.
// k_da_mark      every strong candidate flags its component's root.
// k_da_edges     255 on candidates whose root is flagged.
// k_da_dir       the adjustment's per-pixel decision from the edge map: the direction (0, 2, 4, 6) of a pixel the
//                ordered pass can change (an interior edge pixel with a direction and DP >= 0), DA_IDLE elsewhere;
//                copies the map into the output.
// k_da_adjust    the in-place raster-order pass.  A pixel reads its first neighbour at (h-1, .) or (h, w-1) --
//                possibly rewritten -- and its second at (h+1, .) or (h, w+1) -- never yet rewritten -- so every
//                pixel depends on at most ONE earlier pixel: the dependencies are a forest whose roots are the
//                pixels with an idle first neighbour.  The thread of such a root walks its tree depth-first
//                without a stack (parent and next sibling follow from the direction plane), reading second
//                neighbours from the input map and first neighbours from the output it wrote itself.  No
//                atomics, no iteration count, one launch; the result is the raster-order result by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_kernels.h"
#include "sm_refine_map.h"

namespace sm {

namespace {

__device__ __forceinline__ uint8_t* da_plane(const DaArgs& a, int b, int plane) {
    return a.u8 + ((size_t)b * DA_PLANES + plane) * ((size_t)a.H * a.W);
}

// FROM_DP: the stage's own entry (DP[0] -> plane DA_EQ); else the histogram of the image already in the plane
template <bool FROM_DP>
__global__ __launch_bounds__(256) void k_da_hist(DaArgs a, const int16_t* __restrict__ dp) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const Pix p = pixel_of(a.H, a.W);
    if (p.ok) {
        const size_t o = (size_t)p.v * a.W + p.u;
        uint8_t* img = da_plane(a, p.b, DA_EQ);
        int x;
        if (FROM_DP) {
            x = dp[(size_t)p.b * a.H * a.W + o];
            x = min(max(x, 0), 255);
            img[o] = (uint8_t)x;
        } else {
            x = img[o];
        }
        atomicAdd(&h[x], 1);
    }
    __syncthreads();
    const int cnt = h[threadIdx.x];
    if (cnt) atomicAdd(&a.hist[(size_t)p.b * 256 + threadIdx.x], cnt);
}

__global__ __launch_bounds__(256) void k_da_equalize(DaArgs a) {
    __shared__ int s[256];
    __shared__ uint8_t lut[256];
    __shared__ int first, hfirst;
    const Pix p = pixel_of(a.H, a.W);   // p.b is block-uniform
    const int t = threadIdx.x;
    const int mine = a.hist[(size_t)p.b * 256 + t];
    s[t] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const int incl = s[t];
    if (mine > 0 && incl == mine) {   // the first non-empty bin
        first = t;
        hfirst = mine;
    }
    __syncthreads();
    const int total = a.H * a.W;
    int out = t;   // hist[i] == total: the image is the constant i
    if (hfirst != total) {
        const float scale = __fdiv_rn(255.f, (float)(total - hfirst));
        // bins below i are empty, so the reference's running sum over (i, t] is incl - hist[i]
        const int r = t > first ? __float2int_rn(__fmul_rn((float)(incl - hfirst), scale)) : 0;
        out = min(max(r, 0), 255);
    }
    lut[t] = (uint8_t)out;
    __syncthreads();
    if (p.ok) {
        uint8_t* img = da_plane(a, p.b, DA_EQ) + (size_t)p.v * a.W + p.u;
        *img = lut[*img];
    }
}

// BORDER_REFLECT_101: -1 -> 1, len -> len - 2 (a single row or column reflects onto itself)
__device__ __forceinline__ int reflect101(int i, int len) {
    if (len == 1) return 0;
    return i < 0 ? -i : (i >= len ? 2 * len - 2 - i : i);
}

__global__ __launch_bounds__(256) void k_da_blur(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int W = a.W;
    const uint8_t* src = da_plane(a, p.b, DA_EQ);
    const int ul = reflect101(p.u - 1, W), ur = reflect101(p.u + 1, W);
    const unsigned ks = (unsigned)a.ks, kc = (unsigned)a.kc;
    unsigned r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint8_t* row = src + (size_t)reflect101(p.v - 1 + i, a.H) * W;
        r[i] = ks * row[ul] + kc * row[p.u] + ks * row[ur];   // <= 255 * 256: 16 bits
    }
    const unsigned c = ks * r[0] + kc * r[1] + ks * r[2];
    da_plane(a, p.b, DA_BLUR)[(size_t)p.v * W + p.u] = (uint8_t)min((c + 32768u) >> 16, 255u);
}

__global__ __launch_bounds__(256) void k_da_sobel(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int W = a.W;
    const uint8_t* src = da_plane(a, p.b, DA_BLUR);
    const uint8_t* r0 = src + (size_t)max(p.v - 1, 0) * W;
    const uint8_t* r1 = src + (size_t)p.v * W;
    const uint8_t* r2 = src + (size_t)min(p.v + 1, a.H - 1) * W;
    const int c0 = max(p.u - 1, 0), c1 = p.u, c2 = min(p.u + 1, W - 1);
    const int dx = ((int)r0[c2] + 2 * (int)r1[c2] + (int)r2[c2]) - ((int)r0[c0] + 2 * (int)r1[c0] + (int)r2[c0]);
    const int dy = ((int)r2[c0] + 2 * (int)r2[c1] + (int)r2[c2]) - ((int)r0[c0] + 2 * (int)r0[c1] + (int)r0[c2]);
    const int x = abs(dx), y = abs(dy) << 15;   // Canny's 15-bit fixed-point tangents: tan(22.5) = 13573 / 2^15
    const int t22 = x * 13573;
    int sector;
    if (y < t22) sector = 0;                        // compare left / right
    else if (y > t22 + (x << 16)) sector = 1;       // up / down
    else sector = ((dx ^ dy) < 0) ? 3 : 2;          // the diagonal with s = -1 / s = +1
    a.mag[(size_t)p.b * a.H * W + (size_t)p.v * W + p.u] = (uint16_t)((x + abs(dy)) | (sector << 12));
}

__global__ __launch_bounds__(256) void k_da_nms(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int H = a.H, W = a.W;
    const uint16_t* mag = a.mag + (size_t)p.b * H * W;
    auto M = [&](int v, int u) -> int {   // magnitudes outside the image are 0
        return (v >= 0 && v < H && u >= 0 && u < W) ? (mag[(size_t)v * W + u] & 0xfff) : 0;
    };
    const int o = p.v * W + p.u;
    const int packed = mag[o];
    const int m = packed & 0xfff, sector = packed >> 12;
    bool cand = m > a.low;
    if (cand) {
        if (sector == 0) cand = m > M(p.v, p.u - 1) && m >= M(p.v, p.u + 1);
        else if (sector == 1) cand = m > M(p.v - 1, p.u) && m >= M(p.v + 1, p.u);
        else {
            const int s = sector == 3 ? -1 : 1;
            cand = m > M(p.v - 1, p.u - s) && m > M(p.v + 1, p.u + s);
        }
    }
    da_plane(a, p.b, DA_CAND)[o] = cand ? (m > a.high ? 2 : 1) : 0;
    da_plane(a, p.b, DA_FLAG)[o] = 0;
    a.lab[(size_t)p.b * H * W + o] = cand ? o : -1;
}

// Union-find over one pair's candidates.  A parent link only ever decreases and stays inside the component, so a
// stale read costs a step, never correctness; the atomicMin on a root is what publishes a union.
__device__ __forceinline__ int da_find(int* L, int x) {
    for (;;) {
        const int y = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (y == x) return x;
        x = y;
    }
}

__device__ __forceinline__ void da_unite(int* L, int x, int y) {
    for (;;) {
        x = da_find(L, x);
        y = da_find(L, y);
        if (x == y) return;
        if (x < y) {
            const int t = x;
            x = y;
            y = t;
        }
        const int old = atomicMin(&L[x], y);   // x > y: hang the larger root under the smaller
        if (old == x) return;
        x = old;   // x was linked elsewhere meanwhile (old < x): unite that with y
    }
}

__global__ __launch_bounds__(256) void k_da_link(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int W = a.W;
    const uint8_t* cand = da_plane(a, p.b, DA_CAND);
    const int o = p.v * W + p.u;
    if (!cand[o]) return;
    int* L = a.lab + (size_t)p.b * a.H * W;
    if (p.u > 0 && cand[o - 1]) da_unite(L, o, o - 1);
    if (p.v > 0) {
        if (p.u > 0 && cand[o - W - 1]) da_unite(L, o, o - W - 1);
        if (cand[o - W]) da_unite(L, o, o - W);
        if (p.u + 1 < W && cand[o - W + 1]) da_unite(L, o, o - W + 1);
    }
}

__global__ __launch_bounds__(256) void k_da_mark(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int o = p.v * a.W + p.u;
    if (da_plane(a, p.b, DA_CAND)[o] != 2) return;
    da_plane(a, p.b, DA_FLAG)[da_find(a.lab + (size_t)p.b * a.H * a.W, o)] = 1;
}

__global__ __launch_bounds__(256) void k_da_edges(DaArgs a) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int o = p.v * a.W + p.u;
    uint8_t e = 0;
    if (da_plane(a, p.b, DA_CAND)[o]) e = da_plane(a, p.b, DA_FLAG)[da_find(a.lab + (size_t)p.b * a.H * a.W, o)] ? 255 : 0;
    da_plane(a, p.b, DA_EDGE)[o] = e;
}

constexpr int DA_IDLE = 0xff;   // the ordered pass leaves the pixel alone

__global__ __launch_bounds__(256) void k_da_dir(DaArgs a, const int16_t* __restrict__ src, int16_t* __restrict__ dst) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int H = a.H, W = a.W;
    const int o = p.v * W + p.u;
    const size_t base = (size_t)p.b * H * W;
    const int16_t d = src[base + o];
    dst[base + o] = d;
    int dir = DA_IDLE;
    const uint8_t* E = da_plane(a, p.b, DA_EDGE) + o;
    if (p.v >= 1 && p.v <= H - 2 && p.u >= 1 && p.u <= W - 2 && d >= 0 && E[0]) {
        const bool ul = E[-W - 1], up = E[-W], ur = E[-W + 1], le = E[-1], ri = E[1], dl = E[W - 1], dn = E[W], dr = E[W + 1];
        // cpp:6079-6098, the two nested ifs that leave -1 included
        if (ul && dr) dir = 4;
        else if (ur && dl) dir = 0;
        else if (up || ul || ur) {
            if (dn || dl || dr) dir = 6;
        } else if (ul || le || dl) {
            if (ur || ri || dr) dir = 2;
        }
    }
    da_plane(a, p.b, DA_DIR)[o] = (uint8_t)dir;
}

// A pixel q's dependants in raster order of their own positions' child slot k: (h+1, w-1) with direction 4,
// (h+1, w) with 2, (h+1, w+1) with 0, (h, w+1) with 6: the pixels whose FIRST neighbour
// (directionsH/W[direction]: 4 -> (-1, +1), 2 -> (-1, 0), 0 -> (-1, -1), 6 -> (0, -1)) is q.
__device__ __forceinline__ int da_child_dv(int k) { return k < 3 ? 1 : 0; }
__device__ __forceinline__ int da_child_du(int k) { return k == 0 ? -1 : (k == 1 ? 0 : 1); }
__device__ __forceinline__ int da_child_dir(int k) { return k < 3 ? 4 - 2 * k : 6; }
__device__ __forceinline__ int da_slot_of(int dir) { return dir == 6 ? 3 : (4 - dir) >> 1; }

// the first dependant of (v, u) in slots [k0, 4), or 4
__device__ __forceinline__ int da_next_child(const uint8_t* dirs, int H, int W, int v, int u, int k0) {
    for (int k = k0; k < 4; k++) {
        const int cv = v + da_child_dv(k), cu = u + da_child_du(k);
        if (cv < H && cu >= 0 && cu < W && dirs[cv * W + cu] == da_child_dir(k)) return k;
    }
    return 4;
}

// vm[0] at a pixel and a disparity of the map; a disparity outside [0, D) reads as -1 (the reference's "invalid":
// for d >= D it reads outside the volume; such a value can only come from sm_set_disp)
__device__ __forceinline__ float da_cost(const float* vm, int D, int o, int d) {
    return (d >= 0 && d < D) ? vm[(size_t)o * D + d] : -1.f;
}

__global__ __launch_bounds__(256) void k_da_adjust(DaArgs a, const int16_t* src, int16_t* dst, const float* __restrict__ vm0,
                                                   int D) {
    const Pix p = pixel_of(a.H, a.W);
    if (!p.ok) return;
    const int H = a.H, W = a.W;
    const uint8_t* dirs = da_plane(a, p.b, DA_DIR);
    const int mydir = dirs[p.v * W + p.u];
    if (mydir == DA_IDLE) return;
    {   // only the root of a dependency tree works: its first neighbour is final from the start
        const int k = da_slot_of(mydir);
        if (dirs[(p.v - da_child_dv(k)) * W + (p.u - da_child_du(k))] != DA_IDLE) return;
    }
    const size_t base = (size_t)p.b * H * W;
    const int16_t* S = src + base;
    int16_t* T = dst + base;
    const float* vm = vm0 + base * D;
    int v = p.v, u = p.u;
    for (;;) {
        {   // cpp:6100-6131 at (v, u)
            const int o = v * W + u;
            const int k = da_slot_of(dirs[o]);
            const int n1 = o - da_child_dv(k) * W - da_child_du(k);   // earlier in raster order: the output
            const int n2 = o + da_child_dv(k) * W + da_child_du(k);   // later: the input
            int dp = S[o];
            float cost = da_cost(vm, D, o, dp);
            const int d1 = T[n1], d2 = S[n2];
            const float cost1 = da_cost(vm, D, n1, d1), cost2 = da_cost(vm, D, n2, d2);
            if (cost1 >= 0 && cost1 < cost) {
                dp = d1;
                cost = cost1;
            }
            if (cost2 != -1 && cost2 < cost) dp = d2;
            T[o] = (int16_t)dp;
        }
        int k = da_next_child(dirs, H, W, v, u, 0);
        if (k < 4) {
            v += da_child_dv(k);
            u += da_child_du(k);
            continue;
        }
        for (;;) {   // no dependant left here: climb to the nearest ancestor with an unvisited one
            if (v == p.v && u == p.u) return;
            const int me = da_slot_of(dirs[v * W + u]);
            const int pv = v - da_child_dv(me), pu = u - da_child_du(me);
            k = da_next_child(dirs, H, W, pv, pu, me + 1);
            if (k < 4) {
                v = pv + da_child_dv(k);
                u = pu + da_child_du(k);
                break;
            }
            v = pv;
            u = pu;
        }
    }
}

}  // namespace

void launch_da_hist(const DaArgs& a, const int16_t* dp, hipStream_t st) {
    const dim3 grid = grid_of(a.n, a.H, a.W);
    if (dp) hipLaunchKernelGGL(k_da_hist<true>, grid, dim3(256), 0, st, a, dp);
    else hipLaunchKernelGGL(k_da_hist<false>, grid, dim3(256), 0, st, a, dp);
}
void launch_da_equalize(const DaArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_da_equalize, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a);
}
void launch_da_blur(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_blur, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_sobel(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_sobel, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_nms(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_nms, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_link(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_link, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_mark(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_mark, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_edges(const DaArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_da_edges, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a); }
void launch_da_dir(const DaArgs& a, const int16_t* src, int16_t* dst, hipStream_t st) {
    hipLaunchKernelGGL(k_da_dir, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a, src, dst);
}
void launch_da_adjust(const DaArgs& a, const int16_t* src, int16_t* dst, const float* vm, int D, hipStream_t st) {
    hipLaunchKernelGGL(k_da_adjust, grid_of(a.n, a.H, a.W), dim3(256), 0, st, a, src, dst, vm, D);
}

}  // namespace sm
