// sm_refine_map.h — the pixel mapping of the refine() kernels (sm_refine.hip, sm_refine_ext.hip): one thread
// per pixel, 256-thread blocks over [pair][row-tile][col-tile] 64 x 4 tiles, so a wave covers one 64-pixel row
// segment (coalesced int16 accesses).
#pragma once
#include <hip/hip_runtime.h>

namespace sm {

constexpr int TX = 64, TY = 4;

struct Pix {
    int b, v, u;
    bool ok;
};

__device__ __forceinline__ Pix pixel_of(int H, int W) {
    const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
    const int per_pair = tiles_x * tiles_y;
    const int blk = blockIdx.x;
    Pix p;
    p.b = blk / per_pair;
    const int t = blk - p.b * per_pair;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    p.u = tx * TX + (int)(threadIdx.x & (TX - 1));
    p.v = ty * TY + (int)(threadIdx.x / TX);
    p.ok = p.u < W && p.v < H;
    return p;
}

inline dim3 grid_of(int n, int H, int W) { return dim3((unsigned)(n * ((W + TX - 1) / TX) * ((H + TY - 1) / TY))); }

}  // namespace sm
