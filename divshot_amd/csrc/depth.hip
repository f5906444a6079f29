// depth.hip — expected depth and accumulated alpha of the last forward (dvs_raster_depth_views), for gfx950.
//
// A replay pass (replay_walk.h) that accumulates per PIXEL: beyond the record it stages the entry's view-space z, per taken entry it
// forms w = alpha T, D += w z, T *= 1 - alpha, and it writes alpha = 1 - T and depth = D / alpha (0 where alpha < 1/255). T is formed by
// the operations of k_render_fwd, in its order, so 1 - T equals 1 - final_T. A wave stores four 64-byte row pieces per output. No atomics.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "replay_walk.h"

__global__ void __launch_bounds__(RB)
k_depth_views(int W, int H, int tiles_x, int tiles_per_view, int num_tiles, const uint2* __restrict__ ranges,
              const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const uint32_t* __restrict__ n_contrib,
              float* __restrict__ out_depth /*[views,H,W]*/, float* __restrict__ out_alpha /*[views,H,W]*/) {
    __shared__ ReplayLds L;                                               // nothing of its own beside the walk's
    const ReplayTile rt = replay_tile(W, H, tiles_x, tiles_per_view, num_tiles, ranges);
    if (rt.none) return;
    const int t = threadIdx.x;
    const uint32_t mine = replay_mine(rt, rt.inside, n_contrib);
    uint32_t wm;
    const uint32_t need = replay_need(L, mine, &wm);

    const float pxf = (float)rt.px, pyf = (float)rt.py;
    float T = 1.0f, D = 0.f;
    for (uint32_t base = 0; base < need; base += RB) {
        const uint32_t cnt = min((uint32_t)RB, need - base);
        __syncthreads();                                                   // the previous batch has been read (and wmax, the first time)
        if ((uint32_t)t < cnt) {
            const uint32_t id = sorted_splat[rt.range.x + base + t];       // batch-wide value: view * n + splat, the record's index
            replay_stage(L, t, splat2d[4 * (size_t)id], splat2d[4 * (size_t)id + 1], splat2d[4 * (size_t)id + 2].y /*DVS_S2D_DEPTH*/);
        }
        __syncthreads();
        const uint32_t stop = replay_stop(mine, base, cnt);
        for (uint32_t j = 0; j < stop; ++j) {
            const float4 B = L.b[j];
            const ReplayEntry e = replay_entry(L.a[j], B, pxf, pyf);
            if (!e.take) continue;
            const float aT = e.alpha * T;
            D = __builtin_fmaf(aT, B.z, D);
            T = T - aT;
        }
    }
    if (rt.inside) {
        const float alpha = 1.0f - T;
        out_alpha[rt.gpix] = alpha;
        out_depth[rt.gpix] = alpha >= DVS_ALPHA_MIN ? D / alpha : 0.f;
    }
}

hipError_t dvs_launch_depth_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges,
                                  const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, float* out_depth,
                                  float* out_alpha) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_views, dim3(replay_grid(num_tiles)), dim3(RB), 0, st, W, H, tiles_x, tiles_pv, num_tiles, (const uint2*)ranges, sorted_splat,
                       (const float4*)splat2d, n_contrib, out_depth, out_alpha);
    return hipGetLastError();
}
