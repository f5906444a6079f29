// depth.hip — expected depth and accumulated alpha of the last forward (dvs_raster_depth_views), for gfx950.
//
// A forward-only pass over the state A7 saved: it does not touch the composite, binning or backward kernels. One 256-thread workgroup
// per (view, tile) as in render.hip; pixel t of the tile is (t & 15, t >> 4), so a wave stores four 64-byte row pieces per output. Per
// pixel it walks the tile's list entries [start, start + n_contrib) in order — n_contrib is the 1-based list position of the pixel's
// last contributor, so the forward's early stop needs no test here — with the forward's two skip rules and its alpha cap, accumulates
// w = alpha T, D += w z, T *= 1 - alpha and writes alpha = 1 - T and depth = D / alpha (0 where alpha < 1/255).
// The seven floats an entry needs (mean x, y | the three conic terms as A7 scales them | opacity | view-space z) go through LDS in
// batches of 256, one gathered record per lane, then broadcast reads: two ds_read_b128 at one address per visit. No atomics.
//
// alpha and T are formed by the operations of k_render_fwd, in its order (explicit fused multiply-adds where it has them; the file is
// compiled without contraction), so that every threshold decision is the forward's and 1 - T equals 1 - final_T.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "render_common.h"

struct __attribute__((aligned(16))) DepthLds {
    float4 a[RB];       // mean x, mean y, cs.x, cs.y        (cs as in render.hip: exp(power) = exp2(cs.x dx^2 + cs.y dx dy + cs.z dy^2))
    float4 b[RB];       // cs.z, opacity, view-space z, -
    uint32_t wmax[RB / 64];
};

__global__ void __launch_bounds__(RB)
k_depth_views(int W, int H, int tiles_x, int tiles_per_view, int num_tiles, const uint2* __restrict__ ranges,
              const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const uint32_t* __restrict__ n_contrib,
              float* __restrict__ out_depth /*[views,H,W]*/, float* __restrict__ out_alpha /*[views,H,W]*/) {
    __shared__ DepthLds L;
    const int tile_g = tile_of_block(blockIdx.x, num_tiles);
    if (tile_g >= num_tiles) return;                                       // (whole workgroup: no barrier is skipped by a part of it)
    const int view = tile_g / tiles_per_view, tile = tile_g - view * tiles_per_view;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int t = threadIdx.x;
    const int px = tx * DVS_TILE + (t & 15), py = ty * DVS_TILE + (t >> 4);
    const bool inside = px < W && py < H;
    const size_t pix = (size_t)view * W * H + (size_t)py * W + px;
    const uint2 range = ranges[tile_g];
    const uint32_t total = range.y - range.x;
    // entries this pixel walks; never more than the tile's list holds
    const uint32_t mine = inside ? min(n_contrib[pix], total) : 0u;
    // entries the workgroup stages: the largest count among its pixels
    uint32_t wm = mine;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, d, 64));
    if ((t & 63) == 0) L.wmax[t >> 6] = wm;
    __syncthreads();
    const uint32_t need = max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]));

    const float pxf = (float)px, pyf = (float)py;
    float T = 1.0f, D = 0.f;
    for (uint32_t base = 0; base < need; base += RB) {
        const uint32_t cnt = min((uint32_t)RB, need - base);
        __syncthreads();                                                   // the previous batch has been read (and wmax, the first time)
        if ((uint32_t)t < cnt) {
            const uint32_t id = sorted_splat[range.x + base + t];          // batch-wide value: view * n + splat, the record's index
            const float4 r0 = splat2d[4 * (size_t)id], r1 = splat2d[4 * (size_t)id + 1], r2 = splat2d[4 * (size_t)id + 2];
            L.a[t] = make_float4(r0.x, r0.y, -0.72134752044448170f * r0.z, -1.4426950408889634f * r0.w);
            L.b[t] = make_float4(-0.72134752044448170f * r1.x, r1.y, r2.y /*DVS_S2D_DEPTH*/, 0.f);
        }
        __syncthreads();
        const uint32_t stop = mine > base ? min(cnt, mine - base) : 0u;
        for (uint32_t j = 0; j < stop; ++j) {
            const float4 A = L.a[j], B = L.b[j];
            const float dx = A.x - pxf, dy = A.y - pyf;
            const float p2 = __builtin_fmaf(B.x * dy, dy, __builtin_fmaf(A.w, dy, A.z * dx) * dx);
            const float alpha = fminf(DVS_ALPHA_MAX, B.y * __builtin_amdgcn_exp2f(p2));
            if (p2 > 0.f || alpha < DVS_ALPHA_MIN) continue;
            const float aT = alpha * T;
            D = __builtin_fmaf(aT, B.z, D);
            T = T - aT;
        }
    }
    if (inside) {
        const float alpha = 1.0f - T;
        out_alpha[pix] = alpha;
        out_depth[pix] = alpha >= DVS_ALPHA_MIN ? D / alpha : 0.f;
    }
}

hipError_t dvs_launch_depth_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges,
                                  const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, float* out_depth,
                                  float* out_alpha) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0) return hipSuccess;
    const int grid = ((num_tiles + 7) >> 3) << 3;
    hipLaunchKernelGGL(k_depth_views, dim3(grid), dim3(RB), 0, st, W, H, tiles_x, tiles_pv, num_tiles, (const uint2*)ranges, sorted_splat,
                       (const float4*)splat2d, n_contrib, out_depth, out_alpha);
    return hipGetLastError();
}
