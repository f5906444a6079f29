// importance.hip — per-splat blend weight of the last forward (dvs_raster_importance_views), for gfx950.
//
// A forward-only pass over the state A7 saved, shaped like depth.hip: one 256-thread workgroup per (view, tile), pixel t of the tile is
// (t & 15, t >> 4), the tile's list entries [start, start + n_contrib) staged through LDS in batches of 256 and walked per pixel with
// the forward's two skip rules and its alpha cap. alpha and T are formed by the operations of k_render_fwd, in its order (explicit
// fused multiply-adds where it has them; the file is compiled without contraction): every take decision is the forward's own.
// Where depth.hip accumulates per PIXEL, this pass accumulates per ENTRY: w = alpha T of every taken (pixel, entry) pair goes to the
// entry's splat as
//   score_sum += q, q = (uint32_t)rintf(w 2^24)    an integer on purpose: integer adds commute, so the sums are bit-reproducible for any
//                                                  order of the reductions and atomics below, from run to run and across ranks
//   score_max  = max(score_max, bits(w))           w >= 0: the unsigned order of the bits is the order of the floats
//   hits      += 1
// Per entry a wave first asks whether any of its 64 pixels took it (ballot): most (wave, entry) pairs of a 3-sigma rectangle are
// empty and cost nothing more. For the others the hit count is the ballot's popcount and sum / max are reduced over the wave — four
// DPP steps leave each 16-lane row's result in all its lanes, four v_readlane and scalar adds join the rows — and lane 0 stores the
// three into the wave's own LDS table slot of the entry: no LDS atomics. After the batch thread j folds the four waves' slots of
// entry j and issues at most one non-returning global atomic per statistic, none for a zero.
// q <= 0.99 2^24, so a wave's 64 and a tile's 256 pixels fit a uint32; the sum over tiles and views is a uint64.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "render_common.h"

struct __attribute__((aligned(16))) ImportanceLds {
    float4 a[RB];       // mean x, mean y, cs.x, cs.y        (as depth.hip)
    float4 b[RB];       // cs.z, opacity, -, -
    uint32_t sum[RB / 64][RB], max[RB / 64][RB], hits[RB / 64][RB];       // [wave][entry of the batch]
    uint32_t wmax[RB / 64];
};
struct ImportanceMasks { const float* m[DVS_MAX_VIEWS]; };                 // per view: [H,W] or null

// every lane of a 16-lane row <- the row's sum / max (all 64 lanes active): lane ^ 1, lane ^ 2, then the mirrored 4 and 8 lanes
template <int CTRL> __device__ __forceinline__ uint32_t imp_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t imp_row(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint32_t imp_wave_sum(uint32_t v) {
    v += imp_dpp<0xB1>(v);            // quad_perm [1,0,3,2]
    v += imp_dpp<0x4E>(v);            // quad_perm [2,3,0,1]
    v += imp_dpp<0x141>(v);           // row_half_mirror
    v += imp_dpp<0x140>(v);           // row_mirror
    return imp_row(v, 0) + imp_row(v, 16) + imp_row(v, 32) + imp_row(v, 48);
}
__device__ __forceinline__ uint32_t imp_wave_max(uint32_t v) {
    v = max(v, imp_dpp<0xB1>(v));
    v = max(v, imp_dpp<0x4E>(v));
    v = max(v, imp_dpp<0x141>(v));
    v = max(v, imp_dpp<0x140>(v));
    return max(max(imp_row(v, 0), imp_row(v, 16)), max(imp_row(v, 32), imp_row(v, 48)));
}

__global__ void __launch_bounds__(RB)
k_importance_views(ImportanceMasks masks, int W, int H, int tiles_x, int tiles_per_view, int num_tiles, int n, const uint2* __restrict__ ranges,
                   const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const uint32_t* __restrict__ n_contrib,
                   unsigned long long* __restrict__ score_sum /*[n]*/, uint32_t* __restrict__ score_max /*[n] or null*/,
                   uint32_t* __restrict__ hits /*[n] or null*/) {
    __shared__ ImportanceLds L;
    const int tile_g = tile_of_block(blockIdx.x, num_tiles);
    if (tile_g >= num_tiles) return;                                       // (whole workgroup: no barrier is skipped by a part of it)
    const int view = tile_g / tiles_per_view, tile = tile_g - view * tiles_per_view;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int t = threadIdx.x, wave = t >> 6;
    const int px = tx * DVS_TILE + (t & 15), py = ty * DVS_TILE + (t >> 4);
    const float* const mask = masks.m[view];
    // a pixel outside the image or masked out walks nothing
    const bool counts = px < W && py < H && !(mask && mask[(size_t)py * W + px] == 0.f);
    const size_t pix = (size_t)view * W * H + (size_t)py * W + px;
    const uint2 range = ranges[tile_g];
    const uint32_t total = range.y - range.x;
    const uint32_t mine = counts ? min(n_contrib[pix], total) : 0u;        // entries this pixel walks; never more than the tile's list holds
    uint32_t wm = mine;                                                    // ... and the largest count among the wave's pixels
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, d, 64));
    if ((t & 63) == 0) L.wmax[wave] = wm;
    __syncthreads();
    const uint32_t need = max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]));   // entries the workgroup stages

    const float pxf = (float)px, pyf = (float)py;
    float T = 1.0f;
    for (uint32_t base = 0; base < need; base += RB) {
        const uint32_t cnt = min((uint32_t)RB, need - base);
        uint32_t id = 0;
        if ((uint32_t)t < cnt) {
            id = sorted_splat[range.x + base + t];                         // batch-wide value: view * n + splat, the record's index
            const float4 r0 = splat2d[4 * (size_t)id], r1 = splat2d[4 * (size_t)id + 1];
            L.a[t] = make_float4(r0.x, r0.y, -0.72134752044448170f * r0.z, -1.4426950408889634f * r0.w);
            L.b[t] = make_float4(-0.72134752044448170f * r1.x, r1.y, 0.f, 0.f);
#pragma unroll
            for (int w = 0; w < RB / 64; ++w) { L.sum[w][t] = 0u; L.max[w][t] = 0u; L.hits[w][t] = 0u; }
        }
        __syncthreads();
        const uint32_t stop = mine > base ? min(cnt, mine - base) : 0u;
        const uint32_t wave_stop = wm > base ? min(cnt, wm - base) : 0u;   // wave-uniform: the cross-lane steps below run with all 64 lanes
        for (uint32_t j = 0; j < wave_stop; ++j) {
            const float4 A = L.a[j], B = L.b[j];
            const float dx = A.x - pxf, dy = A.y - pyf;
            const float p2 = __builtin_fmaf(B.x * dy, dy, __builtin_fmaf(A.w, dy, A.z * dx) * dx);
            const float alpha = fminf(DVS_ALPHA_MAX, B.y * __builtin_amdgcn_exp2f(p2));
            const bool take = j < stop && !(p2 > 0.f || alpha < DVS_ALPHA_MIN);
            const uint64_t took = __ballot(take);
            if (took == 0ull) continue;
            const float aT = take ? alpha * T : 0.f;
            T = T - aT;
            const uint32_t s = imp_wave_sum((uint32_t)rintf(aT * 16777216.0f));
            const uint32_t m = imp_wave_max(__float_as_uint(aT));
            if ((t & 63) == 0) { L.sum[wave][j] = s; L.max[wave][j] = m; L.hits[wave][j] = (uint32_t)__popcll(took); }
        }
        __syncthreads();
        if ((uint32_t)t < cnt) {
            const uint32_t splat = id - (uint32_t)view * (uint32_t)n;
            const uint32_t s = L.sum[0][t] + L.sum[1][t] + L.sum[2][t] + L.sum[3][t];
            if (s != 0u && splat < (uint32_t)n) {                          // (a taken pair has q >= 6: s == 0 means nobody took the entry)
                (void)atomicAdd(&score_sum[splat], (unsigned long long)s);
                if (score_max) (void)atomicMax(&score_max[splat], max(max(L.max[0][t], L.max[1][t]), max(L.max[2][t], L.max[3][t])));
                if (hits) (void)atomicAdd(&hits[splat], L.hits[0][t] + L.hits[1][t] + L.hits[2][t] + L.hits[3][t]);
            }
        }
        // (the next batch's staging writes only what this thread has just read, and the barrier after it orders the rest)
    }
}

hipError_t dvs_launch_importance_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges,
                                       const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, const float* const* masks,
                                       uint64_t* score_sum, uint32_t* score_max, uint32_t* hits) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0 || n <= 0) return hipSuccess;
    if (n_views > DVS_MAX_VIEWS) return hipErrorInvalidValue;
    ImportanceMasks mk{};
    for (int v = 0; v < n_views; ++v) mk.m[v] = masks ? masks[v] : nullptr;
    const int grid = ((num_tiles + 7) >> 3) << 3;
    hipLaunchKernelGGL(k_importance_views, dim3(grid), dim3(RB), 0, st, mk, W, H, tiles_x, tiles_pv, num_tiles, n, (const uint2*)ranges, sorted_splat,
                       (const float4*)splat2d, n_contrib, (unsigned long long*)score_sum, score_max, hits);
    return hipGetLastError();
}
