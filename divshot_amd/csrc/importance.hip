// importance.hip — per-splat blend weight of the last forward (dvs_raster_importance_views), for gfx950.
//
// A replay pass (replay_walk.h) that accumulates per ENTRY: w = alpha T of every taken (pixel, entry) pair goes to the entry's splat as
//   score_sum += q, q = (uint32_t)rintf(w 2^24)    an integer on purpose: integer adds commute, so the sums are bit-reproducible for any
//                                                  order of the reductions and atomics below, from run to run and across ranks
//   score_max  = max(score_max, bits(w))           w >= 0: the unsigned order of the bits is the order of the floats
//   hits      += 1
// Per entry a wave first asks whether any of its 64 pixels took it (ballot): most (wave, entry) pairs of a 3-sigma rectangle are
// empty and cost nothing more. For the others the hit count is the ballot's popcount, sum / max are reduced over the wave and lane 0
// stores the three into the wave's own LDS slot of the entry: no LDS atomics. After the batch thread j folds the four waves' slots of
// entry j and issues at most one non-returning global atomic per statistic, none for a zero.
// q <= 0.99 2^24, so a wave's 64 and a tile's 256 pixels fit a uint32; the sum over tiles and views is a uint64.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "replay_walk.h"

struct __attribute__((aligned(16))) ImportanceLds {
    ReplayLds walk;
    uint32_t sum[RB / 64][RB], max[RB / 64][RB], hits[RB / 64][RB];       // [wave][entry of the batch]
};
struct ImportanceMasks { const float* m[DVS_MAX_VIEWS]; };                 // per view: [H,W] or null

__global__ void __launch_bounds__(RB)
k_importance_views(ImportanceMasks masks, int W, int H, int tiles_x, int tiles_per_view, int num_tiles, int n, const uint2* __restrict__ ranges,
                   const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const uint32_t* __restrict__ n_contrib,
                   unsigned long long* __restrict__ score_sum /*[n]*/, uint32_t* __restrict__ score_max /*[n] or null*/,
                   uint32_t* __restrict__ hits /*[n] or null*/) {
    __shared__ ImportanceLds L;
    const ReplayTile rt = replay_tile(W, H, tiles_x, tiles_per_view, num_tiles, ranges);
    if (rt.none) return;
    const int t = threadIdx.x, wave = t >> 6;
    const float* const mask = masks.m[rt.view];
    // a pixel outside the image or masked out walks nothing
    const uint32_t mine = replay_mine(rt, rt.inside && !(mask && mask[rt.pix] == 0.f), n_contrib);
    uint32_t wm;
    const uint32_t need = replay_need(L.walk, mine, &wm);

    const float pxf = (float)rt.px, pyf = (float)rt.py;
    float T = 1.0f;
    for (uint32_t base = 0; base < need; base += RB) {
        const uint32_t cnt = min((uint32_t)RB, need - base);
        uint32_t id = 0;
        if ((uint32_t)t < cnt) {
            id = sorted_splat[rt.range.x + base + t];                      // batch-wide value: view * n + splat, the record's index
            replay_stage(L.walk, t, splat2d[4 * (size_t)id], splat2d[4 * (size_t)id + 1], 0.f);
#pragma unroll
            for (int w = 0; w < RB / 64; ++w) { L.sum[w][t] = 0u; L.max[w][t] = 0u; L.hits[w][t] = 0u; }
        }
        __syncthreads();
        const uint32_t stop = replay_stop(mine, base, cnt);
        const uint32_t wave_stop = replay_stop(wm, base, cnt);             // wave-uniform: the cross-lane steps below run with all 64 lanes
        for (uint32_t j = 0; j < wave_stop; ++j) {
            const ReplayEntry e = replay_entry(L.walk.a[j], L.walk.b[j], pxf, pyf);
            const bool take = j < stop && e.take;
            const uint64_t took = __ballot(take);
            if (took == 0ull) continue;
            const float aT = take ? e.alpha * T : 0.f;
            T = T - aT;
            const uint32_t s = wave_sum_u32((uint32_t)rintf(aT * 16777216.0f));
            const uint32_t m = wave_max_u32(__float_as_uint(aT));
            if ((t & 63) == 0) { L.sum[wave][j] = s; L.max[wave][j] = m; L.hits[wave][j] = (uint32_t)__popcll(took); }
        }
        __syncthreads();
        if ((uint32_t)t < cnt && replay_owns(id, rt.view, n)) {
            const uint32_t splat = id - (uint32_t)rt.view * (uint32_t)n;
            const uint32_t s = replay_fold_sum(L.sum, t);
            if (s != 0u) {                                                 // (a taken pair has q >= 6: s == 0 means nobody took the entry)
                (void)atomicAdd(&score_sum[splat], (unsigned long long)s);
                if (score_max) (void)atomicMax(&score_max[splat], replay_fold_max(L.max, t));
                if (hits) (void)atomicAdd(&hits[splat], replay_fold_sum(L.hits, t));
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
    hipLaunchKernelGGL(k_importance_views, dim3(replay_grid(num_tiles)), dim3(RB), 0, st, mk, W, H, tiles_x, tiles_pv, num_tiles, n, (const uint2*)ranges, sorted_splat,
                       (const float4*)splat2d, n_contrib, (unsigned long long*)score_sum, score_max, hits);
    return hipGetLastError();
}
