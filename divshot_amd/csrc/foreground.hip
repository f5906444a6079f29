// foreground.hip — where every splat's blend weight of the last forward landed, on foreground or on background pixels
// (dvs_raster_foreground_views), and the plan that keeps the splats the foreground voted for (dvs_foreground_plan), for gfx950.
//
// The votes are a replay pass (replay_walk.h) in the form of importance.hip: one walk, two accumulators. Every taken (pixel, entry)
// pair gives q = (uint32_t)rintf(alpha T 2^24), importance.hip's quantisation on purpose, and q goes to the entry's splat as
//   fg_sum += q    when the pixel's fg value is nonzero, or the view has no fg plane
//   bg_sum += q    otherwise
// so that fg_sum + bg_sum is, bit for bit, the score_sum of the importance pass under masks = valid_masks. A pixel whose valid value
// is 0 walks nothing. Per entry a wave first asks whether any of its 64 pixels took it (ballot); for the others the foreground lanes'
// q and the background lanes' q are reduced over the wave and lane 0 stores the two into the wave's own LDS slot of the entry: no
// LDS atomics. After the batch thread j folds the four waves' slots of entry j and issues at most one non-returning global atomic per
// non-zero sum. q <= 0.99 2^24, so a wave's 64 and a tile's 256 pixels fit a uint32; the sum over tiles and views is a uint64.
//
// The plan is three launches in the shape of dvs_region_plan (region.hip): flags + block sums | one workgroup scans the block sums
// (scan.hip) | offsets. Integers only.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "replay_walk.h"
#include "block_scan.h"
#include "../../include/dvs_train.h"

struct __attribute__((aligned(16))) ForegroundLds {
    ReplayLds walk;
    uint32_t fg[RB / 64][RB], bg[RB / 64][RB];                             // [wave][entry of the batch]
};
struct ForegroundMasks { const float* fg[DVS_MAX_VIEWS]; const float* valid[DVS_MAX_VIEWS]; };   // per view: [H,W] or null

__global__ void __launch_bounds__(RB)
k_foreground_views(ForegroundMasks masks, int W, int H, int tiles_x, int tiles_per_view, int num_tiles, int n, const uint2* __restrict__ ranges,
                   const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const uint32_t* __restrict__ n_contrib,
                   unsigned long long* __restrict__ fg_sum /*[n]*/, unsigned long long* __restrict__ bg_sum /*[n]*/) {
    __shared__ ForegroundLds L;
    const ReplayTile rt = replay_tile(W, H, tiles_x, tiles_per_view, num_tiles, ranges);
    if (rt.none) return;
    const int t = threadIdx.x, wave = t >> 6;
    const float* const fgm = masks.fg[rt.view];
    const float* const valid = masks.valid[rt.view];
    // a pixel outside the image or without a source (valid == 0) walks nothing; the planes are read inside the image only
    const bool walks = rt.inside && !(valid && valid[rt.pix] == 0.f);
    const bool is_fg = !(walks && fgm && fgm[rt.pix] == 0.f);
    const uint32_t mine = replay_mine(rt, walks, n_contrib);
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
            for (int w = 0; w < RB / 64; ++w) { L.fg[w][t] = 0u; L.bg[w][t] = 0u; }
        }
        __syncthreads();
        const uint32_t stop = replay_stop(mine, base, cnt);
        const uint32_t wave_stop = replay_stop(wm, base, cnt);             // wave-uniform: the cross-lane steps below run with all 64 lanes
        for (uint32_t j = 0; j < wave_stop; ++j) {
            const ReplayEntry e = replay_entry(L.walk.a[j], L.walk.b[j], pxf, pyf);
            const bool take = j < stop && e.take;
            if (__ballot(take) == 0ull) continue;
            const float aT = take ? e.alpha * T : 0.f;
            T = T - aT;
            const uint32_t q = (uint32_t)rintf(aT * 16777216.0f);          // 0 for a lane that did not take the entry
            const uint32_t sf = wave_sum_u32(is_fg ? q : 0u);
            const uint32_t sb = wave_sum_u32(is_fg ? 0u : q);
            if ((t & 63) == 0) { L.fg[wave][j] = sf; L.bg[wave][j] = sb; }
        }
        __syncthreads();
        if ((uint32_t)t < cnt && replay_owns(id, rt.view, n)) {
            const uint32_t splat = id - (uint32_t)rt.view * (uint32_t)n;
            const uint32_t sf = replay_fold_sum(L.fg, t), sb = replay_fold_sum(L.bg, t);
            if (sf != 0u) (void)atomicAdd(&fg_sum[splat], (unsigned long long)sf);
            if (sb != 0u) (void)atomicAdd(&bg_sum[splat], (unsigned long long)sb);
        }
        // (the next batch's staging writes only what this thread has just read, and the barrier after it orders the rest)
    }
}

hipError_t dvs_launch_foreground_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges,
                                       const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, const float* const* fg_masks,
                                       const float* const* valid_masks, uint64_t* fg_sum, uint64_t* bg_sum) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0 || n <= 0) return hipSuccess;
    if (n_views > DVS_MAX_VIEWS) return hipErrorInvalidValue;
    ForegroundMasks mk{};
    for (int v = 0; v < n_views; ++v) { mk.fg[v] = fg_masks ? fg_masks[v] : nullptr; mk.valid[v] = valid_masks ? valid_masks[v] : nullptr; }
    hipLaunchKernelGGL(k_foreground_views, dim3(replay_grid(num_tiles)), dim3(RB), 0, st, mk, W, H, tiles_x, tiles_pv, num_tiles, n, (const uint2*)ranges, sorted_splat,
                       (const float4*)splat2d, n_contrib, (unsigned long long*)fg_sum, (unsigned long long*)bg_sum);
    return hipGetLastError();
}

// ---- the plan: splat i stays iff fg[i] > 0 and fg[i] (100 - percent) >= bg[i] percent -------------------------------------------------
// Both products are formed in 128 bits (low word, __umul64hi), so the rule holds for every 64-bit input.
__device__ __forceinline__ bool foreground_keeps(unsigned long long fg, unsigned long long bg, unsigned long long percent) {
    const unsigned long long mf = 100ull - percent;
    const unsigned long long f_lo = fg * mf, f_hi = __umul64hi(fg, mf), b_lo = bg * percent, b_hi = __umul64hi(bg, percent);
    return fg > 0ull && (f_hi > b_hi || (f_hi == b_hi && f_lo >= b_lo));
}
__global__ void __launch_bounds__(DB)
k_foreground_flags(int n, const unsigned long long* __restrict__ fg, const unsigned long long* __restrict__ bg, int percent, uint8_t* __restrict__ action,
                   uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    const bool keep = i < n && foreground_keeps(fg[i], bg[i], (unsigned long long)percent);
    if (i < n) action[i] = (uint8_t)(keep ? DVS_DENSIFY_KEEP : DVS_DENSIFY_PRUNE);
    uint32_t tot;
    (void)dvs_block_excl_scan(keep ? 1u : 0u, tmp, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(DB)
k_foreground_offsets(int n, const uint8_t* __restrict__ action, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    const bool keep = i < n && action[i] == DVS_DENSIFY_KEEP;
    uint32_t tot;
    const uint32_t ex = dvs_block_excl_scan(keep ? 1u : 0u, tmp, &tot);
    if (i < n) offsets[i] = block_offsets[blockIdx.x] + ex;
}

hipError_t dvs_launch_foreground_plan(hipStream_t st, int n, const uint64_t* fg, const uint64_t* bg, int percent, uint8_t* action, uint32_t* offsets,
                                      uint32_t* scratch, uint64_t* new_count) {
    const uint32_t nb = (uint32_t)(((int64_t)n + DB - 1) / DB);
    hipLaunchKernelGGL(k_foreground_flags, dim3(nb), dim3(DB), 0, st, n, (const unsigned long long*)fg, (const unsigned long long*)bg, percent, action, scratch);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "new_count is the scan's 64-bit total");
    const hipError_t e = dvs_launch_block_sums_excl(st, scratch, nb, (unsigned long long*)new_count);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_foreground_offsets, dim3(nb), dim3(DB), 0, st, n, (const uint8_t*)action, (const uint32_t*)scratch, offsets);
    return hipGetLastError();
}
