// replay_walk.h — the one walk over the lists A7 (k_render_fwd) saved, for the passes that replay it: depth.hip, importance.hip, sky.hip's rows.
//
// One 256-thread workgroup per (view, tile) as in render.hip; pixel t of the tile is (t & 15, t >> 4). Pixel p walks the tile's list
// entries [range.x, range.x + n_contrib(p)) in order: n_contrib is the 1-based list position of the pixel's last contributor, so the
// forward's early stop needs no test. The entries go through LDS in batches of RB, one gathered record per lane, then broadcast reads.
// alpha is formed by the operations of k_render_fwd, in its order (explicit fused multiply-adds where it has them; the including files
// are compiled without contraction), so every take decision is the forward's own. A pass supplies what it stages beyond the record,
// what it accumulates per taken pair and what it writes; DESIGN.md, "Replay passes".
#pragma once
#include "render_common.h"

struct ReplayTile {
    bool none;          // this workgroup has no tile: return, the whole workgroup, before any barrier
    int view, px, py;
    bool inside;        // the pixel is in the image
    size_t pix, gpix;   // py W + px; view W H + pix (n_contrib, final_T and the [views,H,W] outputs)
    uint2 range;        // the tile's entries in sorted_splat
    uint32_t total;
};
__device__ __forceinline__ ReplayTile replay_tile(int W, int H, int tiles_x, int tiles_per_view, int num_tiles, const uint2* __restrict__ ranges) {
    ReplayTile r{};
    const int tile_g = tile_of_block(blockIdx.x, num_tiles);
    r.none = tile_g >= num_tiles;
    if (r.none) return r;
    r.view = tile_g / tiles_per_view;
    const int tile = tile_g - r.view * tiles_per_view, t = threadIdx.x;
    r.px = tile % tiles_x * DVS_TILE + (t & 15); r.py = tile / tiles_x * DVS_TILE + (t >> 4);
    r.inside = r.px < W && r.py < H;
    r.pix = (size_t)r.py * W + r.px; r.gpix = (size_t)r.view * W * H + r.pix;
    r.range = ranges[tile_g]; r.total = r.range.y - r.range.x;
    return r;
}
// entries a pixel walks (none unless `walks`); never more than the tile's list holds
__device__ __forceinline__ uint32_t replay_mine(const ReplayTile& r, bool walks, const uint32_t* __restrict__ n_contrib) {
    return walks ? min(n_contrib[r.gpix], r.total) : 0u;
}

struct ReplayLds {      // the first member of each pass's LDS struct
    float4 a[RB];       // mean x, mean y, cs.x, cs.y        (cs as in render.hip, DVS_CS_SQ / DVS_CS_XY)
    float4 b[RB];       // cs.z, opacity, the pass's own (depth.hip: view-space z), -
    uint32_t wmax[RB / 64];
};
// entries the workgroup stages: the largest count among its pixels; *wm <- the largest among the wave's (wave-uniform). One barrier.
__device__ __forceinline__ uint32_t replay_need(ReplayLds& L, uint32_t mine, uint32_t* wm_out) {
    uint32_t wm = mine;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, d, 64));
    if ((threadIdx.x & 63) == 0) L.wmax[threadIdx.x >> 6] = wm;
    __syncthreads();
    *wm_out = wm;
    return max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]));
}
// of a batch of cnt entries at base, those a pixel (or wave) with `count` entries walks
__device__ __forceinline__ uint32_t replay_stop(uint32_t count, uint32_t base, uint32_t cnt) { return count > base ? min(cnt, count - base) : 0u; }
// r0, r1: the first two float4 of the entry's splat2d record
__device__ __forceinline__ void replay_stage(ReplayLds& L, int t, float4 r0, float4 r1, float b_z) {
    L.a[t] = make_float4(r0.x, r0.y, DVS_CS_SQ * r0.z, DVS_CS_XY * r0.w);
    L.b[t] = make_float4(DVS_CS_SQ * r1.x, r1.y, b_z, 0.f);
}

struct ReplayEntry {
    float dx, dy, p2, G, oa, alpha;     // mean - pixel | log2 of the Gaussian, the Gaussian, opacity * G, ... capped
    bool take;                          // the forward's two skip rules passed (the caller ANDs in its j < stop)
};
__device__ __forceinline__ ReplayEntry replay_entry(float4 A, float4 B, float pxf, float pyf) {
    ReplayEntry e;
    e.dx = A.x - pxf; e.dy = A.y - pyf;
    e.p2 = __builtin_fmaf(B.x * e.dy, e.dy, __builtin_fmaf(A.w, e.dy, A.z * e.dx) * e.dx);
    e.G = __builtin_amdgcn_exp2f(e.p2);
    e.oa = B.y * e.G;
    e.alpha = fminf(DVS_ALPHA_MAX, e.oa);
    e.take = !(e.p2 > 0.f || e.alpha < DVS_ALPHA_MIN);
    return e;
}

// Wave reductions, all 64 lanes active, the result wave-uniform. (a DPP source outside the 16-lane row reads 0)
template <int CTRL, class T> __device__ __forceinline__ T wave_dpp(T v) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// every lane of a 16-lane row <- the row's fold: lane ^ 1, lane ^ 2, then the mirrored 4 and 8 lanes
template <class T, class F> __device__ __forceinline__ T wave_rows(T v, F op) {
    v = op(v, wave_dpp<0xB1>(v));           // quad_perm [1,0,3,2]
    v = op(v, wave_dpp<0x4E>(v));           // quad_perm [2,3,0,1]
    v = op(v, wave_dpp<0x141>(v));          // row_half_mirror
    v = op(v, wave_dpp<0x140>(v));          // row_mirror
    return v;
}
template <class T> __device__ __forceinline__ T wave_row(T v, int lane) { return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v = wave_rows(v, [](uint32_t x, uint32_t y) { return x + y; });
    return wave_row(v, 0) + wave_row(v, 16) + wave_row(v, 32) + wave_row(v, 48);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = wave_rows(v, [](uint32_t x, uint32_t y) { return max(x, y); });
    return max(max(wave_row(v, 0), wave_row(v, 16)), max(wave_row(v, 32), wave_row(v, 48)));
}
__device__ __forceinline__ float wave_sum_f32(float v) {
    v = wave_rows(v, [](float x, float y) { return x + y; });
    return (wave_row(v, 0) + wave_row(v, 16)) + (wave_row(v, 32) + wave_row(v, 48));
}

// Per-entry accumulators: lane 0 of wave w stores the wave's value for entry j in slot[w][j]; after the batch thread t folds entry t's column
__device__ __forceinline__ uint32_t replay_fold_sum(const uint32_t (&s)[RB / 64][RB], int t) { return s[0][t] + s[1][t] + s[2][t] + s[3][t]; }
__device__ __forceinline__ uint32_t replay_fold_max(const uint32_t (&s)[RB / 64][RB], int t) { return max(max(s[0][t], s[1][t]), max(s[2][t], s[3][t])); }
__device__ __forceinline__ float replay_fold_sum(const float (&s)[RB / 64][RB], int t) { return (s[0][t] + s[1][t]) + (s[2][t] + s[3][t]); }
// id = view * n + splat, a sorted_splat value: does it name a splat of this view?
__device__ __forceinline__ bool replay_owns(uint32_t id, int view, int n) { return id - (uint32_t)view * (uint32_t)n < (uint32_t)n; }
