// render_common.h — device helpers shared by the composite kernels (render.hip, render_blocks.hip, render_tr.hip) and the replay passes (replay_walk.h).
#pragma once
#include "dvs_device.h"

#define RB 256

// Per-view backgrounds of a multi-view batch: FIRST kernel parameter of the composite kernels, read through the kernarg segment
// pointer (see DvsCams in dvs_device.h). One launch covers the tiles of all views: global tile t = view * tiles_per_view + tile.
struct ViewBg { float bg[DVS_MAX_VIEWS][4]; };
__device__ __forceinline__ float3 dvs_load_bg(int v) {
    typedef const __attribute__((address_space(4))) float* KF;
    const KF f = (KF)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)v * 4;
    return make_float3(f[0], f[1], f[2]);
}

static inline ViewBg make_view_bg(int n_views, const float* bgs /*[n_views][3]*/) {
    ViewBg b{};
    for (int v = 0; v < n_views && v < DVS_MAX_VIEWS; ++v) for (int k = 0; k < 3; ++k) b.bg[v][k] = bgs[3 * v + k];
    return b;
}

// blockIdx -> tile: consecutive workgroups land on different XCDs (b % 8), so give each XCD a
// contiguous band of tiles; neighbouring tiles share splats and therefore L2 lines.
__device__ __forceinline__ int tile_of_block(int b, int num_tiles) {
    const int chunk = (num_tiles + 7) >> 3;
    return (b & 7) * chunk + (b >> 3);
}
// ... and the grid that goes with it: eight bands of equal length (workgroups with tile_of_block() >= num_tiles have no tile)
static inline int replay_grid(int num_tiles) { return ((num_tiles + 7) >> 3) << 3; }

// The staged conic: exp(-0.5 (a dx^2 + c dy^2) - b dx dy) = exp2(cs.x dx^2 + cs.y dx dy + cs.z dy^2), cs = (CS_SQ a, CS_XY b, CS_SQ c)
constexpr float DVS_CS_SQ = -0.72134752044448170f;      // -0.5 log2(e)
constexpr float DVS_CS_XY = -1.4426950408889634f;       // -log2(e)

// The gfx950 packing swaps behind the composite backwards' cross-lane sums: two registers of per-lane partials become one.
// v_permlane32_swap: lanes 32-63 of A <-> lanes 0-31 of B; v_permlane16_swap: odd 16-lane rows of A <-> even rows of B.
__device__ __forceinline__ float swap32_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap16_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
