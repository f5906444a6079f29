// region.hip — the focus region (include/dvs_region.h): which splats an oriented box keeps (dvs_region_plan) and which pixels' rays cross
// it (dvs_region_mask_views), for gfx950. Both are streaming passes: 12 B read and 5 B written per splat (plus the byte the offsets
// pass reads back), 4 to 8 B per pixel. The region is a kernel parameter passed by value: its 18 floats are wave-uniform and are read
// through the kernarg segment into SGPRs. No atomics, no contraction (the Makefile compiles this file with -ffp-contract=off: the
// local coordinate is the three explicit fused multiply-adds the header writes down, and nothing else is fused).
//
//   k_region_flags    one thread per splat. A full 256-splat block of a 16-byte aligned position array is 192 float4: threads 0..191
//                     load one each (coalesced 16-byte words) into LDS and every thread reads its three floats back with stride 3
//                     (odd: no bank conflict). The last, partial block and a misaligned array take the scalar path. Writes
//                     action[i] and the block's kept count.
//   (scan.hip)        dvs_launch_block_sums_excl: one workgroup over the block counts, block offsets in place, the total to *new_count.
//   k_region_offsets  offsets[i] = the block's offset + the exclusive scan of the kept flags inside the block, from action[].
//   k_region_mask     one thread per pixel (scalar path) or per four consecutive pixels (16-byte path), blockIdx.y = the view, so that
//                     what a view needs (its ray matrix, its origin in the box, its two pointers) is wave-uniform and comes from the
//                     kernarg segment by index. The ray is pixel_ray.h's, the one the sky lookup uses.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "../../include/dvs_region.h"
#include "../../include/dvs_train.h"
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "block_scan.h"
#include "pixel_ray.h"

__device__ __forceinline__ bool region_inside(const dvs_region& r, float x, float y, float z) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = __builtin_fmaf(r.w2b[4 * k + 2], z, __builtin_fmaf(r.w2b[4 * k + 1], y, __builtin_fmaf(r.w2b[4 * k], x, r.w2b[4 * k + 3])));
        in = in && c >= r.lo[k] && c <= r.hi[k];                // (a NaN fails both)
    }
    return in;
}

__global__ void __launch_bounds__(DB)
k_region_flags(int n, const float* __restrict__ pos, dvs_region region, int aligned, uint8_t* __restrict__ action, uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t tmp[DB / 64];
    __shared__ float4 stage[3 * DB / 4];
    const int i = blockIdx.x * DB + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    if (aligned && (int64_t)blockIdx.x * DB + DB <= (int64_t)n) {       // workgroup-uniform: the barrier is taken by all or by none
        if (threadIdx.x < 3 * DB / 4) stage[threadIdx.x] = ((const float4*)(pos + 3 * (int64_t)blockIdx.x * DB))[threadIdx.x];
        __syncthreads();
        const float* s = (const float*)stage + 3 * threadIdx.x;
        x = s[0]; y = s[1]; z = s[2];
    } else if (i < n) {
        x = pos[3 * (int64_t)i]; y = pos[3 * (int64_t)i + 1]; z = pos[3 * (int64_t)i + 2];
    }
    const bool keep = i < n && region_inside(region, x, y, z);
    if (i < n) action[i] = (uint8_t)(keep ? DVS_DENSIFY_KEEP : DVS_DENSIFY_PRUNE);
    uint32_t tot;
    (void)dvs_block_excl_scan(keep ? 1u : 0u, tmp, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(DB)
k_region_offsets(int n, const uint8_t* __restrict__ action, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    const bool keep = i < n && action[i] == DVS_DENSIFY_KEEP;
    uint32_t tot;
    const uint32_t ex = dvs_block_excl_scan(keep ? 1u : 0u, tmp, &tot);
    if (i < n) offsets[i] = block_offsets[blockIdx.x] + ex;
}

// What k_region_mask reads by view index through the kernarg segment: MUST stay its first parameter, with the ray matrices first
// (pixel_ray_load). m[v][9..11] = the view's origin in box-local coordinates.
struct RegionMaskArgs {
    PixelRays rays;
    const float* in[DVS_REGION_MAX_VIEWS];
    float* out[DVS_REGION_MAX_VIEWS];
};
static_assert(DVS_REGION_MAX_VIEWS == DVS_MAX_VIEWS, "one table size for the views of a launch");

__device__ __forceinline__ float region_hit(const PixelRay& ray, const float (&o)[3], const dvs_region& r, int x, int y, int W, int H) {
    float dx, dy, dz;
    pixel_ray_dir(ray, x, y, W, H, dx, dy, dz);
    float tmin = -INFINITY, tmax = INFINITY;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float l = __builtin_fmaf(r.w2b[4 * k + 2], dz, __builtin_fmaf(r.w2b[4 * k + 1], dy, r.w2b[4 * k] * dx));
        if (l == 0.f) {
            ok = ok && o[k] >= r.lo[k] && o[k] <= r.hi[k];
        } else {
            const float t0 = (r.lo[k] - o[k]) / l, t1 = (r.hi[k] - o[k]) / l;
            tmin = fmaxf(tmin, fminf(t0, t1)); tmax = fminf(tmax, fmaxf(t0, t1));
        }
    }
    return ok && tmin <= tmax && tmax >= 0.f ? 1.0f : 0.0f;
}

template <bool VEC>
__global__ void __launch_bounds__(DB)
k_region_mask(RegionMaskArgs args /* MUST stay the first parameter */, dvs_region region, int W, int H) {
    (void)args;
    const int view = blockIdx.y;
    const PixelRay ray = pixel_ray_load(view);
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = dvs_karg<float>(offsetof(RegionMaskArgs, rays) + ((size_t)view * 12 + 9 + k) * sizeof(float));
    const float* const in = dvs_karg<const float*>(offsetof(RegionMaskArgs, in) + (size_t)view * sizeof(void*));
    float* const out = dvs_karg<float*>(offsetof(RegionMaskArgs, out) + (size_t)view * sizeof(void*));
    const size_t P = (size_t)W * H;
    const size_t t = (size_t)blockIdx.x * DB + threadIdx.x;
    if (VEC) {                                                   // P % 4 == 0, in / out 16-byte aligned
        if (t >= P / 4) return;
        float h[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t p = 4 * t + q;
            const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
            h[q] = region_hit(ray, o, region, x, y, W, H);
        }
        float4 v = make_float4(h[0], h[1], h[2], h[3]);
        if (in) { const float4 m = ((const float4*)in)[t]; v = make_float4(m.x * h[0], m.y * h[1], m.z * h[2], m.w * h[3]); }
        ((float4*)out)[t] = v;
    } else {
        if (t >= P) return;
        const int y = (int)(t / (size_t)W), x = (int)(t - (size_t)y * W);
        const float h = region_hit(ray, o, region, x, y, W, H);
        out[t] = in ? in[t] * h : h;
    }
}

extern "C" {
int dvs_region_from_trs(const float* pos, const float* rot, const float* scale, const float* lo, const float* hi, dvs_region* out, float* b2w) {
    if (!pos || !rot || !scale || !lo || !hi || !out || !b2w) return DVS_ERR_INVALID;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(scale[k]) || scale[k] == 0.f) return DVS_ERR_INVALID;
        if (!std::isfinite(pos[k]) || !std::isfinite(rot[k]) || !std::isfinite(lo[k]) || !std::isfinite(hi[k]) || lo[k] > hi[k]) return DVS_ERR_INVALID;
    }
    // glm::quat(vec3 euler): the half-angle products of R = Rz Ry Rx, then glm::toMat4 (transform.cpp:129)
    const double cx = std::cos(0.5 * (double)rot[0]), sx = std::sin(0.5 * (double)rot[0]), cy = std::cos(0.5 * (double)rot[1]),
                 sy = std::sin(0.5 * (double)rot[1]), cz = std::cos(0.5 * (double)rot[2]), sz = std::sin(0.5 * (double)rot[2]);
    const double w = cx * cy * cz + sx * sy * sz, x = sx * cy * cz - cx * sy * sz, y = cx * sy * cz + sx * cy * sz, z = cx * cy * sz - sx * sy * cz;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) b2w[4 * r + c] = (float)(R[r][c] * (double)scale[c]);           // F = T R S
        b2w[4 * r + 3] = pos[r];
        b2w[12 + r] = 0.f;
    }
    b2w[15] = 1.f;
    for (int k = 0; k < 3; ++k) {                                           // F^-1 = S^-1 R^T T^-1
        double t = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double m = R[c][k] / (double)scale[k];
            out->w2b[4 * k + c] = (float)m;
            t -= m * (double)pos[c];
        }
        out->w2b[4 * k + 3] = (float)t;
        out->lo[k] = lo[k]; out->hi[k] = hi[k];
    }
    return DVS_OK;
}

int dvs_region_plan(void* stream, int n, const float* pos, const dvs_region* region, uint8_t* action, uint32_t* offsets, uint32_t* scratch,
                    uint64_t* new_count) {
    if (n <= 0 || !pos || !region || !action || !offsets || !scratch || !new_count || ((uintptr_t)new_count & 7u)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)(((int64_t)n + DB - 1) / DB);
    hipLaunchKernelGGL(k_region_flags, dim3(nb), dim3(DB), 0, st, n, pos, *region, ((uintptr_t)pos & 15u) ? 0 : 1, action, scratch);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "new_count is the scan's 64-bit total");
    if (dvs_launch_block_sums_excl(st, scratch, nb, (unsigned long long*)new_count) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_region_offsets, dim3(nb), dim3(DB), 0, st, n, (const uint8_t*)action, (const uint32_t*)scratch, offsets);
    return dvs_launch_status();
}

int dvs_region_mask_views(void* stream, const dvs_region_mask_view* views, int n_views, int width, int height, const dvs_region* region) {
    if (!views || !region || n_views < 1 || n_views > DVS_REGION_MAX_VIEWS || width <= 0 || height <= 0) return DVS_ERR_INVALID;
    RegionMaskArgs a{};
    bool vec = ((size_t)width * height) % 4 == 0;
    for (int v = 0; v < n_views; ++v) {
        const dvs_region_mask_view& w = views[v];
        if (!w.out || w.cam.width != width || w.cam.height != height || !dvs_pixel_ray_matrix(&w.cam, a.rays.m[v])) return DVS_ERR_INVALID;
        for (int k = 0; k < 3; ++k) {
            double o = (double)region->w2b[4 * k + 3];
            for (int c = 0; c < 3; ++c) o += (double)region->w2b[4 * k + c] * (double)w.cam.campos[c];
            a.rays.m[v][9 + k] = (float)o;
        }
        a.in[v] = w.in_mask; a.out[v] = w.out;
        vec = vec && !(((uintptr_t)w.in_mask | (uintptr_t)w.out) & 15u);
    }
    const size_t P = (size_t)width * height, work = vec ? P / 4 : P;
    const dim3 grid((unsigned)((work + DB - 1) / DB), (unsigned)n_views);
    if (vec) hipLaunchKernelGGL(k_region_mask<true>, grid, dim3(DB), 0, (hipStream_t)stream, a, *region, width, height);
    else hipLaunchKernelGGL(k_region_mask<false>, grid, dim3(DB), 0, (hipStream_t)stream, a, *region, width, height);
    return dvs_launch_status();
}
}
