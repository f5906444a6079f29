// undistort.hip — a view taken through a SIMPLE_RADIAL / RADIAL / OPENCV camera -> the view of the pinhole camera with the same fx, fy,
// cx, cy and size (include/dvs_image.h: dvs_undistort_view, where the map and the blend are defined bit for bit; tests/undistort_ref.py
// restates them). A backward remap: every target pixel computes where it falls in the source and blends its four neighbours there.
//   * A lane owns FOUR consecutive target pixels of one row, a wavefront 256 of them, a workgroup (64 x 4) four rows; blockIdx.y runs
//     over groups of four rows — the shape of resample.hip. No LDS, no scratch; every output is written once by one lane.
//   * The map (fp32, about 40 operations) is computed ONCE per pixel and kept as an offset and two 5-bit weights; the planes and the
//     mask reuse it. The taps are byte gathers: neighbouring lanes read neighbouring source bytes (the map is smooth), so a wavefront's
//     256 pixels touch a handful of 128-byte lines per source row, which stay in L1 for the other taps and in L2 for the other rows.
//   * Where dst is on a 4-byte boundary and W is a multiple of 4 the four bytes of a plane leave as ONE dword store (a wavefront then
//     stores 256 contiguous bytes), otherwise as single bytes; the mask likewise as one 16-byte store or four floats. The choice is
//     uniform in a launch and the result does not depend on it.
//   * Invalid pixels are counted inside the wavefront — one ballot and popcount per owned pixel — and leave as ONE integer atomic per
//     wavefront that has any: the sum is exact in any order, so two calls return the same count.
// Compiled without contraction (EXACT): every fp32 operation below rounds on its own, in the order the header writes them.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "../../include/dvs_image.h"

namespace {
constexpr int UD_TX = 64, UD_TY = 4;                       // a workgroup: 4 wavefronts, each on 256 consecutive pixels of one row
constexpr int UD_MAX_SIDE = 65536;

struct Tap {                                               // the map of one target pixel
    uint32_t off;                                          // y0 * W + x0 (< 2^32 for sides up to 65536)
    uint32_t w;                                            // ax | ay << 5 | (x1 - x0) << 10 | (y1 - y0) << 11 | valid << 12; 0 when invalid
};

__device__ __forceinline__ Tap make_tap(const dvs_undistort_desc& d, int x, float v, float v2) {
    const float u = (((float)x + 0.5f) - d.cx) * d.ifx;
    const float u2 = u * u, uv = u * v, r2 = u2 + v2;
    const float rad = (d.k1 + d.k2 * r2) * r2;
    const float du = (u * rad + (2.0f * d.p1) * uv) + d.p2 * (r2 + 2.0f * u2);
    const float dv = (v * rad + (2.0f * d.p2) * uv) + d.p1 * (r2 + 2.0f * v2);
    const float xs = (d.fx * (u + du) + d.cx) - 0.5f, ys = (d.fy * (v + dv) + d.cy) - 0.5f;
    Tap t{0u, 0u};
    if (xs > -1.0f && xs < (float)d.width && ys > -1.0f && ys < (float)d.height) {     // (a NaN fails; |q| < 2^22 below)
        const int qx = (int)floorf(xs * 32.0f + 0.5f), qy = (int)floorf(ys * 32.0f + 0.5f);
        if (qx >= 0 && qx <= 32 * (d.width - 1) && qy >= 0 && qy <= 32 * (d.height - 1)) {
            const int x0 = qx >> 5, y0 = qy >> 5;
            t.off = (uint32_t)y0 * (uint32_t)d.width + (uint32_t)x0;
            t.w = (uint32_t)(qx & 31) | (uint32_t)(qy & 31) << 5 | (x0 + 1 < d.width ? 1u << 10 : 0u) | (y0 + 1 < d.height ? 1u << 11 : 0u) | 1u << 12;
        }
    }
    return t;
}

// the blend of one plane at one VALID tap (every address is inside the plane); scale = 1 for image bytes, 255 for mask bytes
__device__ __forceinline__ uint32_t blend(const uint8_t* __restrict__ s, Tap t, uint32_t W, uint32_t scale) {
    const uint32_t ax = t.w & 31u, ay = (t.w >> 5) & 31u;
    const size_t o00 = t.off, dx = (t.w >> 10) & 1u, dy = (t.w >> 11) & 1u ? (size_t)W : 0;
    const uint32_t s00 = s[o00] * scale, s01 = s[o00 + dx] * scale, s10 = s[o00 + dy] * scale, s11 = s[o00 + dy + dx] * scale;
    return ((32u - ax) * (32u - ay) * s00 + ax * (32u - ay) * s01 + (32u - ax) * ay * s10 + ax * ay * s11 + 512u) >> 10;
}

__global__ void __launch_bounds__(UD_TX * UD_TY)
k_undistort(const dvs_undistort_desc d, int planes, const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask_src,
            uint8_t* __restrict__ dst, float* __restrict__ mask_dst, uint32_t* __restrict__ invalid_count, int vec_dst, int vec_mask) {
    const int W = d.width, H = d.height;
    const int y = (int)(blockIdx.y * UD_TY + threadIdx.y);                     // uniform in a wavefront
    if (y >= H) return;
    const int x0 = (int)(blockIdx.x * UD_TX + threadIdx.x) * 4;
    const int nout = min(4, W - x0);                                           // <= 0: a lane past the row; it still takes part in the ballots
    const float v = (((float)y + 0.5f) - d.cy) * d.ify, v2 = v * v;
    Tap t[4];
    uint32_t n_invalid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[j] = j < nout ? make_tap(d, x0 + j, v, v2) : Tap{0u, 0u};
        n_invalid += (uint32_t)__popcll(__ballot(j < nout && !(t[j].w >> 12)));
    }
    if (invalid_count && n_invalid && threadIdx.x == 0) atomicAdd(invalid_count, n_invalid);
    if (nout <= 0) return;
    const size_t P = (size_t)W * H, row = (size_t)y * W + x0;
    for (int p = 0; p < planes; ++p) {
        const uint8_t* __restrict__ s = src + (size_t)p * P;
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (t[j].w >> 12) ? blend(s, t[j], (uint32_t)W, 1u) : 0u;
        uint8_t* __restrict__ q = dst + (size_t)p * P + row;
        if (vec_dst) *reinterpret_cast<uint32_t*>(q) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;      // (W % 4 == 0: all four exist)
        else for (int j = 0; j < nout; ++j) q[j] = (uint8_t)o[j];
    }
    if (mask_dst) {
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool ok = (t[j].w >> 12) != 0;
            if (ok && mask_src) ok = blend(mask_src, t[j], (uint32_t)W, 255u) > 127u;
            m[j] = ok ? 1.0f : 0.0f;
        }
        float* __restrict__ q = mask_dst + row;
        if (vec_mask) *reinterpret_cast<float4*>(q) = make_float4(m[0], m[1], m[2], m[3]);
        else for (int j = 0; j < nout; ++j) q[j] = m[j];
    }
}
}  // namespace

extern "C" int dvs_undistort_desc_from_colmap(int model, const double* params, int width, int height, dvs_undistort_desc* out) {
    if (!params || !out || model < 2 || model > 4 || width < 1 || width > UD_MAX_SIDE || height < 1 || height > UD_MAX_SIDE) return DVS_ERR_INVALID;
    const int n = model == 2 ? 4 : model == 3 ? 5 : 8;
    for (int k = 0; k < n; ++k) if (!std::isfinite(params[k])) return DVS_ERR_INVALID;
    double fx, fy, cx, cy, c[4] = {0, 0, 0, 0};                                // c = k1, k2, p1, p2
    if (model == 4) { fx = params[0]; fy = params[1]; cx = params[2]; cy = params[3]; for (int k = 0; k < 4; ++k) c[k] = params[4 + k]; }
    else { fx = fy = params[0]; cx = params[1]; cy = params[2]; c[0] = params[3]; if (model == 3) c[1] = params[4]; }
    if (!(fx > 0) || !(fy > 0)) return DVS_ERR_INVALID;
    dvs_undistort_desc d{};
    d.width = width; d.height = height;
    d.fx = (float)fx; d.fy = (float)fy; d.cx = (float)cx; d.cy = (float)cy; d.ifx = (float)(1.0 / fx); d.ify = (float)(1.0 / fy);
    d.k1 = (float)c[0]; d.k2 = (float)c[1]; d.p1 = (float)c[2]; d.p2 = (float)c[3];
    for (float f : {d.fx, d.fy, d.cx, d.cy, d.ifx, d.ify, d.k1, d.k2, d.p1, d.p2}) if (!std::isfinite(f)) return DVS_ERR_INVALID;
    if (!(d.fx > 0.f) || !(d.fy > 0.f)) return DVS_ERR_INVALID;
    *out = d;
    return DVS_OK;
}

extern "C" int dvs_undistort_view(void* stream, const dvs_undistort_desc* desc, int planes, const uint8_t* src, const uint8_t* mask_src,
                                  uint8_t* dst, float* mask_dst, uint32_t* invalid_count) {
    if (!desc || !src || !dst || planes < 1 || planes > 4) return DVS_ERR_INVALID;
    const int W = desc->width, H = desc->height;
    if (W < 1 || W > UD_MAX_SIDE || H < 1 || H > UD_MAX_SIDE) return DVS_ERR_INVALID;
    const size_t bytes = (size_t)planes * W * H;
    const uintptr_t s = (uintptr_t)src, q = (uintptr_t)dst;
    if (q < s + bytes && s < q + bytes) return DVS_ERR_INVALID;                // dst overlaps src
    const int vec_dst = (q & 3u) == 0 && (W & 3) == 0, vec_mask = mask_dst && ((uintptr_t)mask_dst & 15u) == 0 && (W & 3) == 0;
    const dim3 grid((unsigned)(((W + 3) / 4 + UD_TX - 1) / UD_TX), (unsigned)((H + UD_TY - 1) / UD_TY));       // (grid.y <= 16384)
    hipLaunchKernelGGL(k_undistort, grid, dim3(UD_TX, UD_TY), 0, (hipStream_t)stream, *desc, planes, src, mask_src, dst, mask_dst, invalid_count,
                       vec_dst, vec_mask);
    return dvs_launch_status();
}
