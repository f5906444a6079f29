// resample.hip — box downsample of a batch of planar images by 2^k (include/dvs_train.h: dvs_downsample_views): the level targets and
// level masks of the trainer's coarse-to-fine schedule (resolutionSchedule). out(x, y) = mean of the source block
// [x f, x f + f) x [y f, y f + f); the W - (W/f) f rightmost columns and the matching bottom rows are not read.
//   * ONE launch covers all views (blockIdx.z = view; the views' pointers are a kernel argument, as in metrics.hip). A pure
//     streaming kernel: no LDS, no atomics, no scratch; every output is written once by one lane.
//   * A lane owns FOUR consecutive outputs of one output row, i.e. f rows of 4 f source elements: 4 / 8 / 16 / 32 bytes per row of
//     an 8-bit source, 16 .. 128 bytes of an fp32 one. Where the view allows it (source and destination 16-byte aligned, the widths
//     multiples of the vector) those are dword .. 16-byte loads and the four results leave as ONE 16-byte store — a wavefront then
//     stores 1 KiB of one output row, whole lines. Every other view (odd width, offset pointers) takes the scalar path: the same
//     lane-to-output mapping with element loads and stores. The choice is per view and uniform in a workgroup.
//   * The result is defined bit for bit and does not depend on the path: an 8-bit block is summed exactly in integers, then
//     ((float)sum * (1.0f / 255.0f)) * (1.0f / (f f)) — with f = 1 the expansion of the trainer's k_unpack_u8; an fp32 block is added in
//     fp32 in row-major order starting from its first value, then multiplied by 1.0f / (f f). Compiled without contraction (EXACT).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dvs_train.h"
#include "../../include/dvs_raster.h"
#include "dvs_device.h"

namespace {
struct DownsampleViews { dvs_downsample_view v[DVS_DOWNSAMPLE_MAX_VIEWS]; };       // 256 B of kernel arguments
constexpr int DS_TX = 64, DS_TY = 4;                                       // a workgroup: 4 wavefronts, each on 256 consecutive outputs of one output row

template <int N> struct Bytes;                                             // N source bytes of one lane and row, as the widest aligned loads
template <> struct Bytes<4> { uint32_t w[1]; };
template <> struct Bytes<8> { uint32_t w[2]; };
template <> struct Bytes<16> { uint32_t w[4]; };
template <> struct Bytes<32> { uint32_t w[8]; };

template <int N>
__device__ __forceinline__ Bytes<N> load_bytes(const uint8_t* p) {         // p aligned to min(N, 16)
    Bytes<N> b;
    if constexpr (N == 4) b.w[0] = *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (N == 8) { const uint2 v = *reinterpret_cast<const uint2*>(p); b.w[0] = v.x; b.w[1] = v.y; }
    else {
#pragma unroll
        for (int q = 0; q < N / 16; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[q];
            b.w[4 * q] = v.x; b.w[4 * q + 1] = v.y; b.w[4 * q + 2] = v.z; b.w[4 * q + 3] = v.w;
        }
    }
    return b;
}

template <bool U8, int F>
__global__ void __launch_bounds__(DS_TX * DS_TY)
k_downsample(const DownsampleViews views, int planes, int W, int H, int Wd, int Hd) {
    const dvs_downsample_view vw = views.v[blockIdx.z];
    const int x0 = (int)(blockIdx.x * DS_TX + threadIdx.x) * 4;
    const int row = (int)(blockIdx.y * DS_TY + threadIdx.y);               // plane * Hd + y
    if (x0 >= Wd || row >= planes * Hd) return;
    const int plane = row / Hd, y = row - plane * Hd;
    const size_t src0 = ((size_t)plane * H + (size_t)y * F) * W + (size_t)x0 * F;    // first source element of the lane
    float* __restrict__ dst = vw.dst + (size_t)row * Wd + x0;
    constexpr float inv = 1.0f / (float)(F * F);
    // 16-byte path of this view: every row of the source starts on a multiple of the load, every row of the destination on 16 bytes
    const bool vec = ((uintptr_t)vw.src & 15u) == 0 && ((uintptr_t)vw.dst & 15u) == 0 && (Wd & 3) == 0 && (W % (U8 ? 16 : 4)) == 0;
    float o[4];
    if (vec) {                                                             // (Wd % 4 == 0: all four outputs exist)
        if constexpr (U8) {
            const uint8_t* __restrict__ s = (const uint8_t*)vw.src + src0;
            uint32_t sum[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < F; ++r) {
                const Bytes<4 * F> b = load_bytes<4 * F>(s + (size_t)r * W);
#pragma unroll
                for (int e = 0; e < 4 * F; ++e) sum[e / F] += (b.w[e >> 2] >> (8 * (e & 3))) & 0xffu;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ((float)sum[j] * (1.0f / 255.0f)) * inv;
        } else {
            const float* __restrict__ s = (const float*)vw.src + src0;
#pragma unroll
            for (int r = 0; r < F; ++r) {
                float4 t[F];
#pragma unroll
                for (int q = 0; q < F; ++q) t[q] = reinterpret_cast<const float4*>(s + (size_t)r * W)[q];
                const float* tv = reinterpret_cast<const float*>(t);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < F; ++c) o[j] = (r == 0 && c == 0) ? tv[j * F + c] : o[j] + tv[j * F + c];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] *= inv;
        }
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        return;
    }
    const int nout = min(4, Wd - x0);
    for (int j = 0; j < nout; ++j) {
        if constexpr (U8) {
            const uint8_t* __restrict__ s = (const uint8_t*)vw.src + src0 + (size_t)j * F;
            uint32_t sum = 0u;
#pragma unroll
            for (int r = 0; r < F; ++r)
#pragma unroll
                for (int c = 0; c < F; ++c) sum += s[(size_t)r * W + c];
            dst[j] = ((float)sum * (1.0f / 255.0f)) * inv;
        } else {
            const float* __restrict__ s = (const float*)vw.src + src0 + (size_t)j * F;
            float acc = s[0];
#pragma unroll
            for (int r = 0; r < F; ++r)
#pragma unroll
                for (int c = 0; c < F; ++c)
                    if (r != 0 || c != 0) acc += s[(size_t)r * W + c];
            dst[j] = acc * inv;
        }
    }
}

template <bool U8>
void launch(int factor, dim3 grid, hipStream_t st, const DownsampleViews& a, int planes, int W, int H, int Wd, int Hd) {
    switch (factor) {
        case 1: hipLaunchKernelGGL((k_downsample<U8, 1>), grid, dim3(DS_TX, DS_TY), 0, st, a, planes, W, H, Wd, Hd); break;
        case 2: hipLaunchKernelGGL((k_downsample<U8, 2>), grid, dim3(DS_TX, DS_TY), 0, st, a, planes, W, H, Wd, Hd); break;
        case 4: hipLaunchKernelGGL((k_downsample<U8, 4>), grid, dim3(DS_TX, DS_TY), 0, st, a, planes, W, H, Wd, Hd); break;
        default: hipLaunchKernelGGL((k_downsample<U8, 8>), grid, dim3(DS_TX, DS_TY), 0, st, a, planes, W, H, Wd, Hd); break;
    }
}
}  // namespace

extern "C" int dvs_downsample_views(void* stream, const dvs_downsample_view* views, int n_views, int planes, int width, int height, int factor,
                                    int src_u8) {
    if (!views || n_views < 1 || n_views > DVS_DOWNSAMPLE_MAX_VIEWS || planes < 1 || width <= 0 || height <= 0) return DVS_ERR_INVALID;
    if (factor != 1 && factor != 2 && factor != 4 && factor != 8) return DVS_ERR_INVALID;
    const int Wd = width / factor, Hd = height / factor;
    if (Wd == 0 || Hd == 0) return DVS_ERR_INVALID;
    DownsampleViews a{};
    for (int v = 0; v < n_views; ++v) {
        if (!views[v].src || !views[v].dst) return DVS_ERR_INVALID;
        a.v[v] = views[v];
    }
    const int64_t rows = (int64_t)planes * Hd;
    if (rows > (int64_t)65535 * DS_TY) return DVS_ERR_INVALID;                 // (grid.y)
    const dim3 grid((unsigned)(((Wd + 3) / 4 + DS_TX - 1) / DS_TX), (unsigned)((rows + DS_TY - 1) / DS_TY), (unsigned)n_views);
    if (src_u8) launch<true>(factor, grid, (hipStream_t)stream, a, planes, width, height, Wd, Hd);
    else launch<false>(factor, grid, (hipStream_t)stream, a, planes, width, height, Wd, Hd);
    return dvs_launch_status();
}
