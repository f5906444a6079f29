// png_enc.hip — the parallel half of PNG encoding (include/dvs_image.h), the mirror image of png.hip: fp32 planes -> samples -> raw
// scanlines -> per row the cheapest of the five filters -> the filtered stream gstrain/png_io.hpp deflates on the host. Up to 16 views
// of one size in ONE launch (blockIdx.y = view). No scratch, no LDS, no inline assembly, plain vector stores; the one atomic is an
// integer add (the saturation count), so two calls return identical bytes and counts. After the float -> sample step (one fp32
// multiply and one rint: nothing to contract) it is integer arithmetic only. tests/png_enc_ref.py restates all of it.
//   Shape. In the encoding direction a filtered byte depends on RAW bytes only (its own, the one bpp to the left, the one above and
//   the one above that), so every byte of every row is independent: ONE wavefront per row, four rows per workgroup of 256 lanes, no
//   barrier. A lane owns 4 consecutive raw bytes per iteration and the wavefront strides over the row, so any width works.
//   Pass 1: a lane forms its 4 + bpp raw bytes of the row and of the row above from the fp32 planes (the samples are quantised again
//           rather than kept: a row may be longer than any buffer a workgroup could hold), applies all five filters and adds the five
//           costs; the wavefront sums them with integer adds across lanes (order-independent) and every lane picks the same filter.
//   Pass 2: the same bytes again, the chosen filter alone, stored.
//   Stores. Output rows start at y (1 + rowbytes) and so at any byte address. The groups of 4 bytes are laid on the OUTPUT's dwords,
//           not on the row's start: group g holds raw bytes 4 g - sh .. 4 g - sh + 3 with sh = (address of the row's first byte) & 3.
//           A group inside the row leaves as one dword store; the group that hangs over the row's start or end leaves byte by byte,
//           never a byte outside the row's own range: no lane writes what another row's wavefront owns.
//   A source row is read twice as itself and twice as the row above (by the next row's wavefront, which may sit in another workgroup);
//   the repeats are meant to come from the caches. Whether staging raw rows in LDS pays is not measured.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "../../include/dvs_image.h"

namespace {
constexpr int PE_BLOCK = 256, PE_ROWS = PE_BLOCK / 64;   // one wavefront per row

struct PeViews { const float* img[DVS_PNG_ENCODE_MAX_VIEWS]; uint8_t* out[DVS_PNG_ENCODE_MAX_VIEWS]; };

__host__ __device__ constexpr int pe_bpp(int kind) { return kind == DVS_PNG_KIND_RGB8 ? 3 : kind == DVS_PNG_KIND_GRAY8 ? 1 : 2; }

// raw byte i (0 <= i < rowbytes) of row y; bit 8 is set when the byte is the first of a sample that saturated (rint(x * scale) > M)
template <int KIND>
__device__ __forceinline__ uint32_t pe_raw(const float* __restrict__ img, size_t HW, int W, int y, int i, float scale) {
    constexpr float M = KIND == DVS_PNG_KIND_GRAY16 ? 65535.f : 255.f;
    size_t at;
    if (KIND == DVS_PNG_KIND_RGB8) { const int px = i / 3, c = i - 3 * px; at = (size_t)c * HW + (size_t)y * (size_t)W + (size_t)px; }
    else if (KIND == DVS_PNG_KIND_GRAY8) at = (size_t)y * (size_t)W + (size_t)i;
    else at = (size_t)y * (size_t)W + (size_t)(i >> 1);
    const float r = rintf(img[at] * scale);                          // the fp32 product, to nearest even; NaN stays NaN
    const uint32_t sat = r > M ? 0x100u : 0u;                        // (false for a NaN)
    const uint32_t s = r != r ? 0u : (uint32_t)fminf(M, fmaxf(0.f, r));
    if (KIND == DVS_PNG_KIND_GRAY16) return (i & 1) ? (s & 255u) : ((s >> 8) | sat);      // high byte first
    return s | sat;
}

// the 4 + BPP raw bytes from i0 - BPP on, of row y (cur, bit 8 as pe_raw leaves it) and of the row above (up); 0 outside the picture
template <int KIND, int BPP>
__device__ __forceinline__ void pe_fetch(const float* __restrict__ img, size_t HW, int W, int RB, int y, int i0, float scale,
                                         uint32_t (&cur)[4 + BPP], uint32_t (&up)[4 + BPP]) {
#pragma unroll
    for (int j = 0; j < 4 + BPP; ++j) {
        const int i = i0 - BPP + j;
        const bool in = i >= 0 && i < RB;
        cur[j] = in ? pe_raw<KIND>(img, HW, W, y, i, scale) : 0u;
        up[j] = in && y > 0 ? pe_raw<KIND>(img, HW, W, y - 1, i, scale) & 255u : 0u;
    }
}

// the decoder's predictor and tie order (png.hip)
__device__ __forceinline__ int pe_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}
__device__ __forceinline__ int pe_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int KIND>
__global__ void __launch_bounds__(PE_BLOCK) k_png_filter(const PeViews V, int W, int H, float scale, uint32_t* __restrict__ saturated) {
    constexpr int BPP = pe_bpp(KIND);
    const int lane = (int)threadIdx.x & 63, y = (int)blockIdx.x * PE_ROWS + ((int)threadIdx.x >> 6);
    if (y >= H) return;                                              // (a whole wavefront; there is no barrier below)
    const float* __restrict__ const img = V.img[blockIdx.y];
    const int RB = W * BPP;                                          // at most 196 500
    const size_t HW = (size_t)W * (size_t)H;
    uint8_t* const row = V.out[blockIdx.y] + (size_t)y * ((size_t)RB + 1);
    const int sh = (int)((uintptr_t)(row + 1) & 3u);
    const int groups = (RB + sh + 3) >> 2;
    // pass 1: the five costs of the row, and the samples that saturated
    int cost[5] = {0, 0, 0, 0, 0};
    int nsat = 0;
    for (int g = lane; g < groups; g += 64) {
        const int i0 = 4 * g - sh;
        uint32_t cur[4 + BPP], up[4 + BPP];
        pe_fetch<KIND, BPP>(img, HW, W, RB, y, i0, scale, cur, up);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= 0 && i0 + k < RB) {
                const int x = (int)(cur[BPP + k] & 255u), a = (int)(cur[k] & 255u), b = (int)up[BPP + k], c = (int)up[k];
                nsat += (int)(cur[BPP + k] >> 8);
                const int pred[5] = {0, a, b, (a + b) >> 1, pe_paeth(a, b, c)};
#pragma unroll
                for (int f = 0; f < 5; ++f) {
                    const int v = (x - pred[f]) & 255;
                    cost[f] += v < 128 ? v : 256 - v;
                }
            }
        }
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) cost[f] = pe_wave_sum(cost[f]);
    nsat = pe_wave_sum(nsat);
    int ft = 0;
#pragma unroll
    for (int f = 1; f < 5; ++f) if (cost[f] < cost[ft]) ft = f;      // the smallest cost, on a tie the smallest f
    if (lane == 0) {
        if (saturated && nsat) atomicAdd(saturated + blockIdx.y, (uint32_t)nsat);
        row[0] = (uint8_t)ft;
    }
    // pass 2: the chosen filter
    for (int g = lane; g < groups; g += 64) {
        const int i0 = 4 * g - sh;
        uint32_t cur[4 + BPP], up[4 + BPP];
        pe_fetch<KIND, BPP>(img, HW, W, RB, y, i0, scale, cur, up);
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = (int)(cur[BPP + k] & 255u), a = (int)(cur[k] & 255u), b = (int)up[BPP + k], c = (int)up[k];
            const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? pe_paeth(a, b, c) : 0;
            o[k] = (uint32_t)(x - pred) & 255u;
        }
        uint8_t* const dst = row + 1 + i0;                           // on a 4-byte boundary by the choice of sh
        if (i0 >= 0 && i0 + 3 < RB) *reinterpret_cast<uint32_t*>(dst) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (i0 + k >= 0 && i0 + k < RB) dst[k] = (uint8_t)o[k];
        }
    }
}

bool pe_shape_ok(int kind, int width, int height) {
    if (kind != DVS_PNG_KIND_RGB8 && kind != DVS_PNG_KIND_GRAY8 && kind != DVS_PNG_KIND_GRAY16) return false;
    return width >= 1 && height >= 1 && width <= 65500 && height <= 65500;
}
}  // namespace

extern "C" size_t dvs_png_encode_bytes(int kind, int width, int height) {
    if (!pe_shape_ok(kind, width, height)) return 0;
    return (size_t)height * (1 + (size_t)width * (size_t)pe_bpp(kind));
}

extern "C" int dvs_png_encode_views(void* stream, int kind, int width, int height, float scale, const float* const* images,
                                    uint8_t* const* filtered, uint32_t* saturated, int n_views) {
    if (!images || !filtered || n_views < 1 || n_views > DVS_PNG_ENCODE_MAX_VIEWS || !pe_shape_ok(kind, width, height)) return DVS_ERR_INVALID;
    if (!std::isfinite(scale) || !(scale > 0.f)) return DVS_ERR_INVALID;
    PeViews V{};
    for (int v = 0; v < n_views; ++v) {
        if (!images[v] || !filtered[v] || ((uintptr_t)images[v] & 3u)) return DVS_ERR_INVALID;
        V.img[v] = images[v]; V.out[v] = filtered[v];
    }
    const dim3 grid((unsigned)((height + PE_ROWS - 1) / PE_ROWS), (unsigned)n_views);
    hipStream_t st = (hipStream_t)stream;
    if (kind == DVS_PNG_KIND_RGB8) hipLaunchKernelGGL(k_png_filter<DVS_PNG_KIND_RGB8>, grid, dim3(PE_BLOCK), 0, st, V, width, height, scale, saturated);
    else if (kind == DVS_PNG_KIND_GRAY8) hipLaunchKernelGGL(k_png_filter<DVS_PNG_KIND_GRAY8>, grid, dim3(PE_BLOCK), 0, st, V, width, height, scale, saturated);
    else hipLaunchKernelGGL(k_png_filter<DVS_PNG_KIND_GRAY16>, grid, dim3(PE_BLOCK), 0, st, V, width, height, scale, saturated);
    return dvs_launch_status();
}
