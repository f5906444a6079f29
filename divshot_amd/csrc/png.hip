// png.hip — the parallel half of PNG decoding (include/dvs_image.h): filtered scanlines -> unfiltered in place (k_png_unfilter), then
// samples -> planar 8-bit RGB and alpha (k_png_expand); and the mask rule (k_mask_combine). No scratch, no atomics, no inline assembly,
// plain vector stores; integer arithmetic only, so no compiler flag can change a result. tests/png_ref.py restates all of it.
//
// Unfiltering. A byte depends on its left, upper and upper-left neighbours at distance bpp, so the bytes of an anti-diagonal are
// independent: ONE workgroup of DVS_PNG_BAND = 512 lanes walks the picture as a skewed wavefront, lane r on row y0 + r of a band of 512
// rows. At step s lane r undoes chunk s - r of its row, a chunk being CH = 8 pixels (4 at bpp 6 and 8: 8 to 32 bytes, a multiple of 4);
// the row above finished that chunk one step earlier, which is all a chunk needs. Steps per band = chunks per row + rows - 1 instead of
// their product: 1920x1080 RGB8 takes 2 * (240 + 511) + (240 + 55) = 1797 steps of 24 bytes per lane, one barrier each.
//   State: a lane keeps the last bpp bytes it produced (the next chunk's `a`) and the last bpp bytes it read from above (the next
//   chunk's `c`) in registers. The rows exchange chunks through LDS: row q holds PN_STEPS + 1 chunks — chunk 0 is the carry, the last
//   chunk of the stage before, chunks 1..PN_STEPS the stage's own — and lane r at step t reads chunk t of the row above and its own
//   chunk t + 1, which it overwrites with the result. LDS row 0 is the last row of the band before (zeros above the picture), re-read
//   from global memory, where that band's result already is: a band starts from the finished row, nothing else is carried over.
//   Stages: global memory is touched only between stages of PN_STEPS = 4 steps, by all lanes together: the parallelogram of the next
//   4 chunks of every row comes in with consecutive lanes on consecutive dwords of a row (a lane walking its own row would put 64 cache
//   lines under every load), and the finished one leaves the same way. Rows start at any byte address (stride = 1 + rowbytes), so a
//   dword that lies inside the row moves as one unaligned 4-byte access and a dword across its end byte by byte: never a byte outside
//   the row's own range, so no lane writes what another row's lane owns.
//   Why 8 pixels per barrier: a step costs one barrier of 8 waves plus a dependent LDS round trip (about 50 cycles issue-to-use each
//   way) whatever the chunk, and the per-byte arithmetic (about 20 integer instructions, the five filters computed and selected without
//   a branch since the rows of a band differ in theirs) is serial inside a chunk: 8 pixels make the arithmetic the larger part of a
//   step without stretching the pipeline's fill and drain (rows - 1 steps per band) beyond the 240 chunks of a 1920-pixel row.
//   Bank check, by the rule of each instruction: the LDS row stride is (PN_STEPS + 1) * CH + 4 bytes = 11, 21, 31 or 41 dwords, odd,
//   so the 32 lanes of a half access 32 distinct banks with ds_read_b32 / ds_write_b32 at the same chunk offset.
//   512 lanes, not 1024: two waves per SIMD keep the vector issue busy across the other's LDS wait; four would double the drain.
// Expansion: one lane per pixel, the palette in LDS; bytes leave as single-byte stores, consecutive lanes on consecutive bytes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "../../include/dvs_image.h"

namespace {
constexpr int PN_BAND = DVS_PNG_BAND;
constexpr int PN_STEPS = 4;

__host__ __device__ inline int pn_channels(int type) { return type == 0 || type == 3 ? 1 : type == 4 ? 2 : type == 2 ? 3 : type == 6 ? 4 : 0; }

template <int BPP>
__global__ void __launch_bounds__(PN_BAND) k_png_unfilter(uint8_t* buf, int H, int rowbytes) {
    constexpr int CH = (BPP <= 4 ? 8 : 4) * BPP, CW = CH / 4, S = PN_STEPS;
    constexpr int LROW = (S + 1) * CH + 4, LW = LROW / 4;            // bytes / dwords of an LDS row
    __shared__ uint32_t lds[(PN_BAND + 1) * LW];
    const int tid = threadIdx.x;
    const size_t stride = (size_t)rowbytes + 1;
    const int NC = (rowbytes + CH - 1) / CH;
    for (int y0 = 0; y0 < H; y0 += PN_BAND) {
        const int Rb = min(PN_BAND, H - y0);
        const bool mine = tid < Rb;
        int ft = mine ? (int)buf[(size_t)(y0 + tid) * stride] : 0;
        if (ft > 4) ft = 0;                                          // (the host half refuses such files)
        uint32_t a_tail[BPP], c_tail[BPP];
#pragma unroll
        for (int k = 0; k < BPP; ++k) { a_tail[k] = 0u; c_tail[k] = 0u; }
        const int steps = NC + Rb - 1, stages = (steps + S - 1) / S;
        for (int st = 0; st < stages; ++st) {
            const int s0 = st * S;
            // 1. in: LDS row q = 1..Rb is picture row y0 + q - 1, its chunks 1..S; LDS row 0 is row y0 - 1, chunks 0..S (it has no carry).
            //    Dword w of LDS row q (w >= CW for q >= 1) is byte column CH * (s0 - (q - 1)) + 4 w - CH of its picture row.
            for (int idx = tid; idx < (Rb + 1) * (S + 1) * CW; idx += PN_BAND) {
                const int q = idx / ((S + 1) * CW), w = idx - q * ((S + 1) * CW);
                if (q > 0 && w < CW) continue;
                const int y = y0 + q - 1, col = CH * (s0 - (q - 1)) + 4 * w - CH;
                uint32_t v = 0u;
                if (y >= 0 && col + 3 >= 0 && col < rowbytes) {
                    const uint8_t* const src = buf + (size_t)y * stride + 1 + col;       // (col < 0 only with col = -4 * k: then col + 3 < 0)
                    if (col + 3 < rowbytes) memcpy(&v, src, 4);
                    else for (int k = 0; k < 4; ++k) if (col + k < rowbytes) v |= (uint32_t)src[k] << (8 * k);
                }
                lds[q * LW + w] = v;
            }
            __syncthreads();
            // 2. S steps of the wavefront
            for (int t = 0; t < S; ++t) {
                const int ci = s0 + t - tid;                         // the chunk of its row this lane undoes now
                if (mine && ci >= 0 && ci < NC) {
                    const uint32_t* const up = lds + tid * LW + t * CW;
                    uint32_t* const cur = lds + (tid + 1) * LW + (t + 1) * CW;
                    uint32_t uw[CW], xw[CW], ow[CW];
#pragma unroll
                    for (int k = 0; k < CW; ++k) { uw[k] = up[k]; xw[k] = cur[k]; ow[k] = 0u; }
                    uint32_t o[CH];
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
                        const int x = (int)((xw[k >> 2] >> (8 * (k & 3))) & 255u);
                        const int b = (int)((uw[k >> 2] >> (8 * (k & 3))) & 255u);
                        const int a = (int)(k >= BPP ? o[k >= BPP ? k - BPP : 0] : a_tail[k < BPP ? k : 0]);
                        const int c = (int)(k >= BPP ? (uw[(k >= BPP ? k - BPP : 0) >> 2] >> (8 * ((k >= BPP ? k - BPP : 0) & 3))) & 255u : c_tail[k < BPP ? k : 0]);
                        const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                        const int paeth = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
                        const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
                        o[k] = (uint32_t)(x + pred) & 255u;
                        ow[k >> 2] |= o[k] << (8 * (k & 3));
                    }
#pragma unroll
                    for (int k = 0; k < CW; ++k) cur[k] = ow[k];
#pragma unroll
                    for (int k = 0; k < BPP; ++k) {
                        a_tail[k] = o[CH - BPP + k];
                        c_tail[k] = (uw[(CH - BPP + k) >> 2] >> (8 * ((CH - BPP + k) & 3))) & 255u;
                    }
                }
                __syncthreads();
            }
            // 3. out: chunks 1..S of rows 1..Rb, the bytes inside the row only; then chunk S becomes the next stage's carry
            for (int idx = tid; idx < Rb * S * CW; idx += PN_BAND) {
                const int r = idx / (S * CW), w = CW + idx - r * (S * CW);
                const int col = CH * (s0 - r) + 4 * w - CH;
                if (col + 3 < 0 || col >= rowbytes) continue;
                const uint32_t v = lds[(r + 1) * LW + w];
                uint8_t* const dst = buf + (size_t)(y0 + r) * stride + 1 + col;
                if (col + 3 < rowbytes) memcpy(dst, &v, 4);
                else for (int k = 0; k < 4; ++k) if (col + k < rowbytes) dst[k] = (uint8_t)(v >> (8 * k));
            }
            for (int idx = tid; idx < Rb * CW; idx += PN_BAND) {
                const int r = idx / CW, w = idx - r * CW;
                lds[(r + 1) * LW + w] = lds[(r + 1) * LW + S * CW + w];
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) k_png_expand(const dvs_png_desc D, const uint8_t* __restrict__ buf, uint8_t* __restrict__ rgb, uint8_t* __restrict__ alpha) {
    __shared__ uint32_t pal[256];
    {
        const uint8_t* const e = D.palette[threadIdx.x];
        pal[threadIdx.x] = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    }
    __syncthreads();
    const int W = D.width, depth = D.bit_depth, type = D.color_type, ch = pn_channels(type);
    const size_t P = (size_t)W * (size_t)D.height, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t y = i / (size_t)W;
    const int x = (int)(i - y * (size_t)W);
    const size_t rowbytes = ((size_t)W * (size_t)ch * (size_t)depth + 7) / 8;
    const uint8_t* const row = buf + y * (rowbytes + 1) + 1;
    uint32_t s[4] = {0u, 0u, 0u, 0u};                               // the samples at the file's depth
    if (depth < 8) {
        const size_t bit = (size_t)x * (size_t)depth;
        s[0] = ((uint32_t)row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);      // packed MSB first
    } else if (depth == 8) {
        for (int c = 0; c < ch; ++c) s[c] = row[(size_t)x * ch + c];
    } else {
        for (int c = 0; c < ch; ++c) { const uint8_t* const p = row + ((size_t)x * ch + c) * 2; s[c] = (uint32_t)p[0] << 8 | (uint32_t)p[1]; }
    }
    uint32_t v[4];                                                  // the samples as bytes
    const uint32_t scale = depth == 1 ? 255u : depth == 2 ? 85u : depth == 4 ? 17u : 1u;
    for (int c = 0; c < 4; ++c) v[c] = depth == 16 ? (s[c] * 255u + 32895u) >> 16 : s[c] * scale;
    uint32_t R, G, B, A = 255u;
    const uint32_t mask = depth == 16 ? 0xFFFFu : (1u << depth) - 1u;
    if (type == 3) { const uint32_t e = pal[s[0]]; R = e & 255u; G = (e >> 8) & 255u; B = (e >> 16) & 255u; A = e >> 24; }
    else if (type == 0 || type == 4) {
        R = G = B = v[0];
        if (type == 4) A = v[1];
        else if (D.has_key) A = s[0] == ((uint32_t)D.key[0] & mask) ? 0u : 255u;
    } else {
        R = v[0]; G = v[1]; B = v[2];
        if (type == 6) A = v[3];
        else if (D.has_key) A = (s[0] == ((uint32_t)D.key[0] & mask) && s[1] == ((uint32_t)D.key[1] & mask) && s[2] == ((uint32_t)D.key[2] & mask)) ? 0u : 255u;
    }
    rgb[i] = (uint8_t)R; rgb[P + i] = (uint8_t)G; rgb[2 * P + i] = (uint8_t)B;
    if (alpha) alpha[i] = (uint8_t)A;
}

__global__ void __launch_bounds__(256) k_mask_combine(size_t n, const uint8_t* gray, const uint8_t* alpha, const uint8_t* other, uint8_t* out_u8, float* out_f32) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool m = gray ? gray[i] > 127 : true;
    if (alpha) m = m && alpha[i] > 127;
    if (other) m = m && other[i] != 0;
    if (out_u8) out_u8[i] = m ? 1 : 0;
    if (out_f32) out_f32[i] = m ? 1.f : 0.f;
}

bool png_pair_ok(int type, int depth) {
    if (type == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    if (type == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    if (type == 2 || type == 4 || type == 6) return depth == 8 || depth == 16;
    return false;
}
bool png_desc_ok(const dvs_png_desc& d) {
    if (d.width < 1 || d.height < 1 || d.width > 65500 || d.height > 65500) return false;
    if (!png_pair_ok(d.color_type, d.bit_depth)) return false;
    if (d.has_key != 0 && d.has_key != 1) return false;
    if (d.has_key && d.color_type != 0 && d.color_type != 2) return false;      // a key beside an alpha channel or a palette
    return true;
}
size_t png_row_bytes(const dvs_png_desc& d) { return ((size_t)d.width * (size_t)pn_channels(d.color_type) * (size_t)d.bit_depth + 7) / 8; }
}  // namespace

extern "C" int dvs_png_band_rows(void) { return PN_BAND; }

extern "C" size_t dvs_png_filtered_bytes(const dvs_png_desc* desc) {
    if (!desc || !png_desc_ok(*desc)) return 0;
    return (size_t)desc->height * (1 + png_row_bytes(*desc));
}

extern "C" int dvs_png_reconstruct(void* stream, const dvs_png_desc* desc, uint8_t* filtered, uint8_t* rgb, uint8_t* alpha) {
    if (!desc || !filtered || !rgb || !png_desc_ok(*desc)) return DVS_ERR_INVALID;
    const int rowbytes = (int)png_row_bytes(*desc), H = desc->height;          // at most 65500 * 8
    const int bpp = std::max(1, pn_channels(desc->color_type) * desc->bit_depth / 8);
    hipStream_t st = (hipStream_t)stream;
    switch (bpp) {
        case 1: hipLaunchKernelGGL(k_png_unfilter<1>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        case 2: hipLaunchKernelGGL(k_png_unfilter<2>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        case 3: hipLaunchKernelGGL(k_png_unfilter<3>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        case 4: hipLaunchKernelGGL(k_png_unfilter<4>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        case 6: hipLaunchKernelGGL(k_png_unfilter<6>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        case 8: hipLaunchKernelGGL(k_png_unfilter<8>, dim3(1), dim3(PN_BAND), 0, st, filtered, H, rowbytes); break;
        default: return DVS_ERR_INVALID;
    }
    const size_t P = (size_t)desc->width * (size_t)H;
    hipLaunchKernelGGL(k_png_expand, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, *desc, filtered, rgb, alpha);
    return dvs_launch_status();
}

extern "C" int dvs_mask_combine(void* stream, size_t n, const uint8_t* gray, const uint8_t* alpha, const uint8_t* other, uint8_t* out_u8, float* out_f32) {
    if ((!gray && !other) || n == 0 || (!out_u8 && !out_f32) || (n + 255) / 256 > 0x7FFFFFFFull) return DVS_ERR_INVALID;
    hipLaunchKernelGGL(k_mask_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, gray, alpha, other, out_u8, out_f32);
    return dvs_launch_status();
}
