// jpeg_enc.hip — the parallel half of baseline JPEG encoding (include/dvs_image.h): planar fp32 RGB -> quantised DCT coefficients in the
// layout of dvs_jpeg_desc / gsjpeg::Frame, up to 16 views of one size in ONE launch (blockIdx.z = view), no scratch, no atomics, no
// inline assembly, plain vector stores. The result is defined bit for bit in the header and restated in tests/jpeg_enc_ref.py; after
// the float -> byte step (one fp32 multiply and one rint: nothing to contract) it is integer arithmetic only.
//   A workgroup of 256 lanes owns a rectangle of JE_TBX x JE_TBY = 8 x 2 MCUs, as the decoder does: 64 hs x 16 vs pixels.
//   (1) pixels: a lane takes vs rows x 4 columns at a time: per row and colour plane ONE 16-byte load where the
//       image pointer and the width allow (VEC: pointer on a 16-byte boundary, W a multiple of 4, the four columns inside the image),
//       element loads with the coordinates clamped to the last column / row otherwise (that clamp IS the padding of partial MCUs), float
//       -> byte, colour conversion, and at 4:2:0 the 2 x 2 box means of its own eight pixels; Y / Cb / Cr bytes go into the component's
//       sample plane in LDS. Chroma is averaged inside the MCU, so a workgroup reads no pixel outside its rectangle: no ring.   | barrier
//   (2) the blocks of the rectangle (16 hs vs luma + 16 + 16 chroma = 48 or 96) go through the transform 32 at a time, 8 lanes per
//       block, each block in a 72-int slot of LDS:
//         lane r reads row r of the block from the sample plane (8 bytes), level shift, row pass, writes row[r][0..7]     | barrier
//         lane r reads column r (row[0..7][r]), column pass in registers, writes F[0..7][r] in place                      | barrier
//         lane r reads row r (F[r][0..7]), quantises, packs 8 int16 and stores them as ONE 16-byte store                  | barrier
//       Bank check, by the rule of each instruction, NOT measured — the slot geometry is the decoder's (jpeg.hip), so its reasoning
//       carries over: the column accesses (ds_read_b32 / ds_write_b32 at int address 72 slot + 8 k + r) fall on 32 distinct banks
//       per 32-lane half thanks to the 8-int pad; the row accesses (two 16-byte accesses per lane at 72 slot + 8 r) are not
//       conflict-free (2-way on the b128 writes, up to 3-way on the b128 reads). The 8-byte sample-plane reads of a batch come from
//       4 block rows of one plane row set (stride 64 or 128 bytes between rows r of a block, 8 bytes between blocks): lanes r and
//       r + 4 (hs = 1: stride 64 B = 16 banks -> r, r + 2, r + 4, r + 6) of a block share banks; not measured either.
//       The products are v_mad_i32_i24: |s| <= 128, |T| < 2^12, |row| < 2^17, so both factors fit 24 bits.
//       F leaves the column pass in 1/64 units (six fractional bits go into the quantiser: no double rounding). Division:
//       (|F| + 32 q) / (64 q) = n / q with n = (|F| + 32 q) >> 6 < 2^12 (nested floor divisions), and n / q for q in 1..255 is
//       (n * (2^20 / q + 1)) >> 20 in 32 bits, exact for every such n and q (tests/test_jpeg_write_format.py checks all of them; the
//       GPU parity test at quality 1..100 is the check of the kernel itself); the reciprocals are computed once per workgroup into LDS.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "../../include/dvs_image.h"

namespace {
constexpr int JE_BLOCK = 256;
constexpr int JE_TBX = 8, JE_TBY = 2;                    // MCUs a workgroup owns
constexpr int JE_SLOTS = JE_BLOCK / 8;                   // blocks in the transform at a time
constexpr int JE_SLOT = 72;                              // ints per slot: 64 + 8 of padding
constexpr int JE_LW = JE_TBX * 16, JE_LH = JE_TBY * 16;  // luma plane of the rectangle at 2x2
constexpr int JE_CW = JE_TBX * 8, JE_CH = JE_TBY * 8;    // chroma plane
constexpr int JE_ROW_SHIFT = 6, JE_COL_SHIFT = 14;       // 13 - 7 and 13 + 7 - 6: seven fractional bits between the passes, six kept in F
constexpr int JE_CMAX = 1023;

// T[u][x] = round(2^13 * C(u) / 2 * cos((2x + 1) u pi / 16)): the decoder's table (jpeg.hip); the forward pass is its transpose
constexpr int kT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                          {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                          {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                          {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                          {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

struct JeViews { const float* img[DVS_JPEG_ENCODE_MAX_VIEWS]; int16_t* coef[DVS_JPEG_ENCODE_MAX_VIEWS]; };

// the rule of the trainer's 8-bit training views (k_pack_u8): rint to nearest even of the fp32 product, clamped; NaN -> 0
__device__ __forceinline__ int je_byte(float x) { return x != x ? 0 : (int)fminf(255.f, fmaxf(0.f, rintf(x * 255.f))); }
__device__ __forceinline__ int je_quant(int F, int q, uint32_t recip) {
    const int a = F < 0 ? -F : F;
    const int c = min((int)(((uint32_t)((a + (q << 5)) >> 6) * recip) >> 20), JE_CMAX);
    return F < 0 ? -c : c;
}

template <bool VEC>
__global__ void __launch_bounds__(JE_BLOCK)
k_jpeg_encode(const dvs_jpeg_desc D, const JeViews V) {
    __shared__ __align__(16) int ws[JE_SLOTS * JE_SLOT];
    __shared__ __align__(16) uint16_t quant[3 * 64];
    __shared__ __align__(16) uint32_t recip[3 * 64];
    __shared__ __align__(16) uint8_t luma[JE_LH * JE_LW];
    __shared__ __align__(16) uint8_t chroma[2][JE_CH * JE_CW];
    const int tid = threadIdx.x;
    if (tid < 3 * 64) {
        const uint32_t q = D.quant[tid >> 6][tid & 63];              // 1..255, checked on the host
        quant[tid] = (uint16_t)q;
        recip[tid] = (1u << 20) / q + 1u;
    }
    const float* __restrict__ const img = V.img[blockIdx.z];
    int16_t* __restrict__ const coef = V.coef[blockIdx.z];
    const int hs = D.hs, vs = D.vs, W = D.width, H = D.height;
    const size_t HW = (size_t)H * (size_t)W;
    // (1) pixels: vs rows x 4 columns per unit
    const int tw = 64 * hs, th = 16 * vs;
    const int units_x = tw / 4, units = units_x * (th / vs);
    const int x0 = (int)blockIdx.x * tw, y0 = (int)blockIdx.y * th;
    const int lstride = hs == 2 ? JE_LW : JE_CW;                     // the luma plane is 64 bytes wide at 1x1
    for (int unit = tid; unit < units; unit += JE_BLOCK) {
        const int uy = unit / units_x, tx = (unit - uy * units_x) * 4, ty = uy * vs;
        const int X0 = x0 + tx;
        int cb[4], cr[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j >= vs) break;
            const int Y = min(y0 + ty + j, H - 1);
            const float* const row = img + (size_t)Y * (size_t)W;
            float r[4], g[4], b[4];
            if (VEC && X0 + 3 < W) {
                const float4 a = *reinterpret_cast<const float4*>(row + X0);
                const float4 c = *reinterpret_cast<const float4*>(row + HW + X0);
                const float4 e = *reinterpret_cast<const float4*>(row + 2 * HW + X0);
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
                g[0] = c.x; g[1] = c.y; g[2] = c.z; g[3] = c.w;
                b[0] = e.x; b[1] = e.y; b[2] = e.z; b[3] = e.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int X = min(X0 + k, W - 1);
                    r[k] = row[X]; g[k] = row[HW + X]; b[k] = row[2 * HW + X];
                }
            }
            uint32_t yy = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int R = je_byte(r[k]), G = je_byte(g[k]), B = je_byte(b[k]);
                yy |= (uint32_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) << (8 * k);
                const int pb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16;
                const int pr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
                cb[k] = j == 0 ? pb : cb[k] + pb;
                cr[k] = j == 0 ? pr : cr[k] + pr;
            }
            *reinterpret_cast<uint32_t*>(luma + (ty + j) * lstride + tx) = yy;
        }
        if (hs == 2) {                                               // 2 x 2 box means: two chroma samples of one row
            uint8_t* const pb = chroma[0] + uy * JE_CW + (tx >> 1);
            uint8_t* const pr = chroma[1] + uy * JE_CW + (tx >> 1);
            *reinterpret_cast<uint16_t*>(pb) = (uint16_t)(((cb[0] + cb[1] + 2) >> 2) | (((cb[2] + cb[3] + 2) >> 2) << 8));
            *reinterpret_cast<uint16_t*>(pr) = (uint16_t)(((cr[0] + cr[1] + 2) >> 2) | (((cr[2] + cr[3] + 2) >> 2) << 8));
        } else {
            *reinterpret_cast<uint32_t*>(chroma[0] + ty * JE_CW + tx) = (uint32_t)(cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24));
            *reinterpret_cast<uint32_t*>(chroma[1] + ty * JE_CW + tx) = (uint32_t)(cr[0] | (cr[1] << 8) | (cr[2] << 16) | (cr[3] << 24));
        }
    }
    __syncthreads();
    // (2) blocks
    const int lbx = JE_TBX * hs, lby = JE_TBY * vs;                  // luma blocks of the rectangle
    const int n_luma = lbx * lby, n_chroma = JE_TBX * JE_TBY, total = n_luma + 2 * n_chroma;
    const int slot = tid >> 3, r = tid & 7;
    int* const w = ws + slot * JE_SLOT;
    for (int base = 0; base < total; base += JE_SLOTS) {
        const int id = base + slot;
        int c = 0, lx, ly, bx, by;
        if (id < n_luma) { ly = id / lbx; lx = id - ly * lbx; bx = (int)blockIdx.x * lbx + lx; by = (int)blockIdx.y * lby + ly; }
        else {
            int k = id - n_luma;
            c = 1;
            if (k >= n_chroma) { k -= n_chroma; c = 2; }
            ly = k / JE_TBX; lx = k - ly * JE_TBX; bx = (int)blockIdx.x * JE_TBX + lx; by = (int)blockIdx.y * JE_TBY + ly;
        }
        const int bw = c ? D.blocks_w[1] : D.blocks_w[0], bh = c ? D.blocks_h[1] : D.blocks_h[0];
        const bool live = id < total && bx < bw && by < bh;          // a block past the MCU grid is not computed and not stored
        if (live) {                                                  // rows: lane r owns row y = r
            const uint8_t* const plane = c == 0 ? luma : chroma[c - 1];
            const int stride = c == 0 ? lstride : JE_CW;
            const uint2 p = *reinterpret_cast<const uint2*>(plane + (ly * 8 + r) * stride + lx * 8);
            int s[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) s[x] = (int)(((x < 4 ? p.x : p.y) >> (8 * (x & 3))) & 0xFFu) - 128;
            int o[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int acc = 1 << (JE_ROW_SHIFT - 1);
#pragma unroll
                for (int x = 0; x < 8; ++x) acc += __mul24(kT[u][x], s[x]);
                o[u] = acc >> JE_ROW_SHIFT;
            }
            *reinterpret_cast<int4*>(w + r * 8) = make_int4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<int4*>(w + r * 8 + 4) = make_int4(o[4], o[5], o[6], o[7]);
        }
        __syncthreads();
        if (live) {                                                  // columns: lane r owns column u = r
            int col[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) col[k] = w[k * 8 + r];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                int acc = 1 << (JE_COL_SHIFT - 1);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += __mul24(kT[v][k], col[k]);
                w[v * 8 + r] = acc >> JE_COL_SHIFT;
            }
        }
        __syncthreads();
        if (live) {                                                  // lane r owns row v = r of the block: quantise, one 16-byte store
            const int4 a = *reinterpret_cast<const int4*>(w + r * 8), b = *reinterpret_cast<const int4*>(w + r * 8 + 4);
            const int F[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i0 = c * 64 + r * 8 + 2 * k;
                const int lo = je_quant(F[2 * k], (int)quant[i0], recip[i0]), hi = je_quant(F[2 * k + 1], (int)quant[i0 + 1], recip[i0 + 1]);
                out[k] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
            }
            const uint64_t off = c == 0 ? D.offset[0] : c == 1 ? D.offset[1] : D.offset[2];
            *reinterpret_cast<uint4*>(coef + off + ((uint64_t)by * (uint64_t)bw + (uint64_t)bx) * 64 + (uint64_t)r * 8) = make_uint4(out[0], out[1], out[2], out[3]);
        }
        __syncthreads();
    }
}

// what an encode accepts: three components, 1x1 or 2x2, the block counts of the size, offsets that are multiples of 8 and leave the
// components disjoint, quantisers a baseline stream can carry
bool encode_desc_ok(const dvs_jpeg_desc& d) {
    if (d.width < 1 || d.height < 1 || d.width > 65500 || d.height > 65500 || d.components != 3) return false;
    if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
    if (d.blocks_w[0] != mx * d.hs || d.blocks_h[0] != my * d.vs) return false;
    uint64_t lo[3], hi[3];
    for (int c = 0; c < 3; ++c) {
        if (c && (d.blocks_w[c] != mx || d.blocks_h[c] != my)) return false;
        if (d.offset[c] & 7u) return false;
        lo[c] = d.offset[c]; hi[c] = d.offset[c] + (uint64_t)d.blocks_w[c] * (uint64_t)d.blocks_h[c] * 64;
        for (int k = 0; k < c; ++k) if (lo[c] < hi[k] && lo[k] < hi[c]) return false;
        for (int k = 0; k < 64; ++k) if (d.quant[c][k] < 1 || d.quant[c][k] > 255) return false;
    }
    return true;
}

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
const uint8_t kAnnexK[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
}  // namespace

extern "C" int dvs_jpeg_encode_desc(int width, int height, int sampling, int quality, dvs_jpeg_desc* desc) {
    if (!desc || width < 1 || height < 1 || width > 65500 || height > 65500 || quality < 1 || quality > 100) return DVS_ERR_INVALID;
    if (sampling != DVS_JPEG_SAMPLING_420 && sampling != DVS_JPEG_SAMPLING_444) return DVS_ERR_INVALID;
    dvs_jpeg_desc d{};
    d.width = width; d.height = height; d.components = 3;
    d.hs = d.vs = sampling == DVS_JPEG_SAMPLING_420 ? 2 : 1;
    const int mx = (width + 8 * d.hs - 1) / (8 * d.hs), my = (height + 8 * d.vs - 1) / (8 * d.vs);
    uint64_t total = 0;
    for (int c = 0; c < 3; ++c) {
        d.blocks_w[c] = c ? mx : mx * d.hs; d.blocks_h[c] = c ? my : my * d.vs;
        d.offset[c] = total;
        total += (uint64_t)d.blocks_w[c] * (uint64_t)d.blocks_h[c] * 64;
    }
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;       // the IJG quality rule
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) {
            const int v = ((int)kAnnexK[c ? 1 : 0][k] * scale + 50) / 100;
            d.quant[c][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    *desc = d;
    return DVS_OK;
}

extern "C" size_t dvs_jpeg_encode_coef_count(const dvs_jpeg_desc* desc) {
    if (!desc || !encode_desc_ok(*desc)) return 0;
    uint64_t end = 0;
    for (int c = 0; c < 3; ++c) {
        const uint64_t e = desc->offset[c] + (uint64_t)desc->blocks_w[c] * (uint64_t)desc->blocks_h[c] * 64;
        if (e > end) end = e;
    }
    return (size_t)end;
}

extern "C" int dvs_jpeg_encode_views(void* stream, const dvs_jpeg_desc* desc, const float* const* images, int16_t* const* coef, int n_views) {
    if (!desc || !images || !coef || n_views < 1 || n_views > DVS_JPEG_ENCODE_MAX_VIEWS || !encode_desc_ok(*desc)) return DVS_ERR_INVALID;
    JeViews V{};
    bool vec = desc->width % 4 == 0;
    for (int v = 0; v < n_views; ++v) {
        if (!images[v] || !coef[v] || ((uintptr_t)coef[v] & 15u) || ((uintptr_t)images[v] & 3u)) return DVS_ERR_INVALID;
        V.img[v] = images[v]; V.coef[v] = coef[v];
        vec = vec && ((uintptr_t)images[v] & 15u) == 0;
    }
    const int mx = desc->blocks_w[0] / desc->hs, my = desc->blocks_h[0] / desc->vs;
    const dim3 grid((unsigned)((mx + JE_TBX - 1) / JE_TBX), (unsigned)((my + JE_TBY - 1) / JE_TBY), (unsigned)n_views);
    if (vec) hipLaunchKernelGGL(k_jpeg_encode<true>, grid, dim3(JE_BLOCK), 0, (hipStream_t)stream, *desc, V);
    else hipLaunchKernelGGL(k_jpeg_encode<false>, grid, dim3(JE_BLOCK), 0, (hipStream_t)stream, *desc, V);
    return dvs_launch_status();
}
