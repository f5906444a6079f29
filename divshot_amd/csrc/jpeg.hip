// jpeg.hip — the parallel half of baseline JPEG decoding (include/dvs_image.h): quantised DCT coefficients -> planar 8-bit RGB, ONE
// kernel, no scratch, no atomics, no inline assembly, plain vector stores. The result is defined bit for bit in the header and restated
// in tests/jpeg_ref.py; integer arithmetic only, so no compiler flag can change it.
//   A workgroup of 256 lanes owns a rectangle of JP_TBX x JP_TBY = 8 x 2 MCUs: 64 hs x 16 vs pixels (hs x vs = the luma sampling).
//   (1) the blocks of the rectangle — its luma blocks and, where chroma is subsampled, its chroma blocks plus a ring of one block,
//       recomputed from the neighbours so that the triangle filter's one-sample halo is in reach and workgroups stay independent — go
//       through the transform 32 at a time, 8 lanes per block, each block in a 72-int slot of LDS:
//         lane r loads row r of the block (8 coefficients = ONE 16-byte load), dequantises, clamps, writes F[r][0..7]   | barrier
//         lane r reads column r (F[0..7][r]), column pass in registers, writes col[0..7][r] in place                     | barrier
//         lane r reads row r (col[r][0..7]), row pass, +128, clamp, writes 8 bytes into the component's sample plane in LDS | barrier
//       Bank check, by the rule of each instruction, not measured. The column accesses are ds_read_b32 / ds_write_b32 (bank =
//       (address / 4) mod 32 within a 32-lane half): a half is 4 slots x 8 columns at int address 72 slot + 8 v + r -> bank
//       (8 slot + r + 8 v) mod 32 for slot 0..3, r 0..7: 32 distinct banks for every v — the 8-int pad of the slot is what separates
//       the four slots (a 64-int slot would be 4-way). The row accesses are NOT conflict-free: a lane moves the 32 bytes of its row as
//       two 16-byte accesses at int address 72 slot + 8 r (+ 4); ds_write_b128 (groups of 8 consecutive lanes, 32 banks) puts rows
//       r and r + 4 of a slot on the same four banks (2-way), and ds_read_b128 (64 banks, 16-lane groups that mix three slots, e.g.
//       lanes 0-3, 12-15, 20-27) meets slot 0 row 0, slot 1 row 7 and slot 2 row 6 on banks 0-3 (up to 3-way). Two of the six LDS
//       steps of a block pay that; a layout that also frees the rows was not tried.
//       The products are v_mad_i32_i24: |F| < 2^11, |T| < 2^12, |col| < 2^17 by the clamp, so both factors fit 24 bits.
//   (2) a lane produces 16 consecutive pixels of a row: luma from its plane, chroma through the triangle filter from the chroma planes
//       (indices clamped to the cropped chroma extent: edge replication), colour conversion, then three 16-byte stores when the
//       output allows (VEC) or up to 48 byte stores. Pixels past the image edge in partial MCUs are computed and not stored.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "../../include/dvs_image.h"

namespace {
constexpr int JP_BLOCK = 256;
constexpr int JP_TBX = 8, JP_TBY = 2;                    // MCUs a workgroup owns
constexpr int JP_SLOTS = JP_BLOCK / 8;                   // blocks in the transform at a time
constexpr int JP_SLOT = 72;                              // ints per slot: 64 + 8 of padding (see the bank check above)
constexpr int JP_LW = JP_TBX * 16, JP_LH = JP_TBY * 16;  // luma plane of the rectangle at 2x2
constexpr int JP_CW = (JP_TBX + 2) * 8, JP_CH = (JP_TBY + 2) * 8;   // chroma plane with its ring
constexpr int JP_FMIN = -2048, JP_FMAX = 2047;

// T[u][x] = round(2^13 * C(u) / 2 * cos((2x + 1) u pi / 16))
#define JP_T(u, x) (kT[u][x])
constexpr int kT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                          {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                          {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                          {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                          {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

__device__ __forceinline__ int jp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int jp_dequant(int c, int q) { return jp_clamp(c * q, JP_FMIN, JP_FMAX); }

// one upsampled chroma sample at pixel (X, Y): `p` is the chroma plane in LDS whose sample (0, 0) is chroma sample (cx0, cy0)
__device__ __forceinline__ int jp_chroma(const uint8_t* __restrict__ p, int hs, int vs, int X, int Y, int cx0, int cy0, int cw, int ch) {
    if (hs == 1) return p[(Y - cy0) * JP_CW + (X - cx0)];
    const int i = min(X >> 1, cw - 1), odd = X & 1;       // (the clamp acts only on pixels past the image edge, which are not stored)
    const int li = i - cx0, ln = jp_clamp(odd ? i + 1 : i - 1, 0, cw - 1) - cx0;
    if (vs == 1) {
        const uint8_t* row = p + (Y - cy0) * JP_CW;
        return (3 * row[li] + row[ln] + (odd ? 2 : 1)) >> 2;
    }
    const int j = Y >> 1, vodd = Y & 1;
    const uint8_t* near = p + (j - cy0) * JP_CW;
    const uint8_t* far = p + (jp_clamp(vodd ? j + 1 : j - 1, 0, ch - 1) - cy0) * JP_CW;
    const int t = 3 * near[li] + far[li], tn = 3 * near[ln] + far[ln];
    return (3 * t + tn + (odd ? 7 : 8)) >> 4;
}

template <bool VEC>
__global__ void __launch_bounds__(JP_BLOCK)
k_jpeg_reconstruct(const dvs_jpeg_desc D, const int16_t* __restrict__ coef, uint8_t* __restrict__ rgb) {
    __shared__ __align__(16) int ws[JP_SLOTS * JP_SLOT];
    __shared__ __align__(16) uint16_t quant[3 * 64];
    __shared__ __align__(16) uint8_t luma[JP_LH * JP_LW];
    __shared__ __align__(16) uint8_t chroma[2][JP_CH * JP_CW];
    const int tid = threadIdx.x;
    if (tid < 64 * D.components) quant[tid] = D.quant[tid >> 6][tid & 63];
    const int hs = D.hs, vs = D.vs, W = D.width, H = D.height;
    const int hx = hs == 2 ? 1 : 0, hy = vs == 2 ? 1 : 0;
    const int lbx = JP_TBX * hs, lby = JP_TBY * vs;                  // luma blocks of the rectangle
    const int cbx = JP_TBX + 2 * hx, cby = JP_TBY + 2 * hy;          // chroma blocks with the ring
    const int n_luma = lbx * lby, n_chroma = D.components == 3 ? cbx * cby : 0, total = n_luma + 2 * n_chroma;
    const int l0x = (int)blockIdx.x * lbx, l0y = (int)blockIdx.y * lby;             // block (0, 0) of the luma plane
    const int c0x = (int)blockIdx.x * JP_TBX - hx, c0y = (int)blockIdx.y * JP_TBY - hy;   // and of the chroma planes (-1 in the first ring)
    const int slot = tid >> 3, r = tid & 7;
    int* const w = ws + slot * JP_SLOT;
    __syncthreads();
    for (int base = 0; base < total; base += JP_SLOTS) {
        const int id = base + slot;
        int c = 0, lx, ly, bx, by;
        if (id < n_luma) { ly = id / lbx; lx = id - ly * lbx; bx = l0x + lx; by = l0y + ly; }
        else {
            int k = id - n_luma;
            c = 1;
            if (k >= n_chroma) { k -= n_chroma; c = 2; }
            ly = k / cbx; lx = k - ly * cbx; bx = c0x + lx; by = c0y + ly;
        }
        const int bw = c ? D.blocks_w[1] : D.blocks_w[0], bh = c ? D.blocks_h[1] : D.blocks_h[0];
        const bool live = id < total && bx >= 0 && by >= 0 && bx < bw && by < bh;       // a block outside the component is never read below
        if (live) {
            const uint64_t off = c == 0 ? D.offset[0] : c == 1 ? D.offset[1] : D.offset[2];
            const int4 v = *reinterpret_cast<const int4*>(coef + off + ((uint64_t)by * (uint64_t)bw + (uint64_t)bx) * 64 + (uint64_t)r * 8);
            const uint4 q = *reinterpret_cast<const uint4*>(quant + c * 64 + r * 8);
            int4 a, b;
            a.x = jp_dequant((int)(int16_t)v.x, (int)(q.x & 0xFFFFu)); a.y = jp_dequant(v.x >> 16, (int)(q.x >> 16));
            a.z = jp_dequant((int)(int16_t)v.y, (int)(q.y & 0xFFFFu)); a.w = jp_dequant(v.y >> 16, (int)(q.y >> 16));
            b.x = jp_dequant((int)(int16_t)v.z, (int)(q.z & 0xFFFFu)); b.y = jp_dequant(v.z >> 16, (int)(q.z >> 16));
            b.z = jp_dequant((int)(int16_t)v.w, (int)(q.w & 0xFFFFu)); b.w = jp_dequant(v.w >> 16, (int)(q.w >> 16));
            *reinterpret_cast<int4*>(w + r * 8) = a;
            *reinterpret_cast<int4*>(w + r * 8 + 4) = b;
        }
        __syncthreads();
        if (live) {                                                  // columns: lane r owns column u = r
            int F[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) F[k] = w[k * 8 + r];
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                int acc = 1 << 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += __mul24(JP_T(k, y), F[k]);
                w[y * 8 + r] = acc >> 9;
            }
        }
        __syncthreads();
        if (live) {                                                  // rows: lane r owns row y = r
            const int4 a = *reinterpret_cast<const int4*>(w + r * 8), b = *reinterpret_cast<const int4*>(w + r * 8 + 4);
            const int col[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t out[2] = {0u, 0u};
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                int acc = 1 << 16;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += __mul24(col[k], JP_T(k, x));
                out[x >> 2] |= (uint32_t)jp_clamp((acc >> 17) + 128, 0, 255) << (8 * (x & 3));
            }
            uint8_t* const plane = c == 0 ? luma : chroma[c - 1];
            const int stride = c == 0 ? JP_LW : JP_CW;
            *reinterpret_cast<uint2*>(plane + (ly * 8 + r) * stride + lx * 8) = make_uint2(out[0], out[1]);
        }
        __syncthreads();
    }
    // (2) pixels: 16 of a row per lane
    const int tw = 64 * hs, th = 16 * vs, units_x = tw / 16, units = units_x * th;
    const int x0 = (int)blockIdx.x * tw, y0 = (int)blockIdx.y * th;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const int cx0 = c0x * 8, cy0 = c0y * 8;
    const size_t HW = (size_t)H * (size_t)W;
    for (int unit = tid; unit < units; unit += JP_BLOCK) {
        const int ty = unit / units_x, tx = (unit - ty * units_x) * 16;
        const int Y = y0 + ty, X0 = x0 + tx;
        if (Y >= H || X0 >= W) continue;
        uint32_t pr[4] = {0u, 0u, 0u, 0u}, pg[4] = {0u, 0u, 0u, 0u}, pb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int X = X0 + k;
            const int lum = luma[ty * JP_LW + tx + k];
            int R = lum, G = lum, B = lum;
            if (D.components == 3) {
                const int cb = jp_chroma(chroma[0], hs, vs, X, Y, cx0, cy0, cw, ch) - 128;
                const int cr = jp_chroma(chroma[1], hs, vs, X, Y, cx0, cy0, cw, ch) - 128;
                R = jp_clamp(lum + ((91881 * cr + 32768) >> 16), 0, 255);
                G = jp_clamp(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
                B = jp_clamp(lum + ((116130 * cb + 32768) >> 16), 0, 255);
            }
            pr[k >> 2] |= (uint32_t)R << (8 * (k & 3)); pg[k >> 2] |= (uint32_t)G << (8 * (k & 3)); pb[k >> 2] |= (uint32_t)B << (8 * (k & 3));
        }
        uint8_t* const dst = rgb + (size_t)Y * (size_t)W + (size_t)X0;
        if (VEC) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(pr[0], pr[1], pr[2], pr[3]);
            *reinterpret_cast<uint4*>(dst + HW) = make_uint4(pg[0], pg[1], pg[2], pg[3]);
            *reinterpret_cast<uint4*>(dst + 2 * HW) = make_uint4(pb[0], pb[1], pb[2], pb[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (X0 + k < W) {
                    dst[k] = (uint8_t)(pr[k >> 2] >> (8 * (k & 3)));
                    dst[HW + k] = (uint8_t)(pg[k >> 2] >> (8 * (k & 3)));
                    dst[2 * HW + k] = (uint8_t)(pb[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
}

bool jpeg_desc_ok(const dvs_jpeg_desc& d) {
    if (d.width < 1 || d.height < 1 || d.width > 65500 || d.height > 65500) return false;
    if (d.components != 1 && d.components != 3) return false;
    const bool sampling = (d.hs == 1 && d.vs == 1) || (d.components == 3 && d.hs == 2 && (d.vs == 1 || d.vs == 2));
    if (!sampling) return false;
    const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
    if (d.blocks_w[0] != mx * d.hs || d.blocks_h[0] != my * d.vs || (d.offset[0] & 7u)) return false;
    for (int c = 1; c < d.components; ++c)
        if (d.blocks_w[c] != mx || d.blocks_h[c] != my || (d.offset[c] & 7u)) return false;
    return true;
}
}  // namespace

extern "C" int dvs_jpeg_reconstruct(void* stream, const dvs_jpeg_desc* desc, const int16_t* coef, uint8_t* rgb) {
    if (!desc || !coef || !rgb || ((uintptr_t)coef & 15u) || !jpeg_desc_ok(*desc)) return DVS_ERR_INVALID;
    const int mx = desc->blocks_w[0] / desc->hs, my = desc->blocks_h[0] / desc->vs;
    const dim3 grid((unsigned)((mx + JP_TBX - 1) / JP_TBX), (unsigned)((my + JP_TBY - 1) / JP_TBY));
    const bool vec = ((uintptr_t)rgb & 15u) == 0 && desc->width % 16 == 0;
    if (vec) hipLaunchKernelGGL(k_jpeg_reconstruct<true>, grid, dim3(JP_BLOCK), 0, (hipStream_t)stream, *desc, coef, rgb);
    else hipLaunchKernelGGL(k_jpeg_reconstruct<false>, grid, dim3(JP_BLOCK), 0, (hipStream_t)stream, *desc, coef, rgb);
    return dvs_launch_status();
}
