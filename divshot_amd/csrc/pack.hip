// pack.hip — model export packers (include/dvs_export.h): the device-resident splats into the payload of DIVSHOT's chunked, quantised
// .compressed.ply (external/tinygsplat/tiny_gsplat.cpp:293-396, tiny_gsplat.hpp:342-468) and into 32-byte .splat records
// (tiny_gsplat.cpp:243-291): a per-splat streaming job over 56 B of input per splat, shN is never read; and into / out of the six byte
// sections of .spz version 3 (external/spz/src/load-spz.cc), which also carries the 45 higher-order SH floats.
//   (a) k_pack_bounds / k_pack_bounds_final: min / max of pos per axis. Every workgroup writes its partial result to its own slot, one
//       small workgroup combines the slots: no float atomics, the result does not depend on the schedule.
//   (b) k_pack_morton: one 30-bit Morton key (10 bits per axis over the model's box) and the splat index per splat.
//   (c) the stable one-segment pair sort of frontend.hip (dvs_launch_pair_sort, 30 bits in four passes, ballot ranking): equal
//       keys stay in index order.
//   (d) k_pack_chunks: one workgroup of 256 lanes per chunk of 256 consecutive sorted entries (the last may be partial). A lane gathers
//       its splat by sorted index; the chunk's bounds of pos and of the raw scale are taken over the chunk's OWN members (the reference's
//       calcMinMax seeds them with p[start] instead of p[indices[start]], tiny_gsplat.hpp:332, which can only widen the box: not
//       reproduced); a lane leaves ONE 16-byte record, so a wavefront stores 1 KiB contiguously; lanes 0-11 write the chunk row.
//   (e) k_pack_splat32: one 32-byte record per splat in the model's order, two 16-byte stores per lane.
//   (f) k_pack_spz / k_unpack_spz: one wavefront per 64-splat tile, the sections' slices staged in LDS (see there).
// Results are defined bit for bit (tests/compressed_ply_ref.py and tests/spz_ref.py restate them in numpy): compiled without contraction (EXACT), IEEE
// division and square root, min / max are order-independent. No atomics, no inline assembly, plain vector stores.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "export_common.h"
#include "../../include/dvs_raster.h"
#include "../../include/dvs_export.h"

namespace {
constexpr int PK_BLOCK = 256, PK_WAVES = PK_BLOCK / 64;
constexpr int PK_BOUNDS_BLOCKS = 512;                      // at most this many partial slots; the workgroups stride over the splats
constexpr int PK_CHUNK = 256;                              // splats per chunk of the format

__device__ __forceinline__ float pk_wave_min(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float pk_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// workgroup-wide min of lo[0..K) and max of hi[0..K): every lane returns with the results. lds = [PK_WAVES][2 K] floats.
template <int K>
__device__ __forceinline__ void pk_block_minmax(float (&lo)[K], float (&hi)[K], float* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) { lo[k] = pk_wave_min(lo[k]); hi[k] = pk_wave_max(hi[k]); }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) { lds[wave * 2 * K + k] = lo[k]; lds[wave * 2 * K + K + k] = hi[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float a = lds[k], b = lds[K + k];
#pragma unroll
        for (int w = 1; w < PK_WAVES; ++w) { a = fminf(a, lds[w * 2 * K + k]); b = fmaxf(b, lds[w * 2 * K + K + k]); }
        lo[k] = a; hi[k] = b;
    }
}
// the same result for ONE of the 2 K values, chosen by a lane-dependent index t (0 .. K - 1: minima, K .. 2 K - 1: maxima), read from
// what pk_block_minmax left in LDS: no dynamically indexed register array
template <int K>
__device__ __forceinline__ float pk_block_result(const float* lds, int t) {
    float r = lds[t];
#pragma unroll
    for (int w = 1; w < PK_WAVES; ++w) { const float o = lds[w * 2 * K + t]; r = t < K ? fminf(r, o) : fmaxf(r, o); }
    return r;
}

// (a) slots[block] = {min xyz, max xyz} over the splats block * 256 + tid, + gridDim * 256, ...
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_bounds(int n, const float* __restrict__ pos, float* __restrict__ slots) {
    __shared__ float lds[PK_WAVES * 6];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PK_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float p = pos[3 * i + k]; lo[k] = fminf(lo[k], p); hi[k] = fmaxf(hi[k], p); }
    }
    pk_block_minmax<3>(lo, hi, lds);
    if (threadIdx.x < 6) slots[blockIdx.x * 6 + threadIdx.x] = pk_block_result<3>(lds, (int)threadIdx.x);
}
// one workgroup: bounds[0..6) = the slots combined
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_bounds_final(int n_slots, const float* __restrict__ slots, float* __restrict__ bounds) {
    __shared__ float lds[PK_WAVES * 6];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int s = threadIdx.x; s < n_slots; s += PK_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], slots[s * 6 + k]); hi[k] = fmaxf(hi[k], slots[s * 6 + 3 + k]); }
    }
    pk_block_minmax<3>(lo, hi, lds);
    if (threadIdx.x < 6) bounds[threadIdx.x] = pk_block_result<3>(lds, (int)threadIdx.x);
}

// bits 0..9 of q spread to every third bit
__device__ __forceinline__ uint32_t pk_spread3(uint32_t q) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) r |= ((q >> i) & 1u) << (3 * i);
    return r;
}

// (b) keys[i] = 30-bit Morton code of pos[i] in the model's box, vals[i] = i
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_morton(int n, const float* __restrict__ pos, const float* __restrict__ bounds, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mn = bounds[k], ext = bounds[3 + k] - mn;
        const float rel = ext < 1e-5f ? 0.0f : (pos[3 * i + k] - mn) / ext;
        const float s = fminf(fmaxf(rel * 1023.0f, 0.0f), 1023.0f);       // rel is in [0, 1] already; a NaN position lands in cell 0
        key |= pk_spread3((uint32_t)s) << k;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__device__ __forceinline__ float pk_norm(float x, float mn, float mx) { const float e = mx - mn; return e < 0.00001f ? 0.0f : (x - mn) / e; }
// tiny_gsplat.hpp:342-346: the product in fp32, the rounding in fp64
__device__ __forceinline__ uint32_t pk_unorm(float v, int bits) {
    const int t = (1 << bits) - 1;
    const double r = floor((double)(v * (float)t) + 0.5);
    return (uint32_t)fmin(fmax(r, 0.0), (double)t);                        // (fmax(NaN, 0) = 0)
}
__device__ __forceinline__ uint32_t pk_111011(float x, float y, float z) { return pk_unorm(x, 11) << 21 | pk_unorm(y, 10) << 11 | pk_unorm(z, 11); }

__device__ __forceinline__ uint32_t pk_rot(const float4 r) {
    float q[4];
    dvs_unit_quat(r, q);
    int largest = 0;
    float ql = q[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (fabsf(q[k]) > fabsf(ql)) { largest = k; ql = q[k]; }      // the first of equal magnitudes stays
    const float sgn = ql < 0.0f ? -1.0f : 1.0f;
    uint32_t result = (uint32_t)largest;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k != largest) result = (result << 10) | pk_unorm((sgn * q[k]) * 0.70710678f + 0.5f, 10);
    return result;
}

// (d) chunk c = sorted entries [256 c, min(n, 256 c + 256))
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_chunks(int n, const uint32_t* __restrict__ sorted, const float* __restrict__ pos, const float* __restrict__ sh0,
              const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot,
              float* __restrict__ chunks, uint4* __restrict__ verts, uint32_t* __restrict__ order) {
    __shared__ float lds[PK_WAVES * 12];
    const int64_t j = (int64_t)blockIdx.x * PK_CHUNK + threadIdx.x;
    const bool valid = j < n;
    const uint32_t id = valid ? sorted[j] : 0u;
    float p[3], s[3], lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = pos[3 * (size_t)id + k]; s[k] = scale[3 * (size_t)id + k];
        lo[k] = valid ? p[k] : __builtin_inff(); hi[k] = valid ? p[k] : -__builtin_inff();
        lo[3 + k] = valid ? s[k] : __builtin_inff(); hi[3 + k] = valid ? s[k] : -__builtin_inff();
    }
    pk_block_minmax<6>(lo, hi, lds);
    if (threadIdx.x < 12) {                                                // {pmin, pmax, smin, smax} from the LDS order {pmin, smin, pmax, smax}
        const int t = threadIdx.x;
        chunks[(size_t)blockIdx.x * 12 + t] = pk_block_result<6>(lds, t < 3 ? t : t < 6 ? t + 3 : t < 9 ? t - 3 : t);
    }
    if (!valid) return;
    const float c0 = sh0[3 * (size_t)id], c1 = sh0[3 * (size_t)id + 1], c2 = sh0[3 * (size_t)id + 2];
    const float4 r = reinterpret_cast<const float4*>(rot)[id];
    uint4 w;
    w.x = pk_111011(pk_norm(p[0], lo[0], hi[0]), pk_norm(p[1], lo[1], hi[1]), pk_norm(p[2], lo[2], hi[2]));
    w.y = pk_rot(r);
    w.z = pk_111011(pk_norm(s[0], lo[3], hi[3]), pk_norm(s[1], lo[4], hi[4]), pk_norm(s[2], lo[5], hi[5]));
    w.w = pk_unorm(c0 * DVS_SH_C0 + 0.5f, 8) << 24 | pk_unorm(c1 * DVS_SH_C0 + 0.5f, 8) << 16 | pk_unorm(c2 * DVS_SH_C0 + 0.5f, 8) << 8 |
          pk_unorm(dvs_sigmoid_det(opacity[id]), 8);
    verts[j] = w;
    if (order) order[j] = id;
}

__device__ __forceinline__ uint32_t pk_trunc_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.0f), 255.0f); }

// (e) one 32-byte record per splat
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_splat32(int n, const float* __restrict__ pos, const float* __restrict__ sh0, const float* __restrict__ opacity,
               const float* __restrict__ scale, const float* __restrict__ rot, uint4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x;
    if (i >= n) return;
    float q[4];
    dvs_unit_quat(reinterpret_cast<const float4*>(rot)[i], q);
    uint4 a, b;
    a.x = __float_as_uint(pos[3 * i]); a.y = __float_as_uint(pos[3 * i + 1]); a.z = __float_as_uint(pos[3 * i + 2]);
    a.w = __float_as_uint(dvs_exp_det(scale[3 * i]));
    b.x = __float_as_uint(dvs_exp_det(scale[3 * i + 1])); b.y = __float_as_uint(dvs_exp_det(scale[3 * i + 2]));
    b.z = pk_trunc_u8((0.5f + DVS_SH_C0 * sh0[3 * i]) * 255.0f) | pk_trunc_u8((0.5f + DVS_SH_C0 * sh0[3 * i + 1]) * 255.0f) << 8 |
          pk_trunc_u8((0.5f + DVS_SH_C0 * sh0[3 * i + 2]) * 255.0f) << 16 | pk_trunc_u8(dvs_sigmoid_det(opacity[i]) * 255.0f) << 24;
    b.w = pk_trunc_u8(q[0] * 128.0f + 128.0f) | pk_trunc_u8(q[1] * 128.0f + 128.0f) << 8 | pk_trunc_u8(q[2] * 128.0f + 128.0f) << 16 |
          pk_trunc_u8(q[3] * 128.0f + 128.0f) << 24;
    out[2 * i] = a;
    out[2 * i + 1] = b;
}

// ---- (f) .spz, version 3 (external/spz/src/load-spz.cc packGaussians / unpackGaussians) ---------------------------------------------
// One wavefront owns 64 consecutive splats = one tile of DVS_SHN_TILED; a workgroup of four waves has one LDS image per wave holding the
// tile's slice of the sh, positions, colors and scales sections (64 * (3 DIM + 9 + 3 + 3) bytes: 3840 B at degree 3, 15 KiB per
// workgroup). A lane quantises its own splat into the image byte by byte; the wave then moves each slice as 16-byte words (64 * 9,
// 64 * 3 and 64 * 3 DIM are multiples of 16 and every section starts on a 16-byte boundary, so a whole tile's slice is aligned in every
// section). The last, partial tile goes byte by byte. alphas (one byte per lane, 64 contiguous bytes per wave) and rotations (one dword
// per lane, 256 contiguous bytes) are whole records per lane and are stored directly. DVS_SHN_ROWS input is read as dwords, lane after
// lane through the tile's rows, into the same image. The decoder is the mirror image.
constexpr int SPZ_POS = 64 * 9, SPZ_VEC3 = 64 * 3;         // bytes of one tile in positions / in colors and scales
template <int DIM> constexpr int spz_image_bytes() { return 64 * 3 * DIM + SPZ_POS + 2 * SPZ_VEC3; }

__device__ __forceinline__ void spz_store_slice(const uint8_t* img, uint8_t* dst, int tile_bytes, int valid_bytes, int lane) {
    if (valid_bytes == tile_bytes) {
        for (int k = lane; k < tile_bytes / 16; k += 64) reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(img)[k];
    } else {
        for (int b = lane; b < valid_bytes; b += 64) dst[b] = img[b];
    }
}
__device__ __forceinline__ void spz_load_slice(uint8_t* img, const uint8_t* src, int tile_bytes, int valid_bytes, int lane) {
    if (valid_bytes == tile_bytes) {
        for (int k = lane; k < tile_bytes / 16; k += 64) reinterpret_cast<uint4*>(img)[k] = reinterpret_cast<const uint4*>(src)[k];
    } else {
        for (int b = lane; b < valid_bytes; b += 64) img[b] = src[b];
    }
}

// toUint8 (load-spz.cc:74): round half away from zero, clamp; a NaN gives 0
__device__ __forceinline__ uint32_t spz_u8(float v) { return (uint32_t)fminf(fmaxf(roundf(v), 0.0f), 255.0f); }
// 24-bit fixed point with 12 fractional bits, saturated; a position that is not finite gives 0
__device__ __forceinline__ uint32_t spz_fixed24(float p) {
    if (!(fabsf(p) < __builtin_inff())) return 0u;
    const float f = fminf(fmaxf(roundf(p * 4096.0f), -8388608.0f), 8388607.0f);
    return (uint32_t)(int32_t)f & 0xFFFFFFu;
}
// quantizeSH (load-spz.cc:77-81) with bucket size B; a NaN gives the byte of 0
template <int B> __device__ __forceinline__ uint8_t spz_sh(float x) {
    float r = roundf(x * 128.0f);
    r = r == r ? fminf(fmaxf(r, -512.0f), 512.0f) : 0.0f;
    int q = (int)r + 128;
    q = (q + B / 2) / B * B;
    return (uint8_t)min(max(q, 0), 255);
}
// packQuaternionSmallestThree (load-spz.cc:216-255) of the repository's (w, x, y, z). Its normalisation is NOT dvs_unit_quat: the squares
// are summed in the format's (x, y, z, w) order, w last, as the format's reference does, so the two sums can differ in the last bit.
__device__ __forceinline__ uint32_t spz_rot(const float4 r) {
    float q[4] = {r.y, r.z, r.w, r.x};                                     // the format's (x, y, z, w)
    const float ss = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (!(ss > 0.0f) || !(ss < __builtin_inff())) { q[0] = q[1] = q[2] = 0.0f; q[3] = 1.0f; }
    else {
        const float len = dvs_sqrt_rn(ss);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
    }
    int largest = 0;
    float ql = q[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (fabsf(q[k]) > fabsf(ql)) { largest = k; ql = q[k]; }      // the first of equal magnitudes stays
    const uint32_t negate = ql < 0.0f ? 1u : 0u;
    uint32_t comp = (uint32_t)largest;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k != largest) {
            const uint32_t mag = (uint32_t)(511.0f * (fabsf(q[k]) / 0.70710678f) + 0.5f);
            comp = (comp << 10) | (((q[k] < 0.0f ? 1u : 0u) ^ negate) << 9) | min(mag, 511u);
        }
    return comp;
}

template <int DIM>
__global__ void __launch_bounds__(PK_BLOCK)
k_pack_spz(int n, dvs_spz_layout L /*off[]: positions, alphas, colors, scales, rotations, sh*/, const float* __restrict__ pos, const float* __restrict__ sh0, const float* __restrict__ shN, int tiled,
           const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot, uint8_t* __restrict__ out) {
    constexpr int SHB = 3 * DIM, IMG16 = spz_image_bytes<DIM>() / 16;
    __shared__ uint4 lds[PK_WAVES * IMG16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * PK_WAVES + wave, i0 = tile * 64, i = i0 + lane;
    const int count = (int)(n - i0 >= 64 ? 64 : n - i0 > 0 ? n - i0 : 0);  // splats of this wave's tile (0: a wave past the model)
    uint8_t* const img_sh = reinterpret_cast<uint8_t*>(lds + wave * IMG16);
    uint8_t* const img_pos = img_sh + 64 * SHB;
    uint8_t* const img_col = img_pos + SPZ_POS;
    uint8_t* const img_scl = img_col + SPZ_VEC3;
    if (lane < count) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t f = spz_fixed24(pos[3 * i + k]);
            img_pos[lane * 9 + 3 * k] = (uint8_t)f; img_pos[lane * 9 + 3 * k + 1] = (uint8_t)(f >> 8); img_pos[lane * 9 + 3 * k + 2] = (uint8_t)(f >> 16);
            img_col[lane * 3 + k] = (uint8_t)spz_u8(sh0[3 * i + k] * (0.15f * 255.0f) + (0.5f * 255.0f));
            img_scl[lane * 3 + k] = (uint8_t)spz_u8((scale[3 * i + k] + 10.0f) * 16.0f);
        }
        const float o = opacity[i];
        out[L.off[1] + i] = (uint8_t)(o == o ? spz_u8(dvs_sigmoid_det(o) * 255.0f) : 0u);         // a NaN logit: alpha 0
        reinterpret_cast<uint32_t*>(out + L.off[4])[i] = spz_rot(reinterpret_cast<const float4*>(rot)[i]);
    }
    if (DIM > 0 && count > 0) {
        if (tiled) {                                                       // (whole tiles are allocated: every lane's chunk is in bounds)
#pragma unroll
            for (int c = 0; c < (SHB + 3) / 4; ++c) {
                const float4 v = reinterpret_cast<const float4*>(shN)[dvs_shn_tiled_chunk(i, c)];
                const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * c + k < SHB) img_sh[lane * SHB + 4 * c + k] = 4 * c + k < 9 ? spz_sh<8>(e4[k]) : spz_sh<16>(e4[k]);
            }
        } else {
            for (int idx = lane; idx < count * SHB; idx += 64) {
                const int s = idx / SHB, e = idx - s * SHB;
                const float x = shN[(i0 + s) * 45 + e];
                img_sh[idx] = e < 9 ? spz_sh<8>(x) : spz_sh<16>(x);
            }
        }
    }
    __syncthreads();
    if (count == 0) return;
    if (DIM > 0) spz_store_slice(img_sh, out + L.off[5] + (size_t)tile * (64 * SHB), 64 * SHB, count * SHB, lane);
    spz_store_slice(img_pos, out + L.off[0] + (size_t)tile * SPZ_POS, SPZ_POS, count * 9, lane);
    spz_store_slice(img_col, out + L.off[2] + (size_t)tile * SPZ_VEC3, SPZ_VEC3, count * 3, lane);
    spz_store_slice(img_scl, out + L.off[3] + (size_t)tile * SPZ_VEC3, SPZ_VEC3, count * 3, lane);
}

// unpackGaussians (load-spz.cc:467-531): shN == nullptr skips the higher bands (degree 0 only)
template <int DIM>
__global__ void __launch_bounds__(PK_BLOCK)
k_unpack_spz(int n, dvs_spz_layout L /*off[]: positions, alphas, colors, scales, rotations, sh*/, const uint8_t* __restrict__ in, float* __restrict__ pos, float* __restrict__ sh0, float* __restrict__ shN, int tiled,
             float* __restrict__ opacity, float* __restrict__ scale, float* __restrict__ rot) {
    constexpr int SHB = 3 * DIM, IMG16 = spz_image_bytes<DIM>() / 16;
    __shared__ uint4 lds[PK_WAVES * IMG16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * PK_WAVES + wave, i0 = tile * 64, i = i0 + lane;
    const int count = (int)(n - i0 >= 64 ? 64 : n - i0 > 0 ? n - i0 : 0);
    uint8_t* const img_sh = reinterpret_cast<uint8_t*>(lds + wave * IMG16);
    uint8_t* const img_pos = img_sh + 64 * SHB;
    uint8_t* const img_col = img_pos + SPZ_POS;
    uint8_t* const img_scl = img_col + SPZ_VEC3;
    if (count > 0) {
        if (DIM > 0) spz_load_slice(img_sh, in + L.off[5] + (size_t)tile * (64 * SHB), 64 * SHB, count * SHB, lane);
        spz_load_slice(img_pos, in + L.off[0] + (size_t)tile * SPZ_POS, SPZ_POS, count * 9, lane);
        spz_load_slice(img_col, in + L.off[2] + (size_t)tile * SPZ_VEC3, SPZ_VEC3, count * 3, lane);
        spz_load_slice(img_scl, in + L.off[3] + (size_t)tile * SPZ_VEC3, SPZ_VEC3, count * 3, lane);
    }
    __syncthreads();
    if (count == 0) return;
    const bool valid = lane < count;
    if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint8_t* b = img_pos + lane * 9 + 3 * k;
            const int32_t fixed = (int32_t)(((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16) << 8) >> 8;      // sign extension of bit 23
            pos[3 * i + k] = (float)fixed * (1.0f / 4096.0f);
            sh0[3 * i + k] = (((float)img_col[lane * 3 + k] / 255.0f) - 0.5f) / 0.15f;
            scale[3 * i + k] = (float)img_scl[lane * 3 + k] / 16.0f - 10.0f;
        }
        const float a = (float)in[L.off[1] + i] / 255.0f;
        opacity[i] = logf(a / (1.0f - a));                                 // bytes 0 / 255: -inf / +inf
        uint32_t comp = reinterpret_cast<const uint32_t*>(in + L.off[4])[i];
        const int largest = (int)(comp >> 30);
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sum = 0.0f;                 // (x, y, z, w)
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (k != largest) {
                const float m = (0.70710678f * (float)(comp & 511u)) / 511.0f;
                q[k] = (comp >> 9) & 1u ? -m : m;
                comp >>= 10;
                sum += q[k] * q[k];
            }
        const float big = dvs_sqrt_rn(1.0f - sum);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k == largest) q[k] = big;
        reinterpret_cast<float4*>(rot)[i] = make_float4(q[3], q[0], q[1], q[2]);
    }
    if (!shN) return;
    if (tiled) {                                                           // the whole tile: the pads and the lanes past the model are 0
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            float e4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) e4[k] = (4 * c + k < SHB && valid) ? ((float)img_sh[lane * SHB + 4 * c + k] - 128.0f) / 128.0f : 0.0f;
            reinterpret_cast<float4*>(shN)[dvs_shn_tiled_chunk(i, c)] = make_float4(e4[0], e4[1], e4[2], e4[3]);
        }
    } else {
        for (int idx = lane; idx < count * 45; idx += 64) {
            const int s = idx / 45, e = idx - s * 45;
            shN[(i0 + s) * 45 + e] = e < SHB ? ((float)img_sh[s * SHB + e] - 128.0f) / 128.0f : 0.0f;
        }
    }
}

// the scratch of dvs_pack_compressed: byte offsets of its parts, each on a 256-byte boundary
struct PackScratch { size_t slots, bounds, sort_ws, key[2], val[2], total; };
PackScratch pack_layout(int n) {
    const auto up = dvs_align256;
    PackScratch L;
    size_t o = 0;
    L.slots = o; o += up((size_t)PK_BOUNDS_BLOCKS * 6 * sizeof(float));
    L.bounds = o; o += up(6 * sizeof(float));
    L.sort_ws = o; o += dvs_pair_sort_ws_bytes((uint64_t)n);
    for (int k = 0; k < 2; ++k) { L.key[k] = o; o += up((size_t)n * 4); L.val[k] = o; o += up((size_t)n * 4); }
    L.total = o;
    return L;
}
}  // namespace

extern "C" size_t dvs_pack_scratch_bytes(int n) { return n > 0 ? pack_layout(n).total : 0; }

// (a) - (c) for any caller inside the library (dvs_kernels.h): the model indices in Morton order, the model's box
hipError_t dvs_launch_morton_order(hipStream_t st, int n, const float* pos, void* scratch, const uint32_t** sorted, const float** bounds_out) {
    const PackScratch L = pack_layout(n);
    char* const base = (char*)scratch;
    float* const slots = (float*)(base + L.slots);
    float* const bounds = (float*)(base + L.bounds);
    uint32_t* key[2] = {(uint32_t*)(base + L.key[0]), (uint32_t*)(base + L.key[1])};
    uint32_t* val[2] = {(uint32_t*)(base + L.val[0]), (uint32_t*)(base + L.val[1])};
    const unsigned nblocks = (unsigned)(((int64_t)n + PK_BLOCK - 1) / PK_BLOCK);
    const unsigned bblocks = nblocks < (unsigned)PK_BOUNDS_BLOCKS ? nblocks : (unsigned)PK_BOUNDS_BLOCKS;
    hipLaunchKernelGGL(k_pack_bounds, dim3(bblocks), dim3(PK_BLOCK), 0, st, n, pos, slots);
    hipLaunchKernelGGL(k_pack_bounds_final, dim3(1), dim3(PK_BLOCK), 0, st, (int)bblocks, (const float*)slots, bounds);
    hipLaunchKernelGGL(k_pack_morton, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, pos, (const float*)bounds, key[0], val[0]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int cur = 0;                                                           // ballot ranking: no probe of the device needed
    if ((e = dvs_launch_pair_sort(st, (uint64_t)n, key[0], val[0], key[1], val[1], 0, 30, dvs_pair_sort_ws_at(base + L.sort_ws), 0, &cur)) != hipSuccess)
        return e;
    *sorted = val[cur];
    if (bounds_out) *bounds_out = bounds;
    return hipSuccess;
}
size_t dvs_morton_scratch_bytes(int n) { return n > 0 ? pack_layout(n).total : 0; }

extern "C" int dvs_pack_compressed(void* stream, int n, const float* pos, const float* sh0, const float* opacity, const float* scale,
                                   const float* rot, void* scratch, float* chunks, uint32_t* verts, uint32_t* order) {
    if (n <= 0 || dvs_bad_args({pos, sh0, opacity, scale, rot, scratch, chunks, verts}, {order})) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* sorted = nullptr;
    if (dvs_launch_morton_order(st, n, pos, scratch, &sorted, nullptr) != hipSuccess) return DVS_ERR_HIP;
    const unsigned nchunks = (unsigned)(((int64_t)n + PK_CHUNK - 1) / PK_CHUNK);
    hipLaunchKernelGGL(k_pack_chunks, dim3(nchunks), dim3(PK_BLOCK), 0, st, n, sorted, pos, sh0, opacity, scale, rot, chunks,
                       (uint4*)verts, order);
    return dvs_launch_status();
}

extern "C" int dvs_pack_splat32(void* stream, int n, const float* pos, const float* sh0, const float* opacity, const float* scale,
                                const float* rot, uint8_t* out) {
    if (n <= 0 || dvs_bad_args({pos, sh0, opacity, scale, rot, out})) return DVS_ERR_INVALID;
    const unsigned nblocks = (unsigned)(((int64_t)n + PK_BLOCK - 1) / PK_BLOCK);
    hipLaunchKernelGGL(k_pack_splat32, dim3(nblocks), dim3(PK_BLOCK), 0, (hipStream_t)stream, n, pos, sh0, opacity, scale, rot, (uint4*)out);
    return dvs_launch_status();
}

extern "C" int dvs_spz_layout_for(int n, int sh_degree, dvs_spz_layout* out) {
    if (n <= 0 || sh_degree < 0 || sh_degree > 3 || !out) return DVS_ERR_INVALID;
    static const int dim[4] = {0, 3, 8, 15};
    const uint64_t per[6] = {9, 1, 3, 3, 4, (uint64_t)(3 * dim[sh_degree])};
    uint64_t o = 0;
    for (int k = 0; k < 6; ++k) { out->off[k] = o; out->bytes[k] = per[k] * (uint64_t)n; o = (o + out->bytes[k] + 15) & ~(uint64_t)15; }
    out->total = o;
    return DVS_OK;
}

namespace {
// the six required pointers of dvs_pack_spz / dvs_unpack_spz; shN may be null at degree 0 only
bool spz_bad_args(int n, int sh_degree, int shn_layout, std::initializer_list<const void*> required, const void* shN) {
    return n <= 0 || sh_degree < 0 || sh_degree > 3 || (!shN && sh_degree > 0) || dvs_bad_args(required, {shN}, shn_layout);
}
}  // namespace

extern "C" int dvs_pack_spz(void* stream, int n, int sh_degree, const float* pos, const float* sh0, const float* shN, int shn_layout,
                            const float* opacity, const float* scale, const float* rot, uint8_t* out) {
    if (spz_bad_args(n, sh_degree, shn_layout, {pos, sh0, opacity, scale, rot, out}, shN)) return DVS_ERR_INVALID;
    dvs_spz_layout L;
    (void)dvs_spz_layout_for(n, sh_degree, &L);                           // (the arguments were checked above)
    const unsigned nblocks = (unsigned)(((int64_t)n + PK_BLOCK - 1) / PK_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    const int tiled = shn_layout == DVS_SHN_TILED;
    switch (sh_degree) {
        case 0: hipLaunchKernelGGL(k_pack_spz<0>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, pos, sh0, shN, tiled, opacity, scale, rot, out); break;
        case 1: hipLaunchKernelGGL(k_pack_spz<3>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, pos, sh0, shN, tiled, opacity, scale, rot, out); break;
        case 2: hipLaunchKernelGGL(k_pack_spz<8>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, pos, sh0, shN, tiled, opacity, scale, rot, out); break;
        default: hipLaunchKernelGGL(k_pack_spz<15>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, pos, sh0, shN, tiled, opacity, scale, rot, out); break;
    }
    return dvs_launch_status();
}

extern "C" int dvs_unpack_spz(void* stream, int n, int sh_degree, const uint8_t* packed, float* pos, float* sh0, float* shN, int shn_layout,
                              float* opacity, float* scale, float* rot) {
    if (spz_bad_args(n, sh_degree, shn_layout, {packed, pos, sh0, opacity, scale, rot}, shN)) return DVS_ERR_INVALID;
    dvs_spz_layout L;
    (void)dvs_spz_layout_for(n, sh_degree, &L);                           // (the arguments were checked above)
    const unsigned nblocks = (unsigned)(((int64_t)n + PK_BLOCK - 1) / PK_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    const int tiled = shn_layout == DVS_SHN_TILED;
    switch (sh_degree) {
        case 0: hipLaunchKernelGGL(k_unpack_spz<0>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, packed, pos, sh0, shN, tiled, opacity, scale, rot); break;
        case 1: hipLaunchKernelGGL(k_unpack_spz<3>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, packed, pos, sh0, shN, tiled, opacity, scale, rot); break;
        case 2: hipLaunchKernelGGL(k_unpack_spz<8>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, packed, pos, sh0, shN, tiled, opacity, scale, rot); break;
        default: hipLaunchKernelGGL(k_unpack_spz<15>, dim3(nblocks), dim3(PK_BLOCK), 0, st, n, L, packed, pos, sh0, shN, tiled, opacity, scale, rot); break;
    }
    return dvs_launch_status();
}
