// reduced.hip — the producing side of DIVSHOT's .reduced.ply, quantised variant (include/dvs_export.h; the container and its reader are
// external/tinygsplat/tiny_gsplat.cpp save_reduced_ply / load_reduced_ply): a per-splat SH degree, twenty 256-entry scalar codebooks
// built by 1-D k-means, the four per-degree vertex blocks of codebook ids, and the decoder.
//   (a) k_sh_degree<D>: one lane per splat, its 3 ((D + 1)^2 - 1) coefficients in registers, a loop over the camera centres (read through
//       wave-uniform addresses: scalar loads). No atomics, no LDS.
//   (b) per codebook: k_rd_keys (value -> order-preserving uint32 key; a value outside the book's set -> 0xFFFFFFFF, which no finite
//       float maps to and which sorts last), the stable pair sort of frontend.hip (dvs_launch_pair_sort, four 8-bit passes), k_rd_info (m = the
//       keys below the sentinel, the scaling exponent e), k_rd_fixed (k(v) as int64), the inclusive 64-bit scan of scan.hip, and
//       k_rd_lloyd: ONE workgroup of 256 lanes runs every iteration, lane j owning centre j.
//   (c) k_rd_count + the 32-bit scan of scan.hip over the [4][tiles] degree counts: a stable 4-way partition. k_pack_reduced: one workgroup
//       per 256 splats, the 20 x 255 boundaries in LDS, the tile's four runs staged in LDS and stored as 16-byte words where a run covers one.
//   (d) k_unpack_reduced: one lane per output splat.
// Results are defined bit for bit (tests/reduced_ply_ref.py restates them in numpy): compiled without contraction (EXACT); the fp64
// operations used (conversion, add, multiply by 0.5, divide, ldexp, rint, compare) are IEEE-exact. Plain vector stores only.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "block_scan.h"
#include "export_common.h"
#include "../../include/dvs_raster.h"
#include "../../include/dvs_export.h"

namespace {
constexpr int RD_BLOCK = DB;                               // 256: the tile of the partition, the entries of a codebook
constexpr int RD_BOOKS = DVS_REDUCED_BOOKS, RD_K = DVS_REDUCED_ENTRIES;
constexpr uint32_t RD_ABSENT = 0xFFFFFFFFu;                // key of a value that is not in the codebook's set
constexpr int RD_IMG_BYTES = RD_BLOCK * 68 + 128;          // four runs of at most 256 records of 68 bytes, each shifted by < 16 and padded to 16
static_assert(RD_K == RD_BLOCK, "lane j owns centre j");

__device__ __forceinline__ int rd_coeffs(int d) { return (d + 1) * (d + 1) - 1; }
__device__ __forceinline__ int rd_deg(uint8_t d) { return d > 3 ? 3 : (int)d; }
// what is clustered: a value that is not finite, and -0, count as +0
__device__ __forceinline__ float rd_clean(float v) {
    if (!(fabsf(v) < __builtin_inff())) return 0.0f;
    return __float_as_uint(v) == 0x80000000u ? 0.0f : v;
}
__device__ __forceinline__ uint32_t rd_key(float clean) {
    const uint32_t b = __float_as_uint(clean);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float rd_unkey(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k & 0x7FFFFFFFu : ~k); }

// ---- (a) ------------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(RD_BLOCK)
k_sh_degree(int n, const float* __restrict__ pos, const float* __restrict__ shN, int layout, const float* __restrict__ cams, int C, float t,
            uint8_t* __restrict__ degree) {
    constexpr int NC = (D + 1) * (D + 1) - 1;
    const int i = blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= n) return;
    float sh[3 * NC];
    if (layout == DVS_SHN_TILED) {
#pragma unroll
        for (int c = 0; c < (3 * NC + 3) / 4; ++c) {
            const float4 v = reinterpret_cast<const float4*>(shN)[dvs_shn_tiled_chunk(i, c)];
            const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) if (4 * c + k < 3 * NC) sh[4 * c + k] = e4[k];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 3 * NC; ++e) sh[e] = shN[(int64_t)i * 45 + e];
    }
    const float px = pos[3 * (int64_t)i], py = pos[3 * (int64_t)i + 1], pz = pos[3 * (int64_t)i + 2];
    bool ok0 = true, ok1 = true, ok2 = true;               // err_k <= t so far
    for (int c = 0; c < C; ++c) {
        const float vx = px - cams[3 * c], vy = py - cams[3 * c + 1], vz = pz - cams[3 * c + 2];
        const float len = dvs_sqrt_rn((vx * vx + vy * vy) + vz * vz);
        if (!(len > 0.0f) || !(len < __builtin_inff())) continue;
        float b[16];
        dvs_sh_basis(D, vx / len, vy / len, vz / len, b);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float tail = 0.0f;
            if (D >= 3) {
                float s = b[9] * sh[24 + ch];
#pragma unroll
                for (int l = 10; l < 16; ++l) s = s + b[l] * sh[(l - 1) * 3 + ch];
                tail = s;
                ok2 = ok2 && fabsf(tail) <= t;
            }
            if (D >= 2) {
                float s = b[4] * sh[9 + ch];
#pragma unroll
                for (int l = 5; l < 9; ++l) s = s + b[l] * sh[(l - 1) * 3 + ch];
                tail = D >= 3 ? tail + s : s;
                ok1 = ok1 && fabsf(tail) <= t;
            }
            {
                float s = b[1] * sh[ch];
                s = s + b[2] * sh[3 + ch];
                s = s + b[3] * sh[6 + ch];
                tail = D >= 2 ? tail + s : s;
                ok0 = ok0 && fabsf(tail) <= t;             // (a NaN fails the comparison: it exceeds t)
            }
        }
    }
    degree[i] = (uint8_t)(ok0 ? 0 : (D >= 2 && ok1) ? 1 : (D >= 3 && ok2) ? 2 : D);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------------
struct RdInfo { uint32_t m; int32_t e; uint32_t zero; uint32_t _pad; };

// keys[q] for the q-th candidate value of codebook `book` (M = n or 3 n candidates)
__global__ void __launch_bounds__(RD_BLOCK)
k_rd_keys(int book, int n, uint32_t M, const float* __restrict__ sh0, const float* __restrict__ shN, int layout, const float* __restrict__ opacity,
          const float* __restrict__ scale, const float* __restrict__ rot, const uint8_t* __restrict__ degree, uint32_t* __restrict__ keys) {
    const uint32_t q = blockIdx.x * RD_BLOCK + threadIdx.x;
    if (q >= M) return;
    float v;
    bool present = true;
    if (book == 0) v = sh0[q];
    else if (book <= 15) {
        const int i = (int)(q / 3u), ch = (int)(q - 3u * (uint32_t)i), j = book - 1;
        present = j < rd_coeffs(rd_deg(degree[i]));
        v = present ? shN[dvs_shn_index(layout, i, j * 3 + ch)] : 0.0f;
    } else if (book == 16) v = opacity[q];
    else if (book == 17) v = scale[q];
    else {
        const int i = book == 18 ? (int)q : (int)(q / 3u);
        float qn[4];
        dvs_unit_quat(reinterpret_cast<const float4*>(rot)[i], qn);
        const int comp = book == 18 ? 0 : 1 + (int)(q - 3u * (uint32_t)i);
        v = comp == 0 ? qn[0] : comp == 1 ? qn[1] : comp == 2 ? qn[2] : qn[3];
    }
    keys[q] = present ? rd_key(rd_clean(v)) : RD_ABSENT;
}

// one lane: m and the exponent e with max |v| < 2^e
__global__ void k_rd_info(const uint32_t* __restrict__ s, uint32_t M, RdInfo* __restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t lo = 0, hi = M;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (s[mid] < RD_ABSENT) lo = mid + 1; else hi = mid; }
    RdInfo r;
    r.m = lo; r.e = 0; r.zero = 1; r._pad = 0;
    if (lo > 0) {
        const float A = fmaxf(fabsf(rd_unkey(s[0])), fabsf(rd_unkey(s[lo - 1])));
        if (A > 0.0f) { int e; (void)frexp((double)A, &e); r.e = e; r.zero = 0; }
    }
    *info = r;
}

// P[q] = k(s[q]) (0 past m): the addends of the prefix sum
__global__ void __launch_bounds__(RD_BLOCK)
k_rd_fixed(const uint32_t* __restrict__ s, uint32_t M, const RdInfo* __restrict__ info, uint64_t* __restrict__ P) {
    const uint32_t q = blockIdx.x * RD_BLOCK + threadIdx.x;
    if (q >= M) return;
    const RdInfo I = *info;
    long long k = 0;
    if (q < I.m && !I.zero) k = (long long)__builtin_rint(ldexp((double)rd_unkey(s[q]), 36 - I.e));
    P[q] = (uint64_t)k;
}

// #{q < m : (double)s[q] <= b}
__device__ __forceinline__ uint32_t rd_upper_bound(const uint32_t* __restrict__ s, uint32_t m, double b) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if ((double)rd_unkey(s[mid]) <= b) lo = mid + 1; else hi = mid; }
    return lo;
}
// b[0..255) of one codebook in LDS (slot 255 = +inf) -> ascending. The cluster of v is #{j : b_j < v}, which is its position among the
// SORTED boundaries whatever their order; they are out of order only when the rounding of k moved a centre past an empty cluster's.
// Every lane of the 256-lane workgroup calls it; `mine` = the lane's own slot value; returns the lane's slot value afterwards.
__device__ __forceinline__ double rd_sort_bounds(double* b, double mine) {
    const int j = threadIdx.x;
    const bool unsorted = j > 0 && j < RD_K - 1 && b[j - 1] > mine;
    if (!__syncthreads_or(unsorted ? 1 : 0)) return mine;
    int rank = j;
    if (j < RD_K - 1) {
        rank = 0;
        for (int i = 0; i < RD_K - 1; ++i) { const double o = b[i]; rank += (o < mine || (o == mine && i < j)) ? 1 : 0; }
    }
    __syncthreads();
    b[rank] = mine;
    __syncthreads();
    return b[j];
}

__global__ void __launch_bounds__(RD_BLOCK)
k_rd_lloyd(const uint32_t* __restrict__ s, const uint64_t* __restrict__ P, const RdInfo* __restrict__ info, int max_iters,
           float* __restrict__ centres /*[256] of this book*/, int32_t* __restrict__ iters) {
    __shared__ double bnd[RD_K];
    __shared__ float cs[RD_K + 1];
    __shared__ uint32_t ends[RD_K + 1];
    const int j = threadIdx.x;
    const RdInfo I = *info;
    if (I.zero) {                                          // (uniform)
        centres[j] = 0.0f;
        if (j == 0) *iters = 0;
        return;
    }
    const uint32_t m = I.m;
    float c = rd_unkey(s[(uint32_t)(((uint64_t)(2 * j + 1) * m) / 512u)]);
    uint32_t prev_end = 0xFFFFFFFFu;
    int it = 0;
    for (; it < max_iters; ++it) {
        cs[j] = c;
        __syncthreads();
        double b = j < RD_K - 1 ? ((double)c + (double)cs[j + 1]) * 0.5 : (double)__builtin_inff();
        bnd[j] = b;
        __syncthreads();
        b = rd_sort_bounds(bnd, b);
        const uint32_t end = j < RD_K - 1 ? rd_upper_bound(s, m, b) : m;
        if (!__syncthreads_or(end != prev_end ? 1 : 0)) break;
        prev_end = end;
        if (j == 0) ends[0] = 0u;
        ends[j + 1] = end;
        __syncthreads();
        const uint32_t start = ends[j];
        if (end > start) {
            const long long S = (long long)(P[end - 1] - (start > 0 ? P[start - 1] : 0ull));
            c = (float)ldexp((double)S / (double)(end - start), I.e - 36);
        }
    }
    centres[j] = c;
    if (j == 0) *iters = it;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------------------
// cnt[d * tiles + tile] = the tile's splats of degree d
__global__ void __launch_bounds__(RD_BLOCK)
k_rd_count(int n, const uint8_t* __restrict__ degree, uint32_t tiles, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t tmp[DB / 64];
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    const int d = i < n ? rd_deg(degree[i]) : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t tot;
        (void)dvs_block_excl_scan(d == k ? 1u : 0u, tmp, &tot);
        if (threadIdx.x == 0) cnt[(size_t)k * tiles + blockIdx.x] = tot;
    }
}
// counts[d] from the scanned table: base[d][0] = the splats of a lower degree
__global__ void k_rd_counts_out(int n, const uint32_t* __restrict__ base, uint32_t tiles, uint32_t* __restrict__ counts) {
    const int d = threadIdx.x;
    if (d < 4 && blockIdx.x == 0) counts[d] = (d < 3 ? base[(size_t)(d + 1) * tiles] : (uint32_t)n) - base[(size_t)d * tiles];
}

struct RdLayout { uint64_t count[4], off[4], stride[4], cum[4], table_off; int half; };

// round to nearest even; |x| >= 65520 saturates to 65504; NaN -> 0. Integer arithmetic only.
__device__ __forceinline__ uint32_t rd_half(float x) {
    const uint32_t u = __float_as_uint(x), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return 0u;                        // NaN
    if (a >= 0x477FF000u) return sign | 0x7BFFu;           // 65520 and above (infinities included): the largest finite half
    if (a < 0x33000000u) return sign;                      // below 2^-25: rounds to 0 (2^-25 itself is a tie and goes to even = 0 below)
    const int e = (int)(a >> 23) - 127;
    uint32_t mant = (a & 0x7FFFFFu) | 0x800000u;
    if (e >= -14) {                                        // normal half: keep 10 fraction bits of the 23
        const uint32_t keep = mant >> 13, rest = mant & 0x1FFFu;
        uint32_t h = ((uint32_t)(e + 15) << 10) + (keep - 0x400u);
        h += (rest > 0x1000u || (rest == 0x1000u && (keep & 1u))) ? 1u : 0u;      // (a carry out of the fraction raises the exponent: right)
        return sign | h;
    }
    const int shift = 13 + (-14 - e);                      // subnormal half: value = mant 2^(e - 23) in units of 2^-24
    const uint32_t keep = mant >> shift, rest = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    return sign | (keep + ((rest > halfway || (rest == halfway && (keep & 1u))) ? 1u : 0u));
}

// id of the (clean) value x in the codebook whose sorted boundaries are b[0..255)
__device__ __forceinline__ uint32_t rd_id(const double* b, float v) {
    const double x = (double)rd_clean(v);
    int lo = 0, hi = RD_K - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (b[mid] < x) lo = mid + 1; else hi = mid; }
    return (uint32_t)lo;
}

// the table of the file: [256][20] floats at an arbitrary byte offset
__global__ void __launch_bounds__(RD_BLOCK)
k_rd_table(const float* __restrict__ centres, uint8_t* __restrict__ out) {
    const int book = blockIdx.x, entry = threadIdx.x;
    const uint32_t u = __float_as_uint(centres[book * RD_K + entry]);
    uint8_t* p = out + ((size_t)entry * RD_BOOKS + book) * 4;
    p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); p[2] = (uint8_t)(u >> 16); p[3] = (uint8_t)(u >> 24);
}

__global__ void __launch_bounds__(RD_BLOCK)
k_pack_reduced(int n, RdLayout L, const float* __restrict__ pos, const float* __restrict__ sh0, const float* __restrict__ shN, int layout,
               const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot,
               const uint8_t* __restrict__ degree, const float* __restrict__ centres, const uint32_t* __restrict__ base, uint32_t tiles,
               uint8_t* __restrict__ out) {
    __shared__ double bnd[RD_BOOKS * RD_K];
    __shared__ uint4 img16[RD_IMG_BYTES / 16];
    __shared__ uint32_t tmp[DB / 64];
    const int tid = threadIdx.x;
    // the boundaries of the twenty codebooks, each ascending
    for (int book = 0; book < RD_BOOKS; ++book) {
        const float c = centres[book * RD_K + tid];
        const float cn = tid < RD_K - 1 ? centres[book * RD_K + tid + 1] : 0.0f;
        const double b = tid < RD_K - 1 ? ((double)c + (double)cn) * 0.5 : (double)__builtin_inff();
        bnd[book * RD_K + tid] = b;
        __syncthreads();
        (void)rd_sort_bounds(bnd + book * RD_K, b);
    }
    __syncthreads();
    // the tile's four runs: where each starts in its block and in the LDS image
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + tid;
    const bool valid = i < n;
    const int d = valid ? rd_deg(degree[i]) : -1;
    uint32_t local = 0, cnt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t ex = dvs_block_excl_scan(d == k ? 1u : 0u, tmp, &cnt[k]);
        if (d == k) local = ex;
    }
    uint64_t g0[4];
    uint32_t io[4], len[4], at = 0, my_io = 0, my_cnt = 0, my_stride = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t first = base[(size_t)k * tiles + blockIdx.x], r0 = first - L.cum[k];
        if (first < L.cum[k] || r0 + cnt[k] > L.count[k]) { cnt[k] = 0; g0[k] = 0; }       // L does not describe degree[]: nothing of this run is written
        else g0[k] = L.off[k] + r0 * L.stride[k];
        len[k] = cnt[k] * (uint32_t)L.stride[k];
        io[k] = at + (uint32_t)(g0[k] & 15u);
        at = (io[k] + len[k] + 15u) & ~15u;
        if (d == k) { my_io = io[k]; my_cnt = cnt[k]; my_stride = (uint32_t)L.stride[k]; }
    }
    uint8_t* const img = reinterpret_cast<uint8_t*>(img16);
    if (valid && my_cnt > 0) {
        uint8_t* r = img + my_io + local * my_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = pos[3 * i + k];
            if (L.half) { const uint32_t h = rd_half(p); *r++ = (uint8_t)h; *r++ = (uint8_t)(h >> 8); }
            else { const uint32_t u = __float_as_uint(p); *r++ = (uint8_t)u; *r++ = (uint8_t)(u >> 8); *r++ = (uint8_t)(u >> 16); *r++ = (uint8_t)(u >> 24); }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) *r++ = (uint8_t)rd_id(bnd, sh0[3 * i + k]);
        const int ne = 3 * rd_coeffs(d);
        for (int e = 0; e < ne; ++e) *r++ = (uint8_t)rd_id(bnd + (1 + e / 3) * RD_K, shN[dvs_shn_index(layout, (int)i, e)]);
        *r++ = (uint8_t)rd_id(bnd + 16 * RD_K, opacity[i]);
#pragma unroll
        for (int k = 0; k < 3; ++k) *r++ = (uint8_t)rd_id(bnd + 17 * RD_K, scale[3 * i + k]);
        float q[4];
        dvs_unit_quat(reinterpret_cast<const float4*>(rot)[i], q);
        *r++ = (uint8_t)rd_id(bnd + 18 * RD_K, q[0]);
#pragma unroll
        for (int k = 1; k < 4; ++k) *r++ = (uint8_t)rd_id(bnd + 19 * RD_K, q[k]);
    }
    __syncthreads();
    // a run's image starts at the same offset modulo 16 as its place in `out` (16-byte aligned): whole words move as words
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (len[k] == 0) continue;
        const uint64_t g1 = g0[k] + len[k], a0 = g0[k] & ~(uint64_t)15;
        const uint32_t words = (uint32_t)((g1 - a0 + 15) / 16), l0 = io[k] - (uint32_t)(g0[k] & 15u);
        for (uint32_t w = tid; w < words; w += RD_BLOCK) {
            const uint64_t gb = a0 + 16ull * w;
            if (gb >= g0[k] && gb + 16 <= g1) *reinterpret_cast<uint4*>(out + gb) = img16[(l0 >> 4) + w];
            else
                for (uint32_t b = 0; b < 16; ++b) if (gb + b >= g0[k] && gb + b < g1) out[gb + b] = img[l0 + 16u * w + b];
        }
    }
}

// ---- (d) ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rd_load_f32(const uint8_t* p) {
    return __uint_as_float((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
__device__ __forceinline__ float rd_unhalf(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, f = h & 0x3FFu;
    if (e == 0) return __uint_as_float(sign | __float_as_uint((float)f * 5.9604644775390625e-8f));      // f 2^-24, exact
    if (e == 31) return __uint_as_float(sign | 0x7F800000u | (f << 13));
    return __uint_as_float(sign | ((e + 112u) << 23) | (f << 13));
}

__global__ void __launch_bounds__(RD_BLOCK)
k_unpack_reduced(int n, RdLayout L, const uint8_t* __restrict__ in, float* __restrict__ pos, float* __restrict__ sh0, float* __restrict__ shN,
                 int layout, float* __restrict__ opacity, float* __restrict__ scale, float* __restrict__ rot, uint8_t* __restrict__ degree) {
    const int64_t g = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    const bool valid = g < n;
    if (!valid && (layout != DVS_SHN_TILED || g >= ((int64_t)n + 63) / 64 * 64)) return;
    const uint8_t* const tb = in + L.table_off;
    int d = 0, ne = 0;
    const uint8_t* ids = nullptr;
    if (valid) {
        d = (uint64_t)g < L.cum[1] ? 0 : (uint64_t)g < L.cum[2] ? 1 : (uint64_t)g < L.cum[3] ? 2 : 3;
        uint64_t off = L.off[0], cum = L.cum[0], stride = L.stride[0];     // (selected, not indexed: L stays in the kernel arguments)
#pragma unroll
        for (int k = 1; k < 4; ++k) if (d == k) { off = L.off[k]; cum = L.cum[k]; stride = L.stride[k]; }
        const uint8_t* r = in + off + ((uint64_t)g - cum) * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (L.half) { pos[3 * g + k] = rd_unhalf((uint32_t)r[0] | (uint32_t)r[1] << 8); r += 2; }
            else { pos[3 * g + k] = rd_load_f32(r); r += 4; }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) sh0[3 * g + k] = rd_load_f32(tb + ((size_t)r[k] * RD_BOOKS + 0) * 4);
        ids = r + 3;
        ne = 3 * rd_coeffs(d);
        const uint8_t* t = ids + ne;
        opacity[g] = rd_load_f32(tb + ((size_t)t[0] * RD_BOOKS + 16) * 4);
#pragma unroll
        for (int k = 0; k < 3; ++k) scale[3 * g + k] = rd_load_f32(tb + ((size_t)t[1 + k] * RD_BOOKS + 17) * 4);
        float4 q;
        q.x = rd_load_f32(tb + ((size_t)t[4] * RD_BOOKS + 18) * 4);
        q.y = rd_load_f32(tb + ((size_t)t[5] * RD_BOOKS + 19) * 4);
        q.z = rd_load_f32(tb + ((size_t)t[6] * RD_BOOKS + 19) * 4);
        q.w = rd_load_f32(tb + ((size_t)t[7] * RD_BOOKS + 19) * 4);
        reinterpret_cast<float4*>(rot)[g] = q;
        if (degree) degree[g] = (uint8_t)d;
    }
    if (layout == DVS_SHN_TILED) {                         // the whole tile: the pads, the lanes past the model and the absent bands are 0
        for (int c = 0; c < 12; ++c) {
            float e4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * c + k;
                e4[k] = e < ne ? rd_load_f32(tb + ((size_t)ids[e] * RD_BOOKS + 1 + e / 3) * 4) : 0.0f;
            }
            reinterpret_cast<float4*>(shN)[dvs_shn_tiled_chunk(g, c)] = make_float4(e4[0], e4[1], e4[2], e4[3]);
        }
    } else {
        for (int e = 0; e < 45; ++e) shN[g * 45 + e] = e < ne ? rd_load_f32(tb + ((size_t)ids[e] * RD_BOOKS + 1 + e / 3) * 4) : 0.0f;
    }
}

// the scratch: byte offsets of its parts, each on a 256-byte boundary
struct RdScratch { size_t sort_ws, key[2], val[2], P, bsum64, info, cnt, bsum32, total32, total; };
RdScratch rd_scratch(int n) {
    RdScratch S;
    const size_t M = 3 * (size_t)n, tiles = ((size_t)n + RD_BLOCK - 1) / RD_BLOCK;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += dvs_align256(bytes); return at; };
    S.sort_ws = take(dvs_pair_sort_ws_bytes((uint64_t)M));
    for (int k = 0; k < 2; ++k) { S.key[k] = take(M * 4); S.val[k] = take(M * 4); }
    S.P = take(M * 8);
    S.bsum64 = take(((M + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 8);
    S.info = take(sizeof(RdInfo));
    S.cnt = take(4 * tiles * 4);
    S.bsum32 = take(((4 * tiles + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 4);
    S.total32 = take(8);
    S.total = o;
    return S;
}

// degree[] -> the scanned [4][tiles] table in scratch (base[d][tile] = the block-order index of the tile's first splat of degree d)
hipError_t rd_partition(hipStream_t st, int n, const uint8_t* degree, char* scratch, const RdScratch& S, uint32_t tiles) {
    uint32_t* const cnt = (uint32_t*)(scratch + S.cnt);
    hipLaunchKernelGGL(k_rd_count, dim3(tiles), dim3(RD_BLOCK), 0, st, n, degree, tiles, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return dvs_launch_scan_u32(st, cnt, 4 * (size_t)tiles, (uint32_t*)(scratch + S.bsum32), (unsigned long long*)(scratch + S.total32));
}
RdLayout rd_layout(const dvs_reduced_layout* L) {
    RdLayout R;
    uint64_t cum = 0;
    for (int k = 0; k < 4; ++k) { R.count[k] = L->count[k]; R.off[k] = L->off[k]; R.stride[k] = L->stride[k]; R.cum[k] = cum; cum += L->count[k]; }
    R.table_off = L->table_off;
    R.half = L->half;
    return R;
}
// L is what dvs_reduced_layout_for makes of its own counts and half
bool layout_ok(const dvs_reduced_layout* L, int n) {
    if (!L || (L->half != 0 && L->half != 1)) return false;
    uint32_t c[4];
    uint64_t sum = 0;
    for (int k = 0; k < 4; ++k) { if (L->count[k] > 0x7FFFFFFFull) return false; c[k] = (uint32_t)L->count[k]; sum += L->count[k]; }
    dvs_reduced_layout W;
    if (sum != (uint64_t)n || dvs_reduced_layout_for(c, L->half, &W) != DVS_OK) return false;
    for (int k = 0; k < 4; ++k) if (W.off[k] != L->off[k] || W.stride[k] != L->stride[k]) return false;
    return W.table_off == L->table_off && W.total == L->total;
}
}  // namespace

extern "C" size_t dvs_reduced_scratch_bytes(int n) { return n > 0 ? rd_scratch(n).total : 0; }

extern "C" int dvs_sh_degree_select(void* stream, int n, int D, const float* pos, const float* shN, int shn_layout, const float* cams, int C,
                                    float t, uint8_t* degree) {
    if (n <= 0 || D < 0 || D > 3 || C <= 0 || !(t >= 0.0f) || (!shN && D > 0)) return DVS_ERR_INVALID;
    if (dvs_bad_args({pos, cams, degree}, {shN}, shn_layout)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblocks = (unsigned)(((int64_t)n + RD_BLOCK - 1) / RD_BLOCK);
    switch (D) {
        case 0: if (hipMemsetAsync(degree, 0, (size_t)n, st) != hipSuccess) return DVS_ERR_HIP; break;      // err_0 = err_D = 0
        case 1: hipLaunchKernelGGL(k_sh_degree<1>, dim3(nblocks), dim3(RD_BLOCK), 0, st, n, pos, shN, shn_layout, cams, C, t, degree); break;
        case 2: hipLaunchKernelGGL(k_sh_degree<2>, dim3(nblocks), dim3(RD_BLOCK), 0, st, n, pos, shN, shn_layout, cams, C, t, degree); break;
        default: hipLaunchKernelGGL(k_sh_degree<3>, dim3(nblocks), dim3(RD_BLOCK), 0, st, n, pos, shN, shn_layout, cams, C, t, degree); break;
    }
    return dvs_launch_status();
}

extern "C" int dvs_codebooks_build(void* stream, int n, const float* sh0, const float* shN, int shn_layout, const float* opacity,
                                   const float* scale, const float* rot, const uint8_t* degree, int max_iters, void* scratch, float* centres,
                                   int32_t* iters) {
    if (n <= 0 || 3 * (int64_t)n > DVS_REDUCED_MAX_VALUES || max_iters < 1) return DVS_ERR_INVALID;
    if (dvs_bad_args({sh0, shN, opacity, scale, rot, degree, scratch, centres, iters}, {}, shn_layout)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const RdScratch S = rd_scratch(n);
    char* const base = (char*)scratch;
    uint32_t* key[2] = {(uint32_t*)(base + S.key[0]), (uint32_t*)(base + S.key[1])};
    uint32_t* val[2] = {(uint32_t*)(base + S.val[0]), (uint32_t*)(base + S.val[1])};
    uint64_t* const P = (uint64_t*)(base + S.P);
    RdInfo* const info = (RdInfo*)(base + S.info);
    for (int book = 0; book < RD_BOOKS; ++book) {
        const uint32_t M = (book == 16 || book == 18) ? (uint32_t)n : 3u * (uint32_t)n;
        const unsigned nblocks = (M + RD_BLOCK - 1) / RD_BLOCK;
        hipLaunchKernelGGL(k_rd_keys, dim3(nblocks), dim3(RD_BLOCK), 0, st, book, n, M, sh0, shN, shn_layout, opacity, scale, rot, degree, key[0]);
        if (hipGetLastError() != hipSuccess) return DVS_ERR_HIP;
        int cur = 0;                                       // all 32 key bits, ballot ranking. The values ride along uninitialised and unread.
        if (dvs_launch_pair_sort(st, M, key[0], val[0], key[1], val[1], 0, 32, dvs_pair_sort_ws_at(base + S.sort_ws), 0, &cur) != hipSuccess)
            return DVS_ERR_HIP;
        const uint32_t* const s = key[cur];
        hipLaunchKernelGGL(k_rd_info, dim3(1), dim3(64), 0, st, s, M, info);
        hipLaunchKernelGGL(k_rd_fixed, dim3(nblocks), dim3(RD_BLOCK), 0, st, s, M, (const RdInfo*)info, P);
        if (hipGetLastError() != hipSuccess) return DVS_ERR_HIP;
        if (dvs_launch_scan_incl_u64(st, P, (size_t)M, (uint64_t*)(base + S.bsum64)) != hipSuccess) return DVS_ERR_HIP;
        hipLaunchKernelGGL(k_rd_lloyd, dim3(1), dim3(RD_BLOCK), 0, st, s, (const uint64_t*)P, (const RdInfo*)info, max_iters, centres + book * RD_K,
                           iters + book);
    }
    return dvs_launch_status();
}

extern "C" int dvs_reduced_degree_counts(void* stream, int n, const uint8_t* degree, void* scratch, uint32_t* counts) {
    if (n <= 0 || dvs_bad_args({degree, scratch, counts})) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const RdScratch S = rd_scratch(n);
    const uint32_t tiles = (uint32_t)(((int64_t)n + RD_BLOCK - 1) / RD_BLOCK);
    if (rd_partition(st, n, degree, (char*)scratch, S, tiles) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_rd_counts_out, dim3(1), dim3(64), 0, st, n, (const uint32_t*)((char*)scratch + S.cnt), tiles, counts);
    return dvs_launch_status();
}

extern "C" int dvs_reduced_layout_for(const uint32_t counts[4], int half, dvs_reduced_layout* out) {
    if (!counts || !out || half < 0 || half > 1) return DVS_ERR_INVALID;
    const uint64_t sum = (uint64_t)counts[0] + counts[1] + counts[2] + counts[3];
    if (sum == 0 || sum > 0x7FFFFFFFull) return DVS_ERR_INVALID;
    uint64_t o = 0;
    for (int d = 0; d < 4; ++d) {
        out->count[d] = counts[d];
        out->off[d] = o;
        out->stride[d] = (uint64_t)(half ? 6 : 12) + 3 + 3 * (uint64_t)((d + 1) * (d + 1) - 1) + 8;
        o += out->count[d] * out->stride[d];
    }
    out->table_off = o;
    out->total = o + (uint64_t)DVS_REDUCED_BOOKS * DVS_REDUCED_ENTRIES * 4;
    out->half = half;
    out->_pad = 0;
    return DVS_OK;
}

extern "C" int dvs_pack_reduced(void* stream, int n, const float* pos, const float* sh0, const float* shN, int shn_layout, const float* opacity,
                                const float* scale, const float* rot, const uint8_t* degree, const float* centres, void* scratch,
                                const dvs_reduced_layout* L, uint8_t* out) {
    if (n <= 0 || !layout_ok(L, n) || dvs_bad_args({pos, sh0, shN, opacity, scale, rot, degree, centres, scratch, out}, {}, shn_layout)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const RdScratch S = rd_scratch(n);
    const uint32_t tiles = (uint32_t)(((int64_t)n + RD_BLOCK - 1) / RD_BLOCK);
    if (rd_partition(st, n, degree, (char*)scratch, S, tiles) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_pack_reduced, dim3(tiles), dim3(RD_BLOCK), 0, st, n, rd_layout(L), pos, sh0, shN, shn_layout, opacity, scale, rot, degree,
                       centres, (const uint32_t*)((char*)scratch + S.cnt), tiles, out);
    hipLaunchKernelGGL(k_rd_table, dim3(RD_BOOKS), dim3(RD_K), 0, st, centres, out + L->table_off);
    return dvs_launch_status();
}

extern "C" int dvs_unpack_reduced(void* stream, int n, const uint8_t* packed, const dvs_reduced_layout* L, float* pos, float* sh0, float* shN,
                                  int shn_layout, float* opacity, float* scale, float* rot, uint8_t* degree) {
    if (n <= 0 || !layout_ok(L, n) || dvs_bad_args({packed, pos, sh0, shN, opacity, scale, rot}, {degree}, shn_layout)) return DVS_ERR_INVALID;
    const int64_t lanes = shn_layout == DVS_SHN_TILED ? ((int64_t)n + 63) / 64 * 64 : (int64_t)n;
    const unsigned nblocks = (unsigned)((lanes + RD_BLOCK - 1) / RD_BLOCK);
    hipLaunchKernelGGL(k_unpack_reduced, dim3(nblocks), dim3(RD_BLOCK), 0, (hipStream_t)stream, n, rd_layout(L), packed, pos, sh0, shN, shn_layout,
                       opacity, scale, rot, degree);
    return dvs_launch_status();
}
