// knn.hip — splat initialisation from a sparse point cloud (include/dvs_init.h): the mean squared distance of every point to its 3
// nearest neighbours, by the published simple-knn scheme, and the per-point initial parameters.
//   (a) - (c) the model's box, 30-bit Morton keys, the stable segmented sort: pack.hip's kernels through dvs_launch_morton_order.
//   (d) k_knn_gather: one workgroup of 256 lanes per box of 1024 consecutive sorted points; a lane gathers four points by sorted index
//       and leaves them as 16-byte records {x, y, z, model index}; the box's corners go out as two 16-byte records.
//   (e) k_knn_search: one lane owns one point, a wavefront owns 64 Morton-consecutive points (all in ONE box: 1024 = 16 x 64). The
//       +-3 neighbours in sorted order give a first bound `rej` on the third-best distance. Then the wave's own box and after it every
//       other box: a box is skipped for the whole wavefront when every lane's lower bound exceeds min(rej, current third best) — one
//       ballot, no divergence — otherwise its records are streamed to all lanes through WAVE-UNIFORM addresses (the loads are scalar
//       loads of 16-byte records, broadcast by construction; nothing is staged in LDS, so the waves of a workgroup prune
//       independently and never meet at a barrier). Each lane keeps its three best in registers with a branch-free min / max
//       insert; the own point is excluded by its sorted position, not by its distance (a duplicate is a neighbour at 0).
//       dist2 goes back in model order: a scatter by the record's model index.
// Why pruning does not cost exactness (the bit-for-bit test rests on this). Per axis the gap is g = max(bmin - p, p - bmax, 0) and
// the bound lb = (gx gx + gy gy) + gz gz, in the operation order of the distance itself. For a member q of the box, bmin <= q <= bmax,
// hence q - p >= bmin - p and p - q >= p - bmax in exact arithmetic; fp32 rounding is monotone, so |fl(q - p)| >= g, and the same
// holds through each product and each sum: lb <= the member's computed d2. A box is skipped only when lb > t (strictly) for a value
// t that is the third smallest of distances already seen (or of the seed's), i.e. t >= the final third-best value: every member then
// has d2 > t and cannot enter or change the three smallest VALUES. Compiled without contraction (EXACT). No atomics, no inline
// assembly, no LDS in the search kernel, plain vector stores.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "export_common.h"
#include "../../include/dvs_raster.h"
#include "../../include/dvs_init.h"

namespace {
constexpr int KN_BLOCK = 256, KN_WAVES = KN_BLOCK / 64;
constexpr int KN_BOX = 1024;                               // sorted points per box
constexpr int KN_PER_LANE = KN_BOX / KN_BLOCK;             // points a lane of k_knn_gather handles
constexpr float KN_INF = __builtin_inff();

// (d) box b = sorted entries [1024 b, min(n, 1024 b + 1024))
__global__ void __launch_bounds__(KN_BLOCK)
k_knn_gather(int n, const uint32_t* __restrict__ sorted, const float* __restrict__ pos, float4* __restrict__ rec, float4* __restrict__ box) {
    __shared__ float lds[KN_WAVES * 6];
    float lo[3] = {KN_INF, KN_INF, KN_INF}, hi[3] = {-KN_INF, -KN_INF, -KN_INF};
#pragma unroll
    for (int r = 0; r < KN_PER_LANE; ++r) {
        const int64_t j = (int64_t)blockIdx.x * KN_BOX + r * KN_BLOCK + threadIdx.x;
        if (j < n) {
            const uint32_t id = sorted[j];
            const float x = pos[3 * (size_t)id], y = pos[3 * (size_t)id + 1], z = pos[3 * (size_t)id + 2];
            rec[j] = make_float4(x, y, z, __uint_as_float(id));
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d, 64)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d, 64)); }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { lds[wave * 6 + k] = lo[k]; lds[wave * 6 + 3 + k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < KN_WAVES; ++w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], lds[w * 6 + k]); hi[k] = fmaxf(hi[k], lds[w * 6 + 3 + k]); }
        }
        box[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.f);
        box[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

__device__ __forceinline__ float kn_d2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}
// d into the ascending triple (b0, b1, b2), branch-free
__device__ __forceinline__ void kn_insert(float d, float& b0, float& b1, float& b2) {
    const float t0 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    const float t1 = fmaxf(b1, t0);
    b1 = fminf(b1, t0);
    b2 = fminf(b2, t1);
}

// the records [first, last) of one box streamed to every lane: `first`, `last` and the addresses are wave-uniform
__device__ __forceinline__ void kn_stream(const float4* __restrict__ rec, int first, int last, int self, float px, float py, float pz,
                                          float& b0, float& b1, float& b2) {
#pragma unroll 8
    for (int j = first; j < last; ++j) {
        const float4 q = rec[j];
        float d = kn_d2(px, py, pz, q.x, q.y, q.z);
        d = j == self ? KN_INF : d;
        kn_insert(d, b0, b1, b2);
    }
}

// (e) lane = sorted position s; out of range lanes of the last wavefront vote "skip" and store nothing
__global__ void __launch_bounds__(KN_BLOCK)
k_knn_search(int n, int n_boxes, const float4* __restrict__ rec, const float4* __restrict__ box, float* __restrict__ dist2,
             unsigned long long* __restrict__ visited /*nullable: [waves] boxes streamed per wavefront (measurement only)*/) {
    const int64_t s64 = (int64_t)blockIdx.x * KN_BLOCK + threadIdx.x;
    const int wave_first = (int)__builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * KN_BLOCK + threadIdx.x) & ~(int64_t)63));
    if (wave_first >= n) return;                            // a whole wavefront past the end (wave-uniform)
    const bool valid = s64 < n;
    const int s = valid ? (int)s64 : n - 1;
    const float4 me = rec[s];
    const float px = me.x, py = me.y, pz = me.z;
    // seed: the third smallest distance among the +-3 neighbours in sorted order bounds the final third-best from above
    float r0 = KN_INF, r1 = KN_INF, r2 = KN_INF;
#pragma unroll
    for (int o = -3; o <= 3; ++o) {
        if (o == 0) continue;
        const int j = s + o;
        const bool in = j >= 0 && j < n;
        const float4 q = rec[in ? j : s];
        const float d = kn_d2(px, py, pz, q.x, q.y, q.z);
        kn_insert(in ? d : KN_INF, r0, r1, r2);
    }
    const float rej = r2;
    float b0 = KN_INF, b1 = KN_INF, b2 = KN_INF;
    const int own = wave_first / KN_BOX;
    kn_stream(rec, own * KN_BOX, (int)min((int64_t)n, (int64_t)own * KN_BOX + KN_BOX), valid ? s : -1, px, py, pz, b0, b1, b2);
    unsigned long long streamed = 1;
    for (int b = 0; b < n_boxes; ++b) {
        if (b == own) continue;
        const float4 lo = box[2 * (size_t)b], hi = box[2 * (size_t)b + 1];
        const float gx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.0f),
                    gz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.0f);
        const float lb = (gx * gx + gy * gy) + gz * gz;
        const bool skip = !valid || lb > fminf(rej, b2);                     // strictly greater: see the head of the file
        if (__ballot(!skip) == 0ull) continue;
        kn_stream(rec, b * KN_BOX, (int)min((int64_t)n, (int64_t)b * KN_BOX + KN_BOX), -1, px, py, pz, b0, b1, b2);
        ++streamed;
    }
    if (visited && (threadIdx.x & 63) == 0) visited[((int64_t)blockIdx.x * KN_BLOCK + threadIdx.x) >> 6] = streamed;
    if (!valid) return;
    float r;
    if (n >= 4) r = ((b0 + b1) + b2) / 3.0f;
    else if (n == 3) r = (b0 + b1) / 2.0f;
    else if (n == 2) r = b0;
    else r = 0.0f;
    dist2[__float_as_uint(me.w)] = r;
}

__global__ void __launch_bounds__(KN_BLOCK)
k_init_from_points(int n, const uint8_t* __restrict__ rgb, const float* __restrict__ dist2, float opacity0, float* __restrict__ sh0,
                   float* __restrict__ opacity, float* __restrict__ scale, float4* __restrict__ rot) {
    const int64_t i = (int64_t)blockIdx.x * KN_BLOCK + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) sh0[3 * i + k] = ((float)rgb[3 * i + k] / 255.0f - 0.5f) / DVS_SH_C0;
    opacity[i] = opacity0;
    const float sc = 0.5f * logf(fmaxf(dist2[i], 1e-7f));
    scale[3 * i] = sc; scale[3 * i + 1] = sc; scale[3 * i + 2] = sc;
    rot[i] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
}

struct KnnScratch { size_t morton, rec, box, total; };
KnnScratch knn_layout(int n) {
    const auto up = dvs_align256;
    KnnScratch L;
    size_t o = 0;
    L.morton = o; o += up(dvs_morton_scratch_bytes(n));
    L.rec = o; o += up((size_t)n * sizeof(float4));
    L.box = o; o += up((size_t)(((int64_t)n + KN_BOX - 1) / KN_BOX) * 2 * sizeof(float4));
    L.total = o;
    return L;
}

int knn_run(hipStream_t st, int n, const float* pos, void* scratch, float* dist2, unsigned long long* visited) {
    const KnnScratch L = knn_layout(n);
    char* const base = (char*)scratch;
    float4* const rec = (float4*)(base + L.rec);
    float4* const box = (float4*)(base + L.box);
    const uint32_t* sorted = nullptr;
    if (dvs_launch_morton_order(st, n, pos, base + L.morton, &sorted, nullptr) != hipSuccess) return DVS_ERR_HIP;
    const int n_boxes = (int)(((int64_t)n + KN_BOX - 1) / KN_BOX);
    hipLaunchKernelGGL(k_knn_gather, dim3((unsigned)n_boxes), dim3(KN_BLOCK), 0, st, n, sorted, pos, rec, box);
    const unsigned sblocks = (unsigned)(((int64_t)n + KN_BLOCK - 1) / KN_BLOCK);
    hipLaunchKernelGGL(k_knn_search, dim3(sblocks), dim3(KN_BLOCK), 0, st, n, n_boxes, (const float4*)rec, (const float4*)box, dist2, visited);
    return dvs_launch_status();
}
}  // namespace

extern "C" size_t dvs_knn_scratch_bytes(int n) { return n > 0 ? knn_layout(n).total : 0; }

extern "C" int dvs_knn_mean_dist2(void* stream, int n, const float* pos, void* scratch, float* dist2) {
    if (n <= 0 || dvs_bad_args({pos, scratch, dist2})) return DVS_ERR_INVALID;
    return knn_run((hipStream_t)stream, n, pos, scratch, dist2, nullptr);
}

extern "C" int dvs_knn_mean_dist2_stats(void* stream, int n, const float* pos, void* scratch, float* dist2, uint64_t* boxes_streamed) {
    if (n <= 0 || dvs_bad_args({pos, scratch, dist2, boxes_streamed})) return DVS_ERR_INVALID;
    return knn_run((hipStream_t)stream, n, pos, scratch, dist2, (unsigned long long*)boxes_streamed);
}

extern "C" int dvs_init_from_points(void* stream, int n, const float* pos, const uint8_t* rgb, const float* dist2, float* sh0, float* opacity,
                                    float* scale, float* rot) {
    if (n <= 0 || dvs_bad_args({pos, rgb, dist2, sh0, opacity, scale, rot})) return DVS_ERR_INVALID;
    const float opacity0 = (float)std::log((double)(0.1f / 0.9f));          // the logit of 0.1, rounded once
    const unsigned nblocks = (unsigned)(((int64_t)n + KN_BLOCK - 1) / KN_BLOCK);
    hipLaunchKernelGGL(k_init_from_points, dim3(nblocks), dim3(KN_BLOCK), 0, (hipStream_t)stream, n, rgb, dist2, opacity0, sh0, opacity, scale,
                       (float4*)rot);
    return dvs_launch_status();
}
