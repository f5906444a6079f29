// lod.hip — level-of-detail export: the splats of every cell of a lattice merged into one splat that matches their weighted first and
// second moments, for gfx950 (include/dvs_export.h, last section, has the definition; tests/lod_ref.py restates it in numpy). The splat
// counterpart of mesh_decimate.hip, whose two-call shape it shares.
//
// Counting (dvs_lod_merge_count):
//   k_lod_keys        key[i] = the cell of splat i (30 bits; a splat with a non-finite centre, opacity, scale or rotation: DVS_CELL_NONE,
//                     counted), val[i] = i, wgt[i] = alpha (sigma0 sigma1 sigma2)^(2/3)
//   clustering        cell_cluster.hip: the splats sorted by (cell, index) over 31 bits, the dropped ones last; first sorted position of every cluster
//   k_lod_alive       one lane per cluster: a cluster of one member lives; a larger one lives when W = the serial sum of its members'
//                     weights is > 0, else its members are counted as dropped
//   scan              alive -> exclusive: the output index of a live cluster; the total is m
// Writing (dvs_lod_merge_write):
//   k_lod_gather      a 48-byte record {p, w | cov (6)} per member in sorted order, three 16-byte stores by consecutive lanes
//   k_lod_geometry    one lane per cluster over its contiguous run: W and the mean, then the centred second moment (two passes: a one-pass
//                     formula cancels), cyclic Jacobi in registers, pos / scale / rot / opacity; a cluster of one copies its member
//   k_lod_colour      one thread per (cluster, 16-byte chunk of the 45 + 3 colour floats): the weighted means in the same member order
//   k_lod_pads        DVS_SHN_TILED output: the lanes of the last tile past m are zero
//
// The only atomics are integer additions to one counter. No kernel waits for another workgroup: phases are launches. Every device loop
// is bounded by n. No LDS, no scratch memory, no inline assembly. 256-lane workgroups: the kernels stream or gather global memory and
// hold no workgroup-shared state, so four waves per workgroup only set the dispatch granularity; the geometry walk is the one kernel
// with a large live set (two 3 x 3 matrices and the sums) and stays below the 128-register line that halves the waves per SIMD.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include "cell_cluster.h"
#include "export_common.h"
#include "../../include/dvs_export.h"

#define LB 256
#define LOD_SWEEPS 12                                                       /* cyclic Jacobi on 3 x 3 in fp32 converges in 4 - 6 */

namespace {
// the words the passes share and the host reads (one 64-byte block at the end of the scratch)
struct LodBlock {
    unsigned long long n_clusters, m;                                     // the scans' totals
    uint32_t n_dropped, _pad[11];
};
static_assert(sizeof(LodBlock) == 64, "one block of words");

struct LodLayout {
    DvsClusterLayout c;
    size_t wgt, coff, rec[3], block, total;
};
LodLayout lod_layout(uint32_t n_in) {
    LodLayout L{};
    const size_t n = n_in ? n_in : 1;
    L.c = dvs_cluster_layout(n);
    size_t o = L.c.end;
    L.wgt = dvs_carve(o, n * 4);
    L.coff = dvs_carve(o, n * 4);
    for (int k = 0; k < 3; ++k) L.rec[k] = dvs_carve(o, n * 16);
    L.block = dvs_carve(o, sizeof(LodBlock));
    L.total = o;
    return L;
}

__device__ __forceinline__ bool lod_finite(float x) { return fabsf(x) < __builtin_inff(); }

__global__ void k_lod_init(LodBlock* blk) { blk->n_clusters = 0; blk->m = 0; blk->n_dropped = 0; }

// One thread per splat. No lane leaves early: the wave's leader adds the wave's count.
__global__ void __launch_bounds__(LB)
k_lod_keys(uint32_t n, const float* __restrict__ pos, const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot,
           DvsCellLattice g, uint32_t* __restrict__ key, uint32_t* __restrict__ val, float* __restrict__ wgt, LodBlock* blk) {
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    bool dropped = false;
    if (i < n) {
        const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2], o = opacity[i];
        const float s0 = scale[3 * i], s1 = scale[3 * i + 1], s2 = scale[3 * i + 2];
        const float4 r = reinterpret_cast<const float4*>(rot)[i];
        const bool fin = lod_finite(x) && lod_finite(y) && lod_finite(z) && lod_finite(o) && lod_finite(s0) && lod_finite(s1) && lod_finite(s2) &&
                         lod_finite(r.x) && lod_finite(r.y) && lod_finite(r.z) && lod_finite(r.w);
        dropped = !fin;
        uint32_t k = DVS_CELL_NONE;
        float w = 0.0f;
        if (fin) {
            k = dvs_cell_key(x, y, z, g);
            const float alpha = 1.0f / (1.0f + expf(-o));
            w = alpha * expf(((s0 + s1) + s2) * 0.6666666666666666f);      // (sigma0 sigma1 sigma2)^(2/3)
        }
        key[i] = k; val[i] = (uint32_t)i; wgt[i] = w;
    }
    const uint32_t nd = (uint32_t)__popcll(__ballot(dropped));
    if ((threadIdx.x & 63u) == 0u && nd) atomicAdd(&blk->n_dropped, nd);
}
// One lane per cluster: alive[c] = 1 when the cluster is written. W is the serial sum in ascending splat index, the same sum
// k_lod_geometry forms from the records (which hold these very words).
__global__ void __launch_bounds__(LB)
k_lod_alive(uint32_t n, LodBlock* blk, const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ sidx, const float* __restrict__ wgt,
            uint32_t* __restrict__ alive) {
    const size_t c = (size_t)blockIdx.x * LB + threadIdx.x;
    if (c >= n) return;
    uint32_t a = 0u, first, end;
    if (dvs_cluster_run(c, n, blk->n_clusters, cstart, &first, &end)) {
        if (first + 1u == end) a = 1u;
        else {
            float W = 0.0f;
            for (uint32_t m = first; m < end; ++m) { const uint32_t v = sidx[m]; W = W + (v < n ? wgt[v] : 0.0f); }
            if (W > 0.0f) a = 1u;
            else atomicAdd(&blk->n_dropped, end - first);
        }
    }
    alive[c] = a;
}

// ---- writing --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LB)
k_lod_gather(uint32_t n, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const float* __restrict__ pos, const float* __restrict__ scale,
             const float* __restrict__ rot, const float* __restrict__ wgt, float4* __restrict__ rec0, float4* __restrict__ rec1, float4* __restrict__ rec2) {
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    if (i >= n || skey[i] == DVS_CELL_NONE) return;
    const size_t v = sidx[i];
    if (v >= n) return;                                                      // (never: sidx is a permutation of [0, n))
    float q[4], R[9], cov[6];
    dvs_unit_quat(reinterpret_cast<const float4*>(rot)[v], q);
    dvs_quat_to_rot(q[0], q[1], q[2], q[3], R);
    const float s[3] = {expf(scale[3 * v]), expf(scale[3 * v + 1]), expf(scale[3 * v + 2])};
    dvs_cov3d(s, R, cov);
    rec0[i] = make_float4(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2], wgt[v]);
    rec1[i] = make_float4(cov[0], cov[1], cov[2], cov[3]);
    rec2[i] = make_float4(cov[4], cov[5], 0.0f, 0.0f);
}

// one rotation of the cyclic Jacobi method in the (P, Q) plane: every index is a compile-time constant, the matrices stay in registers
template <int P, int Q>
__device__ __forceinline__ void lod_rotate(float (&a)[3][3], float (&v)[3][3]) {
    constexpr int R = 3 - P - Q;
    const float apq = a[P][Q];
    if (apq == 0.0f) return;
    const float theta = (a[Q][Q] - a[P][P]) / (2.0f * apq);
    const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (fabsf(theta) + dvs_sqrt_rn(theta * theta + 1.0f));
    const float c = 1.0f / dvs_sqrt_rn(t * t + 1.0f), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = 0.0f; a[Q][P] = 0.0f;
    const float arp = a[R][P], arq = a[R][Q];
    a[R][P] = c * arp - s * arq; a[P][R] = a[R][P];
    a[R][Q] = s * arp + c * arq; a[Q][R] = a[R][Q];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// One lane per cluster over its records [cstart[c], cstart[c + 1]): the members in ascending splat index. The sums are serial in that
// order — that order is the definition — so a cluster is one lane's work however many members it has.
__global__ void __launch_bounds__(LB)
k_lod_geometry(uint32_t n, const LodBlock* __restrict__ blk, const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ alive, const uint32_t* __restrict__ coff,
               const uint32_t* __restrict__ sidx, const float4* __restrict__ rec0, const float4* __restrict__ rec1, const float4* __restrict__ rec2,
               const float* __restrict__ pos, const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot,
               float* __restrict__ pos_out, float* __restrict__ opacity_out, float* __restrict__ scale_out, float* __restrict__ rot_out) {
    const size_t c = (size_t)blockIdx.x * LB + threadIdx.x;
    uint32_t first, end;
    if (!dvs_cluster_run(c, n, blk->n_clusters, cstart, &first, &end) || !alive[c]) return;
    const size_t o = coff[c];                                                // < m <= n
    if (first + 1u == end) {                                                 // one member: its rows, bit for bit
        const size_t v = sidx[first];
        if (v >= n) return;
        pos_out[3 * o] = pos[3 * v]; pos_out[3 * o + 1] = pos[3 * v + 1]; pos_out[3 * o + 2] = pos[3 * v + 2];
        scale_out[3 * o] = scale[3 * v]; scale_out[3 * o + 1] = scale[3 * v + 1]; scale_out[3 * o + 2] = scale[3 * v + 2];
        reinterpret_cast<float4*>(rot_out)[o] = reinterpret_cast<const float4*>(rot)[v];
        opacity_out[o] = opacity[v];
        return;
    }
    float W = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t m = first; m < end; ++m) {
        const float4 r = rec0[m];
        W = W + r.w; sx = sx + r.w * r.x; sy = sy + r.w * r.y; sz = sz + r.w * r.z;
    }
    const float mx = sx / W, my = sy / W, mz = sz / W;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, c4 = 0.0f, c5 = 0.0f;
    for (uint32_t m = first; m < end; ++m) {
        const float4 r = rec0[m], a = rec1[m], b = rec2[m];
        const float dx = r.x - mx, dy = r.y - my, dz = r.z - mz;
        c0 = c0 + r.w * (a.x + dx * dx); c1 = c1 + r.w * (a.y + dx * dy); c2 = c2 + r.w * (a.z + dx * dz);
        c3 = c3 + r.w * (a.w + dy * dy); c4 = c4 + r.w * (b.x + dy * dz); c5 = c5 + r.w * (b.y + dz * dz);
    }
    float A[3][3], V[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
    A[0][0] = c0 / W; A[0][1] = c1 / W; A[0][2] = c2 / W; A[1][1] = c3 / W; A[1][2] = c4 / W; A[2][2] = c5 / W;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
#pragma nounroll
    for (int sweep = 0; sweep < LOD_SWEEPS; ++sweep) {
        if (A[0][1] == 0.0f && A[0][2] == 0.0f && A[1][2] == 0.0f) break;
        lod_rotate<0, 1>(A, V);
        lod_rotate<0, 2>(A, V);
        lod_rotate<1, 2>(A, V);
    }
    const float lmax = fmaxf(fmaxf(A[0][0], A[1][1]), A[2][2]), lfloor = 1e-7f * lmax;
    const float l0 = logf(fmaxf(A[0][0], lfloor)), l1 = logf(fmaxf(A[1][1], lfloor)), l2 = logf(fmaxf(A[2][2], lfloor));
    // a proper rotation: the third column negated when the determinant is negative
    const float det = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0])) +
                      V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    if (det < 0.0f) { V[0][2] = -V[0][2]; V[1][2] = -V[1][2]; V[2][2] = -V[2][2]; }
    // its quaternion: the branch of the largest of trace, V00, V11, V22 (transform.hip's tf_quat_of in fp32), unit, w >= 0
    float qw, qx, qy, qz;
    const float tr = (V[0][0] + V[1][1]) + V[2][2];
    if (tr >= V[0][0] && tr >= V[1][1] && tr >= V[2][2]) {
        const float S = dvs_sqrt_rn(tr + 1.0f) * 2.0f;
        qw = 0.25f * S; qx = (V[2][1] - V[1][2]) / S; qy = (V[0][2] - V[2][0]) / S; qz = (V[1][0] - V[0][1]) / S;
    } else if (V[0][0] >= V[1][1] && V[0][0] >= V[2][2]) {
        const float S = dvs_sqrt_rn(((1.0f + V[0][0]) - V[1][1]) - V[2][2]) * 2.0f;
        qw = (V[2][1] - V[1][2]) / S; qx = 0.25f * S; qy = (V[0][1] + V[1][0]) / S; qz = (V[0][2] + V[2][0]) / S;
    } else if (V[1][1] >= V[2][2]) {
        const float S = dvs_sqrt_rn(((1.0f + V[1][1]) - V[0][0]) - V[2][2]) * 2.0f;
        qw = (V[0][2] - V[2][0]) / S; qx = (V[0][1] + V[1][0]) / S; qy = 0.25f * S; qz = (V[1][2] + V[2][1]) / S;
    } else {
        const float S = dvs_sqrt_rn(((1.0f + V[2][2]) - V[0][0]) - V[1][1]) * 2.0f;
        qw = (V[1][0] - V[0][1]) / S; qx = (V[0][2] + V[2][0]) / S; qy = (V[1][2] + V[2][1]) / S; qz = 0.25f * S;
    }
    const float len = dvs_sqrt_rn(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / len; qx = qx / len; qy = qy / len; qz = qz / len;
    if (qw < 0.0f) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    // the opacity that keeps the cluster's total weight
    const float gm = expf(((l0 + l1) + l2) / 3.0f);
    const float alpha = fminf(DVS_ALPHA_MAX, W / gm);
    pos_out[3 * o] = mx; pos_out[3 * o + 1] = my; pos_out[3 * o + 2] = mz;
    scale_out[3 * o] = 0.5f * l0; scale_out[3 * o + 1] = 0.5f * l1; scale_out[3 * o + 2] = 0.5f * l2;
    reinterpret_cast<float4*>(rot_out)[o] = make_float4(qw, qx, qy, qz);
    opacity_out[o] = logf(alpha / (1.0f - alpha));
}

// the four colour floats of chunk ch (0 .. 11) of splat v: elements 4 ch .. 4 ch + 3 of shN, and for ch = 11 {shN[44], sh0 r, g, b}
__device__ __forceinline__ float4 lod_colour_chunk(const float* __restrict__ sh0, const float* __restrict__ shN, int tiled, size_t v, int ch) {
    float4 r;
    if (tiled) r = reinterpret_cast<const float4*>(shN)[dvs_shn_tiled_chunk((int64_t)v, ch)];
    else if (ch < 11) r = make_float4(shN[v * 45 + 4 * ch], shN[v * 45 + 4 * ch + 1], shN[v * 45 + 4 * ch + 2], shN[v * 45 + 4 * ch + 3]);
    else r.x = shN[v * 45 + 44];
    if (ch == 11) { r.y = sh0[3 * v]; r.z = sh0[3 * v + 1]; r.w = sh0[3 * v + 2]; }
    return r;
}
// blockIdx.y = the chunk; consecutive lanes hold consecutive clusters, whose outputs are (nearly always) consecutive splats: in the
// tiled layout a wave's stores of one chunk are contiguous. `limit` = the shN elements of the bands <= D (0, 9, 24, 45).
__global__ void __launch_bounds__(LB)
k_lod_colour(uint32_t n, int limit, const LodBlock* __restrict__ blk, const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ alive,
             const uint32_t* __restrict__ coff, const uint32_t* __restrict__ sidx, const float4* __restrict__ rec0, const float* __restrict__ sh0,
             const float* __restrict__ shN, int tiled_in, float* __restrict__ sh0_out, float* __restrict__ shN_out, int tiled_out) {
    const size_t c = (size_t)blockIdx.x * LB + threadIdx.x;
    const int ch = (int)blockIdx.y;
    uint32_t first, end;
    if (!dvs_cluster_run(c, n, blk->n_clusters, cstart, &first, &end) || !alive[c]) return;
    const size_t o = coff[c];
    float4 r;
    if (first + 1u == end) {
        const size_t v = sidx[first];
        if (v >= n) return;
        r = lod_colour_chunk(sh0, shN, tiled_in, v, ch);
    } else {
        float W = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (uint32_t m = first; m < end; ++m) {
            const size_t v = sidx[m];
            if (v >= n) return;
            const float w = rec0[m].w;
            const float4 x = lod_colour_chunk(sh0, shN, tiled_in, v, ch);
            W = W + w; a0 = a0 + w * x.x; a1 = a1 + w * x.y; a2 = a2 + w * x.z; a3 = a3 + w * x.w;
        }
        r = make_float4(a0 / W, a1 / W, a2 / W, a3 / W);
        const int e = 4 * ch;                                                // the bands above D are written as 0
        if (e >= limit) r.x = 0.0f;
        if (ch < 11) { if (e + 1 >= limit) r.y = 0.0f; if (e + 2 >= limit) r.z = 0.0f; if (e + 3 >= limit) r.w = 0.0f; }
    }
    if (ch == 11) {
        sh0_out[3 * o] = r.y; sh0_out[3 * o + 1] = r.z; sh0_out[3 * o + 2] = r.w;
        if (tiled_out) reinterpret_cast<float4*>(shN_out)[dvs_shn_tiled_chunk((int64_t)o, 11)] = make_float4(r.x, 0.0f, 0.0f, 0.0f);      // the three pads
        else shN_out[o * 45 + 44] = r.x;
    } else if (tiled_out) {
        reinterpret_cast<float4*>(shN_out)[dvs_shn_tiled_chunk((int64_t)o, ch)] = r;
    } else {
        shN_out[o * 45 + 4 * ch] = r.x; shN_out[o * 45 + 4 * ch + 1] = r.y; shN_out[o * 45 + 4 * ch + 2] = r.z; shN_out[o * 45 + 4 * ch + 3] = r.w;
    }
}
// 64 x 12 threads: the lanes past m of the last tile (whole tiles are allocated)
__global__ void __launch_bounds__(LB) k_lod_pads(uint32_t n, const LodBlock* __restrict__ blk, float* __restrict__ shN_out) {
    const uint32_t t = blockIdx.x * LB + threadIdx.x;
    if (t >= 64u * 12u) return;
    const unsigned long long m = blk->m < n ? blk->m : n;
    const unsigned long long o = (m & ~63ull) + (t & 63u);
    if ((m & 63ull) == 0ull || o < m) return;
    reinterpret_cast<float4*>(shN_out)[dvs_shn_tiled_chunk((int64_t)o, (int)(t >> 6))] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
}  // namespace

extern "C" int dvs_lod_lattice_for(const float bounds[6], int resolution, dvs_lod_lattice* out) {
    if (!bounds || !out || resolution < 4 || resolution > 1024) return DVS_ERR_INVALID;
    double side[3], longest = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(bounds[k]) || !std::isfinite(bounds[3 + k]) || bounds[3 + k] < bounds[k]) return DVS_ERR_INVALID;
        side[k] = (double)bounds[3 + k] - (double)bounds[k];
        longest = std::fmax(longest, side[k]);
    }
    // 1e-5 of the side is some hundred ulps of any coordinate quotient: the largest coordinate's quotient in dvs_cell_key stays below `resolution`
    const float cell = (float)(longest * (1.0 + 1e-5) / (double)resolution);
    if (!(cell > 0.0f) || !std::isfinite(cell)) return DVS_ERR_INVALID;     // an empty box (or one whose cell is not an fp32 number)
    dvs_lod_lattice g;
    for (int k = 0; k < 3; ++k) {
        g.origin[k] = bounds[k];
        const double cells = std::ceil(side[k] / (double)cell);
        g.dims[k] = (int32_t)std::fmin(1024.0, std::fmax(1.0, cells));
    }
    g.cell = cell;
    *out = g;
    return DVS_OK;
}

extern "C" size_t dvs_lod_scratch_bytes(int n) { return lod_layout(n > 0 ? (uint32_t)n : 0u).total; }

extern "C" int dvs_lod_merge_count(void* stream, int n, const float* pos, const float* opacity, const float* scale, const float* rot,
                                   const dvs_lod_lattice* lattice, void* scratch, uint32_t counts[2]) {
    DvsCellLattice g;
    if (n < 0 || !lattice || !counts || !scratch || ((uintptr_t)scratch & 255u) || !dvs_cell_lattice(lattice->origin, lattice->cell, lattice->dims, &g))
        return DVS_ERR_INVALID;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(lattice->origin[k])) return DVS_ERR_INVALID;
    counts[0] = 0; counts[1] = 0;
    if (n == 0) return DVS_OK;
    if (dvs_bad_args({pos, opacity, scale, rot})) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t un = (uint32_t)n;
    const LodLayout L = lod_layout(un);
    char* const base = (char*)scratch;
    LodBlock* const blk = (LodBlock*)(base + L.block);
    const dim3 grid(dvs_blocks256(un)), block(LB);
    uint32_t *sidx = (uint32_t*)(base + L.c.val[0]), *cex = (uint32_t*)(base + L.c.cex), *coff = (uint32_t*)(base + L.coff);
    float* const wgt = (float*)(base + L.wgt);
    hipLaunchKernelGGL(k_lod_init, dim3(1), dim3(1), 0, st, blk);
    hipLaunchKernelGGL(k_lod_keys, grid, block, 0, st, un, pos, opacity, scale, rot, g, (uint32_t*)(base + L.c.key[0]), sidx, wgt, blk);
    if (dvs_launch_cell_clusters(st, un, 31, base, L.c, nullptr, &blk->n_clusters) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_lod_alive, grid, block, 0, st, un, blk, (const uint32_t*)(base + L.c.cstart), (const uint32_t*)sidx, (const float*)wgt, coff);
    // (alive stays in cex's place for the write call: the scan below turns coff into offsets)
    if (hipMemcpyAsync(cex, coff, (size_t)un * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return DVS_ERR_HIP;
    if (dvs_launch_scan_u32(st, coff, un, (uint32_t*)(base + L.c.bsum), &blk->m) != hipSuccess) return DVS_ERR_HIP;
    LodBlock host{};
    if (dvs_fetch_block(st, blk, &host) != DVS_OK) return DVS_ERR_HIP;
    counts[0] = (uint32_t)host.m; counts[1] = host.n_dropped;
    return DVS_OK;
}

extern "C" int dvs_lod_merge_write(void* stream, int n, int sh_degree, const float* pos, const float* sh0, const float* shN, const float* opacity,
                                   const float* scale, const float* rot, int shn_layout_in, const void* scratch, float* pos_out, float* sh0_out,
                                   float* shN_out, float* opacity_out, float* scale_out, float* rot_out, int shn_layout_out) {
    if (n < 0 || sh_degree < 0 || sh_degree > 3 || !scratch || ((uintptr_t)scratch & 255u)) return DVS_ERR_INVALID;
    if (dvs_bad_args({}, {}, shn_layout_in) || dvs_bad_args({}, {}, shn_layout_out)) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    if (dvs_bad_args({pos, sh0, shN, opacity, scale, rot, pos_out, sh0_out, shN_out, opacity_out, scale_out, rot_out})) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t un = (uint32_t)n;
    const LodLayout L = lod_layout(un);
    const char* const base = (const char*)scratch;
    const LodBlock* blk = (const LodBlock*)(base + L.block);
    const uint32_t *skey = (const uint32_t*)(base + L.c.key[0]), *sidx = (const uint32_t*)(base + L.c.val[0]), *alive = (const uint32_t*)(base + L.c.cex),
                   *cstart = (const uint32_t*)(base + L.c.cstart), *coff = (const uint32_t*)(base + L.coff);
    const float* wgt = (const float*)(base + L.wgt);
    // the record area is this call's workspace inside the scratch; what dvs_lod_merge_count left there is read only
    float4* rec[3];
    for (int k = 0; k < 3; ++k) rec[k] = (float4*)const_cast<char*>(base + L.rec[k]);
    const dim3 grid(dvs_blocks256(un)), block(LB);
    static const int limit[4] = {0, 9, 24, 45};
    const int tin = shn_layout_in == DVS_SHN_TILED ? 1 : 0, tout = shn_layout_out == DVS_SHN_TILED ? 1 : 0;
    hipLaunchKernelGGL(k_lod_gather, grid, block, 0, st, un, skey, sidx, pos, scale, rot, wgt, rec[0], rec[1], rec[2]);
    hipLaunchKernelGGL(k_lod_geometry, grid, block, 0, st, un, blk, cstart, alive, coff, sidx, (const float4*)rec[0], (const float4*)rec[1], (const float4*)rec[2],
                       pos, opacity, scale, rot, pos_out, opacity_out, scale_out, rot_out);
    hipLaunchKernelGGL(k_lod_colour, dim3(dvs_blocks256(un), 12), block, 0, st, un, limit[sh_degree], blk, cstart, alive, coff, sidx, (const float4*)rec[0], sh0, shN,
                       tin, sh0_out, shN_out, tout);
    if (tout) hipLaunchKernelGGL(k_lod_pads, dim3(3), block, 0, st, un, blk, shN_out);
    return dvs_launch_status();
}
