// mesh_decimate.hip — decimation of an indexed mesh by vertex clustering (Rossignac-Borrel) on a lattice of cells, for gfx950: the last
// stage of the mesh line (include/dvs_mesh.h has the definition, tests/mesh_decimate_ref.py restates it in numpy). All vertices of a
// cell become one vertex with their mean position, colour and normal; triangles are re-indexed; collapsed and repeated triangles and
// the clusters no surviving triangle uses are dropped.
//
// Vertices (dvs_mesh_decimate_count):
//   k_dec_keys        key[v] = the cell of v (30 bits), val[v] = v
//   clustering        cell_cluster.hip: the vertices sorted by (cell, index), cluster_of[vertex], first sorted position of every cluster
// Triangles:
//   k_dec_canon       bad / degenerate triangles counted and given the words (0, 0, 0); the others their three cluster numbers rotated so
//                     that the smallest comes first (winding kept) -> w0, w1, w2
//   sort x 3          the one-segment pair sort of frontend.hip (stable, ballot ranking) of (word, triangle id) over w2, then w1, then w0
//                     (k_dec_regather loads the next word in the order the last sort left), each over the bits min(n_vertices, cells) - 1
//                     needs — the host's bound on n_clusters - 1, known without waiting for the device
//   k_dec_dups        a surviving triangle whose three words equal its predecessor's in that order repeats it: the run's first member
//                     is the one with the smallest triangle index (the sorts are stable), the others are counted and dropped
//   scan              keep -> exclusive: the new index of a kept triangle
//   k_dec_mark_used   used[cluster] = 1 for the corners of the kept triangles: plain stores of the same value, idempotent
//   scan              used -> exclusive: the new index of a used cluster
// Writing (dvs_mesh_decimate_write):
//   k_dec_gather      the vertex records in sorted order, 16-byte stores by consecutive lanes (as k_knn_gather): {x, y, z, rgb} and the
//                     normal, so that the walk below reads one contiguous run per cluster
//   k_dec_walk        one lane per cluster: the serial sums over its members in ascending vertex index (the definition), mean / rounded
//                     mean / renormalised sum
//   k_dec_write_t     kept triangles in their old order and corner order, through cluster_of and the clusters' new indices
//
// The only atomics are integer additions to three counters (one per wave), whose sums do not depend on order. No kernel waits for
// another workgroup: phases are launches. Every device loop is bounded by n_vertices. No scratch memory, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "../../include/dvs_mesh.h"
#include "cell_cluster.h"

#define MB 256

namespace {
// the words the passes share and the host reads (one 64-byte block at the end of the scratch)
struct DecBlock {
    unsigned long long n_clusters, out_vertices, out_triangles;       // the scans' totals
    uint32_t n_degenerate, n_duplicate, n_bad, _pad[7];
};
static_assert(sizeof(DecBlock) == 64, "one block of words");

struct DecLayout {
    DvsClusterLayout c;                                                // the vertex clusters; its sort workspace also serves the triangle sorts
    size_t vclu, used, coff;                                           // per vertex
    size_t rec, recn;                                                  // the gathered records (written by dvs_mesh_decimate_write)
    size_t w[3], tkey[2], tval[2], keep, toff, bsum_t;                 // per triangle
    size_t block, total;
};
DecLayout dec_layout(uint32_t nv, uint32_t nt) {
    DecLayout L{};
    const size_t v = nv ? nv : 1, t = nt ? nt : 1;
    L.c = dvs_cluster_layout(v, t);
    size_t o = L.c.end;
    L.vclu = dvs_carve(o, v * 4);
    L.used = dvs_carve(o, v);
    L.coff = dvs_carve(o, v * 4);
    L.rec = dvs_carve(o, v * 16);
    L.recn = dvs_carve(o, v * 16);
    for (int k = 0; k < 3; ++k) L.w[k] = dvs_carve(o, t * 4);
    for (int k = 0; k < 2; ++k) { L.tkey[k] = dvs_carve(o, t * 4); L.tval[k] = dvs_carve(o, t * 4); }
    L.keep = dvs_carve(o, t);
    L.toff = dvs_carve(o, t * 4);
    L.bsum_t = dvs_carve(o, ((t + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 4);
    L.block = dvs_carve(o, sizeof(DecBlock));
    L.total = o;
    return L;
}

__global__ void k_dec_init(DecBlock* blk) {
    blk->n_clusters = 0; blk->out_vertices = 0; blk->out_triangles = 0;
    blk->n_degenerate = 0; blk->n_duplicate = 0; blk->n_bad = 0;
}
__global__ void __launch_bounds__(MB)
k_dec_keys(uint32_t nv, const float* __restrict__ xyz, DvsCellLattice g, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= nv) return;
    key[v] = dvs_cell_key(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], g);
    val[v] = (uint32_t)v;
}

// One thread per triangle. No lane leaves early: the wave's leader adds the wave's counts.
__global__ void __launch_bounds__(MB)
k_dec_canon(uint32_t nv, const uint32_t* __restrict__ tri, uint32_t nt, const uint32_t* __restrict__ vclu, uint32_t* __restrict__ w0,
            uint32_t* __restrict__ w1, uint32_t* __restrict__ w2, uint32_t* __restrict__ key, uint32_t* __restrict__ val, DecBlock* blk) {
    const size_t t = (size_t)blockIdx.x * MB + threadIdx.x;
    bool bad = false, degenerate = false;
    if (t < nt) {
        const uint32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
        uint32_t a = 0, b = 0, c = 0;
        bad = v0 >= nv || v1 >= nv || v2 >= nv;
        if (!bad) {
            const uint32_t c0 = vclu[v0], c1 = vclu[v1], c2 = vclu[v2];
            degenerate = c0 == c1 || c1 == c2 || c0 == c2;
            if (!degenerate) {
                if (c0 < c1 && c0 < c2) { a = c0; b = c1; c = c2; }
                else if (c1 < c0 && c1 < c2) { a = c1; b = c2; c = c0; }
                else { a = c2; b = c0; c = c1; }
            }
        }
        w0[t] = a; w1[t] = b; w2[t] = c;
        key[t] = c; val[t] = (uint32_t)t;                                // the first sort is over the last word
    }
    const uint32_t nb = (uint32_t)__popcll(__ballot(bad)), nd = (uint32_t)__popcll(__ballot(degenerate));
    if ((threadIdx.x & 63u) == 0u) {
        if (nb) atomicAdd(&blk->n_bad, nb);
        if (nd) atomicAdd(&blk->n_degenerate, nd);
    }
}
__global__ void __launch_bounds__(MB)
k_dec_regather(uint32_t nt, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ w, uint32_t* __restrict__ key) {
    const size_t i = (size_t)blockIdx.x * MB + threadIdx.x;
    if (i >= nt) return;
    const uint32_t t = perm[i];
    key[i] = t < nt ? w[t] : 0u;                                         // (a permutation of [0, nt): always true)
}
// perm = the triangles ordered by (w0, w1, w2, triangle index). A surviving triangle has three different words, a dropped one (0, 0, 0):
// w0 != w1 tells them apart, and a survivor never equals a dropped predecessor.
__global__ void __launch_bounds__(MB)
k_dec_dups(uint32_t nt, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ w0, const uint32_t* __restrict__ w1,
           const uint32_t* __restrict__ w2, uint8_t* __restrict__ keep, uint32_t* __restrict__ toff, DecBlock* blk) {
    const size_t i = (size_t)blockIdx.x * MB + threadIdx.x;
    bool dup = false;
    if (i < nt) {
        const uint32_t t = perm[i];
        if (t < nt) {
            const uint32_t a = w0[t], b = w1[t], c = w2[t];
            const bool alive = a != b;
            if (alive && i > 0) {
                const uint32_t p = perm[i - 1];
                dup = p < nt && w0[p] == a && w1[p] == b && w2[p] == c;
            }
            const uint32_t k = alive && !dup ? 1u : 0u;
            keep[t] = (uint8_t)k;
            toff[t] = k;
        }
    }
    const uint32_t nd = (uint32_t)__popcll(__ballot(dup));
    if ((threadIdx.x & 63u) == 0u && nd) atomicAdd(&blk->n_duplicate, nd);
}
__global__ void __launch_bounds__(MB) k_dec_zero_used(uint32_t nv, uint8_t* __restrict__ used, uint32_t* __restrict__ coff) {
    const size_t c = (size_t)blockIdx.x * MB + threadIdx.x;
    if (c < nv) { used[c] = 0; coff[c] = 0u; }
}
// every writer stores the same value: the outcome does not depend on who comes first
__global__ void __launch_bounds__(MB)
k_dec_mark_used(uint32_t nv, const uint32_t* __restrict__ tri, uint32_t nt, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ vclu,
                uint8_t* used, uint32_t* coff) {
    const size_t t = (size_t)blockIdx.x * MB + threadIdx.x;
    if (t >= nt || !keep[t]) return;                                     // (kept: its three indices are < nv)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = tri[3 * t + k];
        if (v < nv) { const uint32_t c = vclu[v]; used[c] = 1; coff[c] = 1u; }
    }
}

// ---- writing --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MB)
k_dec_gather(uint32_t nv, const uint32_t* __restrict__ sidx, const float* __restrict__ xyz, const uint8_t* __restrict__ rgb,
             const float* __restrict__ normals, float4* __restrict__ rec, float4* __restrict__ recn) {
    const size_t i = (size_t)blockIdx.x * MB + threadIdx.x;
    if (i >= nv) return;
    const size_t v = sidx[i];
    if (v >= nv) return;                                                 // (never: sidx is a permutation of [0, nv))
    const uint32_t col = (uint32_t)rgb[3 * v] | ((uint32_t)rgb[3 * v + 1] << 8) | ((uint32_t)rgb[3 * v + 2] << 16);
    rec[i] = make_float4(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], __uint_as_float(col));
    if (normals) recn[i] = make_float4(normals[3 * v], normals[3 * v + 1], normals[3 * v + 2], 0.0f);
}
// One lane per cluster over its records [cstart[c], cstart[c + 1]): the members in ascending vertex index. The sums are serial in that
// order — that order is the definition — so a cluster is one lane's work however many members it has.
__global__ void __launch_bounds__(MB)
k_dec_walk(uint32_t nv, const DecBlock* __restrict__ blk, const uint32_t* __restrict__ cstart, const uint8_t* __restrict__ used,
           const uint32_t* __restrict__ coff, const float4* __restrict__ rec, const float4* __restrict__ recn, float* __restrict__ out_xyz,
           uint8_t* __restrict__ out_rgb, float* __restrict__ out_normals) {
    const size_t c = (size_t)blockIdx.x * MB + threadIdx.x;
    uint32_t first, end;
    if (!dvs_cluster_run(c, nv, blk->n_clusters, cstart, &first, &end) || !used[c]) return;
    const size_t o = coff[c];                                            // < out_vertices
    float4 r = rec[first];
    float sx = r.x, sy = r.y, sz = r.z;
    uint32_t col = __float_as_uint(r.w);
    unsigned long long sr = col & 0xFFu, sg = (col >> 8) & 0xFFu, sb = (col >> 16) & 0xFFu;
    for (uint32_t m = first + 1u; m < end; ++m) {
        r = rec[m];
        sx = sx + r.x; sy = sy + r.y; sz = sz + r.z;
        col = __float_as_uint(r.w);
        sr += col & 0xFFu; sg += (col >> 8) & 0xFFu; sb += (col >> 16) & 0xFFu;
    }
    const uint32_t count = end - first;
    const float fc = (float)count;
    out_xyz[3 * o] = sx / fc; out_xyz[3 * o + 1] = sy / fc; out_xyz[3 * o + 2] = sz / fc;
    const unsigned long long c2 = 2ull * count;
    out_rgb[3 * o] = (uint8_t)((2ull * sr + count) / c2);
    out_rgb[3 * o + 1] = (uint8_t)((2ull * sg + count) / c2);
    out_rgb[3 * o + 2] = (uint8_t)((2ull * sb + count) / c2);
    if (out_normals) {
        float4 q = recn[first];
        float nx = q.x, ny = q.y, nz = q.z;
        for (uint32_t m = first + 1u; m < end; ++m) {
            q = recn[m];
            nx = nx + q.x; ny = ny + q.y; nz = nz + q.z;
        }
        dvs_unit_or_zero(nx, ny, nz);
        out_normals[3 * o] = nx; out_normals[3 * o + 1] = ny; out_normals[3 * o + 2] = nz;
    }
}
__global__ void __launch_bounds__(MB)
k_dec_write_t(uint32_t nv, const uint32_t* __restrict__ tri, uint32_t nt, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ toff,
              const uint32_t* __restrict__ vclu, const uint32_t* __restrict__ coff, uint32_t* __restrict__ out_tri) {
    const size_t t = (size_t)blockIdx.x * MB + threadIdx.x;
    if (t >= nt || !keep[t]) return;
    const uint32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    if (v0 >= nv || v1 >= nv || v2 >= nv) return;                        // (never: a kept triangle is not bad)
    const size_t o = toff[t];                                            // < out_triangles
    out_tri[3 * o] = coff[vclu[v0]]; out_tri[3 * o + 1] = coff[vclu[v1]]; out_tri[3 * o + 2] = coff[vclu[v2]];
}

// bits of the largest value a word can take: the cluster numbers are below min(n_vertices, cells)
int bits_for(uint64_t max_value) { int b = 0; while (b < 32 && (max_value >> b)) ++b; return b; }
}  // namespace

extern "C" size_t dvs_mesh_decimate_scratch_bytes(uint32_t n_vertices, uint32_t n_triangles) { return dec_layout(n_vertices, n_triangles).total; }

extern "C" int dvs_mesh_decimate_count(void* stream, uint32_t n_vertices, const float* xyz, const uint32_t* tri, uint32_t n_triangles, const float origin[3],
                                       float cell, const int32_t ncell[3], void* scratch, dvs_mesh_decimate_info* info) {
    DvsCellLattice g;
    if (!scratch || ((uintptr_t)scratch & 255u) || !info || !dvs_cell_lattice(origin, cell, ncell, &g)) return DVS_ERR_INVALID;
    if ((n_vertices > 0 && !xyz) || (n_triangles > 0 && !tri)) return DVS_ERR_INVALID;
    if (n_vertices > 0x7FFFFFFFu || n_triangles > 0x7FFFFFFFu) return DVS_ERR_CAPACITY;      // the sort counts in int
    *info = dvs_mesh_decimate_info{};
    hipStream_t st = (hipStream_t)stream;
    if (n_vertices == 0) {                                               // every index is >= n_vertices: nothing to look at
        info->n_bad = n_triangles;
        return hipStreamSynchronize(st) == hipSuccess ? DVS_OK : DVS_ERR_HIP;
    }
    const uint32_t nv = n_vertices, nt = n_triangles;
    const DecLayout L = dec_layout(nv, nt);
    char* const base = (char*)scratch;
    DecBlock* const blk = (DecBlock*)(base + L.block);
    const dim3 gv(dvs_blocks256(nv)), gt(dvs_blocks256(nt)), block(MB);
    uint32_t *vclu = (uint32_t*)(base + L.vclu), *coff = (uint32_t*)(base + L.coff);
    uint8_t* used = (uint8_t*)(base + L.used);

    hipLaunchKernelGGL(k_dec_init, dim3(1), dim3(1), 0, st, blk);
    hipLaunchKernelGGL(k_dec_keys, gv, block, 0, st, nv, xyz, g, (uint32_t*)(base + L.c.key[0]), (uint32_t*)(base + L.c.val[0]));
    if (dvs_launch_cell_clusters(st, nv, 30, base, L.c, vclu, &blk->n_clusters) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_dec_zero_used, gv, block, 0, st, nv, used, coff);

    if (nt > 0) {
        uint32_t* w[3] = {(uint32_t*)(base + L.w[0]), (uint32_t*)(base + L.w[1]), (uint32_t*)(base + L.w[2])};
        uint32_t* tkey[2] = {(uint32_t*)(base + L.tkey[0]), (uint32_t*)(base + L.tkey[1])};
        uint32_t* tval[2] = {(uint32_t*)(base + L.tval[0]), (uint32_t*)(base + L.tval[1])};
        uint8_t* keep = (uint8_t*)(base + L.keep);
        uint32_t* toff = (uint32_t*)(base + L.toff);
        hipLaunchKernelGGL(k_dec_canon, gt, block, 0, st, nv, tri, nt, (const uint32_t*)vclu, w[0], w[1], w[2], tkey[0], tval[0], blk);
        const DvsPairSortWs ws = dvs_pair_sort_ws_at(base + L.c.sort_ws);
        const uint64_t cells = (uint64_t)g.n[0] * g.n[1] * g.n[2];
        const int bits = bits_for((cells < nv ? cells : (uint64_t)nv) - 1u);          // 0 when there can be one cluster only: nothing to sort
        for (int word = 2; word >= 0; --word) {
            if (word < 2) hipLaunchKernelGGL(k_dec_regather, gt, block, 0, st, nt, (const uint32_t*)tval[0], (const uint32_t*)w[word], tkey[0]);
            int c = 0;
            if (dvs_launch_pair_sort(st, nt, tkey[0], tval[0], tkey[1], tval[1], 0, bits, ws, 0, &c) != hipSuccess) return DVS_ERR_HIP;
            if (c) { std::swap(tkey[0], tkey[1]); std::swap(tval[0], tval[1]); }       // buffers 0: the order so far
        }
        hipLaunchKernelGGL(k_dec_dups, gt, block, 0, st, nt, (const uint32_t*)tval[0], (const uint32_t*)w[0], (const uint32_t*)w[1], (const uint32_t*)w[2],
                           keep, toff, blk);
        if (dvs_launch_scan_u32(st, toff, nt, (uint32_t*)(base + L.bsum_t), &blk->out_triangles) != hipSuccess) return DVS_ERR_HIP;
        hipLaunchKernelGGL(k_dec_mark_used, gt, block, 0, st, nv, tri, nt, (const uint8_t*)keep, (const uint32_t*)vclu, used, coff);
    }
    if (dvs_launch_scan_u32(st, coff, nv, (uint32_t*)(base + L.c.bsum), &blk->out_vertices) != hipSuccess) return DVS_ERR_HIP;
    DecBlock host{};
    if (dvs_fetch_block(st, blk, &host) != DVS_OK) return DVS_ERR_HIP;
    info->out_vertices = (uint32_t)host.out_vertices; info->out_triangles = (uint32_t)host.out_triangles; info->n_clusters = (uint32_t)host.n_clusters;
    info->n_degenerate = host.n_degenerate; info->n_duplicate = host.n_duplicate; info->n_bad = host.n_bad;
    return DVS_OK;
}

extern "C" int dvs_mesh_decimate_write(void* stream, uint32_t n_vertices, const float* xyz, const uint8_t* rgb, const float* normals, const uint32_t* tri,
                                       uint32_t n_triangles, const void* scratch, float* out_xyz, uint8_t* out_rgb, float* out_normals, uint32_t* out_tri) {
    if (!scratch || ((uintptr_t)scratch & 255u) || (normals != nullptr) != (out_normals != nullptr)) return DVS_ERR_INVALID;
    if (n_vertices == 0 || n_triangles == 0) return DVS_OK;           // no triangle survives: no cluster is used
    if (!xyz || !rgb || !tri || !out_xyz || !out_rgb || !out_tri) return DVS_ERR_INVALID;
    if (n_vertices > 0x7FFFFFFFu || n_triangles > 0x7FFFFFFFu) return DVS_ERR_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nv = n_vertices, nt = n_triangles;
    const DecLayout L = dec_layout(nv, nt);
    const char* const base = (const char*)scratch;
    const DecBlock* blk = (const DecBlock*)(base + L.block);
    const uint32_t *sidx = (const uint32_t*)(base + L.c.val[0]), *vclu = (const uint32_t*)(base + L.vclu), *cstart = (const uint32_t*)(base + L.c.cstart),
                   *coff = (const uint32_t*)(base + L.coff), *toff = (const uint32_t*)(base + L.toff);
    const uint8_t *used = (const uint8_t*)(base + L.used), *keep = (const uint8_t*)(base + L.keep);
    // the record area is this call's workspace inside the scratch; what dvs_mesh_decimate_count left there is read only
    float4 *rec = (float4*)const_cast<char*>(base + L.rec), *recn = (float4*)const_cast<char*>(base + L.recn);
    const dim3 gv(dvs_blocks256(nv)), gt(dvs_blocks256(nt)), block(MB);
    hipLaunchKernelGGL(k_dec_gather, gv, block, 0, st, nv, sidx, xyz, rgb, normals, rec, recn);
    hipLaunchKernelGGL(k_dec_walk, gv, block, 0, st, nv, blk, cstart, used, coff, (const float4*)rec, (const float4*)recn, out_xyz, out_rgb, out_normals);
    hipLaunchKernelGGL(k_dec_write_t, gt, block, 0, st, nv, tri, nt, keep, toff, vclu, coff, out_tri);
    return dvs_launch_status();
}
