// cell_cluster.hip — elements keyed by the cell of a lattice they fall into, grouped into clusters, for gfx950: the part the mesh
// decimation (mesh_decimate.hip) and the LOD merge (lod.hip) share, up to where they diverge into what a cluster becomes. The caller
// writes key[0][i] = dvs_cell_key(...) or DVS_CELL_NONE and val[0][i] = i (cell_cluster.h); dvs_launch_cell_clusters then runs
//   sort              the one-segment pair sort, ballot ranking: (key, index) over `bits` bits; equal keys stay in index order and the
//                     elements without a cell end up last; the result is copied into buffers 0 if the passes left it in buffers 1
//   k_cluster_heads   head[i] = the sorted position i starts a run of equal keys that has a cell
//   scan              head -> exclusive: a head's value is its cluster's number in key order; the total is n_clusters
//   k_cluster_starts  first sorted position of every cluster (and the end of the last); optionally the cluster of every element
// Integer only. No atomics, no kernel waits for another workgroup, no LDS, no scratch memory, no inline assembly.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include "cell_cluster.h"

#define CCB 256

namespace {
__global__ void __launch_bounds__(CCB) k_cluster_heads(uint32_t n, const uint32_t* __restrict__ skey, uint32_t* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * CCB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = skey[i];
    head[i] = (k != DVS_CELL_NONE && (i == 0 || k != skey[i - 1])) ? 1u : 0u;
}
// cex = the exclusive scan of the heads: a head's value is its cluster's number, a follower's is that number + 1. The elements with a
// cell are the sorted positions [0, ns): the last of them closes the last cluster.
__global__ void __launch_bounds__(CCB)
k_cluster_starts(uint32_t n, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ cex,
                 uint32_t* __restrict__ cluster_of /*nullable*/, uint32_t* __restrict__ cstart) {
    const size_t i = (size_t)blockIdx.x * CCB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = skey[i];
    if (k == DVS_CELL_NONE) return;
    const bool head = i == 0 || k != skey[i - 1];
    const uint32_t c = head ? cex[i] : cex[i] - 1u;                          // (a follower has a head before it: cex >= 1)
    if (cluster_of) {
        const uint32_t v = sidx[i];
        if (v < n) cluster_of[v] = c;                                        // (the sort permutes [0, n): always true)
    }
    if (head) cstart[c] = (uint32_t)i;
    if (i + 1 == n || skey[i + 1] == DVS_CELL_NONE) cstart[c + 1u] = (uint32_t)(i + 1);      // c + 1 = n_clusters <= n: inside the n + 1 words
}
}  // namespace

bool dvs_cell_lattice(const float origin[3], float cell, const int32_t dims[3], DvsCellLattice* g) {
    if (!origin || !dims || !(cell > 0.0f) || !std::isfinite(cell)) return false;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 1 || dims[k] > 1024) return false;
        g->o[k] = origin[k]; g->n[k] = (uint32_t)dims[k];
    }
    g->cell = cell;
    return true;
}

DvsClusterLayout dvs_cluster_layout(size_t n, size_t sort_n) {
    DvsClusterLayout L{};
    size_t o = 0;
    L.sort_ws = dvs_carve(o, dvs_pair_sort_ws_bytes((uint64_t)(sort_n > n ? sort_n : n)));
    for (int k = 0; k < 2; ++k) { L.key[k] = dvs_carve(o, n * 4); L.val[k] = dvs_carve(o, n * 4); }
    L.cex = dvs_carve(o, n * 4);
    L.bsum = dvs_carve(o, ((n + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 4);
    L.cstart = dvs_carve(o, (n + 1) * 4);
    L.end = o;
    return L;
}

hipError_t dvs_launch_cell_clusters(hipStream_t st, uint32_t n, int bits, void* base, const DvsClusterLayout& L, uint32_t* cluster_of,
                                    unsigned long long* n_clusters_dev) {
    char* const b = (char*)base;
    uint32_t *key0 = (uint32_t*)(b + L.key[0]), *val0 = (uint32_t*)(b + L.val[0]), *key1 = (uint32_t*)(b + L.key[1]), *val1 = (uint32_t*)(b + L.val[1]);
    uint32_t *cex = (uint32_t*)(b + L.cex), *cstart = (uint32_t*)(b + L.cstart);
    int cur = 0;
    hipError_t e = dvs_launch_pair_sort(st, n, key0, val0, key1, val1, 0, bits, dvs_pair_sort_ws_at(b + L.sort_ws), 0, &cur);      // ballot ranking
    // the caller's write call looks for the sorted order in buffers 0, without knowing where the passes left it
    if (e == hipSuccess && cur != 0) e = hipMemcpyAsync(key0, key1, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && cur != 0) e = hipMemcpyAsync(val0, val1, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
    const dim3 grid(dvs_blocks256(n)), block(CCB);
    hipLaunchKernelGGL(k_cluster_heads, grid, block, 0, st, n, (const uint32_t*)key0, cex);
    if ((e = dvs_launch_scan_u32(st, cex, n, (uint32_t*)(b + L.bsum), n_clusters_dev)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cluster_starts, grid, block, 0, st, n, (const uint32_t*)key0, (const uint32_t*)val0, (const uint32_t*)cex, cluster_of, cstart);
    return hipSuccess;
}
