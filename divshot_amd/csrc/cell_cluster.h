// cell_cluster.h — the device-side definitions of cell_cluster.hip: the cell of a point on a lattice, and the members of a cluster.
#pragma once
#include "dvs_kernels.h"

// the key of an element that belongs to no cell: bit 30 alone, above every cell key (< 1024^3 = 2^30), so a 31-bit sort puts it last
#define DVS_CELL_NONE 0x40000000u

// n[0] x n[1] x n[2] cubic cells of side `cell` from the corner o (by value to the key kernels; filled by dvs_cell_lattice)
struct DvsCellLattice { float o[3]; float cell; uint32_t n[3]; };

// The cell of a coordinate along one axis: one subtraction, one IEEE division, clamped into the lattice; !(q >= 0) also catches NaN.
// tests/mesh_decimate_ref.py and tests/lod_ref.py pin this rule bit for bit.
__device__ __forceinline__ uint32_t dvs_cell_axis(float x, float o, float cell, uint32_t n) {
    const float q = (x - o) / cell;
    if (!(q >= 0.0f)) return 0u;
    if (q >= (float)n) return n - 1u;
    return (uint32_t)q;
}
__device__ __forceinline__ uint32_t dvs_cell_key(float x, float y, float z, const DvsCellLattice& g) {
    const uint32_t ix = dvs_cell_axis(x, g.o[0], g.cell, g.n[0]), iy = dvs_cell_axis(y, g.o[1], g.cell, g.n[1]), iz = dvs_cell_axis(z, g.o[2], g.cell, g.n[2]);
    return (iz * g.n[1] + iy) * g.n[0] + ix;                                 // < 1024^3 = 2^30
}

// The members of cluster c of n elements: the sorted positions [*first, *end) from the cstart dvs_launch_cell_clusters left; false when c
// is no cluster. The bound of the caller's loop comes from the input (end <= n), whatever the scratch holds.
__device__ __forceinline__ bool dvs_cluster_run(size_t c, uint32_t n, unsigned long long n_clusters, const uint32_t* __restrict__ cstart, uint32_t* first,
                                                uint32_t* end) {
    if (c >= n || c >= n_clusters) return false;
    const uint32_t e = cstart[c + 1];
    *first = cstart[c];
    *end = e > n ? n : e;
    return *first < *end;                                                    // (always: a cluster has a member)
}
