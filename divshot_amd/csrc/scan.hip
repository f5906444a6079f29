// scan.hip — the device-wide exclusive scan of 32-bit words and inclusive scan of 64-bit words (dvs_kernels.h), for gfx950: a plain
// reduce-then-scan. Block sums of DVS_SCAN_TILE elements, one workgroup scans the block sums with a 64-bit carry, the blocks rescan their
// elements from their offset. The three kernels are templates over the word; the 32-bit instances are what they always were.
// Integer only; no atomics: every output word has exactly one writer. Users: mesh.hip (vertex and triangle offsets), mesh_clean.hip
// (compaction), cell_cluster.hip (cluster numbers), mesh_decimate.hip and lod.hip (compaction), region.hip (the middle step alone, over its own block counts),
// reduced.hip (degree block offsets; the int64 prefix sums of the codebooks' sorted values).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dvs_kernels.h"
#include "block_scan.h"

#define SCAN_ITEMS 8
#define SCAN_TILE (DB * SCAN_ITEMS)
static_assert(SCAN_TILE == DVS_SCAN_TILE, "dvs_kernels.h tells the scan's users how many block sums it needs");

namespace {
template <class T>
__global__ void __launch_bounds__(DB) k_scan_reduce(const T* __restrict__ v, size_t n, T* __restrict__ bsum) {
    __shared__ T tmp[DB / 64];
    const size_t first = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    T s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) if (first + k < n) s += v[first + k];
    T tot;
    (void)dvs_block_excl_scan(s, tmp, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
// one workgroup: block sums -> exclusive offsets (32-bit words; the true total in 64 bits, for the caller's range check)
template <class T>
__global__ void __launch_bounds__(DB) k_scan_block_sums(T* __restrict__ bsum, uint32_t nb, unsigned long long* __restrict__ total) {
    __shared__ T tmp[DB / 64];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += DB) {
        const uint32_t i = base + threadIdx.x;
        const T s = i < nb ? bsum[i] : (T)0;
        T tot;
        const T ex = dvs_block_excl_scan(s, tmp, &tot);
        if (i < nb) bsum[i] = (T)carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
// INCL: v[i] = the sum up to and including element i
template <class T, bool INCL>
__global__ void __launch_bounds__(DB) k_scan_apply(T* __restrict__ v, size_t n, const T* __restrict__ bsum) {
    __shared__ T tmp[DB / 64];
    const size_t first = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    T item[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { item[k] = first + k < n ? v[first + k] : (T)0; s += item[k]; }
    T tot;
    T run = bsum[blockIdx.x] + dvs_block_excl_scan(s, tmp, &tot);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { if (INCL) run += item[k]; if (first + k < n) v[first + k] = run; if (!INCL) run += item[k]; }
}
}  // namespace

hipError_t dvs_launch_block_sums_excl(hipStream_t st, uint32_t* bsum, uint32_t nb, unsigned long long* total) {
    hipLaunchKernelGGL(k_scan_block_sums<uint32_t>, dim3(1), dim3(DB), 0, st, bsum, nb, total);
    return hipGetLastError();
}
hipError_t dvs_launch_scan_u32(hipStream_t st, uint32_t* v, size_t n, uint32_t* bsum, unsigned long long* total) {
    const uint32_t nb = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL(k_scan_reduce<uint32_t>, dim3(nb), dim3(DB), 0, st, (const uint32_t*)v, n, bsum);
    hipLaunchKernelGGL(k_scan_block_sums<uint32_t>, dim3(1), dim3(DB), 0, st, bsum, nb, total);
    hipLaunchKernelGGL((k_scan_apply<uint32_t, false>), dim3(nb), dim3(DB), 0, st, v, n, (const uint32_t*)bsum);
    return hipGetLastError();
}
hipError_t dvs_launch_scan_incl_u64(hipStream_t st, uint64_t* v, size_t n, uint64_t* bsum) {
    const uint32_t nb = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL(k_scan_reduce<uint64_t>, dim3(nb), dim3(DB), 0, st, (const uint64_t*)v, n, bsum);
    hipLaunchKernelGGL(k_scan_block_sums<uint64_t>, dim3(1), dim3(DB), 0, st, bsum, nb, (unsigned long long*)nullptr);
    hipLaunchKernelGGL((k_scan_apply<uint64_t, true>), dim3(nb), dim3(DB), 0, st, v, n, (const uint64_t*)bsum);
    return hipGetLastError();
}
