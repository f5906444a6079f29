// scan.hip — the device-wide exclusive scan of 32-bit words (dvs_kernels.h), for gfx950: a plain reduce-then-scan. Block sums of
// DVS_SCAN_TILE elements, one workgroup scans the block sums with a 64-bit carry, the blocks rescan their elements from their offset.
// Integer only; no atomics: every output word has exactly one writer. Users: mesh.hip (vertex and triangle offsets), mesh_clean.hip
// (compaction), mesh_decimate.hip (cluster numbers, compaction), region.hip (the middle step alone, over its own block counts).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dvs_kernels.h"
#include "block_scan.h"

#define SCAN_ITEMS 8
#define SCAN_TILE (DB * SCAN_ITEMS)
static_assert(SCAN_TILE == DVS_SCAN_TILE, "dvs_kernels.h tells the scan's users how many block sums it needs");

namespace {
__global__ void __launch_bounds__(DB) k_scan_reduce(const uint32_t* __restrict__ v, size_t n, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t tmp[DB / 64];
    const size_t first = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) if (first + k < n) s += v[first + k];
    uint32_t tot;
    (void)dvs_block_excl_scan(s, tmp, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
// one workgroup: block sums -> exclusive offsets (32-bit words; the true total in 64 bits, for the caller's range check)
__global__ void __launch_bounds__(DB) k_scan_block_sums(uint32_t* __restrict__ bsum, uint32_t nb, unsigned long long* __restrict__ total) {
    __shared__ uint32_t tmp[DB / 64];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += DB) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t s = i < nb ? bsum[i] : 0u;
        uint32_t tot;
        const uint32_t ex = dvs_block_excl_scan(s, tmp, &tot);
        if (i < nb) bsum[i] = (uint32_t)carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(DB) k_scan_apply(uint32_t* __restrict__ v, size_t n, const uint32_t* __restrict__ bsum) {
    __shared__ uint32_t tmp[DB / 64];
    const size_t first = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t item[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { item[k] = first + k < n ? v[first + k] : 0u; s += item[k]; }
    uint32_t tot;
    uint32_t run = bsum[blockIdx.x] + dvs_block_excl_scan(s, tmp, &tot);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { if (first + k < n) v[first + k] = run; run += item[k]; }
}
}  // namespace

hipError_t dvs_launch_block_sums_excl(hipStream_t st, uint32_t* bsum, uint32_t nb, unsigned long long* total) {
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(DB), 0, st, bsum, nb, total);
    return hipGetLastError();
}
hipError_t dvs_launch_scan_u32(hipStream_t st, uint32_t* v, size_t n, uint32_t* bsum, unsigned long long* total) {
    const uint32_t nb = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(DB), 0, st, (const uint32_t*)v, n, bsum);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(DB), 0, st, bsum, nb, total);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(DB), 0, st, v, n, (const uint32_t*)bsum);
    return hipGetLastError();
}
