// block_scan.h — the exclusive scan of one value per thread over a 256-thread workgroup that the plan kernels share (densify.hip, region.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DB 256

__device__ __forceinline__ uint32_t d_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// -> the sum of v over the threads before this one; *total = the sum over the workgroup. tmp: DB / 64 + 1 words of LDS; two barriers, so
// every thread of the workgroup must call it, and tmp may be used again right after it returns.
__device__ __forceinline__ uint32_t d_block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t* total) {
    const uint32_t lane = d_lane(), wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < DB / 64; ++w) { const uint32_t t = tmp[w]; if ((uint32_t)w < wave) wbase += t; tot += t; }
    __syncthreads();
    *total = tot;
    return wbase + inc - v;
}
