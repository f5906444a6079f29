// block_scan.h — the lane id, the wave64 inclusive scan and the exclusive scan of one value per thread over a 256-thread workgroup: the one
// definition of each for the binning stage (frontend.hip), the plan kernels (densify.hip, region.hip) and the device-wide scan (scan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DB 256

__device__ __forceinline__ uint32_t dvs_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Wave64 inclusive prefix sum in six DPP additions (gfx9 row operations: shift right by 1, 2, 4, 8 inside the 16-lane rows, then lane 15
// of rows 0 / 2 into rows 1 / 3, then lane 31 into rows 2 / 3). No LDS crossbar round trip per step (a __shfl_up step is a ds_bpermute:
// ~60 cycles of latency on a dependent chain). EXEC must be full: a step reads neighbouring lanes, and a disabled one contributes 0.
__device__ __forceinline__ uint32_t dvs_wave_incl_scan(uint32_t v) {
#define DVS_DPP_ADD(ctrl, rmask) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xF, false)
    DVS_DPP_ADD(0x111, 0xF); DVS_DPP_ADD(0x112, 0xF); DVS_DPP_ADD(0x114, 0xF); DVS_DPP_ADD(0x118, 0xF);   // row_shr:1, 2, 4, 8
    DVS_DPP_ADD(0x142, 0xA);                                                                                // row_bcast:15 -> rows 1, 3
    DVS_DPP_ADD(0x143, 0xC);                                                                                // row_bcast:31 -> rows 2, 3
#undef DVS_DPP_ADD
    return v;
}
__device__ __forceinline__ uint32_t dvs_wave_sum(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)dvs_wave_incl_scan(v), 63); }

// -> the sum of v over the threads before this one; *total = the sum over the workgroup. tmp: DB / 64 words of LDS; two barriers, so
// every thread of the DB-thread workgroup must call it (which also makes EXEC full, as the wave scan needs), and tmp may be used again
// right after it returns.
__device__ __forceinline__ uint32_t dvs_block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t* total) {
    const uint32_t lane = dvs_lane(), wave = threadIdx.x >> 6;
    const uint32_t inc = dvs_wave_incl_scan(v);
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < DB / 64; ++w) { const uint32_t t = tmp[w]; if ((uint32_t)w < wave) wbase += t; tot += t; }
    __syncthreads();
    *total = tot;
    return wbase + inc - v;
}
