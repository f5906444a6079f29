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
// The same scan of 64-bit words: both halves of a word come from the same source lane, so each step moves them with two DPP reads and
// adds them as one 64-bit number.
__device__ __forceinline__ uint64_t dvs_wave_incl_scan(uint64_t v) {
#define DVS_DPP_ADD64(ctrl, rmask)                                                                             \
    v += (uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, rmask, 0xF, false) |       \
         (uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, rmask, 0xF, false) << 32
    DVS_DPP_ADD64(0x111, 0xF); DVS_DPP_ADD64(0x112, 0xF); DVS_DPP_ADD64(0x114, 0xF); DVS_DPP_ADD64(0x118, 0xF);
    DVS_DPP_ADD64(0x142, 0xA);
    DVS_DPP_ADD64(0x143, 0xC);
#undef DVS_DPP_ADD64
    return v;
}
__device__ __forceinline__ uint32_t dvs_wave_sum(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)dvs_wave_incl_scan(v), 63); }

// -> the sum of v over the threads before this one; *total = the sum over the workgroup. tmp: DB / 64 words of LDS; two barriers, so
// every thread of the DB-thread workgroup must call it (which also makes EXEC full, as the wave scan needs), and tmp may be used again
// right after it returns.
// One body for words of 32 and of 64 bits (tmp and *total have the word's width).
template <class T>
__device__ __forceinline__ T dvs_block_excl_scan_t(T v, T* tmp, T* total) {
    const uint32_t lane = dvs_lane(), wave = threadIdx.x >> 6;
    const T inc = dvs_wave_incl_scan(v);
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    T wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < DB / 64; ++w) { const T t = tmp[w]; if ((uint32_t)w < wave) wbase += t; tot += t; }
    __syncthreads();
    *total = tot;
    return wbase + inc - v;
}
__device__ __forceinline__ uint32_t dvs_block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t* total) { return dvs_block_excl_scan_t<uint32_t>(v, tmp, total); }
__device__ __forceinline__ uint64_t dvs_block_excl_scan(uint64_t v, uint64_t* tmp, uint64_t* total) { return dvs_block_excl_scan_t<uint64_t>(v, tmp, total); }
