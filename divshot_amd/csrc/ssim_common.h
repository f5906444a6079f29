// ssim_common.h — what the SSIM loss kernels (ssim.hip) and the image-metric kernel (metrics.hip) must agree on: the tile shape,
// the 11-tap window (sigma 1.5, normalised, fp32), the stabilising constants and the workgroup sum.
#pragma once
#include <hip/hip_runtime.h>

#define ST 16
#define HALO 5
#define SP (ST + 2 * HALO)        // 26
#define SSIM_C1 0.0001f
#define SSIM_C2 0.0009f

static __constant__ float c_gauss[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                                         0.21300552785396576f,  0.26601171493530273f,   0.21300552785396576f,  0.10936068743467331f,
                                         0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f};

__device__ __forceinline__ float block_sum256(float v, float* tmp) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    return tmp[0] + tmp[1] + tmp[2] + tmp[3];
}
