// filter3d.hip — the 3D smoothing filter of Mip-Splatting (arXiv 2311.16493; include/dvs_train.h, last section): every splat is low-pass
// filtered in world space by the highest rate at which a training camera samples it.
//   compute      filter[i] = sqrt(0.2) min over the cameras that see splat i of z / focal_x; one thread per splat, the 64-byte camera rows
//                staged through LDS 64 at a time, the maximum over the seen splats folded per workgroup in LDS and then by ONE integer
//                atomic max on the float's bits (filters are > 0: the unsigned order of the bits is the order of the floats, as
//                importance.hip's score_max), the unseen splats filled with it by a second launch
//   apply_range  the raw scale and opacity the rasterizer reads: the splat's Gaussian convolved with the filter's, its opacity scaled by the
//                ratio of the two normalisations
//   chain_range  gradients with respect to those effective values -> gradients with respect to the trained ones, in place
// All three are element-wise: a range is bit-identical to the same rows of a whole-array call. Compiled without FMA contraction
// (Makefile): the float32 restatement in tests/filter3d_ref.py evaluates the same operations one by one.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/dvs_train.h"
#include "dvs_device.h"

namespace {
constexpr int kCamBatch = 64;                  // cameras per LDS batch: 64 rows of 16 floats = 4 KiB, one float4 per thread of the workgroup
constexpr float kNear = 0.2f;                  // the paper code's near bound
constexpr float kMargin = 0.65f;               // half the image plus its 15 % margin
constexpr float kSqrtVariance = 0.44721359549995793f;     // sqrt(0.2), the filter's variance in pixels^2
constexpr float kUnseen = -1.0f;               // what compute leaves for fill (a filter is never negative)

__global__ void __launch_bounds__(256) k_filter3d_compute(int n, const float* __restrict__ pos, const float4* __restrict__ cam_rows, int n_cams,
                                                          float* __restrict__ filter, uint32_t* __restrict__ scratch) {
    __shared__ float4 rows[kCamBatch * 4];
    __shared__ uint32_t blk_max, blk_seen;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) { blk_max = 0u; blk_seen = 0u; }
    float px = 0.f, py = 0.f, pz = 0.f;
    bool finite = false;
    if (i < n) {
        px = pos[3 * (size_t)i]; py = pos[3 * (size_t)i + 1]; pz = pos[3 * (size_t)i + 2];
        finite = isfinite(px) && isfinite(py) && isfinite(pz);
    }
    float best = INFINITY;
    for (int c0 = 0; c0 < n_cams; c0 += kCamBatch) {
        const int nb = min(kCamBatch, n_cams - c0);
        __syncthreads();                                                     // (the batch before this one has been read; the counters are set)
        if ((int)threadIdx.x < nb * 4) rows[threadIdx.x] = cam_rows[(size_t)c0 * 4 + threadIdx.x];
        __syncthreads();
        for (int c = 0; c < nb; ++c) {
            const float4 r0 = rows[4 * c], r1 = rows[4 * c + 1], r2 = rows[4 * c + 2], k = rows[4 * c + 3];     // k = focal_x, width, height, pad
            const float x = ((r0.x * px + r0.y * py) + r0.z * pz) + r0.w;
            const float y = ((r1.x * px + r1.y * py) + r1.z * pz) + r1.w;
            const float z = ((r2.x * px + r2.y * py) + r2.z * pz) + r2.w;
            const bool sees = z > kNear && fabsf(x / z * k.x) <= kMargin * k.y && fabsf(y / z * k.x) <= kMargin * k.z;
            if (sees) best = fminf(best, z / k.x);
        }
    }
    const bool seen = finite && best < INFINITY;
    if (i < n) {
        const float f = seen ? kSqrtVariance * best : kUnseen;
        filter[i] = f;
        if (seen) { (void)atomicMax(&blk_max, __float_as_uint(f)); (void)atomicAdd(&blk_seen, 1u); }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blk_seen > 0u) { (void)atomicMax(&scratch[0], blk_max); (void)atomicAdd(&scratch[1], blk_seen); }
}

__global__ void __launch_bounds__(256) k_filter3d_fill(int n, float* __restrict__ filter, const uint32_t* __restrict__ scratch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && filter[i] < 0.f) filter[i] = __uint_as_float(scratch[0]);
}

// what apply and chain share for one splat with f != 0: r_k = s_k^2 / (s_k^2 + f^2), q_k = 1 - r_k = f^2 / (s_k^2 + f^2) (no cancellation),
// d_k = s_k^2 + f^2, c = sqrt(r_0 r_1 r_2) as a product of roots (the product of the r_k alone would underflow for f >> s),
// 1 - c = (1 - c^2) / (1 + c) with 1 - r_0 r_1 r_2 = q_0 + r_0 q_1 + r_0 r_1 q_2 (sums of non-negative terms only),
// sp = sigmoid(a), sn = sigmoid(-a), u = 1 - o' = sn + sp (1 - c)
struct Filtered { float r[3], q[3], d[3], c, sp, sn, u; };
__device__ __forceinline__ Filtered filtered(const float s[3], float a, float f) {
    Filtered F;
    const float f2 = f * f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float s2 = expf(2.0f * s[k]);
        F.d[k] = s2 + f2;
        F.r[k] = s2 / F.d[k];
        F.q[k] = f2 / F.d[k];
    }
    F.c = (sqrtf(F.r[0]) * sqrtf(F.r[1])) * sqrtf(F.r[2]);
    const float one_minus_c = ((F.q[0] + F.r[0] * F.q[1]) + (F.r[0] * F.r[1]) * F.q[2]) / (1.0f + F.c);
    F.sp = 1.0f / (1.0f + expf(-a));
    F.sn = 1.0f / (1.0f + expf(a));
    F.u = F.sn + F.sp * one_minus_c;
    return F;
}

__global__ void __launch_bounds__(256) k_filter3d_apply(int first, int count, const float* __restrict__ scale, const float* __restrict__ opacity,
                                                        const float* __restrict__ filter, float* __restrict__ scale_eff, float* __restrict__ opacity_eff) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const size_t i = (size_t)first + t;
    const float s[3] = {scale[3 * i], scale[3 * i + 1], scale[3 * i + 2]};
    const float a = opacity[i], f = filter[i];
    if (f == 0.0f) {                                                         // no filter: the trained values as they are, bit for bit
        scale_eff[3 * i] = s[0]; scale_eff[3 * i + 1] = s[1]; scale_eff[3 * i + 2] = s[2];
        opacity_eff[i] = a;
        return;
    }
    const Filtered F = filtered(s, a, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) scale_eff[3 * i + k] = 0.5f * logf(F.d[k]);
    opacity_eff[i] = logf(F.sp * F.c) - logf(F.u);                           // logit(o'), o' = sigmoid(a) c
}

__global__ void __launch_bounds__(256) k_filter3d_chain(int first, int count, const float* __restrict__ scale, const float* __restrict__ opacity,
                                                        const float* __restrict__ filter, float* __restrict__ g_scale, float* __restrict__ g_opacity) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const size_t i = (size_t)first + t;
    const float f = filter[i];
    if (f == 0.0f) return;                                                   // the identity
    const float s[3] = {scale[3 * i], scale[3 * i + 1], scale[3 * i + 2]};
    const Filtered F = filtered(s, opacity[i], f);
    const float go = g_opacity[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) g_scale[3 * i + k] = g_scale[3 * i + k] * F.r[k] + go * F.q[k] / F.u;
    g_opacity[i] = go * F.sn / F.u;
}

bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15u) != 0;
}
bool bad_range(int n, int first, int count) { return n < 0 || first < 0 || count < 0 || (int64_t)first + count > n; }
}  // namespace

extern "C" {
int dvs_filter3d_pack_cameras(const dvs_camera* cams, int n_cams, float* host_rows) {
    if (!cams || !host_rows || n_cams < 1) return DVS_ERR_INVALID;
    for (int c = 0; c < n_cams; ++c) {
        float* o = host_rows + 16 * (size_t)c;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) o[4 * r + k] = cams[c].view[k * 4 + r];      // view[c*4+r]: row r of world -> camera
        o[12] = cams[c].focal_x; o[13] = (float)cams[c].width; o[14] = (float)cams[c].height; o[15] = 0.f;
    }
    return DVS_OK;
}

int dvs_filter3d_compute(void* stream, int n, const float* pos, const float* dev_cam_rows, int n_cams, float* filter, uint32_t* scratch) {
    if (n < 0 || n_cams < 1 || !dev_cam_rows || !scratch || (n > 0 && (!pos || !filter)) || misaligned(pos, dev_cam_rows, filter, scratch)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, 16, st) != hipSuccess) return DVS_ERR_HIP;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_filter3d_compute, dim3(dvs_blocks256((size_t)n)), dim3(256), 0, st, n, pos, (const float4*)dev_cam_rows, n_cams, filter, scratch);
    hipLaunchKernelGGL(k_filter3d_fill, dim3(dvs_blocks256((size_t)n)), dim3(256), 0, st, n, filter, (const uint32_t*)scratch);
    return dvs_launch_status();
}

int dvs_filter3d_apply_range(void* stream, int n, int first, int count, const float* scale, const float* opacity, const float* filter, float* scale_eff,
                             float* opacity_eff) {
    if (bad_range(n, first, count) || (n > 0 && (!scale || !opacity || !filter || !scale_eff || !opacity_eff)) ||
        misaligned(scale, opacity, filter, scale_eff, opacity_eff)) return DVS_ERR_INVALID;
    if (count == 0) return DVS_OK;
    hipLaunchKernelGGL(k_filter3d_apply, dim3(dvs_blocks256((size_t)count)), dim3(256), 0, (hipStream_t)stream, first, count, scale, opacity, filter, scale_eff,
                       opacity_eff);
    return dvs_launch_status();
}
int dvs_filter3d_apply(void* stream, int n, const float* scale, const float* opacity, const float* filter, float* scale_eff, float* opacity_eff) {
    return dvs_filter3d_apply_range(stream, n, 0, n, scale, opacity, filter, scale_eff, opacity_eff);
}

int dvs_filter3d_chain_range(void* stream, int n, int first, int count, const float* scale, const float* opacity, const float* filter, float* g_scale,
                             float* g_opacity) {
    if (bad_range(n, first, count) || (n > 0 && (!scale || !opacity || !filter || !g_scale || !g_opacity)) ||
        misaligned(scale, opacity, filter, g_scale, g_opacity)) return DVS_ERR_INVALID;
    if (count == 0) return DVS_OK;
    hipLaunchKernelGGL(k_filter3d_chain, dim3(dvs_blocks256((size_t)count)), dim3(256), 0, (hipStream_t)stream, first, count, scale, opacity, filter, g_scale,
                       g_opacity);
    return dvs_launch_status();
}
int dvs_filter3d_chain(void* stream, int n, const float* scale, const float* opacity, const float* filter, float* g_scale, float* g_opacity) {
    return dvs_filter3d_chain_range(stream, n, 0, n, scale, opacity, filter, g_scale, g_opacity);
}
}
