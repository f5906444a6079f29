// metrics.hip — image metrics of a batch of rendered views against their targets (include/dvs_train.h: dvs_image_metrics_views):
// MSE, L1, mean SSIM and PSNR per view, for the held-out evaluation of the trainer. The SSIM arithmetic is k_ssim_fwd's (ssim.hip):
// one 16x16 tile per workgroup, the 26x26 patches of both images in LDS, separable 11-tap window as a horizontal pass into LDS and
// a vertical pass. What differs from the loss kernel:
//   * ONE launch covers the tiles of all views (blockIdx.z = view; the views' pointers are a kernel argument) and a workgroup loops
//     over the three channels, reusing its LDS buffers — the mask is read once per pixel, not once per channel;
//   * the inputs are formed while they are staged: x = clamp(img, 0, 1) * mask, y = target * mask, an 8-bit target expanded from
//     its bytes right there. The squared and absolute differences are taken from the STAGED values, so they are the differences of
//     the fp32 x and y whatever the compiler contracts, and identical inputs give exactly 0;
//   * nothing is written per pixel: a workgroup leaves three fp32 partial sums in its own slot of `scratch`. No atomics: the
//     workgroup sum is a fixed tree, the finalising kernel adds a view's slots in a fixed order in fp64 — the result is
//     reproducible bit for bit and a view's row does not depend on which views share the launch.
// All global loads of the workgroup (mask, then the three channels of both images) are issued before the first LDS write, selects
// on clamped addresses instead of branches as in load_patches: vector memory returns in order, so channel 0 is consumed while the
// loads of channels 1 and 2 are still in flight. LDS: 13 728 B, the arrays of k_ssim_fwd without its 16-byte reduction buffer
// (the horizontal-pass rows are reused for the workgroup sum).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dvs_train.h"
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "ssim_common.h"

namespace {
struct MetricsViews { dvs_metrics_view v[DVS_METRICS_MAX_VIEWS]; };       // 384 B of kernel arguments
constexpr int kSlot = 4;                                                   // floats per workgroup slot: sum (x-y)^2, sum |x-y|, sum SSIM, pad
constexpr int IT = (SP * SP + ST * ST - 1) / (ST * ST);                    // patch elements per thread (3)

template <bool U8>
__global__ void __launch_bounds__(ST * ST)
k_image_metrics(const MetricsViews views, int W, int H, float* __restrict__ partial) {
    __shared__ float sx[SP][SP], sy[SP][SP];
    __shared__ float hx[SP][ST], hy[SP][ST], hxx[SP][ST], hyy[SP][ST], hxy[SP][ST];     // after the horizontal pass
    const dvs_metrics_view vw = views.v[blockIdx.z];
    const float* __restrict__ img = vw.img;
    const float* __restrict__ tgt_f = (const float*)vw.target;
    const uint8_t* __restrict__ tgt_b = (const uint8_t*)vw.target;
    const float* __restrict__ mask = vw.mask;
    const size_t P = (size_t)W * H;
    const int x0 = blockIdx.x * ST, y0 = blockIdx.y * ST;

    // stage: every load first (in-bounds address or 0, the value discarded by a select), then the arithmetic
    int at[IT];                                  // LDS element, ~element when outside the image, INT_MIN when past the patch
    float m[IT], rx[3][IT], ry[3][IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = threadIdx.x + it * ST * ST;
        const int py = e / SP, px = e - py * SP;
        const int gx = x0 + px - HALO, gy = y0 + py - HALO;
        const bool inb = e < SP * SP && gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t idx = inb ? (size_t)gy * W + gx : 0;
        at[it] = e < SP * SP ? (inb ? e : ~e) : INT32_MIN;
        m[it] = mask ? mask[idx] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rx[c][it] = img[c * P + idx];
            ry[c][it] = U8 ? (float)tgt_b[c * P + idx] * (1.0f / 255.0f) : tgt_f[c * P + idx];
        }
    }
    const int lx = threadIdx.x % ST, ly = threadIdx.x / ST;
    const bool inside = x0 + lx < W && y0 + ly < H;
    float sse = 0.f, sae = 0.f, ssim = 0.f;
    for (int c = 0; c < 3; ++c) {
        // (the previous channel's readers of sx / sy are behind its second barrier)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            if (at[it] == INT32_MIN) continue;
            const bool inb = at[it] >= 0;
            const int e = inb ? at[it] : ~at[it];
            (&sx[0][0])[e] = inb ? fminf(1.f, fmaxf(0.f, rx[c][it])) * m[it] : 0.f;
            (&sy[0][0])[e] = inb ? ry[c][it] * m[it] : 0.f;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < SP * ST; e += ST * ST) {
            const int py = e / ST, px = e % ST;
            float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float g = c_gauss[k], a = sx[py][px + k], b = sy[py][px + k];
                ax += g * a; ay += g * b; axx += g * a * a; ayy += g * b * b; axy += g * a * b;
            }
            hx[py][px] = ax; hy[py][px] = ay; hxx[py][px] = axx; hyy[py][px] = ayy; hxy[py][px] = axy;
        }
        if (inside) {
            const float d = sx[ly + HALO][lx + HALO] - sy[ly + HALO][lx + HALO];
            sse += d * d; sae += fabsf(d);
        }
        __syncthreads();
        float mu1 = 0.f, mu2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = c_gauss[k];
            mu1 += g * hx[ly + k][lx]; mu2 += g * hy[ly + k][lx]; exx += g * hxx[ly + k][lx]; eyy += g * hyy[ly + k][lx]; exy += g * hxy[ly + k][lx];
        }
        if (inside) {
            const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = exx - mu1s, s2 = eyy - mu2s, s12 = exy - mu12;
            const float A = mu1s + mu2s + SSIM_C1, B = s1 + s2 + SSIM_C2, Cn = 2.f * mu12 + SSIM_C1, Dn = 2.f * s12 + SSIM_C2;
            ssim += Cn * Dn * (1.f / (A * B));
        }
    }
    // workgroup sums: a fixed tree inside each wavefront, then the four wavefronts in order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sse += __shfl_xor(sse, d, 64); sae += __shfl_xor(sae, d, 64); ssim += __shfl_xor(ssim, d, 64); }
    __syncthreads();                             // the last vertical pass has read hx
    float* tmp = &hx[0][0];
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; tmp[w] = sse; tmp[4 + w] = sae; tmp[8 + w] = ssim; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const float* t = tmp + 4 * threadIdx.x;
        const size_t slot = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[slot * kSlot + threadIdx.x] = ((t[0] + t[1]) + t[2]) + t[3];
    }
}

// one workgroup per view: thread t adds the slots t, t + 256, ... in that order, then a fixed tree over the threads, all in fp64
__global__ void __launch_bounds__(256)
k_image_metrics_final(const float* __restrict__ partial, int slots_per_view, double count, double* __restrict__ out) {
    __shared__ double acc[3][256];
    const float* p = partial + (size_t)blockIdx.x * slots_per_view * kSlot;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int s = threadIdx.x; s < slots_per_view; s += 256) { a0 += (double)p[(size_t)s * kSlot]; a1 += (double)p[(size_t)s * kSlot + 1]; a2 += (double)p[(size_t)s * kSlot + 2]; }
    acc[0][threadIdx.x] = a0; acc[1][threadIdx.x] = a1; acc[2][threadIdx.x] = a2;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int k = 0; k < 3; ++k) acc[k][threadIdx.x] += acc[k][threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mse = acc[0][0] / count;
        double* o = out + 4 * (size_t)blockIdx.x;
        o[0] = mse; o[1] = acc[1][0] / count; o[2] = acc[2][0] / count;
        o[3] = -10.0 * log10(fmax(mse, 1e-10));
    }
}
}  // namespace

extern "C" {
size_t dvs_image_metrics_scratch_bytes(int width, int height, int n_views) {
    if (width <= 0 || height <= 0 || n_views <= 0) return 0;
    const size_t tiles = (size_t)((width + ST - 1) / ST) * (size_t)((height + ST - 1) / ST);
    return tiles * (size_t)n_views * kSlot * sizeof(float);
}
int dvs_image_metrics_views(void* stream, const dvs_metrics_view* views, int n_views, int width, int height, int target_u8, void* scratch,
                            double* out) {
    if (!views || n_views < 1 || n_views > DVS_METRICS_MAX_VIEWS || width <= 0 || height <= 0 || !scratch || !out) return DVS_ERR_INVALID;
    MetricsViews a{};
    for (int v = 0; v < n_views; ++v) {
        if (!views[v].img || !views[v].target) return DVS_ERR_INVALID;
        a.v[v] = views[v];
    }
    const dim3 grid((width + ST - 1) / ST, (height + ST - 1) / ST, n_views);
    if (grid.y > 65535u) return DVS_ERR_INVALID;
    if (target_u8) hipLaunchKernelGGL(k_image_metrics<true>, grid, dim3(ST * ST), 0, (hipStream_t)stream, a, width, height, (float*)scratch);
    else hipLaunchKernelGGL(k_image_metrics<false>, grid, dim3(ST * ST), 0, (hipStream_t)stream, a, width, height, (float*)scratch);
    if (hipGetLastError() != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_image_metrics_final, dim3(n_views), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, (int)(grid.x * grid.y),
                       3.0 * (double)width * (double)height, out);
    return dvs_launch_status();
}
}
