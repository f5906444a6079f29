// sky.hip — the sky model: a learned equirectangular texture behind the splats (dvs_sky_forward_views / dvs_sky_backward_views), for gfx950.
//
// The composite kernels are untouched: with cam.bg = 0 they leave C(p) and final_T(p), and the passes below add what a background that
// varies per pixel needs, out(p) = C(p) + final_T(p) s(p), from the state the forward saved (like depth.hip and importance.hip).
//
// The ray of pixel (x, y) is pixel_ray.h's (shared with the focus region's mask): d = M^-1 (ndc_x, ndc_y, 1), M^-1 the FIRST kernel parameter.
// The lookup: u = (atan2(d.x, d.z) / 2 pi + 0.5) Ws - 0.5, v = (asin(d.y / |d|) / pi + 0.5) Hs - 0.5, texel centres at integer (u, v),
// bilinear, u wrapping modulo Ws, v clamped to [0, Hs - 1]. tests/sky_ref.py restates it in fp64.
//
//   k_sky_forward        one thread per pixel, all views in one launch: out_rgb += final_T s in place, and s to sky_rgb when given.
//   k_sky_backward_tex   dL/dtex: final_T g times the four bilinear weights, scattered with non-returning fp32 atomics. It repeats the
//                        lookup's trigonometry (it needs the texel indices and weights, which sky_rgb does not hold). Consecutive lanes
//                        are consecutive pixels of an image row and a texel is many pixels wide (45 at 1080p, 60 degrees, Ws = 256), so
//                        the twelve products are first summed over runs of lanes that share a texel quad: a segmented inclusive scan
//                        inside each 16-lane row with DPP row shifts (no LDS, no barrier), and only the last lane of a run issues the
//                        atomics, none for a zero. Chosen over a per-workgroup LDS footprint because the footprint of 256 pixels of an
//                        image row is not bounded (a row through the zenith sweeps every column of the texture), while runs need no
//                        bound: where they are short the pass falls back to what the naive scatter costs.
//   k_sky_backward_rows  the gradient through final_T = prod (1 - alpha_k): with h(p) = s(p) . g(p), every entry i pixel p took gets
//                        dL/dalpha_i -= h final_T / (1 - alpha_i), chained exactly as k_render_bwd_tr chains its own dL/dalpha:
//                        v5 = G dL/dalpha, gated by the 0.99 cap unless DVS_GRAD_LINEAGE, the moments of v5 about the splat's mean with
//                        d = mean - pixel times the opacity into row columns 0..4, the plain sum into column 5 (dvs_get_bwd_intermediates).
//                        This is the term the constant-bg path forms inside the composite backward from bg_dot. A replay pass
//                        (replay_walk.h) that accumulates six sums per entry the way importance.hip accumulates its three; no
//                        back-to-front T: final_T is saved and alpha_i is recomputed. Columns 9, 10 (abs-grad) are NOT touched: the
//                        densification statistic stays that of the colour path. Pixels with n_contrib == 0 or h == 0 walk nothing.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "replay_walk.h"
#include "pixel_ray.h"

typedef PixelRays SkyRays;
typedef PixelRay SkyRay;
__device__ __forceinline__ SkyRay sky_load_ray(int v) { return pixel_ray_load(v); }

struct SkyTap { int i00, i01, i10, i11; float w00, w01, w10, w11; };      // texel indices (y Ws + x) and bilinear weights
__device__ __forceinline__ SkyTap sky_tap(const SkyRay& r, int x, int y, int W, int H, int Ws, int Hs) {
    float dx, dy, dz;
    pixel_ray_dir(r, x, y, W, H, dx, dy, dz);
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float sy = fminf(1.0f, fmaxf(-1.0f, dy / len));
    const float u = (atan2f(dx, dz) * 0.15915494309189535f + 0.5f) * (float)Ws - 0.5f;
    const float v = fminf((float)(Hs - 1), fmaxf(0.0f, (asinf(sy) * 0.31830988618379069f + 0.5f) * (float)Hs - 0.5f));
    const float uf = floorf(u), vf = floorf(v);
    const float fu = u - uf, fv = v - vf;
    int x0 = (int)uf % Ws;                                      // u in [-0.5, Ws - 0.5] up to rounding: one wrap either way
    if (x0 < 0) x0 += Ws;
    const int x1 = x0 + 1 == Ws ? 0 : x0 + 1;
    const int y0 = min(max((int)vf, 0), Hs - 1), y1 = min(y0 + 1, Hs - 1);
    SkyTap t;
    t.i00 = y0 * Ws + x0; t.i01 = y0 * Ws + x1; t.i10 = y1 * Ws + x0; t.i11 = y1 * Ws + x1;
    t.w00 = (1.0f - fu) * (1.0f - fv); t.w01 = fu * (1.0f - fv); t.w10 = (1.0f - fu) * fv; t.w11 = fu * fv;
    return t;
}

__global__ void __launch_bounds__(RB)
k_sky_forward(SkyRays rays_arg /* MUST stay the first parameter: read through sky_load_ray() */, int W, int H, int n_views, const float* __restrict__ tex,
              int Ws, int Hs, const float* __restrict__ final_T, float* __restrict__ out_rgb /*[views,3,H,W] or null*/,
              float* __restrict__ sky_rgb /*[views,3,H,W] or null*/) {
    (void)rays_arg;
    const size_t P = (size_t)W * H;
    const size_t gid = (size_t)blockIdx.x * RB + threadIdx.x;
    if (gid >= P * (size_t)n_views) return;
    const int view = (int)(gid / P);
    const size_t p = gid - (size_t)view * P;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    const SkyTap t = sky_tap(sky_load_ray(view), x, y, W, H, Ws, Hs);
    const float T = final_T[gid];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = ((t.w00 * tex[3 * (size_t)t.i00 + c] + t.w01 * tex[3 * (size_t)t.i01 + c]) + t.w10 * tex[3 * (size_t)t.i10 + c]) + t.w11 * tex[3 * (size_t)t.i11 + c];
        const size_t o = ((size_t)view * 3 + c) * P + p;
        if (sky_rgb) sky_rgb[o] = s;
        if (out_rgb) out_rgb[o] = out_rgb[o] + T * s;
    }
}

// one step of the segmented inclusive scan inside a 16-lane row: lane l adds lane l - D unless a run starts between them
template <int D> __device__ __forceinline__ void sky_scan_step(float (&val)[12], int& stop) {
    const int ostop = wave_dpp<0x110 + D>(stop);               // row_shr:D
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float o = wave_dpp<0x110 + D>(val[k]);
        val[k] = stop ? val[k] : val[k] + o;
    }
    stop |= ostop;                                              // (lanes l < D of the row already hold the stop of the row's first lane)
}

__global__ void __launch_bounds__(RB)
k_sky_backward_tex(SkyRays rays_arg /* MUST stay the first parameter */, int W, int H, int n_views, int Ws, int Hs, const float* __restrict__ final_T,
                   const float* __restrict__ dL_dout /*[views,3,H,W]*/, float* __restrict__ g_tex /*[Hs,Ws,3], accumulated into*/) {
    (void)rays_arg;
    const size_t P = (size_t)W * H;
    const size_t gid = (size_t)blockIdx.x * RB + threadIdx.x;
    const bool valid = gid < P * (size_t)n_views;               // (no early return: the row shifts below run with all 64 lanes)
    float val[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) val[k] = 0.f;
    SkyTap t{};
    int key = -1;
    if (valid) {
        const int view = (int)(gid / P);
        const size_t p = gid - (size_t)view * P;
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        t = sky_tap(sky_load_ray(view), x, y, W, H, Ws, Hs);
        key = t.i00;                                            // (i01, i10, i11 follow from i00)
        const float T = final_T[gid];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float tg = T * dL_dout[((size_t)view * 3 + c) * P + p];
            val[c] = t.w00 * tg; val[3 + c] = t.w01 * tg; val[6 + c] = t.w10 * tg; val[9 + c] = t.w11 * tg;
        }
    }
    const int lane16 = threadIdx.x & 15;
    const int prev = wave_dpp<0x111>(key), next = wave_dpp<0x101>(key);          // row_shr:1, row_shl:1
    int stop = (lane16 == 0 || prev != key) ? 1 : 0;            // a run starts here
    const bool last = lane16 == 15 || next != key;              // ... and ends here
    sky_scan_step<1>(val, stop);
    sky_scan_step<2>(val, stop);
    sky_scan_step<4>(val, stop);
    sky_scan_step<8>(val, stop);
    if (valid && last) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (val[c] != 0.f) atomicAdd(&g_tex[3 * (size_t)t.i00 + c], val[c]);
            if (val[3 + c] != 0.f) atomicAdd(&g_tex[3 * (size_t)t.i01 + c], val[3 + c]);
            if (val[6 + c] != 0.f) atomicAdd(&g_tex[3 * (size_t)t.i10 + c], val[6 + c]);
            if (val[9 + c] != 0.f) atomicAdd(&g_tex[3 * (size_t)t.i11 + c], val[9 + c]);
        }
    }
}

struct __attribute__((aligned(16))) SkyRowsLds {
    ReplayLds walk;
    float acc[6][RB / 64][RB];                                  // [value][wave][entry of the batch]
};

template <bool LINEAGE>
__global__ void __launch_bounds__(RB)
k_sky_backward_rows(int W, int H, int tiles_x, int tiles_per_view, int num_tiles, int n, const uint2* __restrict__ ranges,
                    const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d, const float* __restrict__ final_T,
                    const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dout /*[views,3,H,W]*/,
                    const float* __restrict__ sky_rgb /*[views,3,H,W]*/, float* __restrict__ grow /*[views,n,12]*/) {
    __shared__ SkyRowsLds L;
    const ReplayTile rt = replay_tile(W, H, tiles_x, tiles_per_view, num_tiles, ranges);
    if (rt.none) return;
    const int t = threadIdx.x, wave = t >> 6;
    const size_t P = (size_t)W * H;
    float c5 = 0.f;                                                        // -h final_T: dL/dalpha_i = c5 / (1 - alpha_i)
    if (rt.inside) {
        const float* const g = dL_dout + (size_t)rt.view * 3 * P + rt.pix;
        const float* const s = sky_rgb + (size_t)rt.view * 3 * P + rt.pix;
        const float h = (s[0] * g[0] + s[P] * g[P]) + s[2 * P] * g[2 * P];
        c5 = -(final_T[rt.gpix] * h);
    }
    const uint32_t mine = replay_mine(rt, rt.inside && c5 != 0.f, n_contrib);
    uint32_t wm;
    const uint32_t need = replay_need(L.walk, mine, &wm);

    const float pxf = (float)rt.px, pyf = (float)rt.py;
    for (uint32_t base = 0; base < need; base += RB) {
        const uint32_t cnt = min((uint32_t)RB, need - base);
        uint32_t id = 0;
        float op = 0.f;
        if ((uint32_t)t < cnt) {
            id = sorted_splat[rt.range.x + base + t];                      // batch-wide value: view * n + splat, the record's and the row's index
            const float4 r1 = splat2d[4 * (size_t)id + 1];
            op = r1.y;
            replay_stage(L.walk, t, splat2d[4 * (size_t)id], r1, 0.f);
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int w = 0; w < RB / 64; ++w) L.acc[k][w][t] = 0.f;
        }
        __syncthreads();
        const uint32_t stop = replay_stop(mine, base, cnt);
        const uint32_t wave_stop = replay_stop(wm, base, cnt);             // wave-uniform: the cross-lane steps below run with all 64 lanes
        for (uint32_t j = 0; j < wave_stop; ++j) {
            const ReplayEntry e = replay_entry(L.walk.a[j], L.walk.b[j], pxf, pyf);
            const bool take = j < stop && e.take;
            // DVS_GRAD_TRUE: the 0.99 clamp blocks the gradient; DVS_GRAD_LINEAGE: it passes as if alpha = opacity * G (k_render_bwd_tr)
            const bool gate = LINEAGE ? take : (take && !(e.oa > DVS_ALPHA_MAX));
            if (__ballot(gate) == 0ull) continue;
            const float v5 = gate ? e.G * (c5 * __builtin_amdgcn_rcpf(1.f - e.alpha)) : 0.f;
            const float vx = v5 * e.dx, vy = v5 * e.dy;
            const float s[6] = {wave_sum_f32(vx), wave_sum_f32(vy), wave_sum_f32(vx * e.dx), wave_sum_f32(vx * e.dy), wave_sum_f32(vy * e.dy), wave_sum_f32(v5)};
            if ((t & 63) == 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) L.acc[k][wave][j] = s[k];
            }
        }
        __syncthreads();
        if ((uint32_t)t < cnt && replay_owns(id, rt.view, n)) {
            float* const row = grow + (size_t)id * 12;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const float v = replay_fold_sum(L.acc[k], t);
                // the moment sums were taken over v5 = G dL/dalpha; the row contract wants them over opacity * v5 (column 5 is dL/dopacity itself)
                if (v != 0.f) atomicAdd(&row[k], k == 5 ? v : v * op);
            }
        }
        // (the next batch's staging writes only what this thread has just read, and the barrier after it orders the rest)
    }
}

static SkyRays make_sky_rays(int n_views, const float* minv /*[n_views][9]*/) { return make_pixel_rays(n_views, minv); }

hipError_t dvs_launch_sky_forward(hipStream_t st, int W, int H, int n_views, const float* minv, const float* tex, int Ws, int Hs, const float* final_T,
                                  float* out_rgb, float* sky_rgb) {
    const size_t total = (size_t)W * H * n_views;
    if (total == 0) return hipSuccess;
    if (n_views > DVS_MAX_VIEWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sky_forward, dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, st, make_sky_rays(n_views, minv), W, H, n_views, tex, Ws, Hs,
                       final_T, out_rgb, sky_rgb);
    return hipGetLastError();
}

hipError_t dvs_launch_sky_backward_tex(hipStream_t st, int W, int H, int n_views, const float* minv, int Ws, int Hs, const float* final_T,
                                       const float* dL_dout, float* g_tex) {
    const size_t total = (size_t)W * H * n_views;
    if (total == 0) return hipSuccess;
    if (n_views > DVS_MAX_VIEWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sky_backward_tex, dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, st, make_sky_rays(n_views, minv), W, H, n_views, Ws, Hs,
                       final_T, dL_dout, g_tex);
    return hipGetLastError();
}

hipError_t dvs_launch_sky_backward_rows(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges,
                                        const uint32_t* sorted_splat, const float* splat2d, const float* final_T, const uint32_t* n_contrib,
                                        const float* dL_dout, const float* sky_rgb, float* grad_rows, int grad_mode) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0 || n <= 0) return hipSuccess;
    const int grid = replay_grid(num_tiles);
#define DVS_SKY_ROWS(LN)                                                                                                                       \
    hipLaunchKernelGGL((k_sky_backward_rows<LN>), dim3(grid), dim3(RB), 0, st, W, H, tiles_x, tiles_pv, num_tiles, n, (const uint2*)ranges,   \
                       sorted_splat, (const float4*)splat2d, final_T, n_contrib, dL_dout, sky_rgb, grad_rows)
    if (grad_mode == 1) DVS_SKY_ROWS(true); else DVS_SKY_ROWS(false);
#undef DVS_SKY_ROWS
    return hipGetLastError();
}
