// pixel_ray.h — the world ray through a pixel, shared by the passes that need one per pixel (sky.hip: the sky lookup; region.hip: the
// focus region's mask), so that the pixel centre and the principal point cannot drift apart between them.
//
// The ray of pixel (x, y) (centre = the integer index: ndc_x = (2 x + 1) / W - 1) is derived from `proj`, not from tan_fov: the loaders
// produce cameras with an off-centre principal point (dvs_make_camera_intrinsics: COLMAP's cx, cy; dvs_camera_downscale: a cropped
// level), and for those (ndc_x tan_fovx, ndc_y tan_fovy, 1) is not the pixel's ray. For a world direction d the clip coordinates are
// (x, y, w) = M d with M the rows 0, 1, 3 of proj's 3x3 part (the camera centre maps to x = y = w = 0), so d = M^-1 (ndc_x, ndc_y, 1);
// the host inverts M in fp64 once per view (dvs_pixel_ray_matrix, dvs_api.cpp) and the nine floats arrive at the START of the kernel's
// first parameter, 12 floats per view, read through the kernarg segment (as ViewBg, render_common.h). For a centred pinhole this is
// R^T (ndc_x tan_fovx, ndc_y tan_fovy, 1). d is not normalised.
#pragma once
#include <hip/hip_runtime.h>
#include "dvs_device.h"

struct PixelRays { float m[DVS_MAX_VIEWS][12]; };               // per view: M^-1 row-major in [0..8] (d_r = m[3 r] nx + m[3 r + 1] ny + m[3 r + 2]); [9..11] are the user's
struct PixelRay { float m[9]; };
// view v's matrix of the PixelRays that lead the kernel's first parameter
__device__ __forceinline__ PixelRay pixel_ray_load(int v) {
    PixelRay r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.m[k] = dvs_karg<float>(((size_t)v * 12 + k) * sizeof(float));
    return r;
}
__device__ __forceinline__ void pixel_ray_dir(const PixelRay& r, int x, int y, int W, int H, float& dx, float& dy, float& dz) {
    const float nx = (float)(2 * x + 1) / (float)W - 1.0f, ny = (float)(2 * y + 1) / (float)H - 1.0f;
    dx = (r.m[0] * nx + r.m[1] * ny) + r.m[2]; dy = (r.m[3] * nx + r.m[4] * ny) + r.m[5]; dz = (r.m[6] * nx + r.m[7] * ny) + r.m[8];
}
static inline PixelRays make_pixel_rays(int n_views, const float* minv /*[n_views][9]*/) {
    PixelRays r{};
    for (int v = 0; v < n_views && v < DVS_MAX_VIEWS; ++v) for (int k = 0; k < 9; ++k) r.m[v][k] = minv[9 * v + k];
    return r;
}
