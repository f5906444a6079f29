/*
 * dvs_scene.h — deterministic synthetic scenes for the rasterizer hot path (host-side C-ABI).
 *
 * BASELINE.json's configs are all "random splats / synthetic cams". This generator is the one source
 * of those scenes for bench.py, the tests and libgstrain's `synthetic:` loader, following SURVEY.md
 * §8(d) "Synthetic inputs". Real captures (a COLMAP sparse model plus undistorted images, the
 * reference's load_train_data at application/diverseshot-cli/source/gs_train.cpp:108-122) are read by
 * libgstrain's dataset loader (divshot_amd/gstrain/dataset_io.hpp), whose cameras come from
 * dvs_make_camera_intrinsics below.
 */
#ifndef DVS_SCENE_H
#define DVS_SCENE_H
#include <stdint.h>
#include "dvs_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dvs_scene_spec {
    int32_t n;             /* splats */
    int32_t width, height;
    int32_t sh_degree;     /* higher bands beyond this degree are generated as zero */
    int32_t n_cams;        /* camera 0 at the origin looking +Z; 1..n_cams-1 on a 0.5-radius ring, all look at (0,0,7) */
    uint64_t seed;         /* 1 for the BASELINE configs */
    float fov_x_deg;       /* 60 */
    float scale_log_offset;/* added to the log-scale mean (C5 uses -ln 2) */
} dvs_scene_spec;

/* Fill HOST arrays in the A0 layout (pos[n*3] sh0[n*3] shN[n*45] opacity[n] scale[n*3] rot[n*4]). */
int dvs_synth_splats(const dvs_scene_spec* spec, float* pos, float* sh0, float* shN, float* opacity, float* scale, float* rot);
/* Camera `index` of the spec (A1 block, background black). */
int dvs_synth_camera(const dvs_scene_spec* spec, int index, dvs_camera* out);
/* Target image for the L2 upstream gradient: U[0,1), [3,H,W] planar, seeded by (seed+1, index). */
int dvs_synth_target(const dvs_scene_spec* spec, int index, float* target);
/* Build a camera from pose (world->camera rotation R row-major [9], translation t[3]) and pinhole fov. */
int dvs_make_camera(const float* R, const float* t, float fov_x_deg, int width, int height, dvs_camera* out);
/* The same camera from pinhole intrinsics in pixels (COLMAP's PINHOLE: fx, fy, cx, cy; SIMPLE_PINHOLE: fx = fy): same view, near / far and
 * conventions as dvs_make_camera. focal_{x,y} = f{x,y}; tan_fovx = W / (2 fx), tan_fovy = H / (2 fy); the x row of proj carries 2 fx / W
 * and the offset 2 cx / W - 1 (on the camera's z), the y row likewise from fy, cy, H. COLMAP puts a pixel's centre at i + 0.5, this
 * rasterizer at i: a camera-space point (X, Y, Z) lands at pixel (fx X / Z + cx - 0.5, fy Y / Z + cy - 0.5). With cx = W / 2,
 * cy = H / 2 and fx = W / (2 tan), fy = H / (2 tan_y) of a field of view the result equals dvs_make_camera's bit for bit. An off-centre
 * principal point leaves the 1.3 tan_fov guard of the covariance clamp where it is, centred on the image (the decision of
 * dvs_camera_downscale below). DVS_ERR_INVALID for a NULL argument, a size <= 0, fx or fy not positive, a non-finite value. */
int dvs_make_camera_intrinsics(const float* R, const float* t, double fx, double fy, double cx, double cy, int width, int height,
                               dvs_camera* out);
/* The camera of `in` for its image box-downsampled by `factor` (1, 2, 4 or 8; dvs_downsample_views, include/dvs_train.h): the level
 * camera of coarse-to-fine training. view, campos, bg unchanged; width = W / d, height = H / d (floor); focal_{x,y} /= d (exact).
 * With s_x = W / (d W_d), s_y = H / (d H_d) in double (1 when d divides the size, > 1 when columns / rows are cropped):
 *   proj'[k*4+0] = s_x proj[k*4+0] + (s_x - 1) proj[k*4+3],   proj'[k*4+1] likewise with s_y (k = 0..3),   rows 2 and 3 unchanged,
 *   tan_fov' = tan_fov / s    (s == 1: proj and tan_fov come out bit-identical to the input).
 * A splat at pixel x of the full image (pixel i has its centre at i) then lands at (x + 0.5) / d - 0.5 of the level image, the
 * centre of mass of the box filter. The cropped principal point is no longer the image centre, which moves the 1.3 tan_fov guard
 * of the covariance clamp by less than half a level pixel; that is left as it is.
 * DVS_ERR_INVALID for a NULL argument, in == out, another factor, or a size that would become 0. Factor 1 is a copy. */
int dvs_camera_downscale(const dvs_camera* in, int factor, dvs_camera* out);

#ifdef __cplusplus
}
#endif
#endif
