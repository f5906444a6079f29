/*
 * dvs_region.h — C-ABI of the focus region: an oriented box in world space. The trainer keeps only the splats whose centre lies inside
 * it and takes its loss only from the pixels whose ray crosses it (GaussianTrainConfig::enableFocusRegion; INTEGRATION.md "Focus region").
 * The reference's own trainer is closed: what "inside" means below is this build's decision.
 *
 * The region is the set of world points p with lo <= F^-1 p <= hi on all three axes, faces included, where F = T(position) R(rotation)
 * S(scale) is the matrix the editor's maths::Transform builds from the three vectors of updateFocusRegion()
 * (diverse/source/maths/transform.cpp:129: glm::translate(position) * glm::toMat4(glm::quat(rotation)) * glm::scale(scale)):
 * `rotation` holds Euler angles in RADIANS, glm::quat(vec3) composes them as R = Rz(rotation.z) Ry(rotation.y) Rx(rotation.x).
 *
 * Conventions of dvs_train.h: `stream` is a hipStream_t, arrays are DEVICE pointers unless marked HOST, calls are asynchronous and
 * return a DVS_* status (dvs_raster.h); the current HIP device is the caller's. No atomics: two calls on the same inputs return
 * identical bytes. fp32 arithmetic without contraction.
 */
#ifndef DVS_REGION_H
#define DVS_REGION_H
#include <stddef.h>
#include <stdint.h>
#include "dvs_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dvs_region {
    float w2b[12];      /* row-major 3x4, world -> box-local: the first three rows of F^-1 */
    float lo[3];        /* the box in local coordinates */
    float hi[3];
} dvs_region;

/* HOST only. Builds F from pos / rot / scale (three floats each, see above), inverts it in double and rounds: out->w2b, out->lo = lo,
 * out->hi = hi, and b2w = F itself as a row-major 4x4. With pos 0, rot 0, scale 1 both matrices are the identity, exactly.
 * DVS_ERR_INVALID (nothing is written) for a NULL pointer, a scale component that is zero or not finite, a non-finite pos, rot, lo
 * or hi, or lo[k] > hi[k]. */
int dvs_region_from_trs(const float* pos, const float* rot, const float* scale, const float* lo, const float* hi, dvs_region* out,
                        float* b2w /* [16] */);

/* Which splats a region prune keeps, in the form dvs_importance_plan leaves, so that dvs_densify_apply (modes 0 and 1) compacts from it:
 *   action[i]   DVS_DENSIFY_KEEP when the centre pos[3 i .. 3 i + 2] is inside the region, else DVS_DENSIFY_PRUNE (extents are not looked at)
 *   offsets[i]  the exclusive scan of the kept splats;  *new_count (DEVICE uint64) = their number (0 when all are outside)
 * The result is defined bit for bit: with (x, y, z) the centre and (m0, m1, m2, m3) row k of w2b, the local coordinate is
 *   c_k = fmaf(m2, z, fmaf(m1, y, fmaf(m0, x, m3)))
 * in that written order, and the centre is inside iff c_k >= lo[k] && c_k <= hi[k] for k = 0, 1, 2. A NaN or infinite centre is outside.
 * Three launches (flags + block sums | one workgroup scans the block sums, with a running carry | offsets); no host round trip.
 *   pos      [n][3] fp32, natural alignment (a 16-byte aligned array is read as 16-byte words)
 *   scratch  at least (n / 256 + 2) uint32, contents irrelevant (as dvs_densify_plan's)
 * DVS_ERR_INVALID for n <= 0, a NULL pointer, or a new_count that is not 8-byte aligned. */
int dvs_region_plan(void* stream, int n, const float* pos, const dvs_region* region /* HOST */, uint8_t* action, uint32_t* offsets,
                    uint32_t* scratch, uint64_t* new_count);

/* The region's loss mask of a batch of views, ONE launch: out(x, y) = in_mask(x, y) * hit(x, y) (hit itself when in_mask is NULL),
 * hit = 1.0f when the ray through the pixel's centre meets the box at some t >= 0 (a camera inside the box always hits), else 0.0f.
 * The ray is the one the sky lookup uses (dvs_sky_forward_views: derived from cam.proj, so an off-centre principal point and the
 * cameras of dvs_camera_downscale are honoured), its origin cam.campos. A slab test in box-local coordinates: the origin o = F^-1
 * campos (formed on the host in double from w2b, then rounded), the direction l_k = fmaf(m2, dz, fmaf(m1, dy, m0 * dx)) (no
 * translation); per axis t = (lo_k - o_k) / l_k and (hi_k - o_k) / l_k, the ray hits iff max_k min(t) <= min_k max(t) and
 * min_k max(t) >= 0. An axis with l_k exactly 0 passes only when lo_k <= o_k <= hi_k and contributes no t (no 0 * inf).
 *   views     HOST array [n_views] (1..DVS_REGION_MAX_VIEWS), copied before the call returns; every cam.width x cam.height must equal
 *             width x height; in_mask / out are DEVICE [height][width] fp32 and may be the same array
 *   alignment natural (4 bytes). When every in_mask and out is 16-byte aligned and width * height is a multiple of 4 the pixels move
 *             as 16-byte words, else one by one; the result is the same.
 * DVS_ERR_INVALID for NULL views / region / out, n_views outside 1..16, non-positive or mismatching sizes, a singular cam.proj. */
#define DVS_REGION_MAX_VIEWS 16
typedef struct dvs_region_mask_view {
    dvs_camera cam;
    const float* in_mask;   /* DEVICE [H][W] or NULL */
    float* out;             /* DEVICE [H][W] */
} dvs_region_mask_view;
int dvs_region_mask_views(void* stream, const dvs_region_mask_view* views /* HOST [n_views] */, int n_views, int width, int height,
                          const dvs_region* region /* HOST */);

#ifdef __cplusplus
}
#endif
#endif
