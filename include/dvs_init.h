/*
 * dvs_init.h — C-ABI of the splat initialisation from a sparse point cloud (the lineage's create_from_pcd): every SfM point becomes
 * one isotropic splat whose log-scale is half the log of the mean squared distance to its 3 nearest neighbours, opacity 0.1, the
 * point's colour in sh0, identity rotation. The 3-NN search is the published simple-knn scheme: Morton order, one box per 1024
 * consecutive sorted points, every point walks the boxes its current third-best distance cannot rule out.
 *
 * Conventions of dvs_export.h: `stream` is a hipStream_t, every array is a DEVICE pointer on a 16-byte boundary, the calls are
 * asynchronous and return a DVS_* status (dvs_raster.h). No atomics anywhere: two calls on the same inputs return identical bytes.
 * All arithmetic below is fp32 without contraction.
 */
#ifndef DVS_INIT_H
#define DVS_INIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch dvs_knn_mean_dist2 needs for n points (0 for n <= 0): the Morton sort's scratch (dvs_pack_scratch_bytes), one
 * 16-byte record per point in Morton order, two 16-byte box corners per 1024 points. No initialisation needed. */
size_t dvs_knn_scratch_bytes(int n);

/* dist2[i] = mean squared distance of point i to its m = min(3, n - 1) nearest other points, defined bit for bit (inputs finite):
 *   d2(i, j) = ((dx dx + dy dy) + dz dz),  dx = pos[j].x - pos[i].x and likewise y, z,  for every j != i (a duplicate of point i
 *   is a neighbour at distance 0);  d0 <= d1 <= d2 the m smallest of them;
 *   dist2[i] = ((d0 + d1) + d2) / 3.0f  (m = 3),  (d0 + d1) / 2.0f  (m = 2),  d0  (m = 1),  0  (n = 1).
 * Only values enter, so ties cannot change the result; the search prunes boxes by a lower bound that is never above a member's
 * computed d2 and only on strict >, so the result equals the all-pairs one exactly.
 * DVS_ERR_INVALID for n <= 0, a NULL pointer, a pointer off a 16-byte boundary. */
int dvs_knn_mean_dist2(void* stream, int n, const float* pos /*[n][3]*/, void* scratch /*dvs_knn_scratch_bytes(n)*/, float* dist2 /*[n]*/);

/* Measurement hook: the same call, and boxes_streamed[w] = the number of boxes wavefront w (sorted points [64 w, 64 w + 64)) did not
 * skip, its own included, out of ceil(n / 1024). dist2 is identical to dvs_knn_mean_dist2's. */
int dvs_knn_mean_dist2_stats(void* stream, int n, const float* pos, void* scratch, float* dist2, uint64_t* boxes_streamed /*[ceil(n/64)]*/);

/* The initial splats of n points, one lane per point:
 *   sh0_c   = (rgb_c / 255.0f - 0.5f) / 0.28209479177387814f
 *   opacity = logf(0.1f / 0.9f): the logit of 0.1 — one constant, the correctly rounded fp32 logarithm of the fp32 quotient
 *   scale_x = scale_y = scale_z = 0.5f * logf(max(dist2, 1e-7f))      (the device's logf)
 *   rot     = (1, 0, 0, 0)
 * shN is the caller's to zero. DVS_ERR_INVALID for n <= 0, a NULL pointer, a pointer off a 16-byte boundary. */
int dvs_init_from_points(void* stream, int n, const float* pos /*[n][3], unused: the splat centres are the points*/, const uint8_t* rgb /*[n][3]*/,
                         const float* dist2 /*[n]*/, float* sh0 /*[n][3]*/, float* opacity /*[n]*/, float* scale /*[n][3]*/, float* rot /*[n][4]*/);

#ifdef __cplusplus
}
#endif
#endif
