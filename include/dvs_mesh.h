/*
 * dvs_mesh.h — C-ABI of surface extraction from a trained model: truncated-signed-distance (TSDF) fusion of rendered depth maps
 * (dvs_raster_depth_views, dvs_raster.h) into a voxel grid, and marching tetrahedra over that grid into a welded, indexed mesh.
 *
 * Conventions of dvs_train.h: `stream` is a hipStream_t, arrays are DEVICE pointers unless marked HOST, calls are asynchronous unless
 * they say otherwise and return a DVS_* status (dvs_raster.h); the current HIP device is the caller's. No atomics anywhere and no
 * dependence on the launch shape: two runs on the same inputs return identical bytes. fp32 arithmetic without contraction.
 */
#ifndef DVS_MESH_H
#define DVS_MESH_H
#include <stddef.h>
#include <stdint.h>
#include "dvs_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DVS_TSDF_MAX_DIM 1024       /* voxels per axis */
#define DVS_TSDF_MAX_VIEWS 16       /* views per dvs_tsdf_integrate call */

/* The grid. Voxel (i, j, k) has index (k * dims[1] + j) * dims[0] + i (x fastest) and its centre at origin + (i, j, k) * voxel.
 * 20 bytes per voxel: tsdf in [-1, 1] (signed distance / truncation, positive in front of the surface), weight = number of
 * observations, rgb = their mean colour. */
typedef struct dvs_tsdf_grid {
    float origin[3];
    float voxel;
    int32_t dims[3];
    int32_t _pad;
    float* tsdf;        /* [voxels] */
    float* weight;      /* [voxels] */
    float* rgb;         /* [voxels][3] */
} dvs_tsdf_grid;

/* Bytes of the three arrays together (20 per voxel); 0 when a dimension is outside [2, DVS_TSDF_MAX_DIM]. */
size_t dvs_tsdf_bytes(const int32_t dims[3]);
/* Allocates the three arrays and clears them (synchronous). DVS_ERR_INVALID for dims outside [2, DVS_TSDF_MAX_DIM] or voxel <= 0,
 * DVS_ERR_CAPACITY when the grid does not fit the free device memory (nothing is allocated then). dvs_tsdf_destroy frees them.
 * A caller may instead point the descriptor at memory of its own (dvs_tsdf_bytes). */
int dvs_tsdf_create(const float origin[3], float voxel, const int32_t dims[3], dvs_tsdf_grid* out);
void dvs_tsdf_destroy(dvs_tsdf_grid* grid);
/* tsdf = 1, weight = 0, rgb = 0 */
int dvs_tsdf_clear(void* stream, const dvs_tsdf_grid* grid);

/* Fuses n_views (<= DVS_TSDF_MAX_VIEWS) views into the grid: one thread per voxel, the views IN ORDER inside the kernel — integrating
 * views one call at a time gives the same bits as one call over all of them. For each view, with p the voxel centre:
 *   1. zc = (view p).z; skip if zc <= 0.01
 *   2. pixel (u, v) = floor(((ndc + 1) * size - 1) / 2 + 0.5) with ndc = (proj p).xy / (proj p).w — the pixel dvs_raster_forward centres
 *      a splat at p on: focal * x / zc + (size - 1) / 2 plus the principal-point offset proj carries
 *   3. skip if outside the image   4. skip if alpha < 0.5   5. skip if the view has a mask and it is 0 there
 *   6. sdf = depth - zc; skip if sdf < -trunc
 *   7. t = min(1, sdf / trunc); tsdf = (tsdf * weight + t) / (weight + 1), rgb likewise with the pixel's colour; weight += 1
 * cams: HOST [n_views], all of W x H. depth, alpha: [n_views][H][W]; rgb: [n_views][3][H][W]; masks: HOST array (or NULL) of n_views
 * device pointers [H][W], each may be NULL. DVS_ERR_INVALID for a bad argument (dims above DVS_TSDF_MAX_DIM, trunc <= 0, ...). */
int dvs_tsdf_integrate(void* stream, const dvs_tsdf_grid* grid, const dvs_camera* cams, int n_views, const float* depth,
                       const float* alpha, const float* rgb, const float* const* masks, int W, int H, float trunc);

/* Marching tetrahedra. Cell (i, j, k) has the corners (i + dx, j + dy, k + dz), corner number b = dx + 2 dy + 4 dz, and takes part
 * only if all 8 have weight > 0; a corner is inside when tsdf < 0. Every cell is split the same way into the six tetrahedra
 * (0, a, a | b, 7) around its main diagonal — a, b single corner bits, in the order (a, b) = (1,2) (1,4) (2,1) (2,4) (4,1) (4,2) — so
 * neighbours agree on the face diagonals and the surface is watertight.
 * A vertex lives on a grid edge from voxel p to voxel p + d, d = (dx, dy, dz) != 0 in {0,1}^3: p owns 7 edge kinds, kind = dx + 2 dy +
 * 4 dz - 1 (0 x, 1 y, 2 xy diagonal, 3 z, 4 xz, 5 yz, 6 body diagonal); edge id = voxel index * 7 + kind. An edge carries a vertex iff
 * it is an edge of a tetrahedron of a participating cell and its ends differ in sign; position and colour are interpolated at
 * a / (a - b) from p (tsdf a) to p + d (tsdf b). Vertices come in edge-id order.
 * Triangles come in cell order, then tetrahedron, then case order: with the tetrahedron's vertices numbered 0..3 as listed above,
 *   one inside vertex i (outside o0 < o1 < o2):   (i o0, i o1, i o2)
 *   three inside (outside o, inside i0 < i1 < i2): (i0 o, i1 o, i2 o)
 *   two inside i0 < i1 (outside o0 < o1):         the quad q = (i0 o0, i0 o1, i1 o1, i1 o0) as (q0, q1, q2), (q0, q2, q3)
 * and the last two indices of a triangle swapped where needed so that its normal points towards positive tsdf (outside).
 *
 * dvs_mesh_extract_count runs the marking, counting and scan passes into `scratch` (dvs_mesh_scratch_bytes(dims) bytes, 256-byte
 * aligned, no initialisation) and synchronises the stream ONCE to return the counts; DVS_ERR_CAPACITY if either exceeds 2^32 - 1.
 * dvs_mesh_extract_write then writes xyz [n_vertices][3], rgb [n_vertices][3] (bytes: floor(clamp(c, 0, 1) * 255 + 0.5)) and
 * tri [n_triangles][3] from the same scratch and the unchanged grid. */
size_t dvs_mesh_scratch_bytes(const int32_t dims[3]);
int dvs_mesh_extract_count(void* stream, const dvs_tsdf_grid* grid, void* scratch, uint32_t* n_vertices, uint32_t* n_triangles);
int dvs_mesh_extract_write(void* stream, const dvs_tsdf_grid* grid, const void* scratch, float* xyz, uint8_t* rgb, uint32_t* tri);

#ifdef __cplusplus
}
#endif
#endif /* DVS_MESH_H */
