/*
 * dvs_mesh.h — C-ABI of surface extraction from a trained model: truncated-signed-distance (TSDF) fusion of rendered depth maps
 * (dvs_raster_depth_views, dvs_raster.h) into a voxel grid, marching tetrahedra over that grid into a welded, indexed mesh, and what
 * is done to that mesh before it is written: vertex normals from the grid, removal of small connected components, decimation by vertex
 * clustering.
 *
 * Conventions of dvs_train.h: `stream` is a hipStream_t, arrays are DEVICE pointers unless marked HOST, calls are asynchronous unless
 * they say otherwise and return a DVS_* status (dvs_raster.h); the current HIP device is the caller's. The only atomics are integer
 * atomics whose result does not depend on order (minimum, maximum, sum — in the component passes below) and there is no dependence
 * on the launch shape: two runs on the same inputs still return identical bytes. fp32 arithmetic without contraction.
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

/* Vertex normals from the grid, for the vertices of dvs_mesh_extract_write in the same order: normals [n_vertices][3], from the scratch
 * dvs_mesh_extract_count filled and the unchanged grid. The gradient g(q) of a voxel q has, per axis with unit step e, the component
 *   (tsdf(q + e) - tsdf(q - e)) / 2   when both neighbours count,
 *   tsdf(q + e) - tsdf(q)  or  tsdf(q) - tsdf(q - e)   when only q + e / only q - e counts,
 *   0   when neither does,
 * where a neighbour counts iff it is inside the grid and has weight > 0. The vertex on the edge from p to p + d, at the extraction's
 * own t = a / (a - b), gets n = (1 - t) * g(p) + t * g(p + d) (two products, one sum per component), divided by its length
 * sqrt((n.x * n.x + n.y * n.y) + n.z * n.z) — or (0, 0, 0) when that sum of squares is < 1e-30. tsdf is positive outside, so n points
 * outwards, to the side the triangles' winding faces. One thread per voxel over its vertices, as the extraction writes them: every
 * normal has one writer, no atomics. */
int dvs_mesh_extract_normals(void* stream, const dvs_tsdf_grid* grid, const void* scratch /*of dvs_mesh_extract_count*/, float* normals);

/* Connected components of an indexed triangle list: two vertices are connected when a triangle uses both. label [n_vertices] receives
 * for every vertex the SMALLEST vertex index of its component (a vertex no triangle uses is its own component) — a function of the mesh
 * alone, identical from run to run. A triangle with an index >= n_vertices is ignored (never dereferenced) and counted in *n_bad
 * (DEVICE, one word, zeroed by the call; may be NULL); an index repeated inside a triangle is legal; n_triangles == 0 (label[v] = v)
 * and n_vertices == 0 (every triangle is bad) are legal.
 * Hook-and-compress union-find with label as the parent array: parent[v] = v; one thread per triangle unions (v0, v1) and (v0, v2) by
 * linking the larger root under the smaller with an atomic minimum, retrying with the displaced link when it loses a race; a last
 * launch follows every vertex to its root. parent[x] <= x throughout, so every walk goes strictly downwards and has at most n_vertices
 * steps, and a retry's larger root is smaller than the one before: every device loop is capped by n_vertices. A loop that reaches its
 * cap (possible only on corrupted memory) sets a device error word; the next dvs_mesh_clean_count on that device returns
 * DVS_ERR_STATE for it, and clears it. No kernel waits for another workgroup. */
int dvs_mesh_components(void* stream, uint32_t n_vertices, const uint32_t* tri, uint32_t n_triangles, uint32_t* label /*[n_vertices]*/,
                        uint32_t* n_bad /*device, 1 word, may be NULL*/);

/* Clean-up of an extracted mesh: the components that are small next to the largest are dropped, with their vertices.
 * A component with c triangles is kept iff c > 0 and (uint64) c * 10000 >= (uint64) largest * min_bp — min_bp in 1/100 of a percent,
 * 0..10000 (DVS_ERR_INVALID above): 0 keeps everything that has a triangle, 10000 only the components that tie for largest. Triangle
 * counts and `largest` are integer sums / maxima at the component's root. Kept triangles keep their order; kept vertices are the
 * vertices a kept triangle uses, in their old order, so vertices without a triangle disappear; indices are remapped through an
 * exclusive scan; xyz, rgb and normals move unchanged, bit for bit.
 * dvs_mesh_clean_count runs the component, counting, marking and scan passes into `scratch` (dvs_mesh_clean_scratch_bytes bytes,
 * 256-byte aligned, no initialisation) and synchronises the stream ONCE to fill *info; DVS_ERR_STATE when a capped device loop ran
 * out (see dvs_mesh_components). dvs_mesh_clean_write then writes out_xyz / out_rgb / out_normals [kept_vertices][3] and out_tri
 * [kept_triangles][3] from the same scratch and the unchanged inputs; normals and out_normals are both given or both NULL. */
typedef struct dvs_mesh_clean_info {
    uint32_t n_components;      /* components with at least one triangle */
    uint32_t largest;           /* triangles of the biggest */
    uint32_t kept_components;
    uint32_t kept_vertices;
    uint32_t kept_triangles;
    uint32_t n_bad;             /* triangles ignored for an index >= n_vertices */
} dvs_mesh_clean_info;
size_t dvs_mesh_clean_scratch_bytes(uint32_t n_vertices, uint32_t n_triangles);
int dvs_mesh_clean_count(void* stream, uint32_t n_vertices, const uint32_t* tri, uint32_t n_triangles, uint32_t min_bp, void* scratch,
                         dvs_mesh_clean_info* info /*HOST*/);
int dvs_mesh_clean_write(void* stream, uint32_t n_vertices, const float* xyz, const uint8_t* rgb, const float* normals /*or NULL*/,
                         const uint32_t* tri, uint32_t n_triangles, const void* scratch, float* out_xyz, uint8_t* out_rgb,
                         float* out_normals /*or NULL*/, uint32_t* out_tri);

/* Decimation by vertex clustering (Rossignac-Borrel), the last stage before the mesh is written: a lattice of ncell[0] x ncell[1] x
 * ncell[2] cubic cells of edge `cell` from `origin`; all vertices of a cell become ONE vertex with their mean position, colour and
 * normal, triangles are re-indexed, collapsed and repeated triangles are dropped, and so are the clusters no surviving triangle uses.
 * Defined bit for bit (tests/mesh_decimate_ref.py restates it):
 * Cell of a vertex, per axis a: q = (x_a - origin_a) / cell (one fp32 subtraction, one fp32 IEEE division); i_a = 0 if !(q >= 0) (a NaN
 *   too), ncell_a - 1 if q >= (float) ncell_a, else (uint32) q; key = (i_z * ncell_y + i_y) * ncell_x + i_x < 2^30.
 * Clusters: the (key, vertex index) pairs in a stable sort by key; a sorted position is a cluster's head iff it is the first or its key
 *   differs from its predecessor's; the exclusive scan of the heads numbers the clusters in key order (n_clusters of them); the members
 *   of a cluster are in ascending vertex index.
 * Triangles: one with an index >= n_vertices is bad — counted in n_bad, dropped, never dereferenced. Otherwise its corners are replaced
 *   by their cluster numbers; it is degenerate — counted, dropped — if two of the three are equal. Two survivors are duplicates if their
 *   cluster triples are equal after each is rotated so that its smallest number comes first; the winding is kept, so (a, b, c),
 *   (b, c, a) and (c, a, b) are one triangle and (a, c, b), which faces the other way, is another. Of a set of duplicates the one with the
 *   smallest triangle index is kept and the others are counted in n_duplicate. (Found by stable LSD sorts of (word, triangle index)
 *   over the three rotated words, last word first, and an equal-to-predecessor test: no hashing, nothing that depends on order.)
 * Output: the kept triangles in their old order and their old corner order (not the rotated one); the vertices are the clusters some
 *   kept triangle uses, in key order; indices are remapped through exclusive scans.
 * Attributes of an output vertex, over its cluster's members m0 < m1 < ... (vertex indices), count of them:
 *   xyz per component: s = x[m0]; s = s + x[m1]; ... (serial, fp32), then s / (float) count;
 *   rgb per channel: the integer sum, then (2 * sum + count) / (2 * count) in integers (the mean, rounded half up);
 *   normals: the same serial fp32 sums n, no division by count; l2 = (n.x * n.x + n.y * n.y) + n.z * n.z; (0, 0, 0) when l2 < 1e-30,
 *   else each component divided by sqrtf(l2) — the rule of dvs_mesh_extract_normals.
 * dvs_mesh_decimate_count runs the key, sort, scan and marking passes into `scratch` (dvs_mesh_decimate_scratch_bytes bytes, 256-byte
 * aligned, no initialisation) and synchronises the stream ONCE to fill *info. dvs_mesh_decimate_write (asynchronous) then writes out_xyz /
 * out_rgb / out_normals [out_vertices][3] and out_tri [out_triangles][3] from the same scratch and the unchanged inputs; it gathers the
 * vertex records in sorted order into a part of the scratch that is its own workspace, and leaves what _count put there unchanged, so it
 * may be called again. normals and out_normals are both given or both NULL.
 * DVS_ERR_INVALID, before any device work: scratch NULL or not 256-byte aligned; info, origin or ncell NULL; cell <= 0 or not finite; an
 * ncell outside 1..1024; normals without out_normals or the reverse. DVS_ERR_CAPACITY for more than 2^31 - 1 vertices or triangles.
 * n_vertices == 0 (every triangle is bad) and n_triangles == 0 are legal and give empty outputs. The only atomics are integer sums. */
typedef struct dvs_mesh_decimate_info {
    uint32_t out_vertices, out_triangles;   /* what dvs_mesh_decimate_write will produce */
    uint32_t n_clusters;                    /* occupied cells, before unused ones are dropped */
    uint32_t n_degenerate, n_duplicate, n_bad;
} dvs_mesh_decimate_info;
size_t dvs_mesh_decimate_scratch_bytes(uint32_t n_vertices, uint32_t n_triangles);
int dvs_mesh_decimate_count(void* stream, uint32_t n_vertices, const float* xyz, const uint32_t* tri, uint32_t n_triangles,
                            const float origin[3] /*HOST*/, float cell, const int32_t ncell[3] /*HOST, each 1..1024*/, void* scratch,
                            dvs_mesh_decimate_info* info /*HOST*/);
int dvs_mesh_decimate_write(void* stream, uint32_t n_vertices, const float* xyz, const uint8_t* rgb, const float* normals /*or NULL*/,
                            const uint32_t* tri, uint32_t n_triangles, const void* scratch, float* out_xyz, uint8_t* out_rgb,
                            float* out_normals /*or NULL*/, uint32_t* out_tri);

#ifdef __cplusplus
}
#endif
#endif /* DVS_MESH_H */
