// mesh.hip — surface extraction (include/dvs_mesh.h) for gfx950: TSDF fusion of depth maps into a voxel grid, marching tetrahedra
// over the grid into a welded, indexed mesh. HBM-streaming kernels, one thread per voxel, no atomics: every output word has exactly
// one writer and every sum a fixed order, so results do not depend on the launch shape.
//
// Extraction passes (scratch: 10 B per voxel + the scans' block sums):
//   k_mesh_cells      cell_ok[v]   = the cell with lower corner v exists and its 8 corners have weight > 0
//   k_mesh_edges      flags[v]     = bit kind of each of the 7 edges v owns that is crossed inside a participating cell; vert_off[v] = popcount
//   scan              vert_off     -> exclusive: first vertex id of voxel v; the vertex of (v, kind) is vert_off[v] + rank of the bit
//   k_mesh_tricount   tri_off[v]   = triangles of cell v (0 if it does not take part)
//   scan              tri_off      -> exclusive
//   k_mesh_verts / k_mesh_tris     write the arrays
// The scan is scan.hip's (dvs_launch_scan_u32), with ceil(voxels / DVS_SCAN_TILE) block sums each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/dvs_mesh.h"
#include "dvs_device.h"
#include "dvs_kernels.h"

#define MB 256

namespace {
struct GridDims { int dx, dy, dz; };
__host__ __device__ inline size_t grid_voxels(const GridDims& g) { return (size_t)g.dx * g.dy * g.dz; }
bool dims_ok(const int32_t d[3]) { return d && d[0] >= 2 && d[1] >= 2 && d[2] >= 2 && d[0] <= DVS_TSDF_MAX_DIM && d[1] <= DVS_TSDF_MAX_DIM && d[2] <= DVS_TSDF_MAX_DIM; }
bool grid_ok(const dvs_tsdf_grid* g) { return g && dims_ok(g->dims) && g->voxel > 0.f && g->tsdf && g->weight && g->rgb; }

// ---- the 16-case table of the six tetrahedra, derived at compile time -------------------------------------------------------------
// Tetrahedron t has the cell corners c[0] = 0, c[1] = 1 << p0, c[2] = c[1] | 1 << p1, c[3] = 7 for the t-th permutation (p0, p1, p2) of
// the axes in lexicographic order. Case m: bit i set = tetrahedron vertex i inside. An entry lists the triangles' corners as edges
// (lo << 3 | hi), lo a sub-mask of hi: the edge from cell corner lo to cell corner hi. The winding is decided here, on the edge
// midpoints of the unit cell in integer arithmetic (coordinates doubled): a triangle that separates the inside vertices from the outside
// ones keeps its orientation wherever its corners lie on their edges, so the sign found at the midpoints holds for every surface.
struct MtTable { uint8_t ntri[6][16]; uint8_t edge[6][16][6]; };
constexpr int mt_coord(int corner, int axis) { return (corner >> axis) & 1; }
constexpr MtTable mt_build() {
    MtTable tb{};
    const int perm[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};
    for (int t = 0; t < 6; ++t) {
        const int c[4] = {0, 1 << perm[t][0], (1 << perm[t][0]) | (1 << perm[t][1]), 7};
        for (int m = 0; m < 16; ++m) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) { if ((m >> i) & 1) in[ni++] = i; else out[no++] = i; }
            int ea[4] = {}, eb[4] = {}, ne = 0;                      // polygon corners as tetrahedron vertex pairs (ea < eb)
            if (ni == 1) { for (int k = 0; k < 3; ++k) { ea[k] = in[0] < out[k] ? in[0] : out[k]; eb[k] = in[0] < out[k] ? out[k] : in[0]; } ne = 3; }
            else if (ni == 3) { for (int k = 0; k < 3; ++k) { ea[k] = in[k] < out[0] ? in[k] : out[0]; eb[k] = in[k] < out[0] ? out[0] : in[k]; } ne = 3; }
            else if (ni == 2) {
                const int qi[4] = {in[0], in[0], in[1], in[1]}, qo[4] = {out[0], out[1], out[1], out[0]};
                for (int k = 0; k < 4; ++k) { ea[k] = qi[k] < qo[k] ? qi[k] : qo[k]; eb[k] = qi[k] < qo[k] ? qo[k] : qi[k]; }
                ne = 4;
            }
            if (ne == 0) continue;
            // doubled midpoints, the direction from the inside vertices' centroid to the outside ones' (scaled by ni * no)
            int P[4][3] = {}, g[3] = {};
            for (int k = 0; k < ne; ++k) for (int a = 0; a < 3; ++a) P[k][a] = mt_coord(c[ea[k]], a) + mt_coord(c[eb[k]], a);
            for (int a = 0; a < 3; ++a) {
                int si = 0, so = 0;
                for (int k = 0; k < ni; ++k) si += mt_coord(c[in[k]], a);
                for (int k = 0; k < no; ++k) so += mt_coord(c[out[k]], a);
                g[a] = ni * so - no * si;
            }
            const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
            const int nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
            const bool flip = nx * g[0] + ny * g[1] + nz * g[2] < 0;
            const int tris[2][3] = {{0, 1, 2}, {0, 2, 3}};
            tb.ntri[t][m] = (uint8_t)(ne - 2);
            for (int k = 0; k < ne - 2; ++k)
                for (int e = 0; e < 3; ++e) {
                    const int q = tris[k][e == 0 ? 0 : (flip ? 3 - e : e)];
                    tb.edge[t][m][3 * k + e] = (uint8_t)((c[ea[q]] << 3) | c[eb[q]]);
                }
        }
    }
    return tb;
}
__constant__ MtTable c_mt = mt_build();

// the tetrahedron vertices' cell corners again, for the kernels (which case a cell's sign mask selects in tetrahedron t)
__device__ __forceinline__ uint32_t tet_case(uint32_t cube, int t) {
    const int p0 = t >> 1, p1 = (t & 1) ? (p0 == 2 ? 1 : 2) : (p0 == 0 ? 1 : 0);
    const uint32_t c1 = 1u << p0, c2 = c1 | (1u << p1);
    return (cube & 1u) | (((cube >> c1) & 1u) << 1) | (((cube >> c2) & 1u) << 2) | (((cube >> 7) & 1u) << 3);
}

// ---- TSDF ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MB) k_tsdf_clear(size_t nv, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= nv) return;
    tsdf[v] = 1.0f; weight[v] = 0.f;
    rgb[3 * v] = 0.f; rgb[3 * v + 1] = 0.f; rgb[3 * v + 2] = 0.f;
}

// the views of one call: FIRST kernel parameter, read through the kernarg segment pointer (dvs_device.h DvsCams)
struct TsdfViews { DvsCams cams; const float* mask[DVS_MAX_VIEWS]; };
__device__ __forceinline__ const float* tsdf_load_mask(int v) {
    typedef const __attribute__((address_space(4))) uint64_t* KQ;
    const KQ q = (KQ)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(DvsCams)) + v;
    return (const float*)(uintptr_t)*q;
}
__global__ void __launch_bounds__(MB)
k_tsdf_integrate(TsdfViews views_arg /* MUST stay the first parameter */, int n_views, GridDims g, float ox, float oy, float oz, float voxel,
                 float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb, const float* __restrict__ depth,
                 const float* __restrict__ alpha, const float* __restrict__ color, int W, int H, float trunc) {
    (void)views_arg;
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    const int i = (int)(v % (size_t)g.dx), j = (int)((v / (size_t)g.dx) % (size_t)g.dy), k = (int)(v / ((size_t)g.dx * g.dy));
    const float x = ox + (float)i * voxel, y = oy + (float)j * voxel, z = oz + (float)k * voxel;
    float w = weight[v], tv = tsdf[v], c0 = rgb[3 * v], c1 = rgb[3 * v + 1], c2 = rgb[3 * v + 2];
    const float w_in = w;
    const size_t P = (size_t)W * H;
    for (int view = 0; view < n_views; ++view) {
        const DvsCam cam = dvs_load_cam(view);
        const float zc = dvs_xform(cam.view, x, y, z, 2);
        if (!(zc > 0.01f)) continue;
        const float hx = dvs_xform(cam.proj, x, y, z, 0), hy = dvs_xform(cam.proj, x, y, z, 1), hw = dvs_xform(cam.proj, x, y, z, 3);
        const float u = floorf(((hx / hw + 1.0f) * (float)W - 1.0f) * 0.5f + 0.5f);
        const float r = floorf(((hy / hw + 1.0f) * (float)H - 1.0f) * 0.5f + 0.5f);
        if (!(u >= 0.f && u < (float)W && r >= 0.f && r < (float)H)) continue;       // (NaN-safe: a failed comparison skips the view)
        const size_t pix = (size_t)(int)r * W + (size_t)(int)u;
        if (alpha[(size_t)view * P + pix] < 0.5f) continue;
        const float* mask = tsdf_load_mask(view);
        if (mask && mask[pix] == 0.f) continue;
        const float sdf = depth[(size_t)view * P + pix] - zc;
        if (sdf < -trunc) continue;
        const float t = fminf(1.0f, sdf / trunc);
        const float* col = color + (size_t)view * 3 * P + pix;
        const float w1 = w + 1.0f;
        tv = (tv * w + t) / w1;
        c0 = (c0 * w + col[0]) / w1; c1 = (c1 * w + col[P]) / w1; c2 = (c2 * w + col[2 * P]) / w1;
        w = w1;
    }
    if (w != w_in) {
        tsdf[v] = tv; weight[v] = w;
        rgb[3 * v] = c0; rgb[3 * v + 1] = c1; rgb[3 * v + 2] = c2;
    }
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t corner_step(const GridDims& g, int b) {
    return (size_t)(b & 1) + (size_t)((b >> 1) & 1) * g.dx + (size_t)((b >> 2) & 1) * g.dx * g.dy;
}
__global__ void __launch_bounds__(MB) k_mesh_cells(GridDims g, const float* __restrict__ weight, uint8_t* __restrict__ cell_ok) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    const int i = (int)(v % (size_t)g.dx), j = (int)((v / (size_t)g.dx) % (size_t)g.dy), k = (int)(v / ((size_t)g.dx * g.dy));
    bool ok = i + 1 < g.dx && j + 1 < g.dy && k + 1 < g.dz;
    if (ok) {
#pragma unroll
        for (int b = 0; b < 8; ++b) ok = ok && weight[v + corner_step(g, b)] > 0.f;
    }
    cell_ok[v] = ok ? 1 : 0;
}
// The edge (v, v + d) belongs to the cells with lower corner v - s for every corner s with s & d == 0 (there it runs from corner s to
// corner s | d, and every such pair is an edge of the six-tetrahedra split: 12 axis edges, 6 face diagonals, the body diagonal).
__global__ void __launch_bounds__(MB)
k_mesh_edges(GridDims g, const float* __restrict__ tsdf, const uint8_t* __restrict__ cell_ok, uint8_t* __restrict__ flags, uint32_t* __restrict__ vert_cnt) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    const int i = (int)(v % (size_t)g.dx), j = (int)((v / (size_t)g.dx) % (size_t)g.dy), k = (int)(v / ((size_t)g.dx * g.dy));
    uint32_t cells = 0;                                            // bit s: the cell with lower corner v - s takes part
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const bool in = i >= (s & 1) && j >= ((s >> 1) & 1) && k >= ((s >> 2) & 1);
        if (in && cell_ok[v - corner_step(g, s)]) cells |= 1u << s;
    }
    uint32_t f = 0;
    if (cells) {
        const bool a_in = tsdf[v] < 0.f;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            uint32_t users = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) if ((s & d) == 0) users |= 1u << s;
            if (!(cells & users)) continue;                        // (a participating cell around the edge: v + d is inside the grid)
            const bool b_in = tsdf[v + corner_step(g, d)] < 0.f;
            if (a_in != b_in) f |= 1u << (d - 1);
        }
    }
    flags[v] = (uint8_t)f;
    vert_cnt[v] = (uint32_t)__popc(f);
}
__global__ void __launch_bounds__(MB)
k_mesh_verts(GridDims g, float ox, float oy, float oz, float voxel, const float* __restrict__ tsdf, const float* __restrict__ rgb,
             const uint8_t* __restrict__ flags, const uint32_t* __restrict__ vert_off, float* __restrict__ xyz, uint8_t* __restrict__ out_rgb) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    uint32_t f = flags[v];
    if (!f) return;
    const int i = (int)(v % (size_t)g.dx), j = (int)((v / (size_t)g.dx) % (size_t)g.dy), k = (int)(v / ((size_t)g.dx * g.dy));
    const float a = tsdf[v], ca[3] = {rgb[3 * v], rgb[3 * v + 1], rgb[3 * v + 2]};
    size_t id = vert_off[v];
    while (f) {
        const int d = __ffs((int)f);                               // kind + 1 = the corner the edge runs to
        f &= f - 1;
        const size_t q = v + corner_step(g, d);
        const float b = tsdf[q];
        const float t = a / (a - b);
        xyz[3 * id] = ox + ((float)i + t * (float)(d & 1)) * voxel;
        xyz[3 * id + 1] = oy + ((float)j + t * (float)((d >> 1) & 1)) * voxel;
        xyz[3 * id + 2] = oz + ((float)k + t * (float)((d >> 2) & 1)) * voxel;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float c = ca[ch] + t * (rgb[3 * q + ch] - ca[ch]);
            out_rgb[3 * id + ch] = (uint8_t)floorf(fminf(fmaxf(c, 0.f), 1.f) * 255.0f + 0.5f);
        }
        ++id;
    }
}
__device__ __forceinline__ uint32_t cube_signs(const GridDims& g, const float* __restrict__ tsdf, size_t v) {
    uint32_t cube = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) cube |= (tsdf[v + corner_step(g, b)] < 0.f ? 1u : 0u) << b;
    return cube;
}
__global__ void __launch_bounds__(MB)
k_mesh_tricount(GridDims g, const float* __restrict__ tsdf, const uint8_t* __restrict__ cell_ok, uint32_t* __restrict__ tri_cnt) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    uint32_t cnt = 0;
    if (cell_ok[v]) {
        const uint32_t cube = cube_signs(g, tsdf, v);
        if (cube != 0u && cube != 0xFFu) {
#pragma unroll
            for (int t = 0; t < 6; ++t) cnt += c_mt.ntri[t][tet_case(cube, t)];
        }
    }
    tri_cnt[v] = cnt;
}
__global__ void __launch_bounds__(MB)
k_mesh_tris(GridDims g, const float* __restrict__ tsdf, const uint8_t* __restrict__ cell_ok, const uint8_t* __restrict__ flags,
            const uint32_t* __restrict__ vert_off, const uint32_t* __restrict__ tri_off, uint32_t* __restrict__ tri) {
    const size_t v = (size_t)blockIdx.x * MB + threadIdx.x;
    if (v >= grid_voxels(g)) return;
    if (!cell_ok[v]) return;
    const uint32_t cube = cube_signs(g, tsdf, v);
    if (cube == 0u || cube == 0xFFu) return;
    size_t o = (size_t)tri_off[v] * 3;
    for (int t = 0; t < 6; ++t) {
        const uint32_t m = tet_case(cube, t);
        const int nt = c_mt.ntri[t][m];
        for (int e = 0; e < 3 * nt; ++e) {
            const uint32_t code = c_mt.edge[t][m][e], lo = code >> 3, hi = code & 7u;
            const size_t owner = v + corner_step(g, (int)lo);
            const uint32_t below = (1u << ((lo ^ hi) - 1u)) - 1u;      // the owner's crossed edges of a lower kind
            tri[o++] = vert_off[owner] + (uint32_t)__popc((uint32_t)flags[owner] & below);
        }
    }
}

struct MeshScratch { size_t vert_off, tri_off, flags, cell_ok, bsum_v, bsum_t, totals, total; uint32_t nb; };
MeshScratch mesh_layout(size_t nv) {
    MeshScratch L{};
    L.nb = (uint32_t)((nv + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE);
    size_t o = 0;
    L.vert_off = o; o = dvs_align256(o + nv * 4);
    L.tri_off = o; o = dvs_align256(o + nv * 4);
    L.flags = o; o = dvs_align256(o + nv);
    L.cell_ok = o; o = dvs_align256(o + nv);
    L.bsum_v = o; o = dvs_align256(o + (size_t)L.nb * 4);
    L.bsum_t = o; o = dvs_align256(o + (size_t)L.nb * 4);
    L.totals = o; o = dvs_align256(o + 16);
    L.total = o;
    return L;
}
}  // namespace

// for mesh_clean.hip (dvs_kernels.h): where the extraction's scratch keeps what the normals read
bool dvs_mesh_scratch_parts(const int32_t dims[3], size_t* vert_off, size_t* flags) {
    if (!dims_ok(dims)) return false;
    const MeshScratch L = mesh_layout((size_t)dims[0] * dims[1] * dims[2]);
    *vert_off = L.vert_off; *flags = L.flags;
    return true;
}

extern "C" size_t dvs_tsdf_bytes(const int32_t dims[3]) { return dims_ok(dims) ? (size_t)dims[0] * dims[1] * dims[2] * 20 : 0; }

extern "C" int dvs_tsdf_clear(void* stream, const dvs_tsdf_grid* grid) {
    if (!grid_ok(grid)) return DVS_ERR_INVALID;
    const size_t nv = (size_t)grid->dims[0] * grid->dims[1] * grid->dims[2];
    hipLaunchKernelGGL(k_tsdf_clear, dim3(dvs_blocks256(nv)), dim3(MB), 0, (hipStream_t)stream, nv, grid->tsdf, grid->weight, grid->rgb);
    return dvs_launch_status();
}

extern "C" int dvs_tsdf_create(const float origin[3], float voxel, const int32_t dims[3], dvs_tsdf_grid* out) {
    if (!origin || !out || !dims_ok(dims) || !(voxel > 0.f)) return DVS_ERR_INVALID;
    const size_t nv = (size_t)dims[0] * dims[1] * dims[2];
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return DVS_ERR_HIP;
    if (dvs_tsdf_bytes(dims) + (64u << 20) > free_b) return DVS_ERR_CAPACITY;       // (64 MiB left for the allocator's own rounding)
    dvs_tsdf_grid g{};
    for (int k = 0; k < 3; ++k) { g.origin[k] = origin[k]; g.dims[k] = dims[k]; }
    g.voxel = voxel;
    if (hipMalloc((void**)&g.tsdf, nv * 4) != hipSuccess || hipMalloc((void**)&g.weight, nv * 4) != hipSuccess ||
        hipMalloc((void**)&g.rgb, nv * 12) != hipSuccess) {
        (void)hipGetLastError();
        dvs_tsdf_destroy(&g);
        return DVS_ERR_CAPACITY;
    }
    const int rc = dvs_tsdf_clear(nullptr, &g);
    if (rc != DVS_OK || hipStreamSynchronize(nullptr) != hipSuccess) { dvs_tsdf_destroy(&g); return DVS_ERR_HIP; }
    *out = g;
    return DVS_OK;
}
extern "C" void dvs_tsdf_destroy(dvs_tsdf_grid* grid) {
    if (!grid) return;
    if (grid->tsdf) (void)hipFree(grid->tsdf);
    if (grid->weight) (void)hipFree(grid->weight);
    if (grid->rgb) (void)hipFree(grid->rgb);
    grid->tsdf = grid->weight = grid->rgb = nullptr;
}

extern "C" int dvs_tsdf_integrate(void* stream, const dvs_tsdf_grid* grid, const dvs_camera* cams, int n_views, const float* depth,
                                  const float* alpha, const float* rgb, const float* const* masks, int W, int H, float trunc) {
    static_assert(sizeof(DvsCam) == sizeof(dvs_camera), "DvsCam must mirror dvs_camera");
    if (!grid_ok(grid) || !cams || n_views < 1 || n_views > DVS_TSDF_MAX_VIEWS || !depth || !alpha || !rgb || W <= 0 || H <= 0 || !(trunc > 0.f))
        return DVS_ERR_INVALID;
    for (int v = 0; v < n_views; ++v) if (cams[v].width != W || cams[v].height != H) return DVS_ERR_INVALID;
    TsdfViews views{};
    for (int v = 0; v < n_views; ++v) { memcpy(&views.cams.c[v], &cams[v], sizeof(DvsCam)); views.mask[v] = masks ? masks[v] : nullptr; }
    const GridDims g{grid->dims[0], grid->dims[1], grid->dims[2]};
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(dvs_blocks256(grid_voxels(g))), dim3(MB), 0, (hipStream_t)stream, views, n_views, g, grid->origin[0],
                       grid->origin[1], grid->origin[2], grid->voxel, grid->tsdf, grid->weight, grid->rgb, depth, alpha, rgb, W, H, trunc);
    return dvs_launch_status();
}

extern "C" size_t dvs_mesh_scratch_bytes(const int32_t dims[3]) { return dims_ok(dims) ? mesh_layout((size_t)dims[0] * dims[1] * dims[2]).total : 0; }

extern "C" int dvs_mesh_extract_count(void* stream, const dvs_tsdf_grid* grid, void* scratch, uint32_t* n_vertices, uint32_t* n_triangles) {
    if (!grid_ok(grid) || !scratch || ((uintptr_t)scratch & 255u) || !n_vertices || !n_triangles) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const GridDims g{grid->dims[0], grid->dims[1], grid->dims[2]};
    const size_t nv = grid_voxels(g);
    const MeshScratch L = mesh_layout(nv);
    char* const base = (char*)scratch;
    uint32_t *vert_off = (uint32_t*)(base + L.vert_off), *tri_off = (uint32_t*)(base + L.tri_off);
    uint8_t *flags = (uint8_t*)(base + L.flags), *cell_ok = (uint8_t*)(base + L.cell_ok);
    unsigned long long* totals = (unsigned long long*)(base + L.totals);
    const dim3 grid_dim(dvs_blocks256(nv)), block(MB);
    hipLaunchKernelGGL(k_mesh_cells, grid_dim, block, 0, st, g, (const float*)grid->weight, cell_ok);
    hipLaunchKernelGGL(k_mesh_edges, grid_dim, block, 0, st, g, (const float*)grid->tsdf, (const uint8_t*)cell_ok, flags, vert_off);
    if (dvs_launch_scan_u32(st, vert_off, nv, (uint32_t*)(base + L.bsum_v), totals) != hipSuccess) return DVS_ERR_HIP;
    hipLaunchKernelGGL(k_mesh_tricount, grid_dim, block, 0, st, g, (const float*)grid->tsdf, (const uint8_t*)cell_ok, tri_off);
    if (dvs_launch_scan_u32(st, tri_off, nv, (uint32_t*)(base + L.bsum_t), totals + 1) != hipSuccess) return DVS_ERR_HIP;
    unsigned long long host_totals[2] = {0, 0};
    if (hipMemcpyAsync(host_totals, totals, sizeof host_totals, hipMemcpyDeviceToHost, st) != hipSuccess) return DVS_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return DVS_ERR_HIP;
    if (host_totals[0] > 0xFFFFFFFFull || host_totals[1] > 0xFFFFFFFFull) return DVS_ERR_CAPACITY;
    *n_vertices = (uint32_t)host_totals[0];
    *n_triangles = (uint32_t)host_totals[1];
    return DVS_OK;
}

extern "C" int dvs_mesh_extract_write(void* stream, const dvs_tsdf_grid* grid, const void* scratch, float* xyz, uint8_t* rgb, uint32_t* tri) {
    if (!grid_ok(grid) || !scratch || ((uintptr_t)scratch & 255u) || !xyz || !rgb || !tri) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const GridDims g{grid->dims[0], grid->dims[1], grid->dims[2]};
    const size_t nv = grid_voxels(g);
    const MeshScratch L = mesh_layout(nv);
    const char* const base = (const char*)scratch;
    const uint32_t *vert_off = (const uint32_t*)(base + L.vert_off), *tri_off = (const uint32_t*)(base + L.tri_off);
    const uint8_t *flags = (const uint8_t*)(base + L.flags), *cell_ok = (const uint8_t*)(base + L.cell_ok);
    const dim3 grid_dim(dvs_blocks256(nv)), block(MB);
    hipLaunchKernelGGL(k_mesh_verts, grid_dim, block, 0, st, g, grid->origin[0], grid->origin[1], grid->origin[2], grid->voxel, (const float*)grid->tsdf,
                       (const float*)grid->rgb, flags, vert_off, xyz, rgb);
    hipLaunchKernelGGL(k_mesh_tris, grid_dim, block, 0, st, g, (const float*)grid->tsdf, cell_ok, flags, vert_off, tri_off, tri);
    return dvs_launch_status();
}
