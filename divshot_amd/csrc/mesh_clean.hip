// mesh_clean.hip — what happens to an extracted mesh before it is written (include/dvs_mesh.h) for gfx950: connected components of the
// indexed triangle list, removal of the components that are small next to the largest, vertex normals from the TSDF gradient.
//
// Components are a hook-and-compress union-find over parent[] (= the caller's label array):
//   k_cc_init       parent[v] = v
//   k_cc_union      one thread per triangle: union (v0, v1), (v0, v2) — the larger root is linked under the smaller with atomicMin
//   k_cc_flatten    label[v] = the root of v
// parent[x] <= x always, so the root of a component is its smallest vertex index whatever the order the links were made in, and the
// labels are the same from run to run. The per-component counts are integer atomicAdd / atomicMax at the root: sums and maxima of
// integers, independent of arrival order. Nothing here is a float atomic.
//
// Clean-up passes (scratch: 12 B per vertex + 4 B per triangle + the scans' block sums + one block of words):
//   k_clean_tricount   cnt[label[v0]] += 1 for every triangle with three valid indices
//   k_clean_largest    largest = max over roots of cnt
//   k_clean_mark_v     voff[v] = the component of v has a triangle and passes the rule; roots count the components (all, kept)
//   k_clean_mark_t     toff[t] = triangle t is valid and its component passes the rule
//   scan, scan         voff, toff -> exclusive: the new index of a kept vertex / triangle (the scan of mesh.hip)
//   k_clean_finish     gathers the counts and the device error word into the block the host copies
//   k_clean_write_v / k_clean_write_t    move what is kept
// Every vertex of a component that has a triangle is used by one of its triangles (that is what connects it), so "used by a kept
// triangle" is "in a kept component": the vertex pass needs no flags from the triangle pass.
//
// No kernel waits for another workgroup: phases are launches. Every device loop has a trip cap derived from its input; a loop that
// reaches it sets g_mesh_err, which the next dvs_mesh_clean_count returns as DVS_ERR_STATE (and clears).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dvs_mesh.h"
#include "dvs_kernels.h"

#define CB 256

namespace {
__device__ uint32_t g_mesh_err;        // != 0: a capped loop ran out (one word per device)

__device__ __forceinline__ uint32_t ld_relaxed(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x while links are still being made. parent[x] <= x for every x at every moment (initially equal, and every later write is
// an atomicMin or a compare-and-swap with a smaller value), so each step of the walk goes to a strictly smaller index or stops: at
// most n steps. The cap can therefore only be reached on corrupted memory; it is there so that even then the loop ends. On the way
// parent[x] is moved from its parent p to p's parent (path halving) — only if it still is p, so a link made meanwhile is never undone.
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x, uint32_t n) {
    for (uint32_t step = 0; step <= n; ++step) {
        const uint32_t p = ld_relaxed(parent + x);
        if (p >= x) return x;                                          // (p == x: a root; p > x cannot happen)
        const uint32_t gp = ld_relaxed(parent + p);
        if (gp >= p) return p;
        (void)atomicCAS(parent + x, p, gp);
        x = gp;
    }
    atomicOr(&g_mesh_err, 1u);
    return x;
}
// Links the components of a and b. The larger root `hi` goes under the smaller `lo`: atomicMin(&parent[hi], lo) returns hi when hi was
// still a root — done. Otherwise another thread linked hi first, under `old` < hi, and parent[hi] is now min(old, lo): the smaller of
// the two keeps hi, and the other still has to be joined to it, so the loop goes on with (old, lo). Both are < hi: the larger root of a
// retry is strictly smaller than that of the attempt before, hence at most n attempts.
__device__ __forceinline__ void cc_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t n) {
    for (uint32_t attempt = 0; attempt <= n; ++attempt) {
        a = cc_find(parent, a, n);
        b = cc_find(parent, b, n);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old; b = lo;
    }
    atomicOr(&g_mesh_err, 2u);
}

__global__ void __launch_bounds__(CB) k_cc_init(uint32_t n, uint32_t* __restrict__ parent) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v < n) parent[v] = (uint32_t)v;
}
__global__ void __launch_bounds__(CB) k_cc_union(uint32_t n, const uint32_t* __restrict__ tri, uint32_t nt, uint32_t* parent, uint32_t* n_bad) {
    const size_t t = (size_t)blockIdx.x * CB + threadIdx.x;
    if (t >= nt) return;
    const uint32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    if (v0 >= n || v1 >= n || v2 >= n) { if (n_bad) atomicAdd(n_bad, 1u); return; }
    if (v1 != v0) cc_union(parent, v0, v1, n);
    if (v2 != v0 && v2 != v1) cc_union(parent, v0, v2, n);
}
// after the unions the forest no longer changes shape: a thread that overwrites parent[v] with v's root leaves every other walk correct
__global__ void __launch_bounds__(CB) k_cc_flatten(uint32_t n, uint32_t* parent) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v >= n) return;
    uint32_t x = (uint32_t)v;
    bool found = false;
    for (uint32_t step = 0; step <= n; ++step) {                      // parent[x] <= x: strictly downwards, at most n steps
        const uint32_t p = ld_relaxed(parent + x);
        if (p >= x) { found = true; break; }
        x = p;
    }
    if (!found) atomicOr(&g_mesh_err, 4u);
    if (x != (uint32_t)v) __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- clean-up -------------------------------------------------------------------------------------------------------------------
// the words the passes share and the host reads (one 64-byte block at the end of the scratch)
struct CleanBlock {
    unsigned long long kept_vertices, kept_triangles;                 // the scans' totals
    uint32_t largest, n_components, kept_components, n_bad, min_bp, err, _pad[2];
};
struct CleanLayout { size_t label, cnt, voff, toff, bsum_v, bsum_t, block, total; };
CleanLayout clean_layout(uint32_t nv, uint32_t nt) {
    CleanLayout L{};
    const size_t v = nv ? nv : 1, t = nt ? nt : 1;
    size_t o = 0;
    L.label = o; o = dvs_align256(o + v * 4);
    L.cnt = o; o = dvs_align256(o + v * 4);
    L.voff = o; o = dvs_align256(o + v * 4);
    L.toff = o; o = dvs_align256(o + t * 4);
    L.bsum_v = o; o = dvs_align256(o + ((v + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 4);
    L.bsum_t = o; o = dvs_align256(o + ((t + DVS_SCAN_TILE - 1) / DVS_SCAN_TILE) * 4);
    L.block = o; o = dvs_align256(o + sizeof(CleanBlock));
    L.total = o;
    return L;
}
// integers only: the host, the device and the tests agree exactly
__device__ __forceinline__ bool clean_keeps(uint32_t c, uint32_t largest, uint32_t min_bp) {
    return c > 0 && (unsigned long long)c * 10000ull >= (unsigned long long)largest * min_bp;
}
__device__ __forceinline__ bool tri_valid(const uint32_t* __restrict__ tri, size_t t, uint32_t n) {
    return tri[3 * t] < n && tri[3 * t + 1] < n && tri[3 * t + 2] < n;
}

__global__ void k_clean_init(CleanBlock* blk, uint32_t min_bp) {
    blk->kept_vertices = 0; blk->kept_triangles = 0;
    blk->largest = 0; blk->n_components = 0; blk->kept_components = 0; blk->n_bad = 0; blk->min_bp = min_bp; blk->err = 0;
}
__global__ void __launch_bounds__(CB) k_clean_zero(uint32_t n, uint32_t* __restrict__ cnt) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v < n) cnt[v] = 0u;
}
__global__ void __launch_bounds__(CB)
k_clean_tricount(uint32_t n, const uint32_t* __restrict__ tri, uint32_t nt, const uint32_t* __restrict__ label, uint32_t* cnt) {
    const size_t t = (size_t)blockIdx.x * CB + threadIdx.x;
    const bool valid = t < nt && tri_valid(tri, t, n);
    const uint32_t root = valid ? label[tri[3 * t]] : 0xFFFFFFFFu;
    // Most triangles belong to one component: the lanes that share the first valid lane's root add their number once instead of
    // queueing on one word; the others add 1 each. The sum is the same integer either way.
    const unsigned long long any = __ballot(valid);
    if (!any) return;
    const int first = __ffsll(any) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)root, first, 64);
    const unsigned long long same = __ballot(valid && root == r0);
    if (!valid) return;
    if (root != r0) atomicAdd(cnt + root, 1u);
    else if ((int)(threadIdx.x & 63u) == first) atomicAdd(cnt + r0, (uint32_t)__popcll(same));
}
__global__ void __launch_bounds__(CB) k_clean_largest(uint32_t n, const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt, CleanBlock* blk) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v >= n || label[v] != (uint32_t)v) return;
    const uint32_t c = cnt[v];
    if (c > 0) atomicMax(&blk->largest, c);
}
__global__ void __launch_bounds__(CB)
k_clean_mark_v(uint32_t n, const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt, CleanBlock* blk, uint32_t* __restrict__ voff) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v >= n) return;
    const uint32_t root = label[v], c = cnt[root];
    const bool keep = clean_keeps(c, blk->largest, blk->min_bp);
    voff[v] = keep ? 1u : 0u;
    if (root == (uint32_t)v && c > 0) {
        atomicAdd(&blk->n_components, 1u);
        if (keep) atomicAdd(&blk->kept_components, 1u);
    }
}
__global__ void __launch_bounds__(CB)
k_clean_mark_t(uint32_t n, const uint32_t* __restrict__ tri, uint32_t nt, const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt,
               const CleanBlock* __restrict__ blk, uint32_t* __restrict__ toff) {
    const size_t t = (size_t)blockIdx.x * CB + threadIdx.x;
    if (t >= nt) return;
    toff[t] = tri_valid(tri, t, n) && clean_keeps(cnt[label[tri[3 * t]]], blk->largest, blk->min_bp) ? 1u : 0u;
}
__global__ void k_clean_finish(CleanBlock* blk) {
    blk->err = g_mesh_err;
    g_mesh_err = 0u;
}
__global__ void __launch_bounds__(CB)
k_clean_write_v(uint32_t n, const float* __restrict__ xyz, const uint8_t* __restrict__ rgb, const float* __restrict__ normals,
                const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ voff,
                const CleanBlock* __restrict__ blk, float* __restrict__ out_xyz, uint8_t* __restrict__ out_rgb, float* __restrict__ out_normals) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v >= n || !clean_keeps(cnt[label[v]], blk->largest, blk->min_bp)) return;
    const size_t o = voff[v];                                          // < kept_vertices
#pragma unroll
    for (int k = 0; k < 3; ++k) { out_xyz[3 * o + k] = xyz[3 * v + k]; out_rgb[3 * o + k] = rgb[3 * v + k]; }
    if (normals && out_normals) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[3 * o + k] = normals[3 * v + k];
    }
}
__global__ void __launch_bounds__(CB)
k_clean_write_t(uint32_t n, const uint32_t* __restrict__ tri, uint32_t nt, const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt,
                const uint32_t* __restrict__ voff, const uint32_t* __restrict__ toff, const CleanBlock* __restrict__ blk, uint32_t* __restrict__ out_tri) {
    const size_t t = (size_t)blockIdx.x * CB + threadIdx.x;
    if (t >= nt || !tri_valid(tri, t, n)) return;
    const uint32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    if (!clean_keeps(cnt[label[v0]], blk->largest, blk->min_bp)) return;
    const size_t o = toff[t];                                          // < kept_triangles
    out_tri[3 * o] = voff[v0]; out_tri[3 * o + 1] = voff[v1]; out_tri[3 * o + 2] = voff[v2];
}

// ---- normals --------------------------------------------------------------------------------------------------------------------
struct NDims { int dx, dy, dz; };
// the difference of the header along one axis at voxel q (index v, coordinate c of extent n, stride s elements)
__device__ __forceinline__ float grad_axis(const float* __restrict__ tsdf, const float* __restrict__ weight, size_t v, int c, int n, size_t s) {
    const bool lo = c > 0 && weight[v - s] > 0.f, hi = c + 1 < n && weight[v + s] > 0.f;
    if (lo && hi) return (tsdf[v + s] - tsdf[v - s]) * 0.5f;          // (/ 2, exactly)
    if (hi) return tsdf[v + s] - tsdf[v];
    if (lo) return tsdf[v] - tsdf[v - s];
    return 0.f;
}
__device__ __forceinline__ void grad_at(const NDims& g, const float* __restrict__ tsdf, const float* __restrict__ weight, size_t v, int i, int j, int k, float out[3]) {
    out[0] = grad_axis(tsdf, weight, v, i, g.dx, 1);
    out[1] = grad_axis(tsdf, weight, v, j, g.dy, (size_t)g.dx);
    out[2] = grad_axis(tsdf, weight, v, k, g.dz, (size_t)g.dx * g.dy);
}
// One thread per voxel, its (up to 7) vertices in kind order as k_mesh_verts writes them: the gradient at p is formed once for all of
// them, and every normal has exactly one writer.
__global__ void __launch_bounds__(CB)
k_mesh_normals(NDims g, const float* __restrict__ tsdf, const float* __restrict__ weight, const uint8_t* __restrict__ flags,
               const uint32_t* __restrict__ vert_off, float* __restrict__ normals) {
    const size_t v = (size_t)blockIdx.x * CB + threadIdx.x;
    if (v >= (size_t)g.dx * g.dy * g.dz) return;
    uint32_t f = flags[v];
    if (!f) return;
    const int i = (int)(v % (size_t)g.dx), j = (int)((v / (size_t)g.dx) % (size_t)g.dy), k = (int)(v / ((size_t)g.dx * g.dy));
    const float a = tsdf[v];
    float gp[3];
    grad_at(g, tsdf, weight, v, i, j, k, gp);
    size_t id = vert_off[v];
    for (int e = 0; e < 7 && f; ++e) {                                 // (at most the 7 edge kinds)
        const int d = __ffs((int)f);                                   // kind + 1 = the corner the edge runs to
        f &= f - 1;
        const int di = d & 1, dj = (d >> 1) & 1, dk = (d >> 2) & 1;
        const size_t q = v + (size_t)di + (size_t)dj * g.dx + (size_t)dk * g.dx * g.dy;
        const float b = tsdf[q];
        const float t = a / (a - b);                                   // the extraction's own t
        float gq[3], nrm[3];
        grad_at(g, tsdf, weight, q, i + di, j + dj, k + dk, gq);
        const float s = 1.0f - t;
#pragma unroll
        for (int c = 0; c < 3; ++c) nrm[c] = s * gp[c] + t * gq[c];
        dvs_unit_or_zero(nrm[0], nrm[1], nrm[2]);
        normals[3 * id] = nrm[0]; normals[3 * id + 1] = nrm[1]; normals[3 * id + 2] = nrm[2];
        ++id;
    }
}
}  // namespace

extern "C" int dvs_mesh_components(void* stream, uint32_t n_vertices, const uint32_t* tri, uint32_t n_triangles, uint32_t* label, uint32_t* n_bad) {
    if ((n_vertices > 0 && !label) || (n_triangles > 0 && !tri)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n_bad && hipMemsetAsync(n_bad, 0, sizeof(uint32_t), st) != hipSuccess) return DVS_ERR_HIP;
    if (n_vertices > 0) hipLaunchKernelGGL(k_cc_init, dim3(dvs_blocks256(n_vertices)), dim3(CB), 0, st, n_vertices, label);
    // (with no vertex every triangle is bad: the union pass still counts them, and dereferences nothing but tri)
    if (n_triangles > 0) hipLaunchKernelGGL(k_cc_union, dim3(dvs_blocks256(n_triangles)), dim3(CB), 0, st, n_vertices, tri, n_triangles, label, n_bad);
    if (n_vertices > 0 && n_triangles > 0) hipLaunchKernelGGL(k_cc_flatten, dim3(dvs_blocks256(n_vertices)), dim3(CB), 0, st, n_vertices, label);
    return dvs_launch_status();
}

extern "C" size_t dvs_mesh_clean_scratch_bytes(uint32_t n_vertices, uint32_t n_triangles) { return clean_layout(n_vertices, n_triangles).total; }

extern "C" int dvs_mesh_clean_count(void* stream, uint32_t n_vertices, const uint32_t* tri, uint32_t n_triangles, uint32_t min_bp, void* scratch,
                                    dvs_mesh_clean_info* info) {
    if (!scratch || ((uintptr_t)scratch & 255u) || !info || min_bp > 10000u || (n_triangles > 0 && !tri)) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const CleanLayout L = clean_layout(n_vertices, n_triangles);
    char* const base = (char*)scratch;
    uint32_t *label = (uint32_t*)(base + L.label), *cnt = (uint32_t*)(base + L.cnt), *voff = (uint32_t*)(base + L.voff), *toff = (uint32_t*)(base + L.toff);
    CleanBlock* blk = (CleanBlock*)(base + L.block);
    const dim3 gv(dvs_blocks256(n_vertices)), gt(dvs_blocks256(n_triangles)), block(CB);
    hipLaunchKernelGGL(k_clean_init, dim3(1), dim3(1), 0, st, blk, min_bp);
    const int rc = dvs_mesh_components(stream, n_vertices, tri, n_triangles, label, &blk->n_bad);
    if (rc != DVS_OK) return rc;
    if (n_vertices > 0) {
        hipLaunchKernelGGL(k_clean_zero, gv, block, 0, st, n_vertices, cnt);
        if (n_triangles > 0) hipLaunchKernelGGL(k_clean_tricount, gt, block, 0, st, n_vertices, tri, n_triangles, (const uint32_t*)label, cnt);
        hipLaunchKernelGGL(k_clean_largest, gv, block, 0, st, n_vertices, (const uint32_t*)label, (const uint32_t*)cnt, blk);
        hipLaunchKernelGGL(k_clean_mark_v, gv, block, 0, st, n_vertices, (const uint32_t*)label, (const uint32_t*)cnt, blk, voff);
        if (dvs_launch_scan_u32(st, voff, n_vertices, (uint32_t*)(base + L.bsum_v), &blk->kept_vertices) != hipSuccess) return DVS_ERR_HIP;
        if (n_triangles > 0) {
            hipLaunchKernelGGL(k_clean_mark_t, gt, block, 0, st, n_vertices, tri, n_triangles, (const uint32_t*)label, (const uint32_t*)cnt,
                               (const CleanBlock*)blk, toff);
            if (dvs_launch_scan_u32(st, toff, n_triangles, (uint32_t*)(base + L.bsum_t), &blk->kept_triangles) != hipSuccess) return DVS_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(k_clean_finish, dim3(1), dim3(1), 0, st, blk);
    CleanBlock host{};
    if (dvs_fetch_block(st, blk, &host) != DVS_OK) return DVS_ERR_HIP;
    info->n_components = host.n_components; info->largest = host.largest; info->kept_components = host.kept_components;
    info->kept_vertices = (uint32_t)host.kept_vertices; info->kept_triangles = (uint32_t)host.kept_triangles; info->n_bad = host.n_bad;
    return host.err ? DVS_ERR_STATE : DVS_OK;
}

extern "C" int dvs_mesh_clean_write(void* stream, uint32_t n_vertices, const float* xyz, const uint8_t* rgb, const float* normals, const uint32_t* tri,
                                    uint32_t n_triangles, const void* scratch, float* out_xyz, uint8_t* out_rgb, float* out_normals, uint32_t* out_tri) {
    if (!scratch || ((uintptr_t)scratch & 255u) || (normals != nullptr) != (out_normals != nullptr)) return DVS_ERR_INVALID;
    if (n_vertices == 0 || n_triangles == 0) return DVS_OK;           // nothing has a triangle: nothing is kept
    if (!xyz || !rgb || !tri || !out_xyz || !out_rgb || !out_tri) return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const CleanLayout L = clean_layout(n_vertices, n_triangles);
    const char* const base = (const char*)scratch;
    const uint32_t *label = (const uint32_t*)(base + L.label), *cnt = (const uint32_t*)(base + L.cnt), *voff = (const uint32_t*)(base + L.voff),
                   *toff = (const uint32_t*)(base + L.toff);
    const CleanBlock* blk = (const CleanBlock*)(base + L.block);
    hipLaunchKernelGGL(k_clean_write_v, dim3(dvs_blocks256(n_vertices)), dim3(CB), 0, st, n_vertices, xyz, rgb, normals, label, cnt, voff, blk, out_xyz, out_rgb,
                       out_normals);
    hipLaunchKernelGGL(k_clean_write_t, dim3(dvs_blocks256(n_triangles)), dim3(CB), 0, st, n_vertices, tri, n_triangles, label, cnt, voff, toff, blk, out_tri);
    return dvs_launch_status();
}

extern "C" int dvs_mesh_extract_normals(void* stream, const dvs_tsdf_grid* grid, const void* scratch, float* normals) {
    size_t flags_off = 0, vert_off_off = 0;
    if (!grid || !grid->tsdf || !grid->weight || !scratch || ((uintptr_t)scratch & 255u) || !normals ||
        !dvs_mesh_scratch_parts(grid->dims, &vert_off_off, &flags_off))
        return DVS_ERR_INVALID;
    const NDims g{grid->dims[0], grid->dims[1], grid->dims[2]};
    const size_t nv = (size_t)g.dx * g.dy * g.dz;
    const char* const base = (const char*)scratch;
    hipLaunchKernelGGL(k_mesh_normals, dim3(dvs_blocks256(nv)), dim3(CB), 0, (hipStream_t)stream, g, (const float*)grid->tsdf, (const float*)grid->weight,
                       (const uint8_t*)(base + flags_off), (const uint32_t*)(base + vert_off_off), normals);
    return dvs_launch_status();
}
