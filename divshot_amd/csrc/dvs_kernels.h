// dvs_kernels.h — host-callable launchers of the gfx950 kernels (internal to libdvsraster.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dvs_device.h"

// preprocess.hip
hipError_t dvs_launch_preprocess_fwd(hipStream_t st, int n, const float* pos, const float* sh0, const float* shN,
                                     const float* opacity, const float* scale, const float* rot, const DvsCams& cams, int n_views,
                                     int deg, int antialias, int tiles_x, int tiles_y, int* radii /*per-view outputs are [n_views][n]*/, float* splat2d,
                                     float* depth, uint32_t* flags,
                                     uint32_t* tiles_touched, uint32_t* depth_key, int shn_tiled,
                                     uint32_t* rect /*[n_views][n] tile-rectangle records of format rect_fmt*/, int rect_fmt /*DVS_FE_RECT_* (below)*/,
                                     uint32_t* kred /*segmented front end: the views' key ranges [n_views][64][16] (zeroed by the caller)*/,
                                     int first, int count /*splat range of this launch: [first, first + count), count < 0 = up to n*/);
hipError_t dvs_launch_preprocess_bwd(hipStream_t st, int n, const float* pos, const float* shN, const float* opacity,
                                     const float* scale, const float* rot, const DvsCam& cam, int deg, int antialias,
                                     const int* radii, const uint32_t* flags, float* grad_rows /*[n,12], read then re-zeroed*/,
                                     float* g_pos, float* g_sh0, float* g_shN, float* g_opacity, float* g_scale,
                                     float* g_rot, float* out_absgrad2d /*nullable*/, float* out_mean2d /*nullable*/,
                                     float* out_dcolor /*nullable*/, int accumulate, int rezero_rows, int shn_tiled, int grad_mode);
// A9 for all views of a batch in one pass (DVS_SHN_TILED layout only): radii / flags / grad_rows are [n_views][n]; writes the
// geometry gradients (sums over the views) and out_dcolor [n_views][n][3]; the SH rows follow from dcolor (dvs_launch_sh_grad_combine).
// [first, first + count) is the splat range of this launch (A9 can run in chunks). g_sh0 / g_shN both given: the kernel builds the SH
// rows itself (tiled layout) from the views' colour gradients and does NOT write out_dcolor — the one-GPU path.
hipError_t dvs_launch_preprocess_bwd_views(hipStream_t st, int n, int n_views, const float* pos, const float* shN, const float* opacity,
                                           const float* scale, const float* rot, const DvsCams& cams, int deg, int antialias,
                                           const int* radii, const uint32_t* flags, float* grad_rows, float* g_pos, float* g_opacity,
                                           float* g_scale, float* g_rot, float* out_absgrad2d, float* out_mean2d, float* out_dcolor,
                                           int accumulate, int rezero_rows, int grad_mode, int first, int count, float* g_sh0 /*nullable*/,
                                           float* g_shN /*nullable*/);
// g_sh0 / g_shN may be nullptr in dvs_launch_preprocess_bwd (factorised exchange); this rebuilds them from dcolor[n_views,n,3].
hipError_t dvs_launch_sh_grad_combine(hipStream_t st, int n, const float* pos, int deg, int n_views, const float* campos_host,
                                      const float* dcolor, float* g_sh0, float* g_shN, int accumulate, int shn_tiled);
// reference rows [n][45] <-> tiled [ceil(n/64)][45][64]
hipError_t dvs_launch_dcolor_from_rows(hipStream_t st, int64_t total, const int* radii, const uint32_t* flags, const float* rows, float* dcolor);
hipError_t dvs_launch_shn_relayout(hipStream_t st, int n, const float* src, float* dst, int to_tiled);

// frontend.hip — the segmented (per-view) binning stage of round 5
// One segment of a segmented sort / scan (device memory, 32 B): a view's run of elements and its rows of the histogram table.
struct DvsSeg {
    uint32_t base;      // first element of the segment in the key / value arrays
    uint32_t count;     // its elements
    uint32_t pstart;    // its first row (partition) in the histogram table
    uint32_t sub;       // depth sort: the view's smallest key (digits are taken from key - sub)
    uint32_t bits;      // depth sort: digit width b = ceil(bits(max - min) / 3), 1..11
    uint32_t _r0, _r1, _r2;
};
// tile-rectangle record formats (A2 writes, A3 gathers, A4 streams)
enum { DVS_FE_RECT_U8 = 0 /*4 B: minx | miny << 8 | width << 16 | height << 24 (tiles_x, tiles_y <= 255: up to 4080 x 4080 pixels)*/,
       DVS_FE_RECT_U16 = 1 /*8 B: [minx | maxx << 16, miny | maxy << 16] (larger images)*/,
       DVS_FE_RECT_TIGHT = 2 /*16 B: the 8-B rectangle + the 64-bit tile mask of DVS_TILES_TIGHT*/ };
// The record of each format: `pack` is what A2 writes (tiles [minx, maxx) x [miny, maxy); `mask` is read by TIGHT alone), the
// accessors are what A3 / A4 read; zero() is the record of a culled splat (count 0).
template <int FMT> struct FeRect;
template <> struct FeRect<DVS_FE_RECT_U8> {
    typedef uint32_t T;
    static __device__ __forceinline__ T pack(uint32_t minx, uint32_t miny, uint32_t maxx, uint32_t maxy, unsigned long long) {
        return minx | (miny << 8) | ((maxx - minx) << 16) | ((maxy - miny) << 24);
    }
    static __device__ __forceinline__ uint32_t count(T r) { return ((r >> 16) & 0xFFu) * (r >> 24); }
    static __device__ __forceinline__ uint32_t minx(T r) { return r & 0xFFu; }
    static __device__ __forceinline__ uint32_t miny(T r) { return (r >> 8) & 0xFFu; }
    static __device__ __forceinline__ uint32_t width(T r) { return (r >> 16) & 0xFFu; }
    static __device__ __forceinline__ T zero() { return 0u; }
};
template <> struct FeRect<DVS_FE_RECT_U16> {
    typedef uint2 T;
    static __device__ __forceinline__ T pack(uint32_t minx, uint32_t miny, uint32_t maxx, uint32_t maxy, unsigned long long) {
        return make_uint2(minx | (maxx << 16), miny | (maxy << 16));
    }
    static __device__ __forceinline__ uint32_t count(T r) { return ((r.x >> 16) - (r.x & 0xFFFFu)) * ((r.y >> 16) - (r.y & 0xFFFFu)); }
    static __device__ __forceinline__ uint32_t minx(T r) { return r.x & 0xFFFFu; }
    static __device__ __forceinline__ uint32_t miny(T r) { return r.y & 0xFFFFu; }
    static __device__ __forceinline__ uint32_t width(T r) { return (r.x >> 16) - (r.x & 0xFFFFu); }
    static __device__ __forceinline__ T zero() { return make_uint2(0u, 0u); }
};
template <> struct FeRect<DVS_FE_RECT_TIGHT> {
    typedef uint4 T;
    static __device__ __forceinline__ T pack(uint32_t minx, uint32_t miny, uint32_t maxx, uint32_t maxy, unsigned long long mask) {
        return make_uint4(minx | (maxx << 16), miny | (maxy << 16), (uint32_t)mask, (uint32_t)(mask >> 32));
    }
    static __device__ __forceinline__ uint32_t count(T r) {
        const uint32_t both = r.z & r.w;
        return both == 0xFFFFFFFFu ? ((r.x >> 16) - (r.x & 0xFFFFu)) * ((r.y >> 16) - (r.y & 0xFFFFu)) : (uint32_t)(__popc(r.z) + __popc(r.w));
    }
    static __device__ __forceinline__ uint32_t minx(T r) { return r.x & 0xFFFFu; }
    static __device__ __forceinline__ uint32_t miny(T r) { return r.y & 0xFFFFu; }
    static __device__ __forceinline__ uint32_t width(T r) { return (r.x >> 16) - (r.x & 0xFFFFu); }
    static __device__ __forceinline__ T zero() { return make_uint4(0u, 0u, 0u, 0u); }
};
#define DVS_FE_KRED_WORDS (DVS_MAX_VIEWS * 64 * 16)        /* key-range slots: [view][64][16 words] */
#define DVS_FE_MAXBINS 2048                                     /* 11-bit digits: 3 x 11 >= 31 bits, every positive float's range */
#define DVS_FE_SUPER_STRIDE 32                                  /* u64 words between two super-sum counters (256 B: own memory channel) */
size_t dvs_fe_hist_words(uint64_t max_elems, int n_views, int max_bins);       // histogram table words for sorts of up to max_elems elements in n_views segments
uint32_t dvs_depth_sort_rows_per_view(int n, int V);
uint32_t dvs_fe_part_for(uint64_t grid_elems);                                 // keys per partition for a sort of about that many elements
void dvs_fe_block_counts(int n, uint32_t* nbv, uint32_t* nsb);                 // A3 workgroups per view, 64-bit super sums per view
hipError_t dvs_launch_seg_init(hipStream_t st, int n, int V, uint32_t rows_per_view, DvsSeg* seg_all);
// A5 (depth): keys0 [V][n] (culled = 0xFFFFFFFF) -> vals1[v * n + j] = index of the j-th nearest visible splat of view v, j < seg_vis[v].count
hipError_t dvs_launch_depth_sort(hipStream_t st, int n, int V, uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1,
                                 DvsSeg* seg_all, DvsSeg* seg_vis, const uint32_t* kred, uint32_t* hist, uint32_t* totals /*[V][DVS_FE_MAXBINS]*/,
                                 int rank_atomic = 0 /*scatter ranks by returning LDS adds: only after dvs_fe_probe_rank_atomic passed*/);
// stable LSD sort of every segment's pairs over the key bits [bit_lo, bit_lo + bits) (digits <= 9 bits); result in buffers *result_in
hipError_t dvs_launch_seg_sort(hipStream_t st, int V, uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1, DvsSeg* seg, int bit_lo, int bits,
                               uint64_t grid_elems, uint32_t part, uint32_t nbtot, uint32_t* hist, uint32_t* totals, uint32_t key_add_per_view,
                               int* result_in, uint32_t* ranges_enc = nullptr /*A6 fused into the last pass: tile ranges as (~start, end), see k_seg_scatter*/,
                               int write_last_keys = 1, int first_keys16 = 0 /*keys0 holds 16-bit keys (A4's tile ids)*/, int rank_atomic = 0);
// The same sort for ONE segment [0, n): what every user outside the multi-view front end calls (the packers' Morton order, the codebooks,
// the cell clustering and the mesh decimation's triangle words, dvs_sort_pairs_u32). Buffers 0 hold the input, *cur says which hold the result; bits <= 0 launches nothing and
// leaves *cur = 0. The workspace, never initialised: dvs_pair_sort_ws_bytes(n) bytes carved by dvs_pair_sort_ws_at into {descriptor,
// totals, histogram} on 256-byte boundaries, or three parts the caller owns (hist: dvs_pair_sort_hist_bytes(n), totals: DVS_FE_MAXBINS
// words). rank_atomic = 0 is the ballot ranking: correct by construction, no probe of the device needed.
struct DvsPairSortWs { DvsSeg* seg; uint32_t* totals; uint32_t* hist; };
size_t dvs_pair_sort_hist_bytes(uint64_t n), dvs_pair_sort_ws_bytes(uint64_t n);
DvsPairSortWs dvs_pair_sort_ws_at(void* base);
hipError_t dvs_launch_pair_sort(hipStream_t st, uint64_t n, uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1, int bit_lo, int bits,
                                const DvsPairSortWs& ws, int rank_atomic, int* cur);
// runs the two in-wave rankings of k_seg_scatter side by side on synthetic digits; *bad_dev (zeroed) counts disagreements (frontend.hip)
hipError_t dvs_fe_probe_rank_atomic(hipStream_t st, uint32_t* bad_dev);
// stage 0 = A3 (tile counts in depth order, block / super sums) + the views' instance ranges (seg_tile, total_dev); stage 1 = A4
hipError_t dvs_launch_seg_binning(hipStream_t st, int n, int V, int rect_fmt, const DvsSeg* seg_vis, DvsSeg* seg_tile, const uint32_t* sorted_ids,
                                  const uint32_t* rect, uint32_t* rect_sorted, uint32_t* block_sums, unsigned long long* super, uint32_t* superexcl,
                                  uint32_t tile_part, unsigned long long* total_dev, unsigned long long capacity, int stage, int tiles_x,
                                  uint32_t* inst_tile, uint32_t* inst_splat, int key16 = 0 /*A4 writes the tile ids as 16-bit words*/);

// frontend.hip, continued
// A6: per-tile [start,end) from the sorted tile ids. T_dev (nullable): device-side count, T sizes the grid.
hipError_t dvs_launch_tile_ranges(hipStream_t st, uint64_t T, const uint32_t* sorted_tile, uint32_t* ranges /*zeroed by the caller*/,
                                  const uint64_t* T_dev = nullptr, uint64_t T_expected = 0);
// canonical 64-bit keys of the sorted list (parity export)
hipError_t dvs_launch_export_keys(hipStream_t st, uint64_t T, const uint32_t* sorted_tile, const uint32_t* sorted_splat,
                                  const float* depth, uint64_t* out_keys);

// render.hip — one launch covers the tiles of all n_views views of a batch (view-major ranges / pixel arrays; bgs = [n_views][3])
hipError_t dvs_launch_render_fwd(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges /*ranges_out != null: the
                                 encoded form (~start, end) of the tile sort's last pass, (0, 0) = empty*/,
                                 const uint32_t* sorted_splat, const float* splat2d, const float* bgs, float* out_color, float* final_T,
                                 uint32_t* n_contrib, uint32_t* live_splat /*[T] out (or null): per tile, the entries whose alpha >= 1/255 ellipse
                                 reaches the tile, compacted in list order from ranges[tile].x*/, uint32_t* live_pos /*[T] out (or null): list
                                 position -> number of such entries before it in its tile*/,
                                 uint64_t* take_masks /*test hook (or null): [take_cap][4] zeroed by the caller — per list position and 8x8 quadrant, the pixels that took the entry*/,
                                 uint64_t take_cap, uint32_t* ranges_out = nullptr /*where k_render_fwd leaves (start, end) when `ranges` is encoded*/);
// depth.hip — expected depth and alpha of the saved forward state, all n_views views in one launch (out arrays are [n_views][H][W])
hipError_t dvs_launch_depth_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges /*canonical (start, end)*/,
                                  const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, float* out_depth, float* out_alpha);
// importance.hip — per-splat blend weight of the saved forward state, all n_views views in one launch: accumulates into score_sum [n] (uint64),
// score_max [n] and hits [n] (either may be null); masks = HOST array [n_views] of DEVICE [H,W] pointers, or null, entries may be null
hipError_t dvs_launch_importance_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges /*canonical (start, end)*/,
                                       const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, const float* const* masks,
                                       uint64_t* score_sum, uint32_t* score_max, uint32_t* hits);
// foreground.hip — where the blend weight of the saved forward state landed, all n_views views in one launch: accumulates into fg_sum [n] and
// bg_sum [n] (uint64); fg_masks / valid_masks = HOST arrays [n_views] of DEVICE [H,W] pointers, or null, entries may be null. And the plan over
// the two sums: three launches (flags + block sums | scan.hip's block-sum scan | offsets), scratch = (n / 256 + 2) words
hipError_t dvs_launch_foreground_views(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges /*canonical (start, end)*/,
                                       const uint32_t* sorted_splat, const float* splat2d, const uint32_t* n_contrib, const float* const* fg_masks,
                                       const float* const* valid_masks, uint64_t* fg_sum, uint64_t* bg_sum);
hipError_t dvs_launch_foreground_plan(hipStream_t st, int n, const uint64_t* fg, const uint64_t* bg, int percent, uint8_t* action, uint32_t* offsets,
                                      uint32_t* scratch, uint64_t* new_count);
// sky.hip — the sky texture behind the splats, all n_views views in one launch each. minv = HOST [n_views][9]: per view the inverse of rows
// 0, 1, 3 of proj's 3x3 part, row-major (world ray of a pixel = minv (ndc_x, ndc_y, 1)); tex = DEVICE [Hs][Ws][3].
// forward: out_rgb += final_T s in place (null: skipped), s -> sky_rgb (null: skipped); both are [n_views][3][H][W]
hipError_t dvs_launch_sky_forward(hipStream_t st, int W, int H, int n_views, const float* minv, const float* tex, int Ws, int Hs, const float* final_T,
                                  float* out_rgb, float* sky_rgb);
// g_tex [Hs][Ws][3] += final_T dL_dout times the bilinear weights
hipError_t dvs_launch_sky_backward_tex(hipStream_t st, int W, int H, int n_views, const float* minv, int Ws, int Hs, const float* final_T,
                                       const float* dL_dout, float* g_tex);
// grad_rows [n_views][n][12] columns 0..5 += the gradient of sum_p final_T (sky_rgb . dL_dout) through final_T
hipError_t dvs_launch_sky_backward_rows(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, int n, const uint32_t* ranges /*canonical (start, end)*/,
                                        const uint32_t* sorted_splat, const float* splat2d, const float* final_T, const uint32_t* n_contrib,
                                        const float* dL_dout, const float* sky_rgb, float* grad_rows, int grad_mode);
// dvs_api.cpp — minv [9] <- the matrix of pixel_ray.h for `cam` (the inverse of rows 0, 1, 3 of proj's 3x3 part, fp64 then rounded);
// false for a singular proj. For sky.hip's entry points and region.hip's mask.
struct dvs_camera;
bool dvs_pixel_ray_matrix(const dvs_camera* cam, float* minv);
// A8 kernel variants (dvs_set_backward_variant): same inputs, same 48-B row contract, results equal to fp32 roundoff
enum { DVS_BWD_BLOCKS = 0 /*per-4x4-block lists, four cursors per wave, 12-value group reduction per step (round 2): kept in the release library as
       the independent-summation-order cross-check of the parity tests*/, DVS_BWD_REDUCE = 1 /*per-quadrant masks, wave-wide reduction tree per visit
       (round 1; retired, refused by the setter)*/, DVS_BWD_MM = 2 /*per-quadrant masks, sums contracted on the fp32 matrix pipe (retired, refused)*/,
       DVS_BWD_TR = 3 /*per-4x4-block lists; (v5, w) pairs transposed through LDS and accumulated serially per (block, slot, pixel row):
       render_tr.hip (default since round 3)*/ };

// render_tr.hip
hipError_t dvs_launch_render_bwd_tr(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges,
                                    const uint32_t* sorted_splat, const float* splat2d, const float* bgs /*[n_views][3]*/, const float* final_T,
                                    const uint32_t* n_contrib, const float* dL_dout, float* grad_rows, int absgrad, int grad_mode,
                                    const uint32_t* live_splat /*the forward's live lists (dvs_launch_render_fwd), or null: walk sorted_splat*/,
                                    const uint32_t* live_pos);

// render_blocks.hip
hipError_t dvs_launch_render_bwd_blocks(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges,
                                        const uint32_t* sorted_splat, const float* splat2d, const float* bgs /*[n_views][3]*/, const float* final_T,
                                        const uint32_t* n_contrib, const float* dL_dout, float* grad_rows, int absgrad, int grad_mode);

// pack.hip — stages (a) - (c) of the export packer for other users inside the library (knn.hip): the model's box, 30-bit Morton keys
// over it, the stable segmented sort. *sorted = [n] model indices in Morton order (equal keys in index order), *bounds (nullable) =
// {min xyz, max xyz}; both live inside `scratch` (dvs_morton_scratch_bytes(n) bytes, 256-byte aligned parts, no initialisation).
size_t dvs_morton_scratch_bytes(int n);
hipError_t dvs_launch_morton_order(hipStream_t st, int n, const float* pos, void* scratch, const uint32_t** sorted, const float** bounds);

// scan.hip — the exclusive scan, in place, of n > 0 words (reduce, one workgroup over the block sums, rescan): bsum =
// ceil(n / DVS_SCAN_TILE) words of scratch, *total (device) = the sum in 64 bits. And its middle step alone, for a caller that made the
// block sums itself: bsum [nb] -> exclusive offsets in place (32-bit words), *total = the sum in 64 bits; nb = 0 leaves *total = 0.
#define DVS_SCAN_TILE 2048
hipError_t dvs_launch_scan_u32(hipStream_t st, uint32_t* v, size_t n, uint32_t* bsum, unsigned long long* total);
// the INCLUSIVE scan, in place, of n > 0 64-bit words (sums wrap modulo 2^64, so int64 addends scan as themselves); bsum = ceil(n /
// DVS_SCAN_TILE) 64-bit words of scratch
hipError_t dvs_launch_scan_incl_u64(hipStream_t st, uint64_t* v, size_t n, uint64_t* bsum);
__attribute__((visibility("hidden"))) hipError_t dvs_launch_block_sums_excl(hipStream_t st, uint32_t* bsum, uint32_t nb, unsigned long long* total);
// cell_cluster.hip — elements grouped by the lattice cell they fall into (mesh_decimate.hip, lod.hip; device side: cell_cluster.h).
// dvs_cell_lattice fills *g; false for a null pointer, a cell that is not > 0 and finite, a dim outside 1 .. 1024 (the origin is the
// caller's to judge). dvs_cluster_layout carves the shared parts of a scratch for n > 0 elements from offset 0 (sort_ws sized for the
// largest sort the caller runs in it, sort_n elements if that is more than n); the caller's own parts follow from `end` (dvs_carve).
struct DvsCellLattice;
bool dvs_cell_lattice(const float origin[3], float cell, const int32_t dims[3], DvsCellLattice* g);
struct DvsClusterLayout { size_t sort_ws, key[2], val[2], cex, bsum, cstart, end; };
DvsClusterLayout dvs_cluster_layout(size_t n, size_t sort_n = 0);
// key[0] / val[0] hold (dvs_cell_key or DVS_CELL_NONE, i) for i < n: sorts them over `bits` key bits and leaves in key[0] / val[0] the
// sorted keys and indices (equal keys in index order, DVS_CELL_NONE last), in cstart[0 .. n_clusters] the first sorted position of every
// cluster and the end of the last, in *n_clusters_dev their number, in cluster_of [n] (nullable) the cluster of every element.
hipError_t dvs_launch_cell_clusters(hipStream_t st, uint32_t n, int bits, void* base, const DvsClusterLayout& L, uint32_t* cluster_of,
                                    unsigned long long* n_clusters_dev);
// mesh.hip — for mesh_clean.hip: the byte offsets, inside the scratch of dvs_mesh_extract_count, of vert_off [voxels] (uint32) and
// flags [voxels] (uint8); false for dims the extraction refuses.
bool dvs_mesh_scratch_parts(const int32_t dims[3], size_t* vert_off, size_t* flags);
