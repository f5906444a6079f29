// dvs_api.cpp — the C-ABI of libdvsraster.so (include/dvs_raster.h): context, HBM arenas, and the
// host-side orchestration of one forward / backward pass of the rasterizer on one MI355X.
//
// Replaces, behind a plain-C surface, what the reference's closed `gsplatrast` CUDA library does for
// `gstrain`'s train_step() (call sites application/diverseshot-cli/source/gs_train.cpp:156,
// application/editor/source/editor.cpp:1620).
//
// HBM layout (all arenas are ctx-owned, grow-only, sized for max_splats x max_views / max image at create; ensure_*_arenas):
//   per (view, splat): radii i32 | splat2d 64-B record (mean, conic, opacity, rgb, depth, radius) | depth f32 | flags u32 |
//                 tiles_touched u32 | tile rectangle 16 B x2 (as written, in depth order) | depth_key u32 x2 (ping-pong) |
//                 ids u32 x2 (ping-pong) | the 48-B gradient row of the backward                       = 176 B/splat
//   per instance: tile u32 x2 | splat u32 x2 (ping-pong)                                              = 16 B/instance
//   per tile    : range u32x2 (x2: as the tile sort encodes them, as k_render_fwd decodes them)   per pixel: final_T f32, n_contrib u32
//   backward    : one 48-B row per splat: moments S_x S_y S_xx S_xy S_yy of dL/dG*G about the mean (A9 turns them into
//                 dL/dmean2D and dL/dconic), dL/dopacity, dL/drgb x3, |dL/dmean2D| x2, pad
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/dvs_raster.h"
#include "../../include/dvs_train.h"
#include "dvs_kernels.h"

static thread_local std::string g_last_error;
static void set_error(const char* what, hipError_t e, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_last_error = buf;
}
void dvs_set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }      // shared with dvs_comm.cpp
// every refusal of this file: dvs_last_error() becomes "<who>: <what>", the status goes back to the caller
static int fail(int code, const char* who, const char* what) { g_last_error = std::string(who) + ": " + what; return code; }
#define HIPCHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { set_error(#expr, _e, __FILE__, __LINE__); return DVS_ERR_HIP; } } while (0)
#define TRY(expr) do { int _r = (expr); if (_r != DVS_OK) return _r; } while (0)       /* a failed step ends its caller with that status */

namespace {
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    ~Buf() { if (p) (void)hipFree(p); }                // (the owner has set the device: dvs_destroy)
    int ensure(size_t need) {
        if (need <= bytes) return DVS_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 4;                 // 25 % headroom so a growing scene does not realloc every step
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { e = hipMalloc(&p, need); want = need; }
        if (e != hipSuccess) { set_error("hipMalloc", e, __FILE__, __LINE__); p = nullptr; return DVS_ERR_HIP; }
        bytes = want;
        return DVS_OK;
    }
    template <class T> T* as() const { return (T*)p; }
};
// a cursor over one arena: take<T>(count) hands out the next block; over a null base it only measures
struct Carver {
    char* base; size_t off = 0;
    template <class T> T* take(size_t count) { T* p = base ? (T*)(base + off) : nullptr; off += count * sizeof(T); return p; }
};

// DvsCam (dvs_device.h) mirrors dvs_camera field by field, all of them 4-byte words
static_assert(sizeof(DvsCam) == sizeof(dvs_camera) && offsetof(DvsCam, campos) == offsetof(dvs_camera, campos) &&
              offsetof(DvsCam, bg) == offsetof(dvs_camera, bg), "DvsCam must mirror dvs_camera");
DvsCam to_dev_cam(const dvs_camera& c) { DvsCam d; memcpy(&d, &c, sizeof d); return d; }
DvsCams pack_cams(const dvs_camera* cams, int V) {
    DvsCams d;
    for (int v = 0; v < V; ++v) d.c[v] = to_dev_cam(cams[v]);
    return d;
}
// [V][3] of one vector of every camera: the backgrounds for the composite kernels, the positions for the SH row rebuild
struct CamVec3 {
    float v[DVS_MAX_VIEWS * 3];
    CamVec3(const dvs_camera* cams, int V, float (dvs_camera::*field)[3]) {
        for (int i = 0; i < V; ++i) for (int k = 0; k < 3; ++k) v[3 * i + k] = (cams[i].*field)[k];
    }
};
int bits_for(uint32_t max_value) { int b = 0; while (max_value) { ++b; max_value >>= 1; } return b; }

// the tile grid of an image and the tile-rectangle record format of a forward on it (DVS_TILES_TIGHT is opt-in: only the tiles the
// alpha >= 1/255 ellipse reaches, dvs_raster.h)
struct TileGrid {
    int tiles_x, tiles_y, tiles, rect_fmt;
    TileGrid(int W, int H, int tile_bounds = DVS_TILES_CANONICAL)
        : tiles_x((W + DVS_TILE - 1) / DVS_TILE), tiles_y((H + DVS_TILE - 1) / DVS_TILE), tiles(tiles_x * tiles_y),
          rect_fmt(tile_bounds == DVS_TILES_TIGHT ? DVS_FE_RECT_TIGHT : (tiles_x <= 255 && tiles_y <= 255) ? DVS_FE_RECT_U8 : DVS_FE_RECT_U16) {}
};

struct FwdPass {                               // what the phases of one forward hand to each other
    hipStream_t st;
    const dvs_splats* p; const dvs_camera* cams; int V; const dvs_opts* opts;
    int n; TileGrid g;
    uint64_t T = 0, T_expected = 0;
    const uint64_t* T_dev = nullptr;           // async: the kernels over instances read T on the device, grids sized for the capacity
    int icur = 0;
    int ranges_encoded = 0;                    // A6 fused into the tile sort's last pass: k_render_fwd decodes the ranges
    bool keys_written = true;                  // the sorted tile ids exist (an asynchronous forward with the fused A6 does not write them)
};

// ---- the context, by concern ----
struct Arenas {
    // per (view, splat)
    Buf radii, splat2d, depth, flags, tiles_touched, rect, rect_sorted, key[2], ids[2];
    // per image: `ranges` starts with the front end's zeroed words, the tile ranges follow (FrontEnd::carve_ranges): ONE memset per forward
    Buf ranges, final_T, n_contrib;
    Buf ranges_canon;                    // (start, end) per tile as k_render_fwd decodes them when A6 rides on the tile sort (frontend.hip)
    // per instance
    Buf inst_tile[2], inst_splat[2];
    uint64_t inst_cap = 0;               // instances the instance arenas can hold
    uint64_t inst_grow_events = 0;       // how often they have been enlarged since dvs_create (dvs_get_arena_info)
    uint64_t* total_dev = nullptr;       // [0] = T of the last forward, [1] = number of forwards whose T exceeded the instance capacity
    uint64_t* total_host = nullptr;      // pinned copy of both words (async: refreshed by every forward, read by the next one)
    uint64_t overflow_seen = 0;          // value of total_host[1] already reported
    Buf tmp_keys, tmp_vals;              // dvs_sort_pairs_u32: the other half of its ping-pong
};
// the binning front end (frontend.hip): every view is a segment of the sorts
struct FrontEnd {
    Buf state, hist;                     // `hist`: histogram table of the segmented sorts
    uint32_t nbv = 0, nsb = 0;           // A3 workgroups / super sums per view at max_splats
    int rank_atomic = 0;                 // the sorts' scatters rank by returning LDS adds (frontend.hip): the device passed dvs_fe_probe_rank_atomic
    // blocks of `state` (carve_state), then of Arenas::ranges (carve_ranges): its zeroed prefix of zero_bytes, the tile ranges behind it
    DvsSeg *seg_all = nullptr, *seg_vis = nullptr, *seg_tile = nullptr;
    uint32_t *superexcl = nullptr, *totals = nullptr, *block_sums = nullptr, *kred = nullptr, *tile_ranges = nullptr;
    unsigned long long* super = nullptr;
    size_t zero_bytes = 0;
    int seg_n = -1, seg_V = -1;          // what seg_all currently describes (ensure_segs; -1: nothing a forward can use)
    uint32_t seg_rows = 0;
    // The ONE description of each layout: the block pointers and the byte size (the return value) both come from this walk.
    size_t carve_state(void* base, int max_views) {
        Carver k{(char*)base};
        seg_all = k.take<DvsSeg>(DVS_MAX_VIEWS); seg_vis = k.take<DvsSeg>(DVS_MAX_VIEWS); seg_tile = k.take<DvsSeg>(DVS_MAX_VIEWS);
        superexcl = k.take<uint32_t>((size_t)max_views * nsb);
        totals = k.take<uint32_t>((size_t)max_views * DVS_FE_MAXBINS);
        block_sums = k.take<uint32_t>((size_t)max_views * nbv);
        return k.off;
    }
    size_t carve_ranges(void* base, int max_views, size_t tiles) {
        Carver k{(char*)base};
        kred = k.take<uint32_t>(DVS_FE_KRED_WORDS);                                      // key-range slots of A2
        super = k.take<unsigned long long>((size_t)max_views * nsb * DVS_FE_SUPER_STRIDE);   // super sums of A3
        zero_bytes = k.off = (k.off + 255) & ~(size_t)255;
        tile_ranges = k.take<uint32_t>(tiles * 2);
        return k.off;
    }
};
// What the context knows about the device arenas after the last forward. Who overwrites what, and so what invalidate() must drop:
//   entry point                                clobbers                                                      drops
//   forward_views                              every arena of A2..A7 (A2's only when not prepared)           FWD | ROWS, then PREP (used once)
//   dvs_raster_forward_views_prepare, chunk 0  A2's outputs, the zeroed prefix and the tile ranges           FWD | ROWS | PREP (then records anew)
//   dvs_sort_pairs_u32                         seg_all, hist, totals                                         SEGS
//   dvs_debug_sort_depth_keys                  key[], ids[], kred (A2 outputs), seg_all / seg_vis, hist      FWD | PREP | SEGS
//   dvs_raster_forward_cancel_prepared         nothing                                                       PREP
struct Forward {
    dvs_fwd_state st{};
    int n_views = 1;                     // views of the last forward
    bool have = false;
    uint32_t* live_splat = nullptr;      // A7's compacted per-tile lists of the last forward (in the sort's spare instance arrays), or null
    uint32_t* live_pos = nullptr;
    bool live_lists = true;              // env DVS_LIVE_LISTS=0: A8 walks the full lists (A/B and parity of the two routes)
    uint64_t* rec_masks = nullptr; uint64_t rec_cap = 0;      // dvs_debug_record_decisions
    // dvs_raster_forward_views_prepare: A2 of the NEXT forward already ran for the splats [0, next) with exactly these inputs
    struct Prep {
        bool valid = false;
        int64_t next = 0;
        int n = 0, V = 0;
        dvs_splats p{};
        dvs_opts opts{};
        dvs_camera cams[DVS_MAX_VIEWS];
    } prep;
};
struct Backward {
    Buf g_rows;
    Buf dcolor;                          // [views, n, 3] per-view colour gradients of a batched A9 when the caller gives no buffer
    Buf sky_rgb;                         // [views, 3, H, W] the sky lookup of dvs_sky_backward_views when the caller gives none
    int variant = DVS_BWD_TR;            // which A8 kernel (dvs_set_backward_variant; env DVS_BWD_VARIANT at create): the measured winner
    bool keep_rows = false;              // parity tests: leave the A8 rows in place after the backward
    bool rows_clean = false;             // gradient rows are all-zero (k_preprocess_bwd re-zeroes what it reads)
    bool rows_pending = false;           // dvs_raster_backward_composite ran, dvs_raster_backward_project has not yet
    int64_t proj_next = 0;               // dvs_raster_backward_project_chunk: the next splat a chunk must start at
};
// every stage, synchronising per call (profiling iterations)
struct Timing {
    struct Span { const char* name; size_t begin, end; };                 // (event indices)
    bool on = false;
    std::vector<hipEvent_t> events;
    size_t used = 0;
    std::vector<Span> spans;
    std::vector<const char*> out_names;
    std::vector<float> out_ms;
};
// hipEvent pairs around the composite kernels only, never synchronising — they are read back once, so the kernels are timed under the
// concurrency of the real (pipelined) step
struct Probe {
    bool on = false;
    std::vector<hipEvent_t> ev;          // pairs: [2k] before, [2k+1] after
    std::vector<int> kind;               // per pair: 0 = k_render_fwd, 1 = k_render_bwd
    size_t used = 0;
};
}  // namespace

struct dvs_ctx {
    int device = 0;
    size_t max_splats = 0;
    int max_w = 0, max_h = 0;
    int max_views = 1;                   // views one forward can batch (dvs_create_views)
    bool async_T = false;                // dvs_set_async: no host synchronisation inside dvs_raster_forward
    bool export_tiles = false;           // dvs_set_export_sorted_tiles: asynchronous forwards materialise the sorted tile ids too
    Arenas a;
    FrontEnd fe;
    Forward fwd;
    Backward bwd;
    Timing timing;
    Probe probe;
    ~dvs_ctx() {                         // (dvs_destroy has set the device; the Bufs free themselves)
        if (a.total_dev) (void)hipFree(a.total_dev);
        if (a.total_host) (void)hipHostFree(a.total_host);
        for (const auto* pool : {&timing.events, &probe.ev}) for (hipEvent_t e : *pool) (void)hipEventDestroy(e);
    }
};

namespace {
enum : unsigned { DROP_FWD = 1u, DROP_ROWS = 2u, DROP_PREP = 4u, DROP_SEGS = 8u };
// the one place that forgets what is no longer true of the arenas (table at struct Forward)
void invalidate(dvs_ctx* c, unsigned what) {
    if (what & DROP_FWD) c->fwd.have = false;
    if (what & DROP_ROWS) c->bwd.rows_pending = false;
    if (what & DROP_PREP) c->fwd.prep.valid = false;
    if (what & DROP_SEGS) c->fe.seg_n = -1;
}

// The stage timing of one entry point: entering resets the span list, begin() / stage(name) bracket the stages, finish() is the one
// place that synchronises and collects (append: the rows of a backward follow the forward's in dvs_get_stage_timing).
struct StageScope {
    dvs_ctx* c; hipStream_t st; bool append; size_t last = 0;
    StageScope(dvs_ctx* c_, hipStream_t s, bool append_) : c(c_), st(s), append(append_) { c->timing.used = 0; c->timing.spans.clear(); }
    size_t mark() {
        Timing& t = c->timing;
        if (!t.on) return 0;
        if (t.used == t.events.size()) { hipEvent_t e; (void)hipEventCreate(&e); t.events.push_back(e); }
        (void)hipEventRecord(t.events[t.used], st);
        return t.used++;
    }
    void begin() { last = mark(); }
    void stage(const char* name) { const size_t e = mark(); if (c->timing.on) c->timing.spans.push_back({name, last, e}); last = e; }
    int finish() {
        Timing& t = c->timing;
        if (!t.on) return DVS_OK;
        HIPCHECK(hipStreamSynchronize(st));
        if (!append) { t.out_names.clear(); t.out_ms.clear(); }
        for (const Timing::Span& s : t.spans) {
            float ms = 0.f;
            (void)hipEventSynchronize(t.events[s.end]);
            (void)hipEventElapsedTime(&ms, t.events[s.begin], t.events[s.end]);
            t.out_names.push_back(s.name); t.out_ms.push_back(ms);
        }
        return DVS_OK;
    }
};
// one event of the kernel probe; `opens` >= 0: the first of a pair, around a kernel of that kind
void probe_event(dvs_ctx* c, hipStream_t st, int opens = -1) {
    Probe& pr = c->probe;
    if (!pr.on) return;
    if (pr.used == pr.ev.size()) { hipEvent_t e; (void)hipEventCreate(&e); pr.ev.push_back(e); }
    (void)hipEventRecord(pr.ev[pr.used++], st);
    if (opens >= 0) pr.kind.push_back(opens);
}

bool fe_no_key16() { static const bool v = [] { const char* e = getenv("DVS_FE_NO_KEY16"); return e && e[0] == '1'; }(); return v; }      // cross-check switch (tests): 32-bit tile ids
bool fe_no_fuse() { static const bool v = [] { const char* e = getenv("DVS_FE_NO_FUSE_A6"); return e && e[0] == '1'; }(); return v; }      // cross-check switch (tests): A6 as its own kernel

int ensure_frontend_arenas(dvs_ctx* c) {
    FrontEnd& fe = c->fe;
    dvs_fe_block_counts((int)c->max_splats, &fe.nbv, &fe.nsb);
    TRY(fe.state.ensure(fe.carve_state(nullptr, c->max_views)));
    fe.carve_state(fe.state.p, c->max_views);
    return fe.hist.ensure(dvs_fe_hist_words((uint64_t)c->max_splats * c->max_views, c->max_views, DVS_FE_MAXBINS) * 4);
}
int ensure_splat_arenas(dvs_ctx* c, size_t n) {
    Arenas& a = c->a;
    // bytes per (view, splat); rect: 8 B canonically, 16 B with DVS_TILES_TIGHT (rectangle + tile mask)
    const struct { Buf* buf; size_t each; } need[] = {{&a.radii, 4}, {&a.splat2d, 64}, {&a.depth, 4}, {&a.flags, 4}, {&a.tiles_touched, 4},
        {&a.rect, 16}, {&a.rect_sorted, 16}, {&a.key[0], 4}, {&a.key[1], 4}, {&a.ids[0], 4}, {&a.ids[1], 4}, {&c->bwd.g_rows, 48}};
    for (const auto& x : need) TRY(x.buf->ensure(n * x.each));
    return DVS_OK;
}
int ensure_image_arenas(dvs_ctx* c, int w, int h, int views) {
    const size_t P = (size_t)w * h * views;
    const size_t tiles = (size_t)TileGrid(w, h).tiles * views;
    TRY(c->a.ranges.ensure(c->fe.carve_ranges(nullptr, c->max_views, tiles)));
    c->fe.carve_ranges(c->a.ranges.p, c->max_views, tiles);
    TRY(c->a.ranges_canon.ensure(tiles * 8));
    TRY(c->a.final_T.ensure(P * 4));
    return c->a.n_contrib.ensure(P * 4);
}
int ensure_instance_arenas(dvs_ctx* c, uint64_t T) {
    Arenas& a = c->a;
    if (a.inst_cap && T > a.inst_cap) ++a.inst_grow_events;
    uint64_t cap = (1ull << 32) - 1;                                     // instance offsets are 32-bit
    for (Buf* b : {&a.inst_tile[0], &a.inst_splat[0], &a.inst_tile[1], &a.inst_splat[1]}) {
        TRY(b->ensure(T * 4));
        if (b->bytes / 4 < cap) cap = b->bytes / 4;
    }
    a.inst_cap = cap;
    return c->fe.hist.ensure(dvs_fe_hist_words(a.inst_cap, c->max_views, 512) * 4);
}
}  // namespace

extern "C" {

const char* dvs_last_error(void) { return g_last_error.c_str(); }
const char* dvs_version(void) { return "divshot_amd raster 0.1 (gfx950)"; }

dvs_ctx* dvs_create_views(int device, size_t max_splats, int max_w, int max_h, int max_views) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device < 0 || device >= count) { fail(0, "dvs_create", "no such HIP device (the rasterizer has no CPU fallback)"); return nullptr; }
    if (max_views < 1 || max_views > DVS_MAX_VIEWS) { fail(0, "dvs_create_views", "max_views must be in [1, 16]"); return nullptr; }
    if ((e = hipSetDevice(device)) != hipSuccess) { set_error("hipSetDevice", e, __FILE__, __LINE__); return nullptr; }
    dvs_ctx* c = new dvs_ctx();
    c->device = device; c->max_splats = max_splats; c->max_w = max_w; c->max_h = max_h; c->max_views = max_views;
    // (A/B runs; a request for one of the retired kernels, 1 or 2, falls back to the default)
    if (const char* v = getenv("DVS_BWD_VARIANT")) c->bwd.variant = v[0] == '0' ? DVS_BWD_BLOCKS : DVS_BWD_TR;
    if (const char* v = getenv("DVS_LIVE_LISTS")) c->fwd.live_lists = v[0] != '0';
    if (hipMalloc((void**)&c->a.total_dev, 32) != hipSuccess || hipHostMalloc((void**)&c->a.total_host, 32, hipHostMallocDefault) != hipSuccess ||
        hipMemset(c->a.total_dev, 0, 32) != hipSuccess) {
        fail(0, "dvs_create", "hipMalloc failed");
        delete c;
        return nullptr;
    }
    c->a.total_host[0] = c->a.total_host[1] = c->a.total_host[2] = c->a.total_host[3] = 0;   // [0] T  [1] arena overflows
    {   // how the sorts' scatters rank inside a wave (frontend.hip): returning LDS adds, if this device serves the lanes of one address in
        // lane order — probed once per process and device, on the device; DVS_FE_RANK=ballot keeps the multisplit of rounds 2-5
        static int probed[64];                    // 0 unknown, 1 lane-ordered, 2 not
        static std::mutex probe_mutex;            // (hosts create scenes from worker threads: editor.cpp:2030)
        std::lock_guard<std::mutex> probe_lock(probe_mutex);
        const char* mode = getenv("DVS_FE_RANK");
        if (mode && mode[0] == 'b') c->fe.rank_atomic = 0;
        else {
            if (device < 64 && probed[device] == 0) {
                uint32_t bad = 1u;
                uint32_t* word = nullptr;
                if (hipMalloc((void**)&word, 4) == hipSuccess && hipMemset(word, 0, 4) == hipSuccess && dvs_fe_probe_rank_atomic(nullptr, word) == hipSuccess &&
                    hipMemcpy(&bad, word, 4, hipMemcpyDeviceToHost) == hipSuccess)
                    probed[device] = bad == 0u ? 1 : 2;
                if (word) (void)hipFree(word);
            }
            c->fe.rank_atomic = (device < 64 && probed[device] == 1) ? 1 : 0;
        }
    }
    if (const char* v = getenv("DVS_ASYNC")) c->async_T = v[0] == '1';
    if (ensure_frontend_arenas(c) != DVS_OK ||
        ensure_splat_arenas(c, max_splats * (size_t)max_views) != DVS_OK || ensure_image_arenas(c, max_w, max_h, max_views) != DVS_OK ||
        ensure_instance_arenas(c, (uint64_t)max_splats * 4 * (uint64_t)max_views) != DVS_OK) {
        dvs_destroy(c);
        return nullptr;
    }
    return c;
}
dvs_ctx* dvs_create(int device, size_t max_splats, int max_w, int max_h) { return dvs_create_views(device, max_splats, max_w, max_h, 1); }

void dvs_destroy(dvs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// A2 for the splats [first, first + count) of all views (begin: the front end's zeroed state first — the key-range slots and super sums of
// frontend.hip and the tile ranges behind them, ONE memset)
static int run_a2(dvs_ctx* c, hipStream_t st, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts, int64_t first, int64_t count, bool begin) {
    const TileGrid g(cams[0].width, cams[0].height, opts->tile_bounds);
    Arenas& a = c->a;
    if (begin) HIPCHECK(hipMemsetAsync(a.ranges.p, 0, c->fe.zero_bytes + (size_t)g.tiles * V * 8, st));
    HIPCHECK(dvs_launch_preprocess_fwd(st, p->n, p->pos, p->sh0, p->shN, p->opacity, p->scale, p->rot, pack_cams(cams, V), V, opts->sh_degree,
                                       opts->antialias, g.tiles_x, g.tiles_y, a.radii.as<int>(), a.splat2d.as<float>(),
                                       a.depth.as<float>(), a.flags.as<uint32_t>(), a.tiles_touched.as<uint32_t>(), a.key[0].as<uint32_t>(),
                                       opts->shn_layout, a.rect.as<uint32_t>(), g.rect_fmt, c->fe.kred, (int)first, (int)count));
    return DVS_OK;
}
static bool prep_matches(const dvs_ctx* c, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts) {
    const Forward::Prep& q = c->fwd.prep;
    return q.valid && q.n == p->n && q.V == V && memcmp(&q.p, p, sizeof *p) == 0 && memcmp(&q.opts, opts, sizeof *opts) == 0 &&
           memcmp(q.cams, cams, sizeof(dvs_camera) * (size_t)V) == 0;
}
// records that A2 of the next forward has run for the splats [0, next) of these inputs (the only place that sets Prep::valid)
static void publish_prep(dvs_ctx* c, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts, int64_t next) {
    Forward::Prep& q = c->fwd.prep;
    q.valid = true; q.next = next; q.n = p->n; q.V = V; q.p = *p; q.opts = *opts;
    memcpy(q.cams, cams, sizeof(dvs_camera) * (size_t)V);
}
// the segment descriptors of the depth sort: written when seg_all describes something else
static int ensure_segs(dvs_ctx* c, hipStream_t st, int n, int V, uint32_t rows) {
    FrontEnd& fe = c->fe;
    if (fe.seg_n == n && fe.seg_V == V && fe.seg_rows == rows) return DVS_OK;
    HIPCHECK(dvs_launch_seg_init(st, n, V, rows, fe.seg_all));
    fe.seg_n = n; fe.seg_V = V; fe.seg_rows = rows;
    return DVS_OK;
}

// ---- the forward: A2..A7 for the n_views views of a batch (n_views = 1: the single-view API). Per-splat arrays are view-major
// [view][splat]; the sort value of an element is its global index view * n + splat; tile ids are view * tiles + tile: ONE depth sort,
// ONE scan, ONE duplication, ONE tile sort and ONE composite launch cover the whole iteration. ----

// Phase 1, asynchronous contexts only. No host synchronisation: the arenas are over-allocated, T stays on the device. What the host
// knows is the T of EARLIER forwards on this context (pinned copy, refreshed asynchronously): it grows the arenas ahead of need and
// reports an overflow (T beyond the capacity: that view's outputs are invalid, nothing was written out of bounds) as DVS_ERR_CAPACITY, once.
static int fwd_capacity_policy(dvs_ctx* c, FwdPass& f) {
    if (!c->async_T) return DVS_OK;
    Arenas& a = c->a;
    const uint64_t lastT = a.total_host[0], overflow = a.total_host[1];
    const bool overflowed = overflow != a.overflow_seen;
    if (overflowed || lastT + lastT / 8 > a.inst_cap) {      // or getting close: grow before it can overflow (rare; needs the stream idle)
        a.overflow_seen = overflow;
        HIPCHECK(hipStreamSynchronize(f.st));
        TRY(ensure_instance_arenas(c, lastT + lastT / 2));
        if (overflowed)
            return fail(DVS_ERR_CAPACITY, "dvs_raster_forward (async)", "an earlier forward on this context produced more tile instances than the "
                        "instance arena held; its outputs are invalid. The arena has been enlarged — repeat that view.");
    }
    f.T = a.inst_cap;
    f.T_dev = a.total_dev;
    f.T_expected = lastT > 0 ? lastT + lastT / 16 + 4096 : 0;      // grid size only: the kernels stride over whatever T turns out to be
    return DVS_OK;
}
// Phase 2: A2 — unless dvs_raster_forward_views_prepare already ran it, chunk by chunk, for exactly these inputs (a data-parallel step
// projects the next iteration's splats behind the optimizer's chunks while the gradient exchange is still on the links)
static int fwd_project(dvs_ctx* c, const FwdPass& f, StageScope& tm) {
    const bool prepared = prep_matches(c, f.p, f.cams, f.V, f.opts) && c->fwd.prep.next == (int64_t)f.n;
    invalidate(c, DROP_PREP);                  // a preparation is used once
    tm.begin();
    if (!prepared) TRY(run_a2(c, f.st, f.p, f.cams, f.V, f.opts, 0, f.n, true));
    tm.stage("preprocess_fwd");
    return DVS_OK;
}
// A3 (stage 0) and A4 (stage 1) are one launcher over the same arrays: they differ in the stage, the capacity and A4's three outputs
static hipError_t seg_binning(dvs_ctx* c, const FwdPass& f, uint32_t tile_part, unsigned long long capacity, int stage,
                              uint32_t* inst_tile = nullptr, uint32_t* inst_splat = nullptr, int key16 = 0) {
    Arenas& a = c->a; FrontEnd& fe = c->fe;
    return dvs_launch_seg_binning(f.st, f.n, f.V, f.g.rect_fmt, fe.seg_vis, fe.seg_tile, a.ids[1].as<uint32_t>(), a.rect.as<uint32_t>(),
                                  a.rect_sorted.as<uint32_t>(), fe.block_sums, fe.super, fe.superexcl, tile_part,
                                  (unsigned long long*)a.total_dev, capacity, stage, f.g.tiles_x, inst_tile, inst_splat, key16);
}
// Phase 3: the segmented front end (frontend.hip) A5 -> A3 -> (sync T) -> A4 -> A5 tile -> A6: every view is a segment of the sorts,
// workgroup b works for view b % V
static int fwd_bin(dvs_ctx* c, FwdPass& f, StageScope& tm) {
    Arenas& a = c->a; FrontEnd& fe = c->fe;
    hipStream_t st = f.st;
    const int n = f.n, V = f.V, tiles = f.g.tiles;
    if (n > 0) {
        // A5 (low 32 key bits): three range-adaptive passes per view; the culled splats leave in the first
        TRY(ensure_segs(c, st, n, V, dvs_depth_sort_rows_per_view(n, V)));
        HIPCHECK(dvs_launch_depth_sort(st, n, V, a.key[0].as<uint32_t>(), a.ids[0].as<uint32_t>(), a.key[1].as<uint32_t>(), a.ids[1].as<uint32_t>(),
                                       fe.seg_all, fe.seg_vis, fe.kred, fe.hist.as<uint32_t>(), fe.totals, fe.rank_atomic));
    }
    tm.stage("depth_sort");
    // A3: tile counts in depth order (the one random gather: the tile rectangles), the views' instance ranges; T stays on the device
    const uint64_t lastT = a.total_host[0];
    const uint64_t t_hint = f.T_expected ? f.T_expected : (lastT ? lastT : (uint64_t)n * V * 3);
    const uint32_t tile_part = dvs_fe_part_for(t_hint);
    if (n > 0) HIPCHECK(seg_binning(c, f, tile_part, c->async_T ? a.inst_cap : ~0ull, 0));
    else HIPCHECK(hipMemsetAsync(a.total_dev, 0, 8, st));
    HIPCHECK(hipMemcpyAsync(a.total_host, a.total_dev, 32, hipMemcpyDeviceToHost, st));
    tm.stage("tile_scan");
    if (!c->async_T) {
        HIPCHECK(hipStreamSynchronize(st));
        f.T = a.total_host[0];
        if (f.T >= (1ull << 32)) return fail(DVS_ERR_CAPACITY, "dvs_raster_forward", "more than 2^32 tile instances");
        TRY(ensure_instance_arenas(c, f.T ? f.T : 1));
    }
    // A4 duplicate, view by view. Tile ids inside a view fit 16 bits up to 65 536 tiles (4096 x 4096 pixels): A4, the first
    // histogram and the first tile pass then move 2 B per instance for them instead of 4.
    const int key16 = (tiles <= 65536 && !fe_no_key16()) ? 1 : 0;
    tm.begin();
    if (n > 0) HIPCHECK(seg_binning(c, f, tile_part, a.inst_cap, 1, a.inst_tile[0].as<uint32_t>(), a.inst_splat[0].as<uint32_t>(), key16));
    tm.stage("duplicate");
    // A5 (high key bits): every view's instances by tile id; the last pass hands out view * tiles + tile
    // A6 rides on the last pass (a range boundary is where the scattered tile id changes): k_render_fwd decodes the ranges
    // (DVS_FE_NO_FUSE_A6=1: A6 as its own kernel, a cross-check). An asynchronous forward does not even write the sorted tile ids: nothing on the device reads them, and
    // dvs_fwd_state.sorted_tile is then NULL (dvs_raster.h).
    const bool fuse_a6 = !fe_no_fuse();
    f.keys_written = !(fuse_a6 && c->async_T) || c->export_tiles;
    if (n > 0) {
        const uint64_t cap = c->async_T ? a.inst_cap : f.T;
        const uint32_t nbtot = (uint32_t)(cap / tile_part) + (uint32_t)V + 2u;
        HIPCHECK(dvs_launch_seg_sort(st, V, a.inst_tile[0].as<uint32_t>(), a.inst_splat[0].as<uint32_t>(), a.inst_tile[1].as<uint32_t>(),
                                     a.inst_splat[1].as<uint32_t>(), fe.seg_tile, 0, tiles > 1 ? bits_for((uint32_t)(tiles - 1)) : 1,
                                     c->async_T ? (f.T_expected ? f.T_expected : a.inst_cap) : f.T, tile_part, nbtot, fe.hist.as<uint32_t>(), fe.totals,
                                     (uint32_t)tiles, &f.icur, fuse_a6 ? fe.tile_ranges : nullptr, f.keys_written ? 1 : 0, key16, fe.rank_atomic));
    }
    tm.stage("tile_sort");
    if (fuse_a6) f.ranges_encoded = n > 0 ? 1 : 0;
    else HIPCHECK(dvs_launch_tile_ranges(st, f.T, a.inst_tile[f.icur].as<uint32_t>(), fe.tile_ranges, f.T_dev, f.T_expected));     // (cleared by A2's memset)
    tm.stage("tile_ranges");
    return DVS_OK;
}
// Phase 4: A7 composite, then the forward record of the context (the only place that sets Forward::have)
static int fwd_composite_and_publish(dvs_ctx* c, const FwdPass& f, float* out_rgb, dvs_fwd_state* saved, uint64_t* num_rendered, StageScope& tm) {
    Arenas& a = c->a; Forward& fw = c->fwd;
    const int W = f.cams[0].width, H = f.cams[0].height, icur = f.icur;
    probe_event(c, f.st, 0);
    // the live lists of A7 (entries that reach their tile, compacted) go into the sort's other pair of instance arrays, free by now
    fw.live_splat = nullptr; fw.live_pos = nullptr;
    uint64_t* rec_masks = nullptr; uint64_t rec_cap = 0;          // dvs_debug_record_decisions (parity tests): one view, synchronous T
    if (fw.rec_masks && f.V == 1 && !c->async_T) {
        rec_masks = fw.rec_masks; rec_cap = fw.rec_cap;
        HIPCHECK(hipMemsetAsync(rec_masks, 0, (size_t)(f.T < rec_cap ? f.T : rec_cap) * 32, f.st));
    }
    // Only the "tr" composite backward walks them (the other variant ignores them), and they cost the forward two 4-B stores per
    // instance: none for an inference-only context (dvs_set_live_lists(ctx, 0)) or the other backward. The spare pair of the tile
    // sort's ping-pong buffers is RESERVED for them until the next forward on this context: nothing after the sort may reuse
    // inst_*[icur ^ 1].
    if (fw.live_lists && c->bwd.variant == DVS_BWD_TR) { fw.live_splat = a.inst_splat[icur ^ 1].as<uint32_t>(); fw.live_pos = a.inst_tile[icur ^ 1].as<uint32_t>(); }
    uint32_t* const canon = f.ranges_encoded ? a.ranges_canon.as<uint32_t>() : nullptr;
    HIPCHECK(dvs_launch_render_fwd(f.st, W, H, f.g.tiles_x, f.g.tiles_y, f.V, c->fe.tile_ranges, a.inst_splat[icur].as<uint32_t>(),
                                   a.splat2d.as<float>(), CamVec3(f.cams, f.V, &dvs_camera::bg).v, out_rgb, a.final_T.as<float>(),
                                   a.n_contrib.as<uint32_t>(), fw.live_splat, fw.live_pos, rec_masks, rec_cap, canon));
    probe_event(c, f.st);
    tm.stage("render_fwd");

    dvs_fwd_state& s = fw.st;
    s.radii = a.radii.as<int32_t>(); s.splat2d = a.splat2d.as<float>(); s.depth = a.depth.as<float>();
    s.flags = a.flags.as<uint32_t>();
    s.tiles_touched = a.tiles_touched.as<uint32_t>();
    s.sorted_tile = f.keys_written ? a.inst_tile[icur].as<uint32_t>() : nullptr; s.sorted_splat = a.inst_splat[icur].as<uint32_t>();
    s.ranges = canon ? canon : c->fe.tile_ranges; s.final_T = a.final_T.as<float>(); s.n_contrib = a.n_contrib.as<uint32_t>();
    s.num_rendered = c->async_T ? DVS_T_UNKNOWN : f.T; s.n = f.n; s.width = W; s.height = H; s.tiles_x = f.g.tiles_x; s.tiles_y = f.g.tiles_y;
    s._pad = 0;
    fw.n_views = f.V;
    fw.have = true;
    if (saved) *saved = s;
    if (num_rendered) *num_rendered = s.num_rendered;
    return DVS_OK;
}
static int check_fwd_args(dvs_ctx* c, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts, const float* out_rgb) {
    const char* const who = "dvs_raster_forward";
    if (!c || !p || !cams || !opts || !out_rgb) return fail(DVS_ERR_INVALID, who, "null argument");
    if (V < 1 || V > c->max_views) return fail(DVS_ERR_CAPACITY, who, "n_views exceeds the max_views given to dvs_create_views");
    const dvs_camera* cam = &cams[0];
    if (p->n < 0 || cam->width <= 0 || cam->height <= 0 || opts->sh_degree < 0 || opts->sh_degree > 3 ||
        (opts->shn_layout != DVS_SHN_ROWS && opts->shn_layout != DVS_SHN_TILED) ||
        (opts->tile_bounds != DVS_TILES_CANONICAL && opts->tile_bounds != DVS_TILES_TIGHT))
        return fail(DVS_ERR_INVALID, who, "bad n / image size / sh_degree / shn_layout / tile_bounds");
    for (int v = 1; v < V; ++v)
        if (cams[v].width != cam->width || cams[v].height != cam->height) return fail(DVS_ERR_INVALID, who, "the views of a batch must share one image size");
    if (p->n > 0 && (((uintptr_t)p->pos | (uintptr_t)p->sh0 | (uintptr_t)p->shN | (uintptr_t)p->opacity | (uintptr_t)p->scale | (uintptr_t)p->rot) & 15u))
        return fail(DVS_ERR_INVALID, who, "parameter arrays must be 16-byte aligned");
    if ((size_t)p->n > c->max_splats || cam->width > c->max_w || cam->height > c->max_h)
        return fail(DVS_ERR_CAPACITY, who, "exceeds the capacity given to dvs_create");
    // (the scan / duplication launchers and kernels index the (view, splat) elements with int)
    if ((uint64_t)p->n * (uint64_t)V >= (1ull << 31)) return fail(DVS_ERR_CAPACITY, who, "n * n_views must stay below 2^31");
    return DVS_OK;
}
static int forward_views(dvs_ctx* c, hipStream_t st, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts,
                         float* out_rgb, dvs_fwd_state* saved, uint64_t* num_rendered) {
    TRY(check_fwd_args(c, p, cams, V, opts, out_rgb));
    HIPCHECK(hipSetDevice(c->device));
    FwdPass f{st, p, cams, V, opts, p->n, TileGrid(cams[0].width, cams[0].height, opts->tile_bounds)};
    invalidate(c, DROP_FWD | DROP_ROWS);
    StageScope tm(c, st, /*append=*/false);
    TRY(fwd_capacity_policy(c, f));
    TRY(fwd_project(c, f, tm));
    TRY(fwd_bin(c, f, tm));
    TRY(fwd_composite_and_publish(c, f, out_rgb, saved, num_rendered, tm));
    return tm.finish();
}

int dvs_raster_forward(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cam, const dvs_opts* opts,
                       float* out_rgb, dvs_fwd_state* saved, uint64_t* num_rendered) {
    return forward_views(c, (hipStream_t)stream, p, cam, 1, opts, out_rgb, saved, num_rendered);
}

int dvs_raster_forward_views(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cams, int n_views, const dvs_opts* opts,
                             float* out_rgb) {
    return forward_views(c, (hipStream_t)stream, p, cams, n_views, opts, out_rgb, nullptr, nullptr);
}

int dvs_raster_forward_cancel_prepared(dvs_ctx* c) {
    if (!c) return fail(DVS_ERR_INVALID, "dvs_raster_forward_cancel_prepared", "null context");
    invalidate(c, DROP_PREP);
    return DVS_OK;
}
int dvs_raster_forward_views_prepare(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cams, int n_views, const dvs_opts* opts,
                                     int64_t first, int64_t count) {
    const char* const who = "dvs_raster_forward_views_prepare";
    static float dummy_rgb;                                       // (the argument check wants a non-null image pointer)
    TRY(check_fwd_args(c, p, cams, n_views, opts, &dummy_rgb));
    if (opts->shn_layout != DVS_SHN_TILED) return fail(DVS_ERR_INVALID, who, "needs the DVS_SHN_TILED layout");
    const bool begin = first == 0;
    if (!begin && !(prep_matches(c, p, cams, n_views, opts) && c->fwd.prep.next == first)) {
        invalidate(c, DROP_PREP);
        return fail(DVS_ERR_STATE, who, "chunks must cover [0, n) in ascending order with the same parameters, cameras and options");
    }
    if (count <= 0 || first < 0 || first + count > p->n || (first % 256) != 0) {
        invalidate(c, DROP_PREP);
        return fail(DVS_ERR_INVALID, who, "bad chunk (each starts at a multiple of 256 and lies inside [0, n))");
    }
    HIPCHECK(hipSetDevice(c->device));
    // the state of the previous forward is overwritten from here on: its backward must have been queued already (no backward after this)
    if (begin) invalidate(c, DROP_FWD | DROP_ROWS | DROP_PREP);
    const int r = run_a2(c, (hipStream_t)stream, p, cams, n_views, opts, first, count, begin);
    if (r != DVS_OK) { invalidate(c, DROP_PREP); return r; }
    publish_prep(c, p, cams, n_views, opts, first + count);
    return DVS_OK;
}

int dvs_get_view_state(dvs_ctx* c, int view, dvs_fwd_state* out) {
    if (!c || !out) return fail(DVS_ERR_INVALID, "dvs_get_view_state", "null argument");
    if (!c->fwd.have || view < 0 || view >= c->fwd.n_views) return fail(DVS_ERR_STATE, "dvs_get_view_state", "no such view in the last forward");
    dvs_fwd_state s = c->fwd.st;
    const size_t on = (size_t)view * s.n, op = (size_t)view * s.width * s.height, ot = (size_t)view * s.tiles_x * s.tiles_y;
    s.radii += on; s.splat2d += on * DVS_S2D_FLOATS; s.depth += on; s.flags += on; s.tiles_touched += on;
    s.ranges += 2 * ot; s.final_T += op; s.n_contrib += op;
    *out = s;              // sorted_tile / sorted_splat stay the batch-wide lists: ranges index into them, values are view * n + splat
    return DVS_OK;
}

// What every pass over the saved lists (depth, importance, sky) checks first: the context holds a forward, of n_views views unless n_views < 0
static int need_forward(const dvs_ctx* c, const char* who, int n_views = -1) {
    if (c->fwd.have && (n_views < 0 || n_views == c->fwd.n_views)) return DVS_OK;
    return fail(DVS_ERR_STATE, who, n_views < 0 ? "no forward on this context (valid after dvs_raster_forward / _views until the next forward)"
                                                : "no matching forward on this context (valid after dvs_raster_forward / _views until the next forward)");
}

// Depth and alpha maps of the last forward: a forward-only pass over the saved lists (depth.hip); reads the state, changes none of it
int dvs_raster_depth_views(dvs_ctx* c, void* stream, const dvs_opts* opts, float* out_depth, float* out_alpha) {
    const char* const who = "dvs_raster_depth_views";
    if (!c || !opts || !out_depth || !out_alpha) return fail(DVS_ERR_INVALID, who, "null argument");
    TRY(need_forward(c, who));
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    HIPCHECK(dvs_launch_depth_views((hipStream_t)stream, s.width, s.height, s.tiles_x, s.tiles_y, c->fwd.n_views, s.ranges, s.sorted_splat, s.splat2d,
                                    s.n_contrib, out_depth, out_alpha));
    return DVS_OK;
}

// Per-splat blend weights of the last forward: a forward-only pass over the saved lists (importance.hip); reads the state, changes none of it
int dvs_raster_importance_views(dvs_ctx* c, void* stream, const dvs_opts* opts, const float* const* masks, uint64_t* score_sum, uint32_t* score_max,
                                uint32_t* hits) {
    const char* const who = "dvs_raster_importance_views";
    if (!c || !opts || !score_sum) return fail(DVS_ERR_INVALID, who, "null argument");
    if (((uintptr_t)score_sum | (uintptr_t)score_max | (uintptr_t)hits) & 15u) return fail(DVS_ERR_INVALID, who, "score arrays must be 16-byte aligned");
    TRY(need_forward(c, who));
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    HIPCHECK(dvs_launch_importance_views((hipStream_t)stream, s.width, s.height, s.tiles_x, s.tiles_y, c->fwd.n_views, s.n, s.ranges, s.sorted_splat,
                                         s.splat2d, s.n_contrib, masks, score_sum, score_max, hits));
    return DVS_OK;
}

// Where those blend weights landed, on foreground or on background pixels (foreground.hip); reads the state, changes none of it
int dvs_raster_foreground_views(dvs_ctx* c, void* stream, const dvs_opts* opts, const float* const* fg_masks, const float* const* valid_masks,
                                uint64_t* fg_sum, uint64_t* bg_sum) {
    const char* const who = "dvs_raster_foreground_views";
    if (!c || !opts || !fg_sum || !bg_sum) return fail(DVS_ERR_INVALID, who, "null argument");
    if (((uintptr_t)fg_sum | (uintptr_t)bg_sum) & 15u) return fail(DVS_ERR_INVALID, who, "vote arrays must be 16-byte aligned");
    TRY(need_forward(c, who));
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    HIPCHECK(dvs_launch_foreground_views((hipStream_t)stream, s.width, s.height, s.tiles_x, s.tiles_y, c->fwd.n_views, s.n, s.ranges, s.sorted_splat,
                                         s.splat2d, s.n_contrib, fg_masks, valid_masks, fg_sum, bg_sum));
    return DVS_OK;
}
// The plan over the votes (dvs_train.h; kernels in foreground.hip). Here because its refusals name themselves in dvs_last_error()
int dvs_foreground_plan(void* stream, int n, const uint64_t* fg, const uint64_t* bg, int percent, uint8_t* action, uint32_t* offsets, uint32_t* scratch,
                        uint64_t* new_count) {
    const char* const who = "dvs_foreground_plan";
    if (n <= 0) return fail(DVS_ERR_INVALID, who, "n must be > 0");
    if (percent < 1 || percent > 100) return fail(DVS_ERR_INVALID, who, "percent must be in [1, 100]");
    if (!fg || !bg || !action || !offsets || !scratch || !new_count) return fail(DVS_ERR_INVALID, who, "null argument");
    if ((uintptr_t)new_count & 7u) return fail(DVS_ERR_INVALID, who, "new_count must be 8-byte aligned");
    HIPCHECK(dvs_launch_foreground_plan((hipStream_t)stream, n, fg, bg, percent, action, offsets, scratch, new_count));
    return DVS_OK;
}

// The sky texture behind the splats (sky.hip): separate passes over the saved state, before and after the composite backward; the composite
// kernels run with bg = 0 and know nothing of it.
static int check_dL(const float* dL_drgb, const char* who);
// minv [9] <- the inverse of rows 0, 1, 3 of proj's 3x3 part (fp64, then rounded): the pixel ray of pixel_ray.h; false for a singular proj
extern "C++" bool dvs_pixel_ray_matrix(const dvs_camera* cam, float* minv) {      // (declared in dvs_kernels.h; region.hip calls it too)
    const int rows[3] = {0, 1, 3};
    double m[3][3], inv[3][3];
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) m[i][k] = (double)cam->proj[k * 4 + rows[i]];
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {               // inv[i][k] = cofactor(k, i) / det
            const int r0 = (k + 1) % 3, r1 = (k + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
            inv[i][k] = (m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0]) / det;
        }
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) minv[3 * i + k] = (float)inv[i][k];
    return true;
}
// What both entry points check first; minv [n_views][9] receives, per view, the pixel ray matrix.
static int check_sky(dvs_ctx* c, const dvs_camera* cams, int n_views, const dvs_sky* sky, const char* who, float* minv) {
    if (!c || !cams || !sky || !sky->tex) return fail(DVS_ERR_INVALID, who, "null argument");
    if ((uintptr_t)sky->tex & 15u) return fail(DVS_ERR_INVALID, who, "the texture must be 16-byte aligned");
    if (sky->height < 2 || sky->width != 2 * sky->height) return fail(DVS_ERR_INVALID, who, "the texture must have height >= 2 and width == 2 * height");
    if (n_views < 1 || n_views > DVS_MAX_VIEWS) return fail(DVS_ERR_INVALID, who, "bad n_views");
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].bg[0] != 0.f || cams[v].bg[1] != 0.f || cams[v].bg[2] != 0.f)
            return fail(DVS_ERR_INVALID, who, "cams[v].bg must be zero: the sky texture is the background (never both)");
        if (!dvs_pixel_ray_matrix(&cams[v], minv + 9 * v)) return fail(DVS_ERR_INVALID, who, "cams[v].proj is singular: no ray per pixel");
    }
    TRY(need_forward(c, who, n_views));
    for (int v = 0; v < n_views; ++v)
        if (c->fwd.st.width != cams[v].width || c->fwd.st.height != cams[v].height)
            return fail(DVS_ERR_STATE, who, "a camera's image size is not that of the last forward on this context");
    return DVS_OK;
}
int dvs_sky_forward_views(dvs_ctx* c, void* stream, const dvs_camera* cams, int n_views, const dvs_sky* sky, float* out_rgb, float* sky_rgb) {
    const char* const who = "dvs_sky_forward_views";
    float minv[DVS_MAX_VIEWS * 9];
    if (!out_rgb) return fail(DVS_ERR_INVALID, who, "null argument");
    if (((uintptr_t)out_rgb | (uintptr_t)sky_rgb) & 15u) return fail(DVS_ERR_INVALID, who, "images must be 16-byte aligned");
    TRY(check_sky(c, cams, n_views, sky, who, minv));
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);
    tm.begin();
    HIPCHECK(dvs_launch_sky_forward(tm.st, s.width, s.height, n_views, minv, sky->tex, sky->width, sky->height, s.final_T, out_rgb, sky_rgb));
    tm.stage("sky_fwd");
    return tm.finish();
}
int dvs_sky_backward_views(dvs_ctx* c, void* stream, const dvs_camera* cams, int n_views, const dvs_opts* opts, const dvs_sky* sky,
                           const float* dL_drgb, const float* sky_rgb, float* g_tex) {
    const char* const who = "dvs_sky_backward_views";
    float minv[DVS_MAX_VIEWS * 9];
    if (!opts || !g_tex) return fail(DVS_ERR_INVALID, who, "null argument");
    TRY(check_dL(dL_drgb, who));
    if (((uintptr_t)sky_rgb | (uintptr_t)g_tex) & 15u) return fail(DVS_ERR_INVALID, who, "sky_rgb and g_tex must be 16-byte aligned");
    if (opts->grad_mode != DVS_GRAD_TRUE && opts->grad_mode != DVS_GRAD_LINEAGE) return fail(DVS_ERR_INVALID, who, "bad grad_mode");
    TRY(check_sky(c, cams, n_views, sky, who, minv));
    if (!c->bwd.rows_pending || c->bwd.proj_next != 0)
        return fail(DVS_ERR_STATE, who, "no composite backward pending on this context (call between dvs_raster_backward_composite and the projection)");
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);
    tm.begin();
    if (!sky_rgb) {                                     // the caller kept no lookup: redo it into the context's own buffer
        TRY(c->bwd.sky_rgb.ensure((size_t)n_views * 3 * s.width * s.height * sizeof(float)));
        HIPCHECK(dvs_launch_sky_forward(tm.st, s.width, s.height, n_views, minv, sky->tex, sky->width, sky->height, s.final_T, nullptr,
                                        c->bwd.sky_rgb.as<float>()));
        sky_rgb = c->bwd.sky_rgb.as<float>();
        tm.stage("sky_lookup");
    }
    HIPCHECK(dvs_launch_sky_backward_tex(tm.st, s.width, s.height, n_views, minv, sky->width, sky->height, s.final_T, dL_drgb, g_tex));
    tm.stage("sky_bwd_tex");
    HIPCHECK(dvs_launch_sky_backward_rows(tm.st, s.width, s.height, s.tiles_x, s.tiles_y, n_views, s.n, s.ranges, s.sorted_splat, s.splat2d, s.final_T,
                                          s.n_contrib, dL_drgb, sky_rgb, c->bwd.g_rows.as<float>(), opts->grad_mode));
    tm.stage("sky_bwd_rows");
    return tm.finish();
}

// A8: zero the 48-B rows if needed, then the alpha-composite backward into them (all views of the last forward in one launch)
static int bwd_composite(dvs_ctx* c, hipStream_t st, const dvs_camera* cams, const dvs_opts* opts, const float* dL_drgb, StageScope& tm) {
    const dvs_fwd_state& s = c->fwd.st;
    Backward& b = c->bwd;
    const int V = c->fwd.n_views;
    tm.begin();
    if (!b.rows_clean) HIPCHECK(hipMemsetAsync(b.g_rows.p, 0, b.g_rows.bytes, st));
    b.rows_clean = false;
    tm.stage("bwd_zero");
    const CamVec3 bgs(cams, V, &dvs_camera::bg);
    probe_event(c, st, 1);
    if (b.variant == DVS_BWD_TR)
        HIPCHECK(dvs_launch_render_bwd_tr(st, s.width, s.height, s.tiles_x, s.tiles_y, V, s.ranges, s.sorted_splat, s.splat2d, bgs.v, s.final_T,
                                          s.n_contrib, dL_drgb, b.g_rows.as<float>(), opts->absgrad, opts->grad_mode, c->fwd.live_splat, c->fwd.live_pos));
    else                                                   // DVS_BWD_BLOCKS: the setter and dvs_create_views admit nothing else
        HIPCHECK(dvs_launch_render_bwd_blocks(st, s.width, s.height, s.tiles_x, s.tiles_y, V, s.ranges, s.sorted_splat, s.splat2d,
                                              bgs.v, s.final_T, s.n_contrib, dL_drgb, b.g_rows.as<float>(), opts->absgrad, opts->grad_mode));
    probe_event(c, st);
    tm.stage("render_bwd");
    b.rows_pending = true;
    b.proj_next = 0;
    return DVS_OK;
}
// A9 for the splats [first, first + count): rows -> parameter gradients (re-zeroes the rows it reads); [0, n) is the whole projection,
// dvs_raster_backward_project_chunk walks it in pieces. The tiled layout — one view or a batch — goes through ONE pass that
// reads the parameters once and writes the geometry gradients once (+ the per-view colour gradients), the SH rows are then built from
// those (also for a single view: that pass plus the row rebuild is faster than the fused per-view kernel, 0.09 vs 0.15 ms at C3);
// the reference's row layout goes through the per-view kernel, once per view, accumulating (whole range only).
static int bwd_project(dvs_ctx* c, hipStream_t st, const dvs_splats* p, const dvs_camera* cams, const dvs_opts* opts,
                       const dvs_splat_grads* out, int64_t first, int64_t count, StageScope& tm) {
    const dvs_fwd_state& s = c->fwd.st;
    Backward& b = c->bwd;
    const int V = c->fwd.n_views, n = p->n;
    tm.begin();
    if (opts->shn_layout == DVS_SHN_TILED) {
        // Nobody asked for the per-view colour gradients (one GPU, or the plain all-reduce exchange): the kernel builds the SH rows in its
        // epilogue (k_preprocess_bwd_views<.., FUSE_SH>). With out->dcolor (the factorised exchange, dvs_raster_backward_dcolor's twin) it
        // emits them and dvs_launch_sh_grad_combine builds the rows — here right away if sh0 / shN are given too, else after the all-gather.
        const char* nf = getenv("DVS_A9_NO_FUSE_SH");                      // cross-check switch (tests; read per call so that one process can run both)
        const bool no_fuse = nf && nf[0] == '1';
        const bool fuse = !out->dcolor && out->sh0 && out->shN && !no_fuse;
        float* dcol = out->dcolor;
        if (!dcol && !fuse) { TRY(b.dcolor.ensure((size_t)V * n * 3 * sizeof(float))); dcol = b.dcolor.as<float>(); }
        HIPCHECK(dvs_launch_preprocess_bwd_views(st, n, V, p->pos, p->shN, p->opacity, p->scale, p->rot, pack_cams(cams, V), opts->sh_degree,
                                                 opts->antialias, s.radii, s.flags, b.g_rows.as<float>(), out->pos, out->opacity, out->scale,
                                                 out->rot, opts->absgrad ? out->absgrad2d : nullptr, out->mean2d, dcol, opts->accumulate,
                                                 b.keep_rows ? 0 : 1, opts->grad_mode, (int)first, (int)count, fuse ? out->sh0 : nullptr,
                                                 fuse ? out->shN : nullptr));
        if (!fuse && out->sh0 && out->shN)          // (NULL: the factorised exchange builds them after its all-gather of dcolor)
            HIPCHECK(dvs_launch_sh_grad_combine(st, n, p->pos, opts->sh_degree, V, CamVec3(cams, V, &dvs_camera::campos).v, dcol, out->sh0,
                                                out->shN, opts->accumulate, 1));
    } else {
        for (int v = 0; v < V; ++v) {
            const DvsCam dcam = to_dev_cam(cams[v]);
            const size_t on = (size_t)v * n;
            HIPCHECK(dvs_launch_preprocess_bwd(st, n, p->pos, p->shN, p->opacity, p->scale, p->rot, dcam, opts->sh_degree, opts->antialias,
                                               s.radii + on, s.flags + on, b.g_rows.as<float>() + on * 12, out->pos, out->sh0, out->shN,
                                               out->opacity, out->scale, out->rot, opts->absgrad ? out->absgrad2d : nullptr, out->mean2d,
                                               out->dcolor ? out->dcolor + on * 3 : nullptr, (opts->accumulate || v > 0) ? 1 : 0,
                                               b.keep_rows ? 0 : 1, opts->shn_layout, opts->grad_mode));
        }
    }
    tm.stage("preprocess_bwd");
    b.proj_next = first + count < n ? first + count : 0;
    if (b.proj_next != 0) return DVS_OK;    // more chunks to come
    b.rows_clean = !b.keep_rows;            // every row render_bwd can have touched (radius > 0) was read and re-zeroed
    b.rows_pending = b.keep_rows;           // (kept rows can be projected again: the parity tests compare chunked and unchunked A9 on the same rows)
    return DVS_OK;
}
static int check_bwd_args(dvs_ctx* c, const dvs_splats* p, const dvs_camera* cams, int V /*< 0: those of the last forward*/, const dvs_opts* opts, const char* who) {
    if (!c || !cams || !opts) return fail(DVS_ERR_INVALID, who, "null argument");
    if (V < 0) V = c->fwd.n_views;
    if (opts->grad_mode != DVS_GRAD_TRUE && opts->grad_mode != DVS_GRAD_LINEAGE) return fail(DVS_ERR_INVALID, who, "bad grad_mode");
    if (!c->fwd.have || V != c->fwd.n_views || (p && c->fwd.st.n != p->n) || c->fwd.st.width != cams[0].width || c->fwd.st.height != cams[0].height)
        return fail(DVS_ERR_STATE, who, "no matching forward on this context");
    return DVS_OK;
}
static int check_dL(const float* dL_drgb, const char* who) {
    if (!dL_drgb) return fail(DVS_ERR_INVALID, who, "null argument");
    if ((uintptr_t)dL_drgb & 15u) return fail(DVS_ERR_INVALID, who, "dL_drgb must be 16-byte aligned (the composite backward reads it as 16-byte words)");
    return DVS_OK;
}
static int check_grads(const dvs_splats* p, const dvs_splat_grads* out, const char* who) {
    if (!p || !out) return fail(DVS_ERR_INVALID, who, "null argument");
    if (p->n > 0 && (!out->pos || !out->opacity || !out->scale || !out->rot || ((!out->sh0 || !out->shN) && !out->dcolor)))
        return fail(DVS_ERR_INVALID, who, "null gradient row pointer (sh0/shN may be NULL only when dcolor is given)");
    if (p->n > 0 && (((uintptr_t)out->pos | (uintptr_t)out->sh0 | (uintptr_t)out->shN | (uintptr_t)out->opacity | (uintptr_t)out->scale |
                      (uintptr_t)out->rot | (uintptr_t)out->absgrad2d | (uintptr_t)out->mean2d | (uintptr_t)out->dcolor) & 15u))
        return fail(DVS_ERR_INVALID, who, "gradient arrays must be 16-byte aligned");
    return DVS_OK;
}

// The public backward entry points: validate, scoped timing, the stage(s).
static int backward_views(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cams, int V, const dvs_opts* opts,
                          const float* dL_drgb, const dvs_splat_grads* out, const char* who) {
    TRY(check_dL(dL_drgb, "dvs_raster_backward"));
    TRY(check_grads(p, out, who));
    TRY(check_bwd_args(c, p, cams, V, opts, who));
    HIPCHECK(hipSetDevice(c->device));
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);
    TRY(bwd_composite(c, tm.st, cams, opts, dL_drgb, tm));
    TRY(bwd_project(c, tm.st, p, cams, opts, out, 0, p->n, tm));
    return tm.finish();
}
int dvs_raster_backward(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cam, const dvs_opts* opts,
                        const float* dL_drgb, const dvs_splat_grads* out) {
    return backward_views(c, stream, p, cam, 1, opts, dL_drgb, out, "dvs_raster_backward");
}
int dvs_raster_backward_views(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cams, int n_views, const dvs_opts* opts,
                              const float* dL_drgb, const dvs_splat_grads* out) {
    return backward_views(c, stream, p, cams, n_views, opts, dL_drgb, out, "dvs_raster_backward_views");
}

int dvs_raster_backward_composite(dvs_ctx* c, void* stream, const dvs_camera* cam, const dvs_opts* opts, const float* dL_drgb) {
    const char* const who = "dvs_raster_backward_composite";
    TRY(check_dL(dL_drgb, who));
    TRY(check_bwd_args(c, nullptr, cam, -1, opts, who));
    HIPCHECK(hipSetDevice(c->device));
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);
    TRY(bwd_composite(c, tm.st, cam, opts, dL_drgb, tm));
    return tm.finish();
}

// what both projection entry points check first (`pending`: how each of them words a missing composite)
static int check_project(dvs_ctx* c, const dvs_splats* p, const dvs_camera* cam, const dvs_opts* opts, const dvs_splat_grads* out,
                         const char* who, const char* pending) {
    TRY(check_grads(p, out, who));
    TRY(check_bwd_args(c, p, cam, -1, opts, who));
    return c->bwd.rows_pending ? DVS_OK : fail(DVS_ERR_STATE, who, pending);
}
int dvs_raster_backward_project(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cam, const dvs_opts* opts,
                                const dvs_splat_grads* out) {
    const char* const who = "dvs_raster_backward_project";
    TRY(check_project(c, p, cam, opts, out, who, "no dvs_raster_backward_composite on this context"));
    if (c->bwd.proj_next != 0)     // earlier chunks already consumed (and re-zeroed) their rows: projecting all of [0, n) now would overwrite their gradients with zeros
        return fail(DVS_ERR_STATE, who, "a dvs_raster_backward_project_chunk sequence is in progress on this context (finish it up to n)");
    HIPCHECK(hipSetDevice(c->device));
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);
    TRY(bwd_project(c, tm.st, p, cam, opts, out, 0, p->n, tm));
    return tm.finish();
}

int dvs_raster_backward_project_chunk(dvs_ctx* c, void* stream, const dvs_splats* p, const dvs_camera* cam, const dvs_opts* opts,
                                      const dvs_splat_grads* out, int64_t first, int64_t count) {
    const char* const who = "dvs_raster_backward_project_chunk";
    TRY(check_project(c, p, cam, opts, out, who, "no dvs_raster_backward_composite pending on this context"));
    if (opts->shn_layout != DVS_SHN_TILED || !out->dcolor || out->sh0 || out->shN)
        return fail(DVS_ERR_INVALID, who, "needs the DVS_SHN_TILED layout and the factorised form (out->dcolor given, sh0 / shN NULL)");
    if (first != c->bwd.proj_next || count <= 0 || first + count > p->n || (first % 256) != 0)
        return fail(DVS_ERR_INVALID, who, "chunks must cover [0, n) in ascending order, each starting at a multiple of 256");
    HIPCHECK(hipSetDevice(c->device));
    StageScope tm(c, (hipStream_t)stream, /*append=*/true);                 // (every chunk is a "preprocess_bwd" row of the timing table)
    TRY(bwd_project(c, tm.st, p, cam, opts, out, first, count, tm));
    return tm.finish();
}

int dvs_sort_pairs_u32(dvs_ctx* c, void* stream, uint32_t* keys, uint32_t* vals, uint64_t n, int bit_lo, int bit_hi) {
    if (!c || (n > 0 && (!keys || !vals)) || bit_lo < 0 || bit_hi > 32 || bit_lo > bit_hi) return fail(DVS_ERR_INVALID, "dvs_sort_pairs_u32", "bad argument");
    HIPCHECK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return DVS_OK;
    TRY(c->a.tmp_keys.ensure(n * 4));
    TRY(c->a.tmp_vals.ensure(n * 4));
    uint32_t* k[2] = {keys, c->a.tmp_keys.as<uint32_t>()};
    uint32_t* v[2] = {vals, c->a.tmp_vals.as<uint32_t>()};
    int cur = 0;
    // (partition offsets are 32-bit: the last partition's element indices must not wrap — ADVICE r05)
    if (n > (1ull << 32) - 4097ull) return fail(DVS_ERR_CAPACITY, "dvs_sort_pairs_u32", "n must be at most 2^32 - 4097");
    TRY(c->fe.hist.ensure(dvs_pair_sort_hist_bytes(n)));
    invalidate(c, DROP_SEGS);                                            // the sort writes its one segment over the context's descriptors
    HIPCHECK(dvs_launch_pair_sort(st, n, k[0], v[0], k[1], v[1], bit_lo, bit_hi - bit_lo,
                                  DvsPairSortWs{c->fe.seg_all, c->fe.totals, c->fe.hist.as<uint32_t>()}, c->fe.rank_atomic, &cur));
    if (cur == 1) {
        HIPCHECK(hipMemcpyAsync(keys, k[1], n * 4, hipMemcpyDeviceToDevice, st));
        HIPCHECK(hipMemcpyAsync(vals, v[1], n * 4, hipMemcpyDeviceToDevice, st));
    }
    return DVS_OK;
}

// TEST HOOK (dvs_raster.h): the forward's range-adaptive depth sort (A5, low 32 key bits) on caller-supplied keys, one view.
int dvs_debug_sort_depth_keys(dvs_ctx* c, void* stream, const uint32_t* keys, uint64_t n, uint32_t* sorted_ids, uint32_t* n_sorted, uint32_t* digit_bits) {
    if (!c || !keys || !sorted_ids || !n_sorted || n == 0 || n > c->max_splats * (uint64_t)c->max_views || n >= (1ull << 31))
        return fail(DVS_ERR_INVALID, "dvs_debug_sort_depth_keys", "bad argument (n must be in [1, max_splats * max_views])");
    HIPCHECK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    Arenas& a = c->a; FrontEnd& fe = c->fe;
    // the key range a forward's A2 would have left in the view's 64 slots: here reduced on the host from a copy of the keys
    std::vector<uint32_t> h(n);
    HIPCHECK(hipMemcpyAsync(h.data(), keys, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    uint32_t mn = 0xFFFFFFFFu, mx = 0u; bool any = false;
    for (uint32_t k : h) if (k != 0xFFFFFFFFu) { mn = k < mn ? k : mn; mx = k > mx ? k : mx; any = true; }
    uint32_t slots[64 * 16] = {0};
    if (any) { slots[0] = ~mn; slots[1] = mx; }
    // A2's outputs (key[0], the key-range slots) and the descriptors are overwritten: the forward state and a prepared A2 are gone
    invalidate(c, DROP_FWD | DROP_PREP | DROP_SEGS);
    HIPCHECK(hipMemcpyAsync(fe.kred, slots, sizeof slots, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(a.key[0].p, keys, n * 4, hipMemcpyDeviceToDevice, st));
    HIPCHECK(dvs_launch_seg_init(st, (int)n, 1, dvs_depth_sort_rows_per_view((int)n, 1), fe.seg_all));
    HIPCHECK(dvs_launch_depth_sort(st, (int)n, 1, a.key[0].as<uint32_t>(), a.ids[0].as<uint32_t>(), a.key[1].as<uint32_t>(), a.ids[1].as<uint32_t>(),
                                   fe.seg_all, fe.seg_vis, fe.kred, fe.hist.as<uint32_t>(), fe.totals, fe.rank_atomic));
    DvsSeg sv;
    HIPCHECK(hipMemcpyAsync(&sv, fe.seg_vis, sizeof sv, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *n_sorted = sv.count;
    if (digit_bits) *digit_bits = sv.bits;
    HIPCHECK(hipMemcpyAsync(sorted_ids, a.ids[1].p, (size_t)sv.count * 4, hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemsetAsync(fe.kred, 0, sizeof slots, st));
    return DVS_OK;
}

int dvs_export_sorted_keys(dvs_ctx* c, void* stream, uint64_t* out_keys) {
    const char* const who = "dvs_export_sorted_keys";
    if (!c || !out_keys) return fail(DVS_ERR_INVALID, who, "null argument");
    if (!c->fwd.have) return fail(DVS_ERR_STATE, who, "no forward state");
    const dvs_fwd_state& s = c->fwd.st;
    if (s.num_rendered == DVS_T_UNKNOWN) { uint64_t t; TRY(dvs_get_num_rendered(c, stream, &t)); }
    if (!s.sorted_tile)
        return fail(DVS_ERR_STATE, who, "the last forward was asynchronous (dvs_set_async) and did not materialise the sorted tile ids; "
                    "export the keys of a synchronous forward");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(dvs_launch_export_keys((hipStream_t)stream, s.num_rendered, s.sorted_tile, s.sorted_splat, s.depth, out_keys));
    return DVS_OK;
}

int dvs_shn_relayout(dvs_ctx* c, void* stream, int n, const float* src, float* dst, int to_tiled) {
    if (!c || n < 0 || (n > 0 && (!src || !dst))) return fail(DVS_ERR_INVALID, "dvs_shn_relayout", "bad argument");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(dvs_launch_shn_relayout((hipStream_t)stream, n, src, dst, to_tiled));
    return DVS_OK;
}

int dvs_sh_grad_combine(dvs_ctx* c, void* stream, int n, const float* pos, int sh_degree, int n_views, const float* campos,
                        const float* dcolor, float* g_sh0, float* g_shN, int accumulate, int shn_layout) {
    if (!c || n < 0 || n_views < 0 || sh_degree < 0 || sh_degree > 3 || (n > 0 && n_views > 0 && (!pos || !campos || !dcolor || !g_sh0 || !g_shN)))
        return fail(DVS_ERR_INVALID, "dvs_sh_grad_combine", "bad argument");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(dvs_launch_sh_grad_combine((hipStream_t)stream, n, pos, sh_degree, n_views, campos, dcolor, g_sh0, g_shN, accumulate, shn_layout));
    return DVS_OK;
}

int dvs_raster_backward_dcolor(dvs_ctx* c, void* stream, float* dcolor) {
    const char* const who = "dvs_raster_backward_dcolor";
    if (!c || !dcolor || ((uintptr_t)dcolor & 15u)) return fail(DVS_ERR_INVALID, who, "bad argument (dcolor: 16-byte aligned device array)");
    if (!c->bwd.rows_pending) return fail(DVS_ERR_STATE, who, "no dvs_raster_backward_composite pending on this context");
    HIPCHECK(hipSetDevice(c->device));
    const dvs_fwd_state& s = c->fwd.st;
    HIPCHECK(dvs_launch_dcolor_from_rows((hipStream_t)stream, (int64_t)c->fwd.n_views * s.n, s.radii, s.flags, c->bwd.g_rows.as<float>(), dcolor));
    return DVS_OK;
}

int dvs_set_async(dvs_ctx* c, int enable) {
    if (!c) return fail(DVS_ERR_INVALID, "dvs_set_async", "null context");
    c->async_T = enable != 0;
    return DVS_OK;
}
int dvs_get_num_rendered(dvs_ctx* c, void* stream, uint64_t* T) {
    const char* const who = "dvs_get_num_rendered";
    if (!c || !T) return fail(DVS_ERR_INVALID, who, "null argument");
    if (!c->fwd.have) return fail(DVS_ERR_STATE, who, "no forward state");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    Arenas& a = c->a;
    *T = a.total_host[0];
    c->fwd.st.num_rendered = *T;
    if (a.total_host[1] != a.overflow_seen) {
        a.overflow_seen = a.total_host[1];
        (void)ensure_instance_arenas(c, *T + *T / 2);
        return fail(DVS_ERR_CAPACITY, who, "the last forward produced more tile instances than the instance arena held; its outputs are "
                    "invalid. The arena has been enlarged — repeat that view.");
    }
    return DVS_OK;
}

int dvs_get_sort_rank_mode(dvs_ctx* c) { return c ? c->fe.rank_atomic : -1; }
int dvs_set_export_sorted_tiles(dvs_ctx* c, int enable) {
    if (!c) return fail(DVS_ERR_INVALID, "dvs_set_export_sorted_tiles", "null context");
    c->export_tiles = enable != 0;
    return DVS_OK;
}

int dvs_get_arena_info(dvs_ctx* c, uint64_t* cap, uint64_t* grows, uint64_t* last_T, uint64_t* overflows) {
    if (!c) return fail(DVS_ERR_INVALID, "dvs_get_arena_info", "null context");
    if (cap) *cap = c->a.inst_cap;
    if (grows) *grows = c->a.inst_grow_events;
    if (last_T) *last_T = c->a.total_host[0];
    if (overflows) *overflows = c->a.total_host[1];
    return DVS_OK;
}

int dvs_debug_record_decisions(dvs_ctx* c, uint64_t* take_masks, uint64_t capacity_instances) {
    if (!c || (take_masks && (((uintptr_t)take_masks & 7u) || capacity_instances == 0))) return fail(DVS_ERR_INVALID, "dvs_debug_record_decisions", "bad argument");
    c->fwd.rec_masks = take_masks; c->fwd.rec_cap = take_masks ? capacity_instances : 0;
    return DVS_OK;
}

int dvs_set_backward_variant(dvs_ctx* c, int variant) {
    const char* const who = "dvs_set_backward_variant";
    if (!c || variant < DVS_BWD_BLOCKS || variant > DVS_BWD_TR) return fail(DVS_ERR_INVALID, who, "bad argument");
    if (variant == DVS_BWD_REDUCE || variant == DVS_BWD_MM)
        return fail(DVS_ERR_UNSUPPORTED, who, "the 'reduce' and 'mm' kernels are retired — this library contains 'tr' (default) and 'blocks' only");
    c->bwd.variant = variant;
    return DVS_OK;
}
int dvs_set_live_lists(dvs_ctx* c, int enable) {
    if (!c) return fail(DVS_ERR_INVALID, "dvs_set_live_lists", "null context");
    c->fwd.live_lists = enable != 0;
    return DVS_OK;
}
int dvs_set_forward_variant(dvs_ctx* c, int variant) {
    // 0 = the per-block forward (retired), 1 = the quadrant forward, the only one there is (dvs_raster.h)
    if (!c || (variant != 0 && variant != 1)) return fail(DVS_ERR_INVALID, "dvs_set_forward_variant", "bad argument");
    if (variant == 0)
        return fail(DVS_ERR_UNSUPPORTED, "dvs_set_forward_variant", "the per-block forward is retired — this library contains the quadrant forward only");
    return DVS_OK;
}

int dvs_keep_bwd_intermediates(dvs_ctx* c, int keep) { if (!c) return DVS_ERR_INVALID; c->bwd.keep_rows = keep != 0; return DVS_OK; }

int dvs_get_bwd_intermediates(dvs_ctx* c, const float** rows, int* row_floats) {
    if (!c) return DVS_ERR_INVALID;
    if (rows) *rows = c->bwd.g_rows.as<float>();
    if (row_floats) *row_floats = 12;
    return DVS_OK;
}

int dvs_enable_stage_timing(dvs_ctx* c, int enable) { if (!c) return DVS_ERR_INVALID; c->timing.on = enable != 0; return DVS_OK; }
int dvs_enable_kernel_probe(dvs_ctx* c, int enable) {
    if (!c) return DVS_ERR_INVALID;
    c->probe.on = enable != 0;
    c->probe.used = 0; c->probe.kind.clear();
    return DVS_OK;
}
int dvs_read_kernel_probe(dvs_ctx* c, float mean_ms[2], int count[2]) {
    if (!c || !mean_ms || !count) return DVS_ERR_INVALID;
    HIPCHECK(hipSetDevice(c->device));
    Probe& pr = c->probe;
    double sum[2] = {0, 0};
    count[0] = count[1] = 0;
    for (size_t k = 0; k < pr.kind.size() && 2 * k + 1 < pr.used; ++k) {
        float ms = 0.f;
        HIPCHECK(hipEventSynchronize(pr.ev[2 * k + 1]));
        HIPCHECK(hipEventElapsedTime(&ms, pr.ev[2 * k], pr.ev[2 * k + 1]));
        sum[pr.kind[k]] += ms; count[pr.kind[k]]++;
    }
    for (int i = 0; i < 2; ++i) mean_ms[i] = count[i] ? (float)(sum[i] / count[i]) : 0.f;
    pr.used = 0; pr.kind.clear();
    return DVS_OK;
}
int dvs_get_stage_timing(dvs_ctx* c, const char*** names, const float** ms) {
    if (!c) return 0;
    if (names) *names = c->timing.out_names.data();
    if (ms) *ms = c->timing.out_ms.data();
    return (int)c->timing.out_names.size();
}

int dvs_memcpy_d2h(dvs_ctx* c, void* host_dst, const void* dev_src, size_t bytes) {
    if (!c) return DVS_ERR_INVALID;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return DVS_OK;
}
int dvs_memcpy_h2d(dvs_ctx* c, void* dev_dst, const void* host_src, size_t bytes) {
    if (!c) return DVS_ERR_INVALID;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return DVS_OK;
}
void* dvs_device_malloc(dvs_ctx* c, size_t bytes) {
    if (!c) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return p;
}
void dvs_device_free(dvs_ctx* c, void* p) { if (c && p) { (void)hipSetDevice(c->device); (void)hipFree(p); } }

}  // extern "C"
