// trainer.hpp — GaussianTrainerScene::Impl, the state behind `libgstrain.so`, and what its source files share. The members are defined
// in trainer_load.cpp (allocation, what the loaders share, the synthetic loader), trainer_dataset.cpp (the capture loader), trainer_step.cpp
// (one trainStep), trainer_refine.cpp (densification, pruning), trainer_output.cpp (configuration report, the evaluation context and its
// pass loop, evaluation, export), trainer_render.cpp (rendered views as JPEG and PNG files) and trainer_mesh.cpp (mesh export); the focus
// region's members sit beside the code they feed (trainer_step.cpp, trainer_refine.cpp); gstrain.cpp holds the GaussianTrainerScene
// members and the C symbols.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <functional>
#include <map>
#include <string_view>
#include "../../include/gaussian_trainer_scene.hpp"
#include "../../include/dvs_scene.h"
#include "../../include/dvs_train.h"
#include "../../include/dvs_export.h"
#include "../../include/dvs_init.h"
#include "../../include/dvs_region.h"
#include "device_mem.hpp"
#include "ply_io.hpp"
#include "dataset_io.hpp"
#include "export_frame.hpp"
#include "ext_options.hpp"

namespace {
const int kWidth[6] = {3, 3, 45, 1, 3, 4};          // pos sh0 shN opacity scale rot
enum { P_POS = 0, P_SH0, P_SHN, P_OPA, P_SCALE, P_ROT };
const int kAllGroups[6] = {P_POS, P_SH0, P_SHN, P_OPA, P_SCALE, P_ROT};
const int kGeomGroups[4] = {P_POS, P_OPA, P_SCALE, P_ROT};                // what the factorised exchange all-reduces

__attribute__((format(printf, 1, 2))) inline void logf_(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    fputs("[gstrain] ", stderr); vfprintf(stderr, fmt, ap); fputc('\n', stderr);
    va_end(ap);
}
#define HIP_OR_THROW(expr)                                                                          \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr ": ") + hipGetErrorString(e_)); } while (0)
#define DVS_OR_THROW(expr)                                                                          \
    do { int r_ = (expr); if (r_ != DVS_OK) throw std::runtime_error(std::string(#expr ": ") + dvs_last_error()); } while (0)

// the DVS_* environment overrides: the integer value of `name` (atoi) or `fallback` when it is not set; whether it is set to `value`
inline int env_int(const char* name, int fallback) { const char* e = getenv(name); return e ? atoi(e) : fallback; }
inline bool env_is(const char* name, const char* value) { const char* e = getenv(name); return e && std::string_view(e) == value; }
inline double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
}  // namespace

// Two timing events, created at the first use: how long the device took over what a stream was given between begin() and end(). run() is
// the whole sequence (record, launch, record, wait for the second event). A caller that queues more behind end() and then waits for the
// stream itself (the renders' copy) takes the two steps and asks for ms() after its wait.
struct TimedPair {
    Event e0, e1;
    void begin(hipStream_t s) {
        for (Event* e : {&e0, &e1})
            if (!*e) { hipEvent_t h = nullptr; HIP_OR_THROW(hipEventCreate(&h)); e->reset(h); }
        HIP_OR_THROW(hipEventRecord(e0.get(), s));
    }
    void end(hipStream_t s) { HIP_OR_THROW(hipEventRecord(e1.get(), s)); }
    float ms() const { float v = 0; HIP_OR_THROW(hipEventElapsedTime(&v, e0.get(), e1.get())); return v; }
    template <class F>
    float run(hipStream_t s, F&& launch) { begin(s); launch(); end(s); HIP_OR_THROW(hipEventSynchronize(e1.get())); return ms(); }
};

struct __attribute__((visibility("hidden"))) GaussianTrainerScene::Impl {     // the class is exported (GSTRAIN_API), its implementation is not
    GaussianTrainConfig cfg;
    // the extension options the config struct has no room for (ext_options.hpp, INTEGRATION.md "Extension options"): read from the
    // environment once, when the scene is constructed (a bad value is reported there and leaves the default); the set... methods of
    // GaussianTrainerScene write the same fields, so a setter called at any time wins over the environment
    gsopt::ExtOptions opt;
    int loadItr = -1;
    TrainingStatus status = TrainingStatus::Loading_Prepare;
    bool training = true;
    int device = 0;
    // Members are destroyed in reverse order of declaration: the training stream last, both contexts after every buffer declared below
    // them, the communicator after its stream. Keep these five first, in this order.
    Stream stream;
    Ctx ctx, eval_ctx;                                                       // eval_ctx: created at the first evaluation
    Comm comm; int rank = 0, world = 1;                                      // data-parallel replicas (include/dvs_comm.h)
    Stream comm_stream;                                                      // collectives run beside A9
    int n = 0, W = 0, H = 0, sh_max = 3;
    DevBuf<float> d_param[6], d_m[6], d_v[6];
    DevBuf<float> d_param2[6], d_m2[6], d_v2[6];                             // densification writes old -> new, then the sets swap
    DevBuf<float> d_absgrad;
    DevBuf<float> d_grad_flat; size_t grad_floats = 0;                       // the six gradient groups live in ONE buffer: one all-reduce
    float* d_grad[6] = {};                                                   // (slices of d_grad_flat)
    DevBuf<float> d_mean2d;                                                  // dL/dmean2D (ADC statistic when useAbsGrad is off)
    // Gradient exchange of the replicas. factorised (default): the geometry groups (pos, opacity, scale, rot: 44 B/splat) lead the
    // flat buffer and are all-reduced; of the SH rows only each view's 3-float colour gradient is all-gathered (12 B/splat/view) and
    // every replica rebuilds the summed rows with dvs_sh_grad_combine — at 8 GPUs 161 MB instead of 413 MB through each GPU's links
    // per million splats. DVS_EXCHANGE=allreduce: one all-reduce of all 59-float rows.
    bool factorised = true; size_t geom_floats = 0;
    DevBuf<float> d_dcolor_local, d_dcolor_all;                              // [cap,3] / [world,n,3]
    DevBuf<float> d_dcolor_scratch;                                          // A9's own copy of the colour gradient (the all-gather reads the early one)
    Event ev_dcolor, ev_bwd, ev_comm;
    Event ev_gather; std::vector<Event> ev_chunk;                            // all-gather done / A9 chunk k queued (chunked geometry all-reduce)
    bool pipeline = false;                                                   // DVS_EXCHANGE_PIPELINE=1 (with DVS_A9_CHUNKS > 1): see trainStep
    std::vector<Event> ev_ar;                                                // chunk k's geometry all-reduce has landed (communication stream)
    std::vector<int> next_ci;                                                // the NEXT iteration's cameras, drawn early for the pipelined step
    int a9_chunks = 1;                                                       // DVS_A9_CHUNKS: splat chunks of A9 whose geometry gradients leave one by one (default 1 until
                                                                             // the chunked exchange has run on real multi-GPU hardware: ADVICE r03; equality with the unchunked
                                                                             // exchange is asserted by tests/test_gpu_multirank.py::test_plugin_two_ranks_exchanges_agree)
    // The training views, one entry per camera of `cams`: the image as fp32 or, when packLevel has PackF32ToU8, as 8 bits per channel
    // (gs_train.cpp:91-96, the reference's VRAM saver: a quarter of the HBM footprint, expanded into d_target_f32 right before the
    // loss), and the camera's mask when useMask was on at load time or the capture had a distorted camera (`undistorted`: the views of
    // SIMPLE_RADIAL / RADIAL / OPENCV cameras were remapped to pinhole views at load time and their pixels without a source are masked
    // out; every view of such a capture carries a mask, a pinhole view's being its file mask or all ones)
    // `valid`: only for an undistorted view loaded with useMask while maskCarve was on — the undistortion's validity alone (the mask is
    // "valid AND trainable"), so that the carve can tell a blank pixel from a background pixel
    struct View { DevBuf<float> f32; DevBuf<uint8_t> u8; DevBuf<float> mask, valid; };
    std::vector<View> views;
    std::vector<dvs_camera> cams;
    DevBuf<float> d_target_f32;
    bool views_u8() const { return (cfg.packLevel & PackF32ToU8) != 0; }
    const void* view_pixels(size_t ci) const { return views_u8() ? (const void*)views[ci].u8.get() : (const void*)views[ci].f32.get(); }
    bool undistorted = false;
    const float* view_mask(size_t ci) const { return cfg.useMask || undistorted ? views[ci].mask.get() : nullptr; }   // (nullptr too when loaded without masks)
    void store_view(DevBuf<float> image, DevBuf<float> mask);
    std::vector<float> init_host[6];                                         // initial splats (resetGaussian, getPoints3D)
    bool terminate = false, pruning = false;
    int cap = 0;                                                             // array capacity in splats (cfg.capMax)
    DevBuf<float> d_grad_accum, d_denom; DevBuf<int> d_max_radii;
    DevBuf<uint8_t> d_action; DevBuf<uint32_t> d_offsets, d_dscratch; DevBuf<uint64_t> d_newcount;
    DevBuf<void> d_mcmc;                                                     // dvs_mcmc_* scratch (densifyStrategy 1)
    float extent = 1.f;                                                      // scene extent (camera spread), sets the split/clone scale
    dvs_fwd_state fwd{};                                                     // (views into the context's arrays)
    int vpi = 1;                                                             // views per trainStep and GPU, one multi-view pass (cfg.viewsPerIter / DVS_VIEWS_PER_ITER)
    bool sequential_views = false;                                           // DVS_VIEWS_MODE=sequential: the same views one pass at a time, accumulating (the reference shape)
    DevBuf<int> d_vis_radius;                                                // visibleAdam with vpi > 1: max radius over the step's views
    DevBuf<float> d_out, d_dL, d_loss;                                       // d_loss[0..63] = (1-w) L1 partial sums, d_loss[64..127] = SSIM partial sums
    DevBuf<float> d_ssim_maps[3];
    float last_loss = 0.f;
    int step = 0;
    uint64_t cam_rng = 88172645463325252ULL;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<float> host[6];
    bool host_valid = false;
    // held-out evaluation (cfg.evalHoldout / evalEvery): camera i is a test camera iff i % eval_holdout == 0. Both lists are empty when
    // evaluation is off — the draw is then the reference's, over all cameras. The test views are rendered by a context of their own:
    // the training context's saved forward state, pending backward rows and prepared projection are never touched by an evaluation.
    int eval_holdout = 0, eval_every = 0;
    int loss_every = 100;                                                    // steps between two loss log lines (DVS_LOSS_EVERY, read at load)
    std::vector<int> train_idx, test_idx;
    int eval_views = 0;                                                      // min(n_test, 8) views per pass of eval_ctx
    DevBuf<float> d_eval_out; DevBuf<void> d_eval_scratch; DevBuf<double> d_eval_res;
    // Everything that renders through eval_ctx does it here (trainer_output.cpp): the cameras `which` of `sp` (DVS_SHN_TILED, at most
    // `cap` splats) in list order, eval_views per pass, with eval_opts() — one dvs_raster_forward_views into d_eval_out per pass, then
    // composite_sky when with_sky, then per_pass; nothing else is launched and nothing waits. per_pass runs before the next forward, so
    // it is where the context's saved forward state is consumed (dvs_raster_depth_views, dvs_raster_importance_views).
    //   caller            cameras             sky   masks
    //   score_views       test_idx            yes   view_mask x region_masks (enableFocusRegion), made in per_pass: only the metric reads them
    //   render_to_jpeg    what is asked for   yes   none
    //   render_to_png     what is asked for   yes   none
    //   extract_mesh      training_cameras()  no    view_mask
    //   prune_importance  training_cameras()  no    view_mask
    //   prune_mask_carve  training_cameras()  no    view_mask as the foreground, the view's validity plane when it has one
    struct EvalPass { int first, nb; const int* cam; const dvs_camera* cams; const float* images; };   // views which[first .. first + nb): their indices
                                                                             // (&which[first]), their cameras [nb], d_eval_out [nb][3][H][W]
    void for_each_eval_pass(const dvs_splats& sp, const std::vector<int>& which, bool with_sky, const std::function<void(const EvalPass&)>& per_pass);
    dvs_opts eval_opts() const {                                             // full SH degree, what a viewer shows from the saved PLY
        dvs_opts o{};
        o.sh_degree = sh_max; o.antialias = cfg.mipAntiliased ? 1 : 0; o.shn_layout = DVS_SHN_TILED; o.tile_bounds = DVS_TILES_CANONICAL;
        return o;
    }
    std::vector<int> training_cameras() const {                              // train_idx, or every camera when nothing is held out
        std::vector<int> v = train_idx;
        if (v.empty()) for (int c = 0; c < (int)cams.size(); ++c) v.push_back(c);
        return v;
    }
    std::vector<double> eval_res;                                            // [n_test][4] = {mse, l1, ssim, psnr} of the last evaluation
    double eval_mean[4] = {NAN, NAN, NAN, NAN};
    int eval_it = -1;
    // coarse-to-fine training (cfg.resolutionSchedule = S, cfg.numDownscales = K; both 0 here when the schedule is off): the step with
    // `step` completed steps before it trains at level k = max(K - step / S, 0), on images of W / 2^k x H / 2^k — the stored views
    // box-filtered by ONE dvs_downsample_views call per step into d_level_targets, the cameras those of dvs_camera_downscale. The
    // level is a function of the step number alone (every rank derives the same one; a resume lands on the right one). Everything
    // per pixel of the step (d_out, d_dL, the loss, the densification statistics) has the level's size; the arenas keep the full one.
    int res_every = 0, res_levels = 0;
    std::vector<std::vector<dvs_camera>> level_cams;                        // [k - 1][camera], k = 1..K (level 0: cams)
    DevBuf<float> d_level_targets, d_level_masks;                           // [vpi,3,H/2,W/2] / [vpi,H/2,W/2]: room for the largest level below full size
    int cur_level = -1;                                                      // level of the last step (-1: none yet)
    int lw = 0, lh = 0;                                                      // image size of the last step (W x H when the schedule is off)
    int level_first_step = 0; std::chrono::steady_clock::time_point level_t0;
    // compact exports beside the full PLY (cfg.exportFormats / DVS_EXPORT_FORMATS / the suffix of modelPath): the packers' scratch, the
    // packed payload on the device and its host copy. Nothing is allocated until a save exports.
    GrowBuf<void> d_export_scratch; GrowBuf<uint8_t> d_export_out;
    std::vector<uint8_t> export_host;
    // the fidelity score of the .spz and .reduced.ply exports (evaluation on, rank 0): the packed payload decoded on the device into a
    // second parameter set in the tiled layout, rendered and scored on the test cameras like the full model. Allocated at the first
    // such export. One record per scored format, in the eval JSON's order: the decoded model's means {mse, l1, ssim, psnr} at iteration `it`.
    GrowBuf<float> d_decoded[6];
    enum { SCORED_SPZ = 0, SCORED_REDUCED = 1 };
    struct DecodedScore { const char* name; double mean[4] = {NAN, NAN, NAN, NAN}; int it = -1; /*-1: none*/ };
    DecodedScore decoded_score[2] = {{"spz"}, {"reduced"}};
    // the ending both exports share: reserves d_decoded, `unpack` decodes into it (-> status; `unpacker` names it in the exception), the
    // full model is evaluated unless this step's already is, the decoded one scored and logged. Nothing without test cameras.
    void score_decoded(int format, const char* unpacker, const std::function<int()>& unpack);
    // the .reduced.ply export (EXPORT_REDUCED): per-splat degrees, the camera centres, centres / iteration counts / block counts on the
    // device (one small buffer). Nothing is allocated until the first such export.
    GrowBuf<uint8_t> d_red_degree, d_red_small;
    // opt: SH_CULL_THRESHOLD (colour units, default 0.01: chosen without measurement) and REDUCED_HALF, or what setReducedExport said

    // export frame (INTEGRATION.md "Export frame"): a similarity p' = s R p + t every export but the resume PLY is written in — what
    // DVS_EXPORT_TRANSFORM / DVS_EXPORT_ORIENT said at load, or setExportTransform / setExportOrientation since. At a save rank 0 fills a
    // second set of pos, shN, scale, rot (sh0 and opacity are invariant: the training arrays) with ONE dvs_transform_splats call on the
    // training stream and the packers read that set (ex()); a decoded payload is taken back by the inverse before it is scored, so the
    // evaluation cameras stay as they are. Nothing is allocated, launched, written or logged while no transform is set.
    bool xf_set = false; dvs_similarity xf{}, xf_inv{}; float xf_D[83] = {}, xf_inv_D[83] = {}; std::string xf_how;
    bool xf_filled = false;                                                  // this save's set is in d_xf
    GrowBuf<float> d_xf[4], d_xf_rows;                                       // pos, shN (tiled), scale, rot; shN as rows for the .transformed.ply
    static int xf_slot(int g) { return g == P_POS ? 0 : g == P_SHN ? 1 : g == P_SCALE ? 2 : g == P_ROT ? 3 : -1; }
    const float* ex(int g) const { return xf_filled && xf_slot(g) >= 0 ? d_xf[xf_slot(g)].get() : model_ex(g); }   // what an export packs from
    bool set_export_transform(const dvs_similarity& m, const std::string& how);
    bool set_export_orientation(const char* axis, const char* from);
    void setup_export_transform();
    void report_export_transform() const;
    void fill_transformed();
    void export_transformed();

    // level-of-detail export (INTEGRATION.md "LOD export"; trainer_lod.cpp): opt's EXPORT_LOD = L (0 = off .. 4) and LOD_RESOLUTION = R
    // (32..1024, default 256), or what setLodExport said. At a save rank 0 merges the FULL model on a lattice of
    // R >> (k - 1) cells along the longest side of the finite centres' box, for k = 1..L (include/dvs_export.h, last section), scores each
    // level on the held-out views when evaluation is on and writes <modelPath>_<it>.lod<k>.ply in the full PLY's layout (in the export
    // frame when one is set). Nothing is allocated, launched, written or logged while L is 0.
    GrowBuf<void> d_lod_scratch; GrowBuf<float> d_lod[6], d_lod_rows;       // a level's merged set (shN tiled), its shN as rows for the file
    struct LodScore { int it = -1, m = 0; double mean[4] = {NAN, NAN, NAN, NAN}; };     // it = -1: none
    LodScore lod_score[4];
    void export_lod();

    // rendered views as JPEG files (cfg.renderViews / renderQuality / renderSampling and their DVS_RENDER_* overrides, read at load): at
    // every save rank 0 renders the selected cameras through eval_ctx (for_each_eval_pass: what `eval @it` scored), turns each pass
    // into quantised DCT coefficients with ONE dvs_jpeg_encode_views launch, copies them to the host and Huffman-codes them on up to
    // load_threads() threads (write_files) into <modelPath>_<it>_renders/<name>.jpg. Nothing is allocated until the first render. The training
    // context, its pending rows and its prepared projection are never touched.
    enum { RENDER_TEST = 1, RENDER_TRAIN = 2 };
    int render_views = 0, render_quality = 90, render_sampling = 0;
    std::vector<std::string> cam_names;                                      // per camera, in step with cams: the image's stem, empty for a synthetic camera
    bool cam_names_ok = false;                                               // every camera has a stem and they are unique (else the files are cam_%04d)
    GrowBuf<int16_t> d_render_coef;                                          // [eval_views][coefficients of a view]
    std::vector<int16_t> render_coef_host;
    TimedPair render_timer;                                                  // a pass's encode launches, both formats
    struct RenderStats { size_t views = 0, bytes = 0; double transform_ms = 0, entropy_ms = 0; int threads = 0; };
    void setup_render();
    std::string camera_name(int c) const;
    void ensure_eval_ctx();
    bool render_to_jpeg(const std::vector<int>& which, const std::vector<std::string>& files, RenderStats* stats);
    void render_at_save();
    // the same views as PNG files (DVS_RENDER_FORMAT=png; INTEGRATION.md "Rendered views"): the layers of DVS_RENDER_LAYERS — colour
    // <name>.png (RGB8, scale 255: the JPEG's quantisation), depth <name>_depth.png (GRAY16 of depth x DVS_RENDER_DEPTH_SCALE, 0 = no
    // depth, a tEXt chunk depth_scale) and alpha <name>_alpha.png (GRAY8, scale 255). Depth and alpha are one dvs_raster_depth_views call
    // per pass on eval_ctx (the sky composite only adds to the image: the saved forward state stays valid; the sky is in neither).
    // Per pass one dvs_png_encode_views launch per layer, one copy of the filtered streams and the saturation counts, then the same host
    // threads deflate (DVS_RENDER_PNG_LEVEL) and write one file each. Nothing is allocated until the first PNG render.
    GrowBuf<uint8_t> d_render_png;                                           // 64 bytes of saturation counts, then per layer [views of the pass][stream]
    std::vector<uint8_t> render_png_host;
    GrowBuf<float> d_render_depth, d_render_alpha;                           // [eval_views][H][W]
    struct PngStats { size_t views = 0, files = 0, bytes = 0, saturated = 0; double filter_ms = 0, deflate_ms = 0; int threads = 0; };
    // files[l] (l = 0 colour, 1 depth, 2 alpha): one path per camera of `which`, or empty when the layer is not asked for
    bool render_to_png(const std::vector<int>& which, const std::vector<std::string> (&files)[3], PngStats* stats);

    // mesh export (cfg.meshResolution / DVS_MESH_RESOLUTION; trainer_mesh.cpp): the depth and alpha maps of a pass of eval_ctx. Nothing is
    // allocated until the first mesh. The grid and the extraction scratch live for one extraction.
    GrowBuf<float> d_mesh_depth, d_mesh_alpha;
    int mesh_resolution() const;
    std::string mesh_file(int it) const { return save_path(it, "_mesh.ply"); }
    bool mesh_bounds(float lo[3], float hi[3]);
    bool extract_mesh(const std::string& path, int resolution);
    // what happens to the mesh before it is written, from opt: MESH_MIN_COMPONENT (of the largest component's triangles, in 1/100 percent)
    // and MESH_NORMALS, or what setMeshCleanup said; then MESH_DECIMATE (0 = off, or 2..16 voxels of the extraction grid per cell and
    // axis), or what setMeshDecimate said

    // importance prune (cfg.importancePrune / DVS_IMPORTANCE_PRUNE; trainer_refine.cpp): the per-splat score summed over the training views
    // and the selection's scratch. Nothing is allocated until the first such prune.
    DevBuf<uint64_t> d_imp_score; DevBuf<void> d_imp_scratch;
    int importance_prune() const { return std::min(90, std::max(0, env_int("DVS_IMPORTANCE_PRUNE", cfg.importancePrune))); }   // percent, 0 = off
    void prune_importance(int it);

    // mask carve (opt's MASK_CARVE = T in 1..100, 0 = off, or what setMaskCarve said; trainer_refine.cpp,
    // INTEGRATION.md "Mask carve"): at every prune occasion and before every save the splats whose blend weight over the training views
    // landed on background pixels of the views' masks go (dvs_raster_foreground_views per pass of eval_ctx, dvs_foreground_plan). Inactive
    // when no training view has a mask. Nothing is allocated, launched, written or logged while T is 0.
    bool carve_has_masks() const;                                            // some training view has a mask
    bool carve_has_valid() const;                                            // ... and some view kept its validity plane
    DevBuf<uint64_t> d_carve_votes;                                          // [2][cap rounded up to even]: foreground, background
    void prune_mask_carve(int it);
    void report_mask_carve(const char* by) const;

    // sky model (cfg.enableBg, the reference's "Create Sky Model"; trainer_output.cpp): an equirectangular fp32 texture [sky_h][2 sky_h][3]
    // behind the splats (dvs_sky_forward_views / dvs_sky_backward_views, dvs_raster.h), initialised to zero, its own Adam state, the
    // step's gradient, and the lookup the forward leaves for the backward. Every camera of the trainer has bg = 0 (the loaders set
    // none). Nothing is allocated, launched or written while enableBg is off. opt's SKY_RESOLUTION (128, clamped to 16..1024 at load)
    // and SKY_LR (0.01).
    struct Step;
    bool sky_on = false; int sky_h = 0;
    DevBuf<float> d_sky, d_sky_m, d_sky_v, d_sky_grad, d_sky_rgb;
    size_t sky_floats() const { return (size_t)sky_h * 2 * sky_h * 3; }
    dvs_sky sky() const { dvs_sky s{}; s.tex = d_sky.get(); s.width = 2 * sky_h; s.height = sky_h; return s; }
    std::string sky_file(int it) const { return save_path(it, ".sky"); }
    void setup_sky(bool resumed);
    void step_sky(const Step& s);
    void save_sky();
    // out (+)= final_T s for the nb views `c` just rendered into `out` (for_each_eval_pass); nothing when the sky is off
    void composite_sky(dvs_ctx* c, const dvs_camera* bc, int nb, float* out) {
        if (!sky_on) return;
        const dvs_sky s = sky();
        DVS_OR_THROW(dvs_sky_forward_views(c, stream.get(), bc, nb, &s, out, nullptr));
    }

    // focus region (cfg.enableFocusRegion, which the editor flips live; INTEGRATION.md "Focus region"): the box (focus_lo, focus_hi) is fixed
    // at load — the bounds of the initial centres, or DVS_FOCUS_REGION — and updateFocusRegion() moves it through F = T R S (include/dvs_region.h).
    // While the flag is on, splats whose centre is outside are removed (prune_region) and the loss and the evaluation see only the pixels
    // whose ray crosses the box (region_masks). While it is off nothing below is allocated, launched or written by a step.
    float focus_lo[3] = {0.f, 0.f, 0.f}, focus_hi[3] = {0.f, 0.f, 0.f};
    float focus_trs[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f};       // position, rotation (radians), scale of the region in force
    dvs_region region{};
    float region_b2w[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // F, row-major
    bool region_dirty = false;                                               // the region or the flag changed since the last region prune
    bool region_flag_seen = false;                                           // cfg.enableFocusRegion as the last trainStep saw it
    DevBuf<float> d_region_mask;                                             // [max(vpi, 8), H, W]: a step's or an evaluation pass's masks; allocated at the first use
    void setup_region();
    bool set_region(const float* pos, const float* rot, const float* scale);
    void prune_region(int it);
    const float* region_masks(const dvs_camera* bc, const float* const* in, int nb, int w, int h);

    // 3D smoothing filter (opt's MIP_FILTER3D, or what setMipFilter3d said, read at load and at resetGaussian; trainer_filter3d.cpp,
    // INTEGRATION.md "3D smoothing filter"): d_filter[i] is the world-space standard deviation splat i is smoothed by — the highest rate
    // at which a full-resolution training camera samples it (dvs_filter3d_compute) — and d_scale_eff / d_opacity_eff are what splats()
    // hands to every renderer (dvs_filter3d_apply_range). The trained values stay in d_param: the refinement rules, the opacity reset,
    // MCMC, Adam and the resume PLY read those, and finish_range takes the rasterizer's gradients back to them first
    // (dvs_filter3d_chain_range). The filter is computed again when f3d_dirty (load, resume, anything that changed the splat set:
    // apply_plan, MCMC, resetGaussian) and every 100 optimizer steps; the effective arrays again whenever the trained ones changed since
    // (f3d_fresh). Both happen in filter3d_refresh(), which every reader of splats() calls first; when it does either it cancels a
    // projection the pipelined step prepared from the arrays it rewrites. A save packs the filter of the positions BEING SAVED: when that
    // is not the one training holds, filter3d_for_save() computes it and its effective values into a second set (d_save_*) that only the
    // exports read (model_ex) — training, its schedule and its prepared projection are never touched by a save.
    // Nothing is allocated, launched, logged or written while the option is 0.
    bool f3d_on = false, f3d_dirty = false, f3d_fresh = false, f3d_save = false;
    int f3d_it = 0;                                                          // optimizer steps behind the trained values (= step between two trainSteps)
    int f3d_step = 0, f3d_cams = 0, f3d_cap = 0;                             // f3d_it at the last computation; training cameras in d_f3d_rows; splats the arrays hold
    DevBuf<float> d_filter, d_scale_eff, d_opacity_eff, d_f3d_rows; DevBuf<uint32_t> d_f3d_scratch;
    GrowBuf<float> d_save_filter, d_save_scale, d_save_opacity;              // a save's own set (f3d_save: in use)
    TimedPair f3d_timer;
    void setup_filter3d();
    bool filter3d_due(int optimizer_steps) const { return f3d_on && (f3d_dirty || optimizer_steps - f3d_step >= 100); }
    void filter3d_compute(float* filter, const char* what);
    void filter3d_apply(int first, int count);
    void filter3d_refresh();
    void filter3d_for_save();
    void filter3d_chain(int first, int count);
    void export_fused();
    // scale / opacity: what a renderer reads (the effective arrays while the filter is on); the other groups: d_param
    const float* model(int g) const { return f3d_on && g == P_SCALE ? d_scale_eff.get() : f3d_on && g == P_OPA ? d_opacity_eff.get() : d_param[g].get(); }
    // ... and what an export packs: the save's own set while it is in use
    const float* model_ex(int g) const { return f3d_save && g == P_SCALE ? d_save_scale.get() : f3d_save && g == P_OPA ? d_save_opacity.get() : model(g); }

    ~Impl() { if (device >= 0) (void)hipSetDevice(device); }                // (the members release themselves, after this body)
    // floats of group g on the device: the 45 higher-order SH floats live in the DVS_SHN_TILED layout (48 per splat,
    // whole 64-splat tiles); parameters, gradients and Adam moments share it — the optimizer is element-wise.
    size_t dev_floats_for(int g, int count) const { return g == P_SHN ? (size_t)((count + 63) / 64) * 64 * 48 : (size_t)count * kWidth[g]; }
    size_t dev_floats(int g) const { return dev_floats_for(g, n); }
    void upload(int g, const std::vector<float>& host_rows);
    void alloc_params(int count, int capacity, const std::vector<float> init[6]);
    void reset_stats() {
        HIP_OR_THROW(hipMemsetAsync(d_grad_accum.get(), 0, (size_t)cap * 4, stream.get()));
        HIP_OR_THROW(hipMemsetAsync(d_denom.get(), 0, (size_t)cap * 4, stream.get()));
        HIP_OR_THROW(hipMemsetAsync(d_max_radii.get(), 0, (size_t)cap * 4, stream.get()));
    }
    dvs_densify_params plan_params(int it) const;
    uint64_t plan(const dvs_densify_params& prm);
    void apply_plan(const dvs_densify_params& prm, int new_n, bool zero_moments);
    void densify(int it);
    void densify_mcmc(int it);
    void prune_light(int it);
    void report_config() const;
    void sync_stats();
    const float* target_for(int ci);
    bool mcmc() const { return cfg.densifyStrategy == 1; }
    bool exchange_factorised() const { return comm && factorised; }
    bool visible_adam() const { return cfg.visibleAdam && world == 1; }     // per-rank visibility would let the replicas drift apart
    int sh_degree_at(int s) const { return cfg.progressiveTrain ? std::min(sh_max, s / 1000) : sh_max; }   // SH bands unlocked every 1000 steps
    void setup_exchange();
    // cameras: one xorshift stream shared by all ranks; an iteration draws world x vpi views and rank r renders views r vpi .. r vpi + vpi - 1
    // (vpi = 1: one view per GPU and iteration, as the reference's trainStep renders one camera; vpi = 8 on one GPU: BASELINE config C4)
    void draw_cameras(std::vector<int>& ci) {
        ci.assign((size_t)world * vpi, 0);                  // every rank knows every rank's cameras: the SH rows are rebuilt from them
        for (int& c : ci) {
            cam_rng ^= cam_rng << 13; cam_rng ^= cam_rng >> 7; cam_rng ^= cam_rng << 17;
            if (train_idx.empty()) c = cfg.singleCamera ? 0 : (int)(cam_rng % cams.size());
            else c = train_idx[cfg.singleCamera ? 0 : (size_t)(cam_rng % train_idx.size())];     // held-out cameras are never trained on
        }
    }
    void setup_split();
    bool evaluate(bool write_json, bool force = false);
    void run_evaluation();
    void score_views(const dvs_splats& sp, std::vector<double>& res, double mean[4]);     // [n_test][4] and their means, synchronous
    void write_eval_json() const;
    std::vector<dvs_camera> rank_cameras(const std::vector<int>& ci_all, int level) const {     // this rank's views of an iteration's draw, at a level
        std::vector<dvs_camera> v((size_t)vpi);
        for (int k = 0; k < vpi; ++k) {
            const size_t ci = (size_t)ci_all[(size_t)rank * vpi + k];
            v[(size_t)k] = level > 0 ? level_cams[(size_t)level - 1][ci] : cams[ci];
        }
        return v;
    }
    int level_of(int s) const { return res_every > 0 ? std::max(res_levels - s / res_every, 0) : 0; }   // s: completed steps before the step
    void setup_levels();
    const int* any_view_radii() {                            // max radius over the step's views (view-major fwd.radii of the multi-view pass)
        if (!d_vis_radius) d_vis_radius.alloc((size_t)cap * sizeof(int) + 16);
        DVS_OR_THROW(dvs_any_view_radius(stream.get(), n, vpi, fwd.radii, d_vis_radius.get()));
        return d_vis_radius.get();
    }
    // ---- the phases of one trainStep ----
    struct Step {                                                            // one iteration, carried through its phases
        int it = 0, deg = 0;                                                 // the iteration being computed, its SH degree
        int level = 0, div = 1, Wd = 0, Hd = 0;                              // resolution level of the step, 2^level, the level's image size
        std::vector<int> ci_all;                                             // the iteration's cameras, [rank][local view]
        std::vector<dvs_camera> vcams;                                       // this rank's views
        dvs_opts opts{};
        bool mcmc = false, absgrad = false, want_stats = false;
        bool refine_now = false, reset_now = false, prune_now = false;
        float lr_pos = 0.f;
        dvs_adam_group adam[6] = {};                                         // Adam groups over the whole arrays
        const float* region_mask = nullptr;                                  // (render_backward) enableFocusRegion: the step's masks [vpi, Hd, Wd]
        const int* adam_gate = nullptr;                                      // (render_backward) visible-only Adam: radius > 0 in the step's views
        int chunk_per = 0, n_chunks = 0;                                     // (render_backward) > 0: the geometry gradients left behind A9 in chunks
    };
    Step plan_step();                                                        // decides the step; launches nothing
    void enter_level(const Step& s);
    void close_level();
    void level_targets(const Step& s);
    void loss_of_view(const Step& s, int v);
    void render_backward(Step& s);
    void exchange(const Step& s, bool pipelined);
    void finish_range(const Step& s, int first, int count, const int* groups, int n_groups, const int* gate);
    void finish_pipelined(const Step& s);
    template <class Buf>
    static dvs_splats splats_of(const Buf (&p)[6], int n) {                  // a parameter set in the device layout (d_param, d_decoded)
        dvs_splats s{};
        s.pos = p[P_POS].get(); s.sh0 = p[P_SH0].get(); s.shN = p[P_SHN].get(); s.opacity = p[P_OPA].get();
        s.scale = p[P_SCALE].get(); s.rot = p[P_ROT].get(); s.n = n;
        return s;
    }
    dvs_splats splats() const {                                              // what the rasterizer reads (filter3d_refresh() first, outside a step)
        dvs_splats s = splats_of(d_param, n);
        s.scale = model(P_SCALE); s.opacity = model(P_OPA);
        return s;
    }
    std::string save_path(int it, const char* suffix) const { return cfg.modelPath + "_" + std::to_string(it) + suffix; }   // every file a save writes
    std::string model_file(int it) const { return save_path(it, ".ply"); }
    bool model_path_ends(const char* suffix) const {
        const size_t k = strlen(suffix);
        return cfg.modelPath.size() >= k && cfg.modelPath.compare(cfg.modelPath.size() - k, k, suffix) == 0;
    }
    // EXPORT_* bits of the compact formats a save writes; decided at every use, since the editor sets modelPath after construction
    // EXPORT_TRANSFORMED: <modelPath>_<it>.transformed.ply, the full PLY in the export frame; counts only while a transform is set, and is
    // implied when one is set and no other format is selected (a set transform is never a silent no-op)
    // EXPORT_FUSED: <modelPath>_<it>.fused.ply, the full PLY of the model the 3D smoothing filter fused (in the export frame when one is
    // set); counts only while the filter is on, and is implied when it is on and no other format is selected
    enum { EXPORT_COMPRESSED = 1, EXPORT_SPLAT = 2, EXPORT_SPZ = 4, EXPORT_REDUCED = 8, EXPORT_TRANSFORMED = 16, EXPORT_FUSED = 32 };
    int suffix_formats() const {
        return model_path_ends(".compressed.ply") ? EXPORT_COMPRESSED : model_path_ends(".splat") ? EXPORT_SPLAT : model_path_ends(".spz") ? EXPORT_SPZ :
               model_path_ends(".reduced.ply") ? EXPORT_REDUCED : 0;
    }
    int asked_formats() const { return env_int("DVS_EXPORT_FORMATS", cfg.exportFormats); }   // 0: the suffix of modelPath decides
    int export_formats() const {
        const int f = (asked_formats() ? asked_formats() : suffix_formats()) &
                      (EXPORT_COMPRESSED | EXPORT_SPLAT | EXPORT_SPZ | EXPORT_REDUCED | (xf_set ? EXPORT_TRANSFORMED : 0) | (f3d_on ? EXPORT_FUSED : 0));
        return f != 0 ? f : (xf_set ? (int)EXPORT_TRANSFORMED : 0) | (f3d_on ? (int)EXPORT_FUSED : 0);
    }
    void export_model(int format);
    void export_spz();
    void export_reduced();
    // the tail of every export: `bytes` of d_export_out to the host (stream synchronised), then the file through `write`. -> the file's
    // size (unknown_size when it cannot be read), or -1 when the file could not be written (logged)
    long long write_payload(size_t bytes, const std::string& file, size_t unknown_size, const std::function<bool(std::string*)>& write);
    // write_payload, then the `export @` line of the simple formats (its time includes the write). -> false: not written
    bool write_export(std::chrono::steady_clock::time_point t_start, size_t bytes, const std::string& file, const char* word, size_t unknown_size,
                      const std::function<bool(std::string*)>& write);
    void fetch_host();
    // what the two loaders share: the context and every per-step buffer (W, H, sh_max set by the caller) ...
    void create_context(int count, int capacity, const std::vector<float> init[6]);
    // ... and, once cams and the views are in place: split, levels, extent, resume or the loader's fresh initialisation,
    // upload, report_config, the loader's own verbose line (told whether the run resumed), exchange set-up
    void finish_load(const std::function<void(std::vector<float> (&)[6])>& fresh_init, const char* fresh_name,
                     const std::function<void(bool)>& describe);
    bool load_synthetic(const std::string& spec_str);
    struct CaptureLoad;                                                      // load_dataset's plan, loop state and stages (trainer_dataset.cpp)
    bool load_dataset(const std::string& path);
    // host threads of the capture loader's decode-ahead and of the render writers (DVS_LOAD_THREADS, default 8, 1..16: never sized from
    // the machine's CPU count)
    int load_threads() const { return std::max(1, std::min(env_int("DVS_LOAD_THREADS", 8), 16)); }
};
