// trainer_output.cpp — what the trainer reports and writes: the configuration lines, held-out evaluation, host copies, compact exports.
#include "trainer.hpp"
#include "sky_io.hpp"

// One line per decision: which GaussianTrainConfig fields this build honours and which it ignores (gs_train.cpp:50-103 sets them all).
void GaussianTrainerScene::Impl::report_config() const {
    if (rank != 0) return;
    static const char* strat[3] = {"ADC (clone / split / prune)", "MCMC (relocation + growth)", "ADC+ (ADC on abs-grad statistics with revised opacity)"};
    logf_("config: densifyStrategy %d = %s; pruneStrategy %d (%s) every %d steps after refineStopIter %d; capMax %d; packLevel %d (%s%s); "
          "useMask %d; useAbsGrad %d; mipAntiliased %d; visibleAdam %d; singleCamera %d; progressiveTrain %d; world %d",
          cfg.densifyStrategy, strat[std::min(2, std::max(0, cfg.densifyStrategy))], cfg.pruneStrategy,
          cfg.pruneStrategy > 0 ? "light prune: opacity < pruneOpacity or scale > pruneScale3d" : "off", cfg.pruneInterval, cfg.refineStopIter,
          cfg.capMax, cfg.packLevel, views_u8() ? "PackF32ToU8: 8-bit training views" : "fp32 training views",
          (cfg.packLevel & PackTileID) ? ", PackTileID: always on here (the tile sort's keys are tile ids inside a view, written as 16-bit words while a view has <= 65536 tiles)" : "",
          (int)cfg.useMask, (int)cfg.useAbsGrad, (int)cfg.mipAntiliased, (int)cfg.visibleAdam, (int)cfg.singleCamera, (int)cfg.progressiveTrain, world);
    if (!test_idx.empty()) {
        std::string idx;
        for (int c : test_idx) idx += " " + std::to_string(c);
        logf_("config: evaluation: %zu of %zu cameras held out of training (evalHoldout %d: cameras%s), scored at every save%s", test_idx.size(),
              cams.size(), eval_holdout, idx.c_str(), eval_every > 0 ? (" and every " + std::to_string(eval_every) + " steps").c_str() : "");
    }
    if (res_every > 0)
        logf_("config: resolutionSchedule %d, numDownscales %d: coarse-to-fine training, the step after s completed ones renders 1/2^max(%d - s/%d, 0) of "
              "%dx%d (targets box-filtered per step, cameras of dvs_camera_downscale); full resolution from iteration %d; evaluation always at full size",
              res_every, res_levels, res_levels, res_every, W, H, res_levels * res_every + 1);
    if (const int fmts = export_formats())
        logf_("config: exportFormats %d: every save also writes%s%s%s%s%s%s beside the full PLY, packed on the device%s%s", fmts,
              (fmts & EXPORT_COMPRESSED) ? " <modelPath>_<it>.compressed.ply" : "", (fmts & EXPORT_SPLAT) ? " <modelPath>_<it>.splat" : "",
              (fmts & EXPORT_SPZ) ? " <modelPath>_<it>.spz" : "", (fmts & EXPORT_REDUCED) ? " <modelPath>_<it>.reduced.ply" : "",
              (fmts & EXPORT_TRANSFORMED) ? " <modelPath>_<it>.transformed.ply (the full PLY in the export frame)" : "",
              (fmts & EXPORT_FUSED) ? " <modelPath>_<it>.fused.ply (the full PLY of the model the 3D smoothing filter fused)" : "",
              asked_formats() == 0 ? ((fmts & ~(EXPORT_TRANSFORMED | EXPORT_FUSED)) ? " (turned on by the suffix of modelPath)"
                                      : (fmts & EXPORT_TRANSFORMED) ? " (implied by the export transform)" : " (implied by mipFilter3d)") : "",
              (fmts & EXPORT_SPZ) && !test_idx.empty() ? "; the .spz payload is decoded on the device and scored on the held-out views" : "");
    report_export_transform();
    if (export_formats() & EXPORT_REDUCED)
        logf_("config: reduced export: twenty 256-entry k-means codebooks (at most 100 iterations each), %s positions; cullSH %d: %s%s",
              opt.on(gsopt::REDUCED_HALF) ? "half-float" : "float", (int)cfg.cullSH,
              cfg.cullSH ? ("every splat gets the smallest SH degree that loses at most " + std::to_string(opt.f(gsopt::SH_CULL_THRESHOLD)) +
                            " of colour from any training camera's centre (no visibility test; the 0.01 default was chosen without measurement)").c_str()
                         : "every splat keeps the model's SH degree",
              !test_idx.empty() ? "; the payload is decoded on the device and scored on the held-out views" : "");
    const int render_layers = opt.i(gsopt::RENDER_LAYERS);
    if (render_views && opt.on(gsopt::RENDER_FORMAT))
        logf_("config: renderViews %d: every save also writes the %s cameras as PNG files (layers %s%s%s, depth x %.9g as 16-bit gray with 0 = no depth, "
              "zlib level %d) to <modelPath>_<it>_renders/, rendered with the evaluation's options; samples and the per-row filter choice on the device, "
              "deflate on the host%s", render_views, render_views == RENDER_TEST ? "test" : render_views == RENDER_TRAIN ? "training" : "test and training",
              (render_layers & gsopt::LAYER_COLOR) ? "color" : "", (render_layers & gsopt::LAYER_DEPTH) ? ((render_layers & gsopt::LAYER_COLOR) ? ",depth" : "depth") : "",
              (render_layers & gsopt::LAYER_ALPHA) ? ((render_layers & (gsopt::LAYER_COLOR | gsopt::LAYER_DEPTH)) ? ",alpha" : "alpha") : "",
              (double)opt.f(gsopt::RENDER_DEPTH_SCALE), opt.i(gsopt::RENDER_PNG_LEVEL),
              (render_views & RENDER_TEST) && test_idx.empty() ? " (no camera is held out: every camera is a training camera)" : "");
    else if (render_views)
        logf_("config: renderViews %d: every save also writes the %s cameras as JPEG files (quality %d, %s) to <modelPath>_<it>_renders/, rendered with the "
              "evaluation's options; transform on the device, entropy coding on the host%s", render_views,
              render_views == RENDER_TEST ? "test" : render_views == RENDER_TRAIN ? "training" : "test and training", render_quality,
              render_sampling == 1 ? "4:4:4" : "4:2:0", (render_views & RENDER_TEST) && test_idx.empty() ? " (no camera is held out: every camera is a training camera)" : "");
    if (const int res = mesh_resolution(); res > 0)
        logf_("config: meshResolution %d: a save of the finished model and export_mesh() also write <modelPath>_<it>_mesh.ply — the training cameras' "
              "depth maps fused into a TSDF grid of %d voxels along the longest side, marching tetrahedra, all on the device", res,
              std::min(1024, std::max(16, res)));
    if (const int bp = opt.i(gsopt::MESH_MIN_COMPONENT); bp > 0 || opt.on(gsopt::MESH_NORMALS))
        logf_("config: mesh clean-up: components with fewer than %g %% of the largest one's triangles are dropped%s, on the device, before the mesh "
              "is written%s", bp / 100.0, bp > 0 ? "" : " (off)",
              opt.on(gsopt::MESH_NORMALS) ? "; vertex normals nx ny nz from the TSDF gradient" : "");
    if (const int F = opt.i(gsopt::MESH_DECIMATE); F > 0)
        logf_("config: mesh decimation: vertex clustering on cells of %d voxels of the extraction grid per axis (mean position, colour and normal per "
              "cell; collapsed and repeated triangles dropped), on the device, last before the mesh is written", F);
    if (const int L = opt.i(gsopt::EXPORT_LOD), R = opt.i(gsopt::LOD_RESOLUTION); L > 0)
        logf_("config: lodExport %d levels, resolution %d: every save also writes <modelPath>_<it>.lod<k>.ply, k = 1..%d — the full model's splats merged "
              "per cell of a lattice of %d >> (k - 1) cells along the longest side of the finite centres' box (weighted mean, moment-matched "
              "covariance, weight-preserving opacity), on the device%s", L, R, L, R,
              !test_idx.empty() ? "; every level is scored on the held-out views" : "");
    if (const int P = importance_prune(); P > 0) {
        const int asked = env_int("DVS_IMPORTANCE_PRUNE", cfg.importancePrune);
        if (asked > 90) logf_("config: importancePrune %d clamped to 90", asked);
        logf_("config: importancePrune %d: at every prune occasion%s, after the light prune, the %d %% of the splats with the smallest blend weight "
              "summed over the %zu training cameras are removed (scored and selected on the device, every rank for itself)", P,
              cfg.pruneStrategy > 0 ? "" : " (none: pruneStrategy is 0)", P, train_idx.empty() ? cams.size() : train_idx.size());
    }
    report_mask_carve(nullptr);
    if (sky_on)
        logf_("config: skyModel %dx%d: enableBg — an equirectangular fp32 texture behind the splats, looked up along each pixel's ray and trained with "
              "them (Adam, lr %g); every save also writes <modelPath>_<it>.sky; evaluation and written renders composite it; mesh export, the "
              "importance score and the depth pass do not see it", 2 * sky_h, sky_h, (double)opt.f(gsopt::SKY_LR));
    if (cfg.enableFocusRegion)
        logf_("config: focusRegion box %.9g,%.9g,%.9g .. %.9g,%.9g,%.9g under F = T(%g,%g,%g) R(%g,%g,%g rad, Rz Ry Rx) S(%g,%g,%g): a splat stays while "
              "its centre p has lo <= F^-1 p <= hi (faces included, extents not considered; pruned after load, when the region changes, before every "
              "refinement, prune and save); the loss and the evaluation see only the pixels whose ray crosses the box; mesh export takes its world bounds",
              (double)focus_lo[0], (double)focus_lo[1], (double)focus_lo[2], (double)focus_hi[0], (double)focus_hi[1], (double)focus_hi[2],
              (double)focus_trs[0], (double)focus_trs[1], (double)focus_trs[2], (double)focus_trs[3], (double)focus_trs[4], (double)focus_trs[5],
              (double)focus_trs[6], (double)focus_trs[7], (double)focus_trs[8]);
    std::string ign;
    if (cfg.modelType != 0) ign += " modelType(only 3DGS)";
    if (cfg.pixelGradScale) ign += " pixelGradScale";
    if (cfg.bestQuality) ign += " bestQuality";
    if (cfg.normalConsistencyLoss) ign += " normalConsistencyLoss(2DGS)";
    if (cfg.exportMesh) ign += " exportMesh";
    if (cfg.outputSparsePoints) ign += " outputSparsePoints";
    if (cfg.maxImageCount) ign += " maxImageCount";
    if (!cfg.cameraPosePath.empty() || !cfg.pointCloudPath.empty()) ign += " cameraPosePath/pointCloudPath(dataset ingestion)";
    if (cfg.visibleAdam && world > 1) ign += " visibleAdam(off with WORLD_SIZE > 1: the visible set differs per rank)";
    if (!ign.empty()) logf_("config: IGNORED by this build:%s", ign.c_str());
}

// the maskCarve line of report_config(), and of setMaskCarve (`by`); nothing while it is off
void GaussianTrainerScene::Impl::report_mask_carve(const char* by) const {
    const int T = opt.i(gsopt::MASK_CARVE);
    if (T <= 0 || rank != 0) return;
    const std::string who = by ? std::string(" (") + by + ")" : std::string();
    if (cams.empty()) { logf_("config: maskCarve %d%s: decided when the training views are loaded", T, who.c_str()); return; }
    if (!carve_has_masks()) {
        logf_("config: maskCarve %d%s: inactive: no training view has a mask (%s)", T, who.c_str(),
              cfg.useMask ? "the capture was loaded without masks" : "useMask is off");
        return;
    }
    logf_("config: maskCarve %d%s: at every prune occasion%s before the light prune, and before every save, a splat stays only while its blend weight "
          "over the %zu training cameras landed on foreground pixels of their masks: fg > 0 and fg x %d >= bg x %d (voted and planned on the "
          "device, every rank for itself)%s", T, who.c_str(), cfg.pruneStrategy > 0 ? "" : " (none: pruneStrategy is 0)",
          train_idx.empty() ? cams.size() : train_idx.size(), 100 - T, T,
          !undistorted ? "" : carve_has_valid() ? "; the blank pixels of the undistorted views vote for nothing"
                                                : "; the blank pixels of the undistorted views count as background (their validity was not kept at load)");
}

// Held-out evaluation, on the training stream: the test cameras rendered from the current parameters at the full SH degree (what a
// viewer shows from the saved PLY), min(n_test, 8) views per multi-view pass of a SEPARATE context, each pass scored by one
// dvs_image_metrics_views call against the stored targets (8-bit ones as they are, the camera's mask when useMask or when the capture was undistorted), then ONE copy of
// the [n_test][4] doubles to the host. Only rank 0 evaluates (the replicas are identical). -> false when evaluation is off.
// A save right after the step that was just scored (evalEvery divides the iteration) writes that result: the parameters are the same.
bool GaussianTrainerScene::Impl::evaluate(bool write_json, bool force) {
    if (test_idx.empty() || rank != 0 || !ctx) return false;
    HIP_OR_THROW(hipSetDevice(device));
    if (force || eval_it != step) run_evaluation();
    if (write_json) write_eval_json();
    return true;
}
void GaussianTrainerScene::Impl::run_evaluation() {
    score_views(splats(), eval_res, eval_mean);
    eval_it = step;
    logf_("eval @%d: %d views, PSNR %.17g dB, SSIM %.17g, L1 %.17g", step, (int)test_idx.size(), eval_mean[3], eval_mean[2], eval_mean[1]);
}
// the context the held-out views are rendered by (and the views written as JPEG files): min(n_test, 8) views per pass — of all
// cameras when nothing is held out and only pictures are asked for — created at the first use together with its output images
void GaussianTrainerScene::Impl::ensure_eval_ctx() {
    if (eval_ctx) return;
    eval_views = std::min(test_idx.empty() ? (int)cams.size() : (int)test_idx.size(), 8);
    eval_ctx.reset(dvs_create_views(device, (size_t)cap, W, H, eval_views));
    if (!eval_ctx) throw std::runtime_error(std::string("dvs_create_views (evaluation): ") + dvs_last_error());
    d_eval_out.alloc((size_t)eval_views * 3 * (size_t)W * H * sizeof(float));
}
void GaussianTrainerScene::Impl::for_each_eval_pass(const dvs_splats& sp, const std::vector<int>& which, bool with_sky,
                                                    const std::function<void(const EvalPass&)>& per_pass) {
    ensure_eval_ctx();
    filter3d_refresh();                                                      // (mipFilter3d: splats() of the caller reads the effective arrays)
    const dvs_opts opts = eval_opts();
    std::vector<dvs_camera> bc((size_t)eval_views);
    const int total = (int)which.size();
    for (int first = 0; first < total; first += eval_views) {
        const int nb = std::min(eval_views, total - first);
        for (int k = 0; k < nb; ++k) bc[(size_t)k] = cams[(size_t)which[(size_t)(first + k)]];
        DVS_OR_THROW(dvs_raster_forward_views(eval_ctx.get(), stream.get(), &sp, bc.data(), nb, &opts, d_eval_out.get()));
        if (with_sky) composite_sky(eval_ctx.get(), bc.data(), nb, d_eval_out.get());     // what was trained: the sky behind the splats
        per_pass(EvalPass{first, nb, &which[(size_t)first], bc.data(), d_eval_out.get()});
    }
}
// the test cameras rendered from `sp` and scored: res = [n_test][4] {mse, l1, ssim, psnr}, mean = their means
void GaussianTrainerScene::Impl::score_views(const dvs_splats& sp, std::vector<double>& res, double mean[4]) {
    const int nt = (int)test_idx.size();
    const size_t img = 3 * (size_t)W * H;
    ensure_eval_ctx();
    if (!d_eval_scratch) {
        d_eval_scratch.alloc(dvs_image_metrics_scratch_bytes(W, H, eval_views));
        d_eval_res.alloc((size_t)nt * 4 * sizeof(double));
    }
    for_each_eval_pass(sp, test_idx, true, [&](const EvalPass& p) {
        dvs_metrics_view mv[DVS_METRICS_MAX_VIEWS] = {};
        for (int k = 0; k < p.nb; ++k) {
            const size_t ci = (size_t)p.cam[k];
            mv[k].img = p.images + (size_t)k * img;
            mv[k].target = view_pixels(ci);
            mv[k].mask = view_mask(ci);
        }
        if (cfg.enableFocusRegion) {        // what the loss saw: the camera's mask x the region's hit
            const float* in[DVS_METRICS_MAX_VIEWS];
            for (int k = 0; k < p.nb; ++k) in[k] = mv[k].mask;
            const float* rm = region_masks(p.cams, in, p.nb, W, H);
            for (int k = 0; k < p.nb; ++k) mv[k].mask = rm + (size_t)k * W * H;
        }
        DVS_OR_THROW(dvs_image_metrics_views(stream.get(), mv, p.nb, W, H, views_u8() ? 1 : 0, d_eval_scratch.get(), d_eval_res.get() + (size_t)p.first * 4));
    });
    res.assign((size_t)nt * 4, 0.0);
    HIP_OR_THROW(hipMemcpyAsync(res.data(), d_eval_res.get(), res.size() * sizeof(double), hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    for (int k = 0; k < 4; ++k) {
        double a = 0.0;
        for (int v = 0; v < nt; ++v) a += res[(size_t)v * 4 + k];
        mean[k] = a / nt;
    }
}
// <modelPath>_<it>_eval.json: the last evaluation, every double with 17 significant digits (they read back bit for bit)
void GaussianTrainerScene::Impl::write_eval_json() const {
    const int nt = (int)test_idx.size();
    const std::string file = save_path(step, "_eval.json");
    FILE* f = fopen(file.c_str(), "w");
    if (!f) { logf_("evaluation: cannot write %s", file.c_str()); return; }
    fprintf(f, "{\n  \"iteration\": %d,\n  \"n_splats\": %d,\n  \"sh_degree\": %d,\n  \"holdout\": %d,\n  \"views\": [\n", step, n, sh_max, eval_holdout);
    for (int v = 0; v < nt; ++v) {
        const double* r = &eval_res[(size_t)v * 4];
        fprintf(f, "    {\"camera\": %d, \"psnr\": %.17g, \"ssim\": %.17g, \"l1\": %.17g, \"mse\": %.17g}%s\n", test_idx[(size_t)v], r[3], r[2], r[1], r[0],
                v + 1 < nt ? "," : "");
    }
    fprintf(f, "  ],\n  \"mean\": {\"psnr\": %.17g, \"ssim\": %.17g, \"l1\": %.17g, \"mse\": %.17g}", eval_mean[3], eval_mean[2], eval_mean[1], eval_mean[0]);
    bool any = false;                                                       // the decoded models' means, scored by this save's exports
    for (const DecodedScore& s : decoded_score) {
        if (s.it != step) continue;
        fprintf(f, "%s\"%s\": {\"psnr\": %.17g, \"ssim\": %.17g, \"l1\": %.17g, \"mse\": %.17g}", any ? ", " : ",\n  \"exports\": {", s.name, s.mean[3],
                s.mean[2], s.mean[1], s.mean[0]);
        any = true;
    }
    if (any) fprintf(f, "}");
    any = false;                                                            // the LOD levels of this save (LOD export on)
    for (int k = 0; k < 4; ++k) {
        const LodScore& s = lod_score[k];
        if (s.it != step) continue;
        fprintf(f, "%s\"%d\": {\"n_splats\": %d, \"psnr\": %.17g, \"ssim\": %.17g, \"l1\": %.17g, \"mse\": %.17g}", any ? ", " : ",\n  \"lod\": {", k + 1, s.m,
                s.mean[3], s.mean[2], s.mean[1], s.mean[0]);
        any = true;
    }
    if (any) fprintf(f, "}");
    fprintf(f, "\n}\n");
    fclose(f);
}

// The sky texture: allocated (zero: the first forward is the image over black) when enableBg is on; a resume reads <modelPath>_<it>.sky
// when it is there and fits the configured size, else starts from zero and says so.
void GaussianTrainerScene::Impl::setup_sky(bool resumed) {
    sky_on = cfg.enableBg;
    if (!sky_on) return;
    sky_h = std::min(1024, std::max(16, opt.i(gsopt::SKY_RESOLUTION)));
    const size_t bytes = sky_floats() * sizeof(float);
    for (DevBuf<float>* b : {&d_sky, &d_sky_m, &d_sky_v, &d_sky_grad}) { b->alloc(bytes); HIP_OR_THROW(hipMemset(b->get(), 0, bytes)); }
    d_sky_rgb.alloc((size_t)vpi * 3 * (size_t)W * H * sizeof(float));
    if (!resumed) return;
    uint32_t w = 0, h = 0; std::vector<float> tex; std::string err;
    const std::string file = sky_file(loadItr);
    if (!gssky::read_sky(file, &w, &h, &tex, &err)) { logf_("sky: could not read %s (%s): the texture starts from zero", file.c_str(), err.c_str()); return; }
    if ((int)h != sky_h) { logf_("sky: %s is %ux%u, this run asks for %dx%d: the texture starts from zero", file.c_str(), w, h, 2 * sky_h, sky_h); return; }
    HIP_OR_THROW(hipMemcpy(d_sky.get(), tex.data(), bytes, hipMemcpyHostToDevice));
    logf_("sky: read the %ux%u texture from %s", w, h, file.c_str());
}
void GaussianTrainerScene::Impl::save_sky() {
    if (!sky_on) return;
    std::vector<float> tex(sky_floats());
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    HIP_OR_THROW(hipMemcpy(tex.data(), d_sky.get(), tex.size() * sizeof(float), hipMemcpyDeviceToHost));
    const std::string file = sky_file(step) + (rank != 0 ? ".rank" + std::to_string(rank) : std::string());      // (the PLY's convention)
    std::string err;
    if (!gssky::write_sky(file, (uint32_t)(2 * sky_h), (uint32_t)sky_h, tex.data(), &err)) logf_("save_splat_model: %s", err.c_str());
    else if (cfg.verbose) logf_("saved the %dx%d sky texture to %s", 2 * sky_h, sky_h, file.c_str());
}

void GaussianTrainerScene::Impl::fetch_host() {
    if (host_valid) return;
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    for (int g = 0; g < 6; ++g) {
        host[g].resize((size_t)n * kWidth[g]);             // host copies are always in the reference layout (update_from_cpu)
        DevBuf<float> rows;                                 // (shN: back in the reference layout first)
        if (g == P_SHN) {
            rows.alloc(host[g].size() * sizeof(float) + 4);
            DVS_OR_THROW(dvs_shn_relayout(ctx.get(), stream.get(), n, d_param[g].get(), rows.get(), 0));
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        }
        HIP_OR_THROW(hipMemcpy(host[g].data(), rows ? rows.get() : d_param[g].get(), host[g].size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    host_valid = true;
}

// The tail of a compact export, after its packer: the payload to the host, the file ...
long long GaussianTrainerScene::Impl::write_payload(size_t bytes, const std::string& file, size_t unknown_size, const std::function<bool(std::string*)>& write) {
    if (export_host.size() < bytes) export_host.resize(bytes);
    HIP_OR_THROW(hipMemcpyAsync(export_host.data(), d_export_out.get(), bytes, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    std::string err;
    if (!write(&err)) { logf_("export @%d: %s", step, err.c_str()); return -1; }
    std::error_code ec;
    const auto file_bytes = std::filesystem::file_size(file, ec);
    return (long long)(ec ? unknown_size : file_bytes);
}
// ... and the log line of the simple formats
bool GaussianTrainerScene::Impl::write_export(std::chrono::steady_clock::time_point t_start, size_t bytes, const std::string& file, const char* word,
                                              size_t unknown_size, const std::function<bool(std::string*)>& write) {
    const long long on_disk = write_payload(bytes, file, unknown_size, write);
    if (on_disk >= 0) logf_("export @%d: %s %d splats, %llu bytes, %.2f ms", step, word, n, (unsigned long long)on_disk, ms_since(t_start));
    return on_disk >= 0;
}
// The ending of an export whose payload can be decoded (trainer.hpp): what the compact file costs in dB. The score is reported beside
// the full model's (log line, "exports" in the eval JSON) and never replaces it.
void GaussianTrainerScene::Impl::score_decoded(int format, const char* unpacker, const std::function<int()>& unpack) {
    if (test_idx.empty() || rank != 0) return;
    for (int g = 0; g < 6; ++g) d_decoded[g].reserve(dev_floats_for(g, n) * sizeof(float) + 16);
    if (const int rc = unpack(); rc != DVS_OK) throw std::runtime_error(std::string(unpacker) + ": status " + std::to_string(rc));
    if (xf_filled) {                                                        // the payload is in the export frame: back, in place, to the cameras' frame
        const int rc = dvs_transform_splats(stream.get(), n, sh_max, &xf_inv, xf_inv_D, d_decoded[P_POS].get(), d_decoded[P_SHN].get(), DVS_SHN_TILED,
                                            d_decoded[P_SCALE].get(), d_decoded[P_ROT].get(), d_decoded[P_POS].get(), d_decoded[P_SHN].get(),
                                            d_decoded[P_SCALE].get(), d_decoded[P_ROT].get());
        if (rc != DVS_OK) throw std::runtime_error("dvs_transform_splats (inverse): status " + std::to_string(rc));
    }
    if (eval_it != step) run_evaluation();                                  // the full model of the same parameters: the comparison
    DecodedScore& s = decoded_score[format];
    std::vector<double> res;
    score_views(splats_of(d_decoded, n), res, s.mean);
    s.it = step;
    logf_("export @%d: %s decoded model: PSNR %.17g dB (full model %.17g dB), SSIM %.17g, L1 %.17g", step, s.name, s.mean[3], eval_mean[3], s.mean[2], s.mean[1]);
}

// One compact export of the current model: packed on the training stream from the device arrays (shN is not read, so its tiled layout
// does not matter), the packed payload alone copied to the host and written to <modelPath>_<step>.compressed.ply / .splat.
void GaussianTrainerScene::Impl::export_model(int format) {
    if (format == EXPORT_SPZ) { export_spz(); return; }
    if (format == EXPORT_REDUCED) { export_reduced(); return; }
    if (format == EXPORT_TRANSFORMED) { export_transformed(); return; }
    if (format == EXPORT_FUSED) { export_fused(); return; }
    const auto t_start = std::chrono::steady_clock::now();
    const bool compressed = format == EXPORT_COMPRESSED;
    const size_t n_chunks = ((size_t)n + 255) / 256;
    const size_t chunk_bytes = n_chunks * 12 * sizeof(float);              // (a multiple of 16: the vertex records follow on a 16-byte boundary)
    const size_t bytes = compressed ? chunk_bytes + (size_t)n * 16 : (size_t)n * 32;
    d_export_out.reserve(bytes);
    const float *pos = ex(P_POS), *sh0 = ex(P_SH0), *opa = ex(P_OPA), *scale = ex(P_SCALE), *rot = ex(P_ROT);
    uint8_t* const out = d_export_out.get();
    int status;
    if (compressed) {
        d_export_scratch.reserve(dvs_pack_scratch_bytes(n));
        status = dvs_pack_compressed(stream.get(), n, pos, sh0, opa, scale, rot, d_export_scratch.get(), (float*)out, (uint32_t*)(out + chunk_bytes), nullptr);
    } else {
        status = dvs_pack_splat32(stream.get(), n, pos, sh0, opa, scale, rot, out);
    }
    if (status != DVS_OK) throw std::runtime_error(std::string(compressed ? "dvs_pack_compressed" : "dvs_pack_splat32") + ": status " + std::to_string(status));
    const std::string file = save_path(step, compressed ? ".compressed.ply" : ".splat");
    write_export(t_start, bytes, file, compressed ? "compressed.ply" : "splat", bytes, [&](std::string* err) {
        return compressed ? gsply::write_compressed_ply(file, (size_t)n, (const float*)export_host.data(),
                                                        (const uint32_t*)(export_host.data() + chunk_bytes), cfg.mipAntiliased, err)
                          : gsply::write_splat(file, (size_t)n, export_host.data(), err);
    });
}

// The .spz export: the six sections packed from the tiled arrays at the model's sh_max (the one compact format that keeps the
// higher SH bands), layout.total bytes copied to the host, gzipped into <modelPath>_<step>.spz. With evaluation on, the device payload
// is then decoded into a second parameter set and scored on the test cameras (score_decoded).
void GaussianTrainerScene::Impl::export_spz() {
    const auto t_start = std::chrono::steady_clock::now();
    dvs_spz_layout layout;
    if (dvs_spz_layout_for(n, sh_max, &layout) != DVS_OK) throw std::runtime_error("dvs_spz_layout_for: invalid arguments");
    const size_t bytes = (size_t)layout.total;
    d_export_out.reserve(bytes);
    const int status = dvs_pack_spz(stream.get(), n, sh_max, ex(P_POS), ex(P_SH0), ex(P_SHN), DVS_SHN_TILED, ex(P_OPA), ex(P_SCALE), ex(P_ROT),
                                    d_export_out.get());
    if (status != DVS_OK) throw std::runtime_error("dvs_pack_spz: status " + std::to_string(status));
    const std::string file = save_path(step, ".spz");
    if (!write_export(t_start, bytes, file, "spz", 0, [&](std::string* err) {
            return gsply::write_spz(file, (size_t)n, sh_max, cfg.mipAntiliased, export_host.data(), layout, err);
        })) return;
    score_decoded(SCORED_SPZ, "dvs_unpack_spz", [&] {
        return dvs_unpack_spz(stream.get(), n, sh_max, d_export_out.get(), d_decoded[P_POS].get(), d_decoded[P_SH0].get(), d_decoded[P_SHN].get(),
                              DVS_SHN_TILED, d_decoded[P_OPA].get(), d_decoded[P_SCALE].get(), d_decoded[P_ROT].get());
    });
}

// The .reduced.ply export (include/dvs_export.h, last section): per-splat degrees — dvs_sh_degree_select over the training cameras'
// centres with cullSH, else the model's SH degree (sh_max) for every splat —, the twenty codebooks, the block counts (16 bytes to the host, for
// the layout), the payload; only the payload with its 20 KB table crosses to the host. Rank 0, on the training stream. With evaluation
// on, the device payload is decoded into the second parameter set and scored like the .spz one.
void GaussianTrainerScene::Impl::export_reduced() {
    auto t0 = std::chrono::steady_clock::now();
    const int D = sh_max, half = opt.on(gsopt::REDUCED_HALF) ? 1 : 0;   // the degree the full PLY stores and the evaluation renders (as the .spz export)
    const std::vector<int> tc = training_cameras();
    const size_t o_iters = (size_t)DVS_REDUCED_BOOKS * DVS_REDUCED_ENTRIES * sizeof(float), o_counts = o_iters + 96, o_cams = o_counts + 16;
    d_export_scratch.reserve(dvs_reduced_scratch_bytes(n));
    d_red_degree.reserve(((size_t)n + 15) & ~(size_t)15);
    d_red_small.reserve(o_cams + ((tc.size() * 3 * sizeof(float) + 15) & ~(size_t)15));
    uint8_t* const small = d_red_small.get();
    float* const centres = (float*)small;
    int32_t* const iters = (int32_t*)(small + o_iters);
    uint32_t* const counts = (uint32_t*)(small + o_counts);
    // (with an export transform: degrees are selected on the model as trained, against the real camera centres; codebooks and payload
    // come from the transformed set)
    const float *pos = ex(P_POS), *sh0 = ex(P_SH0), *shN = ex(P_SHN), *opa = ex(P_OPA), *scale = ex(P_SCALE), *rot = ex(P_ROT);
    const auto check = [](int status, const char* what) { if (status != DVS_OK) throw std::runtime_error(std::string(what) + ": status " + std::to_string(status)); };
    if (cfg.cullSH && D > 0) {
        std::vector<float> centre(tc.size() * 3);
        for (size_t k = 0; k < tc.size(); ++k) for (int a = 0; a < 3; ++a) centre[3 * k + a] = cams[(size_t)tc[k]].campos[a];
        HIP_OR_THROW(hipMemcpyAsync(small + o_cams, centre.data(), centre.size() * sizeof(float), hipMemcpyHostToDevice, stream.get()));
        check(dvs_sh_degree_select(stream.get(), n, D, d_param[P_POS].get(), d_param[P_SHN].get(), DVS_SHN_TILED, (const float*)(small + o_cams), (int)tc.size(), opt.f(gsopt::SH_CULL_THRESHOLD),
                                   d_red_degree.get()), "dvs_sh_degree_select");
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));                    // (also: `centre` leaves scope)
    } else {
        HIP_OR_THROW(hipMemsetAsync(d_red_degree.get(), D, (size_t)n, stream.get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    }
    const double ms_select = ms_since(t0);
    auto t1 = std::chrono::steady_clock::now();
    check(dvs_codebooks_build(stream.get(), n, sh0, shN, DVS_SHN_TILED, opa, scale, rot, d_red_degree.get(), 100, d_export_scratch.get(), centres, iters),
          "dvs_codebooks_build");
    check(dvs_reduced_degree_counts(stream.get(), n, d_red_degree.get(), d_export_scratch.get(), counts), "dvs_reduced_degree_counts");
    int32_t h_iters[DVS_REDUCED_BOOKS];
    uint32_t h_counts[4];
    HIP_OR_THROW(hipMemcpyAsync(h_iters, iters, sizeof h_iters, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const double ms_books = ms_since(t1);
    auto t2 = std::chrono::steady_clock::now();
    dvs_reduced_layout layout;
    check(dvs_reduced_layout_for(h_counts, half, &layout), "dvs_reduced_layout_for");
    const size_t bytes = (size_t)layout.total;
    d_export_out.reserve(bytes);
    check(dvs_pack_reduced(stream.get(), n, pos, sh0, shN, DVS_SHN_TILED, opa, scale, rot, d_red_degree.get(), centres, d_export_scratch.get(), &layout,
                           d_export_out.get()), "dvs_pack_reduced");
    const std::string file = save_path(step, ".reduced.ply");
    double ms_pack = 0.0;
    const long long on_disk = write_payload(bytes, file, bytes, [&](std::string* err) {
        ms_pack = ms_since(t2);                                             // the payload is on the host: the pack time ends before the file is written
        return gsply::write_reduced_ply(file, &layout, export_host.data(), bytes, err);
    });
    if (on_disk < 0) return;
    int most = 0;
    for (int it : h_iters) most = std::max(most, it);
    logf_("export @%d: reduced %d splats (%u/%u/%u/%u by degree), %llu bytes, degree select %.2f ms, codebooks %.2f ms (%d iterations at most), pack %.2f ms",
          step, n, h_counts[0], h_counts[1], h_counts[2], h_counts[3], (unsigned long long)on_disk, ms_select, ms_books, most, ms_pack);
    score_decoded(SCORED_REDUCED, "dvs_unpack_reduced", [&] {
        return dvs_unpack_reduced(stream.get(), n, d_export_out.get(), &layout, d_decoded[P_POS].get(), d_decoded[P_SH0].get(), d_decoded[P_SHN].get(),
                                  DVS_SHN_TILED, d_decoded[P_OPA].get(), d_decoded[P_SCALE].get(), d_decoded[P_ROT].get(), nullptr);
    });
}

// ---- export frame (trainer.hpp; INTEGRATION.md "Export frame") ------------------------------------------------------------------------
// Accepts a similarity: its band matrices and its inverse (with the inverse's matrices) are made once, here. -> false (logged, the
// previous state stays) when the host helpers refuse it.
bool GaussianTrainerScene::Impl::set_export_transform(const dvs_similarity& m, const std::string& how) {
    dvs_similarity inv;
    float D[83], Di[83];
    if (dvs_similarity_inverse(&m, &inv) != DVS_OK || dvs_sh_rotation(m.R, D) != DVS_OK || dvs_sh_rotation(inv.R, Di) != DVS_OK) {
        logf_("exportTransform: %s is not a similarity (a rotation, a finite translation, a scale > 0; non-uniform scale and shear cannot be "
              "represented by splats): ignored", how.c_str());
        return false;
    }
    xf = m; xf_inv = inv; xf_how = how; xf_set = true;
    memcpy(xf_D, D, sizeof D); memcpy(xf_inv_D, Di, sizeof Di);
    return true;
}
// R, t from the training cameras (export_frame.hpp), s = 1. -> false (logged, exports stay untransformed) when it is refused.
bool GaussianTrainerScene::Impl::set_export_orientation(const char* axis, const char* from) {
    double a[3], R[9], t[3], up[3];
    if (!gsframe::parse_axis(axis, a)) { logf_("exportTransform: %s '%s' is not one of +x -x +y -y +z -z: ignored", from, axis ? axis : ""); return false; }
    const std::vector<int> tc = training_cameras();
    std::vector<float> views(tc.size() * 16), centres(tc.size() * 3);
    for (size_t k = 0; k < tc.size(); ++k) {
        memcpy(&views[16 * k], cams[(size_t)tc[k]].view, 16 * sizeof(float));
        memcpy(&centres[3 * k], cams[(size_t)tc[k]].campos, 3 * sizeof(float));
    }
    std::string err;
    if (!gsframe::orientation(tc.size(), views.data(), centres.data(), a, R, t, up, &err)) {
        logf_("exportTransform: %s %s refused: %s; exports stay in the training frame", from, axis, err.c_str());
        return false;
    }
    dvs_similarity m;
    for (int k = 0; k < 9; ++k) m.R[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) m.t[k] = (float)t[k];
    m.s = 1.0f;
    char how[256];
    snprintf(how, sizeof how, "%s %s: the mean image-up vector (%.6g, %.6g, %.6g) of %zu training cameras turned onto the axis by the shortest arc, "
             "their centroid moved to the origin", from, axis, up[0], up[1], up[2], tc.size());
    return set_export_transform(m, how);
}
// opt's EXPORT_TRANSFORM = tx,ty,tz,rx,ry,rz,s (Euler angles in radians, R = Rz Ry Rx) / EXPORT_ORIENT, as the environment gave them: taken
// at load, once the cameras are there
void GaussianTrainerScene::Impl::setup_export_transform() {
    const bool et = opt.given[gsopt::EXPORT_TRANSFORM], eo = opt.given[gsopt::EXPORT_ORIENT];
    if (gsopt::two_export_frames(et, eo)) logf_("exportTransform: DVS_EXPORT_TRANSFORM and DVS_EXPORT_ORIENT are both set: DVS_EXPORT_TRANSFORM is used");
    if (et) {
        float v[7];
        for (int k = 0; k < 7; ++k) v[k] = opt.f(gsopt::EXPORT_TRANSFORM, k);
        dvs_similarity m;
        DVS_OR_THROW(dvs_similarity_from_trs(v, v + 3, v[6], &m));          // (finite, s > 0: the row's grammar)
        set_export_transform(m, "DVS_EXPORT_TRANSFORM=" + opt.text[gsopt::EXPORT_TRANSFORM] + " (T R S, R = Rz Ry Rx, radians)");
    } else if (eo) {
        set_export_orientation(opt.text[gsopt::EXPORT_ORIENT].c_str(), "DVS_EXPORT_ORIENT");
    }
}
void GaussianTrainerScene::Impl::report_export_transform() const {
    if (!xf_set || rank != 0) return;
    logf_("config: exportTransform p' = s R p + t with R = [%.9g %.9g %.9g; %.9g %.9g %.9g; %.9g %.9g %.9g], t = (%.9g, %.9g, %.9g), s = %.9g, from %s: "
          "every export but the resume PLY <modelPath>_<it>.ply is written in this frame (positions, scales, rotations and the SH bands above 0 "
          "transformed on the device)%s; decoded payloads are taken back by the inverse before they are scored; the mesh shares the frame",
          (double)xf.R[0], (double)xf.R[1], (double)xf.R[2], (double)xf.R[3], (double)xf.R[4], (double)xf.R[5], (double)xf.R[6], (double)xf.R[7],
          (double)xf.R[8], (double)xf.t[0], (double)xf.t[1], (double)xf.t[2], (double)xf.s, xf_how.c_str(),
          (export_formats() & EXPORT_TRANSFORMED) ? "; <modelPath>_<it>.transformed.ply is the full PLY in it" : "");
    if (cfg.enableBg) logf_("config: exportTransform: the sky texture <modelPath>_<it>.sky is written in the TRAINING frame (resampling it is out of scope)");
}
// this save's transformed set: one launch on the training stream at the model's SH degree
void GaussianTrainerScene::Impl::fill_transformed() {
    const auto t_start = std::chrono::steady_clock::now();
    for (int g : {(int)P_POS, (int)P_SHN, (int)P_SCALE, (int)P_ROT}) d_xf[xf_slot(g)].reserve(dev_floats_for(g, n) * sizeof(float) + 16);
    const int rc = dvs_transform_splats(stream.get(), n, sh_max, &xf, xf_D, d_param[P_POS].get(), d_param[P_SHN].get(), DVS_SHN_TILED,
                                        model_ex(P_SCALE), d_param[P_ROT].get(), d_xf[0].get(), d_xf[1].get(), d_xf[2].get(), d_xf[3].get());
    if (rc != DVS_OK) throw std::runtime_error("dvs_transform_splats: status " + std::to_string(rc));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    xf_filled = true;
    logf_("export @%d: transform %d splats, %.2f ms", step, n, ms_since(t_start));
}
// <modelPath>_<it>.transformed.ply: the full PLY's wire format from the transformed set (sh0 and opacity: the host copies of the save)
void GaussianTrainerScene::Impl::export_transformed() {
    const auto t_start = std::chrono::steady_clock::now();
    fetch_host();
    std::vector<float> h[4];
    const size_t rows = (size_t)n * 45;
    d_xf_rows.reserve(rows * sizeof(float) + 16);
    DVS_OR_THROW(dvs_shn_relayout(ctx.get(), stream.get(), n, d_xf[1].get(), d_xf_rows.get(), 0));
    const float* src[4] = {d_xf[0].get(), d_xf_rows.get(), d_xf[2].get(), d_xf[3].get()};
    const size_t floats[4] = {(size_t)n * 3, rows, (size_t)n * 3, (size_t)n * 4};
    for (int k = 0; k < 4; ++k) {
        h[k].resize(floats[k]);
        HIP_OR_THROW(hipMemcpyAsync(h[k].data(), src[k], floats[k] * sizeof(float), hipMemcpyDeviceToHost, stream.get()));
    }
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const std::string file = save_path(step, ".transformed.ply");
    std::string err;
    std::vector<float> fused_opacity;                                        // mipFilter3d: the exports hold the fused model (the frame leaves opacity alone)
    if (f3d_on) {
        fused_opacity.resize((size_t)n);
        HIP_OR_THROW(hipMemcpy(fused_opacity.data(), ex(P_OPA), fused_opacity.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    const float* const opacity = f3d_on ? fused_opacity.data() : host[P_OPA].data();
    if (!gsply::write_ply(file, (size_t)n, h[0].data(), host[P_SH0].data(), h[1].data(), opacity, h[2].data(), h[3].data(), cfg.mipAntiliased, &err)) {
        logf_("export @%d: %s", step, err.c_str());
        return;
    }
    std::error_code ec;
    const auto bytes = std::filesystem::file_size(file, ec);
    logf_("export @%d: transformed.ply %d splats, %llu bytes, %.2f ms", step, n, (unsigned long long)(ec ? 0 : bytes), ms_since(t_start));
}
