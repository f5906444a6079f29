// trainer_load.cpp — load_train_data: the allocations and the set-up both loaders share (create_context, store_view, setup_*, finish_load) and
// the synthetic-scene loader. The capture-directory loader is trainer_dataset.cpp.
#include "trainer.hpp"

namespace {
__global__ void k_pack_u8(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint8_t)fminf(255.f, fmaxf(0.f, rintf(src[i] * 255.f)));
}

struct Lcg {       // tiny deterministic noise source for the synthetic initialisation
    uint64_t s;
    explicit Lcg(uint64_t seed) : s(seed * 6364136223846793005ULL + 1442695040888963407ULL) {}
    float uni() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (float)((s >> 40) * (1.0 / 16777216.0)); }
    float sym() { return 2.f * uni() - 1.f; }
};
}  // namespace

void GaussianTrainerScene::Impl::upload(int g, const std::vector<float>& host_rows) {
    if (g != P_SHN) { HIP_OR_THROW(hipMemcpy(d_param[g].get(), host_rows.data(), host_rows.size() * sizeof(float), hipMemcpyHostToDevice)); return; }
    DevBuf<float> tmp(host_rows.size() * sizeof(float) + 4);
    HIP_OR_THROW(hipMemcpy(tmp.get(), host_rows.data(), host_rows.size() * sizeof(float), hipMemcpyHostToDevice));
    DVS_OR_THROW(dvs_shn_relayout(ctx.get(), stream.get(), n, tmp.get(), d_param[g].get(), 1));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
}

void GaussianTrainerScene::Impl::alloc_params(int count, int capacity, const std::vector<float> init[6]) {
    n = count; cap = std::max(capacity, count);
    grad_floats = 0;
    size_t goff[6];
    static const int order[6] = {P_POS, P_OPA, P_SCALE, P_ROT, P_SH0, P_SHN};       // geometry first: one contiguous all-reduce
    for (int k = 0; k < 6; ++k) {
        const int g = order[k];
        if (g == P_SH0) geom_floats = grad_floats;
        goff[g] = grad_floats; grad_floats += (dev_floats_for(g, cap) + 3) & ~(size_t)3;                            // 16-B aligned groups
    }
    d_grad_flat.alloc(grad_floats * sizeof(float) + 16);
    HIP_OR_THROW(hipMemset(d_grad_flat.get(), 0, grad_floats * sizeof(float)));
    for (int g = 0; g < 6; ++g) d_grad[g] = d_grad_flat.get() + goff[g];
    d_mean2d.alloc((size_t)cap * 2 * sizeof(float) + 4);
    for (int g = 0; g < 6; ++g) {
        const size_t bytes = dev_floats_for(g, cap) * sizeof(float);
        for (DevBuf<float>* p : {&d_param[g], &d_m[g], &d_v[g], &d_param2[g], &d_m2[g], &d_v2[g]}) {
            p->alloc(bytes ? bytes : 4);
            HIP_OR_THROW(hipMemset(p->get(), 0, bytes));       // pad lanes of the last tile are never written: keep them zero
        }
        upload(g, init[g]);
    }
    d_absgrad.alloc((size_t)cap * 2 * sizeof(float) + 4);
    d_grad_accum.alloc((size_t)cap * 4 + 4); d_denom.alloc((size_t)cap * 4 + 4);
    d_max_radii.alloc((size_t)cap * 4 + 4); d_action.alloc((size_t)cap + 4);
    d_offsets.alloc((size_t)cap * 4 + 4); d_dscratch.alloc(((size_t)cap / 256 + 8) * 4);
    d_newcount.alloc(8);
    d_mcmc.alloc(dvs_mcmc_scratch_bytes(cap));
    DVS_OR_THROW(dvs_mcmc_init_scratch(stream.get(), d_mcmc.get(), cap));
    reset_stats();
}

void GaussianTrainerScene::Impl::create_context(int count, int capacity, const std::vector<float> init[6]) {
    f3d_on = false;                                                          // (decided in finish_load: a loader renders through splats() before)
    vpi = std::max(1, std::min(env_int("DVS_VIEWS_PER_ITER", cfg.viewsPerIter), 16));
    sequential_views = env_is("DVS_VIEWS_MODE", "sequential");
    if (vpi > 1 && rank == 0)
        logf_("config: %d views per trainStep and GPU, %s", vpi, sequential_views ? "one pass per view, gradients accumulated (DVS_VIEWS_MODE=sequential)"
                                                                                : "ONE multi-view pass (dvs_raster_forward_views / _backward_views), gradients summed");
    ctx.reset(dvs_create_views(device, (size_t)capacity, W, H, sequential_views ? 1 : vpi));
    if (!ctx) throw std::runtime_error(std::string("dvs_create_views: ") + dvs_last_error());
    alloc_params(count, capacity, init);
    const size_t img = 3 * (size_t)W * H;
    d_out.alloc((size_t)vpi * img * sizeof(float));
    d_dL.alloc((size_t)vpi * img * sizeof(float));
    d_loss.alloc(2 * DVS_SSIM_SLOTS * sizeof(float));
    HIP_OR_THROW(hipMemset(d_loss.get(), 0, 2 * DVS_SSIM_SLOTS * sizeof(float)));
    if (cfg.ssimWeight > 0.f)
        for (int k = 0; k < 3; ++k) d_ssim_maps[k].alloc(img * sizeof(float));
}

// One more training view (the caller appends its camera to `cams`): the fp32 image as it is or, when the views are kept as bytes,
// packed to 8 bits per channel — the stream is synchronised there and the fp32 copy dropped.
void GaussianTrainerScene::Impl::store_view(DevBuf<float> image, DevBuf<float> mask) {
    View v;
    v.mask = std::move(mask);
    if (views_u8()) {
        const size_t img = 3 * (size_t)W * H;
        v.u8.alloc(img);
        hipLaunchKernelGGL(k_pack_u8, dim3((unsigned)((img + 255) / 256)), dim3(256), 0, stream.get(), image.get(), v.u8.get(), img);
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    } else {
        v.f32 = std::move(image);
    }
    views.push_back(std::move(v));
}

// the train / test split of cfg.evalHoldout (DVS_EVAL_HOLDOUT): a function of the camera index alone, so every rank derives the same one
void GaussianTrainerScene::Impl::setup_split() {
    eval_holdout = env_int("DVS_EVAL_HOLDOUT", cfg.evalHoldout); eval_every = env_int("DVS_EVAL_EVERY", cfg.evalEvery);
    loss_every = std::max(1, env_int("DVS_LOSS_EVERY", 100));
    train_idx.clear(); test_idx.clear();
    if (eval_holdout <= 0) { eval_holdout = 0; return; }
    for (int c = 0; c < (int)cams.size(); ++c) (c % eval_holdout == 0 ? test_idx : train_idx).push_back(c);
    if (train_idx.empty() || test_idx.empty()) {
        if (rank == 0)
            logf_("evaluation is OFF: evalHoldout %d over %zu cameras leaves %zu to train on and %zu to test on; training on every camera",
                  eval_holdout, cams.size(), train_idx.size(), test_idx.size());
        train_idx.clear(); test_idx.clear(); eval_holdout = 0;
    }
}

// cfg.resolutionSchedule / numDownscales (DVS_RESOLUTION_SCHEDULE / DVS_NUM_DOWNSCALES): K clamped once to the largest value that leaves
// min(W, H) >> K >= 16 (and to the factor 8 of dvs_downsample_views); level cameras of every (camera, level) and the staging buffers
void GaussianTrainerScene::Impl::setup_levels() {
    res_every = env_int("DVS_RESOLUTION_SCHEDULE", cfg.resolutionSchedule); res_levels = env_int("DVS_NUM_DOWNSCALES", cfg.numDownscales);
    lw = W; lh = H; cur_level = -1;
    if (res_every <= 0) { res_every = 0; res_levels = 0; return; }
    int k = std::max(0, std::min(res_levels, 3));
    while (k > 0 && (std::min(W, H) >> k) < 16) --k;
    if (k != res_levels && rank == 0)
        logf_("resolutionSchedule: numDownscales %d clamped to %d (levels 1/2 .. 1/8, the smaller side of %dx%d stays >= 16 pixels)", res_levels, k, W, H);
    res_levels = k;
    level_cams.assign((size_t)res_levels, std::vector<dvs_camera>(cams.size()));
    for (int l = 1; l <= res_levels; ++l)
        for (size_t c = 0; c < cams.size(); ++c) DVS_OR_THROW(dvs_camera_downscale(&cams[c], 1 << l, &level_cams[(size_t)l - 1][c]));
    if (res_levels == 0) return;
    const size_t P = (size_t)(W / 2) * (size_t)(H / 2);
    d_level_targets.alloc((size_t)vpi * 3 * P * sizeof(float) + 16);
    if (cfg.useMask || undistorted) d_level_masks.alloc((size_t)vpi * P * sizeof(float) + 16);
}

// factorised exchange: the SH rows are not written by the backward, only each view's colour gradient, which leaves right after
// the composite backward (dvs_raster_backward_dcolor) so that its all-gather runs on the communication stream while A9 computes
void GaussianTrainerScene::Impl::setup_exchange() {
    d_dcolor_local.alloc((size_t)vpi * cap * 3 * sizeof(float) + 16);
    d_dcolor_scratch.alloc((size_t)vpi * cap * 3 * sizeof(float) + 16);
    d_dcolor_all.alloc((size_t)world * vpi * cap * 3 * sizeof(float) + 16);
    hipStream_t cs = nullptr;
    HIP_OR_THROW(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    comm_stream.reset(cs);
    const auto new_event = [] { hipEvent_t h = nullptr; HIP_OR_THROW(hipEventCreateWithFlags(&h, hipEventDisableTiming)); return Event(h); };
    for (Event* e : {&ev_dcolor, &ev_bwd, &ev_comm, &ev_gather}) *e = new_event();
    a9_chunks = std::max(1, std::min(64, env_int("DVS_A9_CHUNKS", a9_chunks)));
    pipeline = env_is("DVS_EXCHANGE_PIPELINE", "1") && a9_chunks > 1;
    ev_chunk.resize((size_t)a9_chunks); ev_ar.resize((size_t)a9_chunks);
    for (Event& e : ev_chunk) e = new_event();
    for (Event& e : ev_ar) e = new_event();
    if (rank == 0 && a9_chunks > 1)
        logf_("gradient exchange: A9 in %d splat chunks, each chunk's geometry all-reduce behind it%s", a9_chunks,
              pipeline ? "; PIPELINED across the iteration boundary: Adam and the next iteration's projection run chunk by chunk as the all-reduces land "
                         "(DVS_EXCHANGE_PIPELINE=1)" : "");
}

void GaussianTrainerScene::Impl::finish_load(const std::function<void(std::vector<float> (&)[6])>& fresh_init, const char* fresh_name,
                                             const std::function<void(bool)>& describe) {
    if (views_u8()) d_target_f32.alloc(3 * (size_t)W * H * sizeof(float));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    setup_split();
    setup_render();
    setup_levels();
    {   // scene extent = 1.1 x the largest distance of a camera centre from their mean (the usual "cameras_extent"); a single
        // camera or a tiny rig falls back to half the depth range of the synthetic slab
        double mean[3] = {0, 0, 0};
        for (auto& c : cams) for (int k = 0; k < 3; ++k) mean[k] += c.campos[k] / cams.size();
        double far = 0;
        for (auto& c : cams) { double d = 0; for (int k = 0; k < 3; ++k) d += (c.campos[k] - mean[k]) * (c.campos[k] - mean[k]); far = std::max(far, std::sqrt(d)); }
        extent = far > 1e-3 ? (float)(1.1 * far) : 5.0f;
    }
    std::vector<float> init[6];
    bool resumed = false;
    if (loadItr >= 0) {
        std::string err;
        resumed = gsply::read_ply(model_file(loadItr), init[0], init[1], init[2], init[3], init[4], init[5], &err) &&
                  !init[3].empty() && (int)init[3].size() <= cap;        // the count may differ from the loader's after densification
        if (resumed) n = (int)init[3].size();
        if (!resumed) logf_("could not resume from %s (%s): starting from the %s initialisation", model_file(loadItr).c_str(), err.c_str(), fresh_name);
        else step = loadItr;
    }
    if (!resumed) fresh_init(init);
    for (int g = 0; g < 6; ++g) { upload(g, init[g]); init_host[g] = init[g]; }
    setup_sky(resumed);
    setup_region();
    setup_export_transform();                                               // (DVS_EXPORT_TRANSFORM / DVS_EXPORT_ORIENT; needs the cameras)
    setup_filter3d();                                                       // (DVS_MIP_FILTER3D / setMipFilter3d; needs the split and the cameras)
    report_config();
    describe(resumed);
    if (cfg.enableFocusRegion) prune_region(step);
    region_dirty = false;
    filter3d_refresh();                                                      // the filter of the loaded or resumed splats, logged at load
    if (exchange_factorised()) setup_exchange();
}

bool GaussianTrainerScene::Impl::load_synthetic(const std::string& spec_str) {
    // "synthetic:N=100000,W=800,H=800,cams=8,sh=3,seed=1"
    std::map<std::string, double> kv = {{"N", 100000}, {"W", 800}, {"H", 800}, {"cams", 8}, {"sh", 3}, {"seed", 1}};
    size_t p = spec_str.find(':');
    std::string rest = p == std::string::npos ? "" : spec_str.substr(p + 1);
    while (!rest.empty()) {
        size_t c = rest.find(',');
        std::string item = rest.substr(0, c);
        rest = c == std::string::npos ? "" : rest.substr(c + 1);
        size_t e = item.find('=');
        if (e == std::string::npos) continue;
        kv[item.substr(0, e)] = atof(item.substr(e + 1).c_str());
    }
    dvs_scene_spec spec{};
    spec.n = (int)kv["N"]; spec.width = (int)kv["W"]; spec.height = (int)kv["H"]; spec.sh_degree = (int)kv["sh"];
    spec.n_cams = (int)kv["cams"]; spec.seed = (uint64_t)kv["seed"]; spec.fov_x_deg = 60.f; spec.scale_log_offset = 0.f;
    if (spec.n <= 0 || spec.width <= 0 || spec.height <= 0 || spec.n_cams <= 0 || spec.sh_degree < 0 || spec.sh_degree > 3) return false;
    if (spec.width > cfg.maxImageWidth || spec.height > cfg.maxImageHeight)
        logf_("note: synthetic image %dx%d exceeds maxImageWidth/Height %dx%d (kept as is)", spec.width, spec.height, cfg.maxImageWidth, cfg.maxImageHeight);
    W = spec.width; H = spec.height; sh_max = spec.sh_degree;
    std::vector<float> gt[6];
    for (int g = 0; g < 6; ++g) gt[g].resize((size_t)spec.n * kWidth[g]);
    DVS_OR_THROW(dvs_synth_splats(&spec, gt[0].data(), gt[1].data(), gt[2].data(), gt[3].data(), gt[4].data(), gt[5].data()));
    const int capacity = std::max(spec.n, cfg.capMax);          // --capMax is the array capacity (gs_train.cpp:89); 1.9 KB of HBM per splat
    // ground-truth views: render the generating scene once per camera
    create_context(spec.n, capacity, gt);
    const size_t img = 3 * (size_t)W * H;
    dvs_opts opts{sh_max, cfg.mipAntiliased ? 1 : 0, 0, 0, DVS_SHN_TILED};
    const dvs_splats sp = splats();
    for (int c = 0; c < spec.n_cams; ++c) {
        dvs_camera cam;
        DVS_OR_THROW(dvs_synth_camera(&spec, c, &cam));
        DevBuf<float> t(img * sizeof(float)), mask;
        DVS_OR_THROW(dvs_raster_forward(ctx.get(), stream.get(), &sp, &cam, &opts, t.get(), nullptr, nullptr));
        cams.push_back(cam);
        cam_names.emplace_back();                           // (a synthetic camera has no file: cam_%04d)
        if (cfg.useMask) {                                     // synthetic mask: an ellipse inscribed in the image (no dataset masks here)
            std::vector<float> mk((size_t)W * H);
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
                const float u = (x + 0.5f) / W * 2.f - 1.f, v = (y + 0.5f) / H * 2.f - 1.f;
                mk[(size_t)y * W + x] = (u * u + v * v <= 1.f) ? 1.f : 0.f;
            }
            mask.alloc(mk.size() * sizeof(float));
            HIP_OR_THROW(hipMemcpy(mask.get(), mk.data(), mk.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        store_view(std::move(t), std::move(mask));
    }
    // trainable initialisation = perturbed ground truth (or the checkpoint when --load_itr is given)
    finish_load([&](std::vector<float> (&init)[6]) {
        Lcg r(spec.seed + 17);
        for (int g = 0; g < 6; ++g) init[g] = gt[g];
        for (int i = 0; i < spec.n; ++i) {
            const float z = gt[0][3 * i + 2];
            for (int k = 0; k < 3; ++k) init[P_POS][3 * i + k] += 0.002f * z * r.sym();
            for (int k = 0; k < 3; ++k) init[P_SH0][3 * i + k] += 0.5f * r.sym();
            for (int k = 0; k < 45; ++k) init[P_SHN][45 * (size_t)i + k] = 0.f;
            init[P_OPA][i] -= 1.0f;
            for (int k = 0; k < 3; ++k) init[P_SCALE][3 * i + k] += 0.15f * r.sym();
        }
    }, "synthetic", [&](bool resumed) {
        if (cfg.verbose) logf_("synthetic scene: %d splats, %d cameras @ %dx%d, SH degree %d%s", spec.n, spec.n_cams, W, H, sh_max, resumed ? " (resumed)" : "");
    });
    return true;
}
