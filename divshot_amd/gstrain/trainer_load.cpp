// trainer_load.cpp — load_train_data: the synthetic-scene and capture-directory loaders and the allocations they share.
#include "trainer.hpp"
#include <condition_variable>
#include <mutex>
#include <thread>
#include "jpeg_io.hpp"
#include "png_io.hpp"
#include "../../include/dvs_image.h"

namespace {
__global__ void k_pack_u8(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint8_t)fminf(255.f, fmaxf(0.f, rintf(src[i] * 255.f)));
}

// Host threads that run the serial half of the compressed files of a capture ahead of the loader: entropy decoding is the serial cost of
// a JPEG and inflate that of a PNG (pictures and masks alike), so up to `threads` files are decoded at once, never more than `window`
// files beyond the one the loader has taken (the memory held is bounded by the window, not by the capture). take() hands the files out
// strictly in order, so nothing depends on the thread count.
class DecodeAhead {
public:
    struct Job { std::string file; bool png = false; };
    struct Result { gsjpeg::Frame frame; gspng::Frame png; std::string err; bool ok = false, done = false; };
    DecodeAhead(std::vector<Job> jobs, int threads) : jobs_(std::move(jobs)), slots_(jobs_.size()), window_(2 * (size_t)threads) {
        for (int t = 0; t < threads && (size_t)t < jobs_.size(); ++t) workers_.emplace_back([this] { work(); });
    }
    ~DecodeAhead() {
        { std::lock_guard<std::mutex> lock(m_); stop_ = true; }
        cv_.notify_all();
        for (std::thread& t : workers_) t.join();
    }
    Result take(size_t i) {                                  // i = 0, 1, 2, ... in this order
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [&] { return slots_[i].done; });
        Result r = std::move(slots_[i]);
        slots_[i] = Result();
        taken_ = i + 1;
        lock.unlock();
        cv_.notify_all();
        return r;
    }
    const std::string& file(size_t i) const { return jobs_[i].file; }
    double wall_ms(bool png) {                               // wall time during which at least one thread was decoding a file of that format: waits on a full window are not in it
        std::lock_guard<std::mutex> lock(m_);
        return busy_ms_[png ? 1 : 0];
    }

private:
    void work() {
        for (;;) {
            size_t i;
            int k;
            {
                std::unique_lock<std::mutex> lock(m_);
                cv_.wait(lock, [&] { return stop_ || next_ >= jobs_.size() || next_ < taken_ + window_; });
                if (stop_ || next_ >= jobs_.size()) return;
                i = next_++;
                k = jobs_[i].png ? 1 : 0;
                if (busy_[k]++ == 0) busy_since_[k] = std::chrono::steady_clock::now();
            }
            Result r;
            r.ok = k ? gspng::decode_filtered(jobs_[i].file, &r.png, &r.err) : gsjpeg::decode_coefficients(jobs_[i].file, &r.frame, &r.err);
            r.done = true;
            {
                std::lock_guard<std::mutex> lock(m_);
                slots_[i] = std::move(r);
                if (--busy_[k] == 0) busy_ms_[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - busy_since_[k]).count();
            }
            cv_.notify_all();
        }
    }
    const std::vector<Job> jobs_;
    std::vector<Result> slots_;
    size_t window_, next_ = 0, taken_ = 0;
    bool stop_ = false;
    int busy_[2] = {0, 0};                                   // threads inside a decode, per format (0 JPEG, 1 PNG)
    double busy_ms_[2] = {0, 0};
    std::chrono::steady_clock::time_point busy_since_[2];
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<std::thread> workers_;
};

dvs_png_desc png_desc_of(const gspng::Frame& f) {
    dvs_png_desc d{};
    d.width = f.width; d.height = f.height; d.bit_depth = f.bit_depth; d.color_type = f.color_type; d.has_key = f.has_key ? 1 : 0;
    for (int k = 0; k < 3; ++k) d.key[k] = f.key[k];
    memcpy(d.palette, f.palette, sizeof d.palette);
    return d;
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
    report_config();
    describe(resumed);
    if (cfg.enableFocusRegion) prune_region(step);
    region_dirty = false;
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

// A capture directory: a COLMAP sparse model and its images, binary PPM, baseline JPEG or PNG (dataset_io.hpp). A JPEG is entropy-decoded
// on the host (jpeg_io.hpp, ahead of the loop by DecodeAhead) and reconstructed on the device (dvs_jpeg_reconstruct) into the same planar
// bytes a PPM is uploaded as; a PNG is inflated on the host (png_io.hpp, by the same threads) and unfiltered and expanded on the device
// (dvs_png_reconstruct) into those bytes too. Under useMask a PNG mask (masks/<stem>.png, masks/<name>.png; gray or gray+alpha) goes the
// same way and a picture's alpha is ANDed into its mask on the device (dvs_mask_combine); without useMask the alpha is ignored. The view of a SIMPLE_RADIAL / RADIAL / OPENCV camera is then remapped on the device into the view of the
// pinhole camera with the same fx, fy, cx, cy and size (dvs_undistort_view); the pixels without a source are blank and masked out, not
// cropped, so a capture with one such camera carries a mask on every view. Everything after that is one path. The views go up as bytes and are box-filtered
// on the device when maxImageWidth / maxImageHeight ask for it; the splats start from the sparse points (include/dvs_init.h).
bool GaussianTrainerScene::Impl::load_dataset(const std::string& path) {
    gsdata::Dataset ds;
    std::string err;
    gsdata::ReadOptions read_opt;
    read_opt.accept_distorted = true;
    if (!gsdata::read_dataset(path, read_opt, &ds, &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
    const int n_pts = (int)std::min<size_t>(ds.xyz.size() / 3, (size_t)0x7FFFFFFF);
    if (n_pts <= 0) {
        logf_("load_train_data('%s'): the sparse model has no usable points (%zu dropped); initialisation without a point cloud is out of scope", path.c_str(), ds.dropped);
        return false;
    }
    // the smallest factor of {1, 2, 4, 8} that fits each image into maxImageWidth x maxImageHeight; one size per run
    const int max_w = cfg.maxImageWidth > 0 ? cfg.maxImageWidth : 0x7FFFFFFF, max_h = cfg.maxImageHeight > 0 ? cfg.maxImageHeight : 0x7FFFFFFF;
    std::vector<int> factor(ds.images.size(), 1);
    int W0 = 0, H0 = 0, model = -1;
    bool one_model = true;
    const auto is_distorted = [](const gsdata::Camera& c) { return c.model >= 2 && c.model <= 4; };
    size_t n_distorted = 0;
    bool distorted_models[5] = {false, false, false, false, false};
    undistorted = false;
    for (size_t i = 0; i < ds.images.size(); ++i) {
        const gsdata::Camera& c = ds.cameras[ds.images[i].camera];
        if (is_distorted(c)) { ++n_distorted; distorted_models[c.model] = true; undistorted = true; }
        const int w = (int)c.width, h = (int)c.height;
        int d = 1;
        while (d <= 8 && (w / d > max_w || h / d > max_h)) d *= 2;
        if (d > 8 || w / d <= 0 || h / d <= 0) {
            logf_("load_train_data('%s'): image %s is %dx%d; even 1/8 of it does not fit maxImageWidth / maxImageHeight %dx%d", path.c_str(),
                  ds.images[i].name.c_str(), w, h, cfg.maxImageWidth, cfg.maxImageHeight);
            return false;
        }
        factor[i] = d;
        if (i == 0) { W0 = w; H0 = h; W = w / d; H = h / d; model = c.model; }
        else if (w / d != W || h / d != H) {
            logf_("load_train_data('%s'): image %s ends up %dx%d but %s ends up %dx%d; this trainer takes one image size per run", path.c_str(),
                  ds.images[i].name.c_str(), w / d, h / d, ds.images[0].name.c_str(), W, H);
            return false;
        }
        one_model = one_model && c.model == model;
    }
    sh_max = 3;
    const int capacity = std::max(n_pts, cfg.capMax);
    std::vector<float> zero[6];
    for (int g = 0; g < 6; ++g) zero[g].assign((size_t)n_pts * kWidth[g], 0.f);
    create_context(n_pts, capacity, zero);
    const bool u8 = views_u8();
    const size_t P = (size_t)W * H, img = 3 * P;
    std::vector<uint8_t> px, planar, mk;
    std::vector<float> mkf;
    // which file each image, and under useMask its mask, is read from; the JPEGs and PNGs among them are decoded ahead by DVS_LOAD_THREADS
    // host threads (default 8, 1..16: never sized from the machine's CPU count), in the order the loop below takes them
    std::vector<DecodeAhead::Job> jobs;
    std::vector<gsdata::ImageKind> kind(ds.images.size(), gsdata::ImageKind::PPM);
    std::vector<gsdata::MaskKind> mask_kind(ds.images.size(), gsdata::MaskKind::NONE);
    size_t n_jpeg = 0, n_png = 0, n_png_masks = 0, n_alpha = 0;
    for (size_t i = 0; i < ds.images.size(); ++i) {
        std::string file;
        if (!gsdata::resolve_image_kind(ds, i, &file, &kind[i], &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
        if (kind[i] == gsdata::ImageKind::JPEG) { jobs.push_back({file, false}); ++n_jpeg; }
        if (kind[i] == gsdata::ImageKind::PNG) { jobs.push_back({file, true}); ++n_png; }
        if (cfg.useMask) {
            if (!gsdata::resolve_mask(ds, i, &file, &mask_kind[i], &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
            if (mask_kind[i] == gsdata::MaskKind::PNG) { jobs.push_back({file, true}); ++n_png_masks; }
        }
    }
    const int load_threads = std::max(1, std::min(env_int("DVS_LOAD_THREADS", 8), 16));
    DecodeAhead ahead(std::move(jobs), load_threads);
    Event ev_j0, ev_j1;
    if (n_jpeg + n_png + n_png_masks) {
        for (Event* e : {&ev_j0, &ev_j1}) { hipEvent_t ev = nullptr; HIP_OR_THROW(hipEventCreate(&ev)); e->reset(ev); }
    }
    double recon_ms = 0, png_ms = 0;
    size_t job_at = 0;
    // a PNG from the ahead-decoder onto the device: rgb (planar, 3 p0 bytes) and, when the file has one and `alpha` is given, its alpha plane
    const auto png_to_device = [&](const gspng::Frame& f, uint8_t* rgb, DevBuf<uint8_t>* alpha) {
        const dvs_png_desc desc = png_desc_of(f);
        DevBuf<uint8_t> d_filtered(f.filtered.size());
        HIP_OR_THROW(hipMemcpy(d_filtered.get(), f.filtered.data(), f.filtered.size(), hipMemcpyHostToDevice));
        if (alpha && gspng::has_alpha(f)) alpha->alloc((size_t)f.width * f.height);
        HIP_OR_THROW(hipEventRecord(ev_j0.get(), stream.get()));
        DVS_OR_THROW(dvs_png_reconstruct(stream.get(), &desc, d_filtered.get(), rgb, alpha ? alpha->get() : nullptr));
        HIP_OR_THROW(hipEventRecord(ev_j1.get(), stream.get()));
        HIP_OR_THROW(hipEventSynchronize(ev_j1.get()));              // the scanlines are freed at the end of this scope
        float ms = 0;
        HIP_OR_THROW(hipEventElapsedTime(&ms, ev_j0.get(), ev_j1.get()));
        png_ms += ms;
    };
    // the undistortion's events and the count of pixels without a source, summed over the distorted views on the device
    Event ev_u0, ev_u1;
    DevBuf<uint32_t> d_invalid;
    double undistort_ms = 0;
    uint64_t undistort_pixels = 0;
    if (undistorted) {
        for (Event* e : {&ev_u0, &ev_u1}) { hipEvent_t ev = nullptr; HIP_OR_THROW(hipEventCreate(&ev)); e->reset(ev); }
        d_invalid.alloc(sizeof(uint32_t));
        HIP_OR_THROW(hipMemset(d_invalid.get(), 0, sizeof(uint32_t)));
    }
    const bool masked = cfg.useMask || undistorted;           // (a capture of pinhole cameras only: cfg.useMask, as ever)
    for (size_t i = 0; i < ds.images.size(); ++i) {
        const gsdata::Image& im = ds.images[i];
        const gsdata::Camera& c = ds.cameras[im.camera];
        const int w = (int)c.width, h = (int)c.height, d = factor[i];
        const size_t p0 = (size_t)w * h;
        // 1. the view as bytes; 2. box-filtered by the image's factor (rounded back to 8 bits when the views are kept as bytes) unless the
        // bytes are the view as they are; 3. its mask. The owners free whatever an early return or a throw leaves behind.
        DevBuf<uint8_t> full8(3 * p0);
        DevBuf<float> t, mask;
        DevBuf<uint8_t> alpha8;                                 // a PNG picture's alpha plane, kept only where a mask is asked for
        if (kind[i] == gsdata::ImageKind::JPEG) {
            DecodeAhead::Result r = ahead.take(job_at++);
            if (!r.ok) { logf_("load_train_data('%s'): %s", path.c_str(), r.err.c_str()); return false; }
            const gsjpeg::Frame& f = r.frame;
            if (f.width != w || f.height != h) {
                logf_("load_train_data('%s'): %s is %dx%d but its camera %u is %dx%d", path.c_str(), ahead.file(job_at - 1).c_str(), f.width, f.height, c.id, w, h);
                return false;
            }
            dvs_jpeg_desc desc{};
            desc.width = f.width; desc.height = f.height; desc.components = f.components; desc.hs = f.hs[0]; desc.vs = f.vs[0];
            for (int k = 0; k < 3; ++k) { desc.blocks_w[k] = f.blocks_w[k]; desc.blocks_h[k] = f.blocks_h[k]; desc.offset[k] = f.offset[k]; }
            memcpy(desc.quant, f.quant, sizeof desc.quant);
            DevBuf<int16_t> d_coef(f.coef.size() * sizeof(int16_t));
            HIP_OR_THROW(hipMemcpy(d_coef.get(), f.coef.data(), f.coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
            HIP_OR_THROW(hipEventRecord(ev_j0.get(), stream.get()));
            DVS_OR_THROW(dvs_jpeg_reconstruct(stream.get(), &desc, d_coef.get(), full8.get()));
            HIP_OR_THROW(hipEventRecord(ev_j1.get(), stream.get()));
            HIP_OR_THROW(hipEventSynchronize(ev_j1.get()));          // the coefficients are freed at the end of this scope
            float ms = 0;
            HIP_OR_THROW(hipEventElapsedTime(&ms, ev_j0.get(), ev_j1.get()));
            recon_ms += ms;
        } else if (kind[i] == gsdata::ImageKind::PNG) {
            DecodeAhead::Result r = ahead.take(job_at++);
            if (!r.ok) { logf_("load_train_data('%s'): %s", path.c_str(), r.err.c_str()); return false; }
            const gspng::Frame& f = r.png;
            if (f.width != w || f.height != h) {
                logf_("load_train_data('%s'): %s is %dx%d but its camera %u is %dx%d", path.c_str(), ahead.file(job_at - 1).c_str(), f.width, f.height, c.id, w, h);
                return false;
            }
            if (gspng::has_alpha(f)) ++n_alpha;
            png_to_device(f, full8.get(), cfg.useMask ? &alpha8 : nullptr);
        } else {
            if (!gsdata::read_image(ds, i, &px, &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
            planar.resize(3 * p0);                              // the file is [H][W][3], the trainer's views are planar [3][H][W]
            for (size_t q = 0; q < p0; ++q) for (int k = 0; k < 3; ++k) planar[(size_t)k * p0 + q] = px[3 * q + k];
            HIP_OR_THROW(hipMemcpy(full8.get(), planar.data(), 3 * p0, hipMemcpyHostToDevice));
        }
        // under useMask, a PNG mask and / or a picture's alpha are combined on the device into mask8, bytes in {0, 1} (dvs_mask_combine);
        // a PGM mask or none beside a picture without alpha stays on the path it always took
        DevBuf<uint8_t> mask8;
        if (cfg.useMask && (mask_kind[i] == gsdata::MaskKind::PNG || alpha8)) {
            mask8.alloc(p0);
            if (mask_kind[i] == gsdata::MaskKind::PNG) {
                DecodeAhead::Result r = ahead.take(job_at++);
                if (!r.ok) { logf_("load_train_data('%s'): %s", path.c_str(), r.err.c_str()); return false; }
                const gspng::Frame& f = r.png;
                const std::string& file = ahead.file(job_at - 1);
                if (f.color_type != 0 && f.color_type != 4) {
                    logf_("load_train_data('%s'): mask %s has colour type %d; a PNG mask must be grayscale or grayscale with alpha (types 0 and 4)", path.c_str(), file.c_str(), f.color_type);
                    return false;
                }
                if (f.width != w || f.height != h) {
                    logf_("load_train_data('%s'): %s is %dx%d but its camera is %dx%d", path.c_str(), file.c_str(), f.width, f.height, w, h);
                    return false;
                }
                DevBuf<uint8_t> gray3(3 * p0), mask_alpha;
                png_to_device(f, gray3.get(), &mask_alpha);
                DVS_OR_THROW(dvs_mask_combine(stream.get(), p0, gray3.get(), mask_alpha.get(), nullptr, mask8.get(), nullptr));
                if (alpha8) DVS_OR_THROW(dvs_mask_combine(stream.get(), p0, alpha8.get(), nullptr, mask8.get(), mask8.get(), nullptr));
                HIP_OR_THROW(hipStreamSynchronize(stream.get()));    // gray3 and mask_alpha are freed at the end of this scope
            } else {
                if (!gsdata::read_mask(ds, i, &mk, &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
                HIP_OR_THROW(hipMemcpy(mask8.get(), mk.data(), p0, hipMemcpyHostToDevice));
                DVS_OR_THROW(dvs_mask_combine(stream.get(), p0, alpha8.get(), nullptr, mask8.get(), mask8.get(), nullptr));
            }
        }
        if (is_distorted(c)) {                                  // full8 := the pinhole camera's view; mask := valid and, with useMask, trainable
            const double prm[8] = {c.fx, c.fy, c.cx, c.cy, c.dist[0], c.dist[1], c.dist[2], c.dist[3]};      // the camera in OPENCV's order (absent coefficients are 0)
            dvs_undistort_desc desc;
            if (dvs_undistort_desc_from_colmap(4, prm, w, h, &desc) != DVS_OK) {
                logf_("load_train_data('%s'): the parameters of camera %u (%s) do not round to finite fp32 values", path.c_str(), c.id, gsdata::model_name(c.model));
                return false;
            }
            DevBuf<uint8_t> pinhole(3 * p0), d_mk;
            if (mask8) d_mk = std::move(mask8);
            else if (cfg.useMask) {
                if (!gsdata::read_mask(ds, i, &mk, &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
                d_mk.alloc(p0);
                HIP_OR_THROW(hipMemcpy(d_mk.get(), mk.data(), p0, hipMemcpyHostToDevice));
            }
            mask.alloc(p0 * sizeof(float));
            HIP_OR_THROW(hipEventRecord(ev_u0.get(), stream.get()));
            DVS_OR_THROW(dvs_undistort_view(stream.get(), &desc, 3, full8.get(), d_mk.get(), pinhole.get(), mask.get(), d_invalid.get()));
            HIP_OR_THROW(hipEventRecord(ev_u1.get(), stream.get()));
            HIP_OR_THROW(hipEventSynchronize(ev_u1.get()));          // the source bytes and the source mask are freed below
            float ms = 0;
            HIP_OR_THROW(hipEventElapsedTime(&ms, ev_u0.get(), ev_u1.get()));
            undistort_ms += ms;
            undistort_pixels += p0;
            full8 = std::move(pinhole);
        }
        if (!(u8 && d == 1)) {
            t.alloc(img * sizeof(float));
            const dvs_downsample_view dv{full8.get(), t.get()};
            DVS_OR_THROW(dvs_downsample_views(stream.get(), &dv, 1, 3, w, h, d, 1));
        }
        if (masked) {                                           // > 127 trains; a level mask keeps the box filter's fractional weights
            if (!is_distorted(c) && mask8) {                    // the device's mask as the floats a view keeps
                mask.alloc(p0 * sizeof(float));
                DVS_OR_THROW(dvs_mask_combine(stream.get(), p0, nullptr, nullptr, mask8.get(), nullptr, mask.get()));
                HIP_OR_THROW(hipStreamSynchronize(stream.get()));    // mask8 is freed at the end of the iteration
            } else if (!is_distorted(c)) {                      // (a distorted view's mask came out of the undistortion)
                if (cfg.useMask) {
                    if (!gsdata::read_mask(ds, i, &mk, &err)) { logf_("load_train_data('%s'): %s", path.c_str(), err.c_str()); return false; }
                    mkf.assign(mk.begin(), mk.end());
                } else {
                    mkf.assign(p0, 1.f);                        // a pinhole view beside distorted ones, no mask files asked for
                }
                mask.alloc(p0 * sizeof(float));
                HIP_OR_THROW(hipMemcpy(mask.get(), mkf.data(), p0 * sizeof(float), hipMemcpyHostToDevice));
            }
            if (d > 1) {
                DevBuf<float> md(P * sizeof(float));
                const dvs_downsample_view dv{mask.get(), md.get()};
                DVS_OR_THROW(dvs_downsample_views(stream.get(), &dv, 1, 1, w, h, d, 0));
                HIP_OR_THROW(hipStreamSynchronize(stream.get()));
                mask = std::move(md);
            }
        }
        if (t) {
            store_view(std::move(t), std::move(mask));
            if (!u8) HIP_OR_THROW(hipStreamSynchronize(stream.get()));       // (u8: store_view has synchronised) full8 was read until here
        } else {
            views.push_back(View{DevBuf<float>(), std::move(full8), std::move(mask)});
        }
        float R[9];
        gsdata::rotation_of(im, R);
        const float t3[3] = {(float)im.t[0], (float)im.t[1], (float)im.t[2]};
        dvs_camera cam, camd;
        DVS_OR_THROW(dvs_make_camera_intrinsics(R, t3, c.fx, c.fy, c.cx, c.cy, w, h, &cam));
        DVS_OR_THROW(dvs_camera_downscale(&cam, d, &camd));
        cams.push_back(camd);
        cam_names.push_back(std::filesystem::path(im.name).stem().string());
    }
    if (rank == 0) {
        char lvl[64] = "";
        if (factor[0] > 1) snprintf(lvl, sizeof lvl, " -> %dx%d (1/%d)", W, H, factor[0]);
        logf_("dataset: %zu cameras (%s), %dx%d%s, %d points (%zu dropped)", ds.images.size(), one_model ? gsdata::model_name(model) : undistorted ? "mixed models" : "mixed pinhole models",
              W0, H0, lvl, n_pts, ds.dropped);
        if (n_jpeg)
            logf_("dataset: jpeg: %zu of %zu images, entropy decode %.3f ms (host, %d threads, wall), reconstruction %.3f ms (device, events)", n_jpeg,
                  ds.images.size(), ahead.wall_ms(false), load_threads, recon_ms);
        if (n_png + n_png_masks)
            logf_("dataset: png: %zu of %zu images, %zu masks, inflate %.3f ms (host, %d threads, wall), reconstruction %.3f ms (device, events)", n_png,
                  ds.images.size(), n_png_masks, ahead.wall_ms(true), load_threads, png_ms);
        if (n_alpha && !cfg.useMask)
            logf_("dataset: png: %zu of %zu images have alpha; it is ignored without useMask (with it, alpha > 127 is ANDed into the mask)", n_alpha, ds.images.size());
        if (undistorted) {
            uint32_t invalid = 0;
            HIP_OR_THROW(hipMemcpy(&invalid, d_invalid.get(), sizeof invalid, hipMemcpyDeviceToHost));
            std::string names;
            for (int m = 2; m <= 4; ++m) if (distorted_models[m]) names += std::string(names.empty() ? "" : ", ") + gsdata::model_name(m);
            logf_("dataset: undistort: %zu of %zu images (%s), %.3f ms (device, events), %u of %llu pixels have no source and are masked out", n_distorted,
                  ds.images.size(), names.c_str(), undistort_ms, invalid, (unsigned long long)undistort_pixels);
        }
    }
    // 4. the points, 5. their 3-NN scales and the initial parameters, straight into the parameter arrays
    {
        DevBuf<uint8_t> d_rgb((size_t)n_pts * 3 + 16);
        DevBuf<float> d_dist2((size_t)n_pts * sizeof(float) + 16);
        DevBuf<void> d_knn(dvs_knn_scratch_bytes(n_pts));
        float* const pos = d_param[P_POS].get();
        HIP_OR_THROW(hipMemcpy(pos, ds.xyz.data(), (size_t)n_pts * 3 * sizeof(float), hipMemcpyHostToDevice));
        HIP_OR_THROW(hipMemcpy(d_rgb.get(), ds.rgb.data(), (size_t)n_pts * 3, hipMemcpyHostToDevice));
        const auto t_init = std::chrono::steady_clock::now();
        DVS_OR_THROW(dvs_knn_mean_dist2(stream.get(), n_pts, pos, d_knn.get(), d_dist2.get()));
        DVS_OR_THROW(dvs_init_from_points(stream.get(), n_pts, pos, d_rgb.get(), d_dist2.get(), d_param[P_SH0].get(), d_param[P_OPA].get(),
                                          d_param[P_SCALE].get(), d_param[P_ROT].get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_init).count();
        if (rank == 0) logf_("init: 3-NN scales for %d points: %.3f ms", n_pts, ms);
    }
    finish_load([&](std::vector<float> (&init)[6]) {          // the device's initialisation, kept on the host too (resetGaussian, getPoints3D)
        for (int g = 0; g < 6; ++g) {
            init[g].assign((size_t)n_pts * kWidth[g], 0.f);
            if (g != P_SHN) HIP_OR_THROW(hipMemcpy(init[g].data(), d_param[g].get(), init[g].size() * sizeof(float), hipMemcpyDeviceToHost));
        }
    }, "point-cloud", [&](bool resumed) {
        if (cfg.verbose && rank == 0)
            logf_("dataset scene: %d splats, %zu cameras @ %dx%d, SH degree %d%s", n, cams.size(), W, H, sh_max, resumed ? " (resumed; cameras and images from the dataset)" : "");
    });
    evaluate(false);                                            // where the point-cloud start stands on the held-out views (evaluation on, rank 0)
    return true;
}
