// trainer_render.cpp — rendered views as JPEG files: the selected cameras through the evaluation context, the forward DCT and
// quantisation on the device (dvs_jpeg_encode_views), the entropy coder on host threads (jpeg_write.hpp). And as PNG files (colour,
// 16-bit depth, alpha): sample conversion and the per-row filter choice on the device (dvs_png_encode_views), deflate on host threads
// (png_io.hpp write_png). Both formats hand their files to write_files, the one host-thread fan-out.
#include "trainer.hpp"
#include <atomic>
#include <thread>
#include "jpeg_write.hpp"
#include "png_io.hpp"
#include "../../include/dvs_image.h"

namespace {
bool write_file(const std::string& file, const std::string& data) {
    FILE* f = fopen(file.c_str(), "wb");
    bool ok = f && fwrite(data.data(), 1, data.size(), f) == data.size();
    if (f && fclose(f) != 0) ok = false;
    return ok;
}

// Files written by host threads. code(task, &out, &err) -> bool produces task's bytes, file_of(task) names its file; the tasks are handed
// out one at a time, so any number of threads finishes them all: up to min(limit, tasks), the calling thread among them, and a thread
// that cannot be started is not needed. A worker never throws: a failed allocation inside a task becomes that task's error, `oom`.
// -> per task the bytes written (0 with its error set), the threads used and the wall time of it all.
struct Written { std::vector<size_t> bytes; std::vector<std::string> errs; int threads = 1; double host_ms = 0; };
template <class Code, class FileOf>
Written write_files(int tasks, int limit, const char* oom, const Code& code, const FileOf& file_of) {
    const auto t_host = std::chrono::steady_clock::now();
    Written w;
    w.bytes.assign((size_t)tasks, 0);
    w.errs.resize((size_t)tasks);
    std::atomic<int> next{0};
    const auto work = [&]() noexcept {
        for (int t = next++; t < tasks; t = next++) {
            try {
                std::string out;
                if (!code(t, &out, &w.errs[(size_t)t])) continue;
                const std::string& file = file_of(t);
                if (write_file(file, out)) w.bytes[(size_t)t] = out.size();
                else w.errs[(size_t)t] = "cannot write " + file;
            } catch (...) {
                try { w.errs[(size_t)t] = oom; } catch (...) {}
            }
        }
    };
    std::vector<std::thread> workers;
    try {
        workers.reserve((size_t)limit);
        for (int t = 1; t < std::min(limit, tasks); ++t) workers.emplace_back(work);
    } catch (...) {}
    w.threads = (int)workers.size() + 1;
    work();
    for (std::thread& t : workers) t.join();
    w.host_ms = ms_since(t_host);
    return w;
}
}  // namespace

void GaussianTrainerScene::Impl::setup_render() {
    render_views = env_int("DVS_RENDER_VIEWS", cfg.renderViews) & (RENDER_TEST | RENDER_TRAIN);
    render_quality = std::max(1, std::min(env_int("DVS_RENDER_QUALITY", cfg.renderQuality), 100));
    render_sampling = env_int("DVS_RENDER_SAMPLING", cfg.renderSampling) == 1 ? DVS_JPEG_SAMPLING_444 : DVS_JPEG_SAMPLING_420;
    if (gsopt::layers_need_png(opt.i(gsopt::RENDER_LAYERS), opt.on(gsopt::RENDER_FORMAT))) {     // (the PNG settings themselves: opt)
        logf_("render: DVS_RENDER_LAYERS='%s' asks for depth or alpha, which JPEG files do not carry (DVS_RENDER_FORMAT=png does): ignored", opt.text[gsopt::RENDER_LAYERS].c_str());
        opt.v[gsopt::RENDER_LAYERS][0] = gsopt::LAYER_COLOR;
    }
    // file names: the image stems when every camera has one and they are unique, cam_%04d otherwise (a synthetic scene). cam_names is
    // filled in step with cams by both loaders.
    std::map<std::string, int> seen;
    cam_names_ok = cam_names.size() == cams.size();
    for (const std::string& s : cam_names) cam_names_ok = cam_names_ok && !s.empty() && seen[s]++ == 0;
}

std::string GaussianTrainerScene::Impl::camera_name(int c) const {
    if (cam_names_ok) return cam_names[(size_t)c];
    char name[32];
    snprintf(name, sizeof name, "cam_%04d", c);
    return name;
}

// cameras `which` rendered from the current parameters and written to `files`: per pass of for_each_eval_pass (the sky composited),
// ONE encode launch (timed by events), one copy of the coefficients, then write_files codes one view per task.
// Synchronous. -> false when a file could not be coded or written (the others are still written).
bool GaussianTrainerScene::Impl::render_to_jpeg(const std::vector<int>& which, const std::vector<std::string>& files, RenderStats* stats) {
    ensure_eval_ctx();
    dvs_jpeg_desc desc;
    if (dvs_jpeg_encode_desc(W, H, render_sampling, render_quality, &desc) != DVS_OK) throw std::runtime_error("dvs_jpeg_encode_desc: invalid arguments");
    const size_t count = dvs_jpeg_encode_coef_count(&desc), img = 3 * (size_t)W * H;
    d_render_coef.reserve((size_t)eval_views * count * sizeof(int16_t));
    if (render_coef_host.size() < (size_t)eval_views * count) render_coef_host.resize((size_t)eval_views * count);
    const int hs[3] = {desc.hs, 1, 1}, vs[3] = {desc.vs, 1, 1};             // (the chroma components are sampled 1x1)
    bool all_ok = true;
    for_each_eval_pass(splats(), which, true, [&](const EvalPass& p) {
        const int first = p.first, nb = p.nb;
        const float* images[DVS_JPEG_ENCODE_MAX_VIEWS];
        int16_t* coefs[DVS_JPEG_ENCODE_MAX_VIEWS];
        for (int k = 0; k < nb; ++k) {
            images[k] = p.images + (size_t)k * img;
            coefs[k] = d_render_coef.get() + (size_t)k * count;
        }
        render_timer.begin(stream.get());
        DVS_OR_THROW(dvs_jpeg_encode_views(stream.get(), &desc, images, coefs, nb));
        render_timer.end(stream.get());
        HIP_OR_THROW(hipMemcpyAsync(render_coef_host.data(), d_render_coef.get(), (size_t)nb * count * sizeof(int16_t), hipMemcpyDeviceToHost, stream.get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        const float ms = render_timer.ms();
        const Written w = write_files(nb, load_threads(), "out of memory while coding the view", [&](int k, std::string* out, std::string* err) {
            return gsjpeg::encode_coefficients(W, H, 3, hs, vs, desc.quant, desc.blocks_w, desc.blocks_h, desc.offset, render_coef_host.data() + (size_t)k * count, count, out, err);
        }, [&](int k) -> const std::string& { return files[(size_t)(first + k)]; });
        for (int k = 0; k < nb; ++k) {
            if (!w.errs[(size_t)k].empty()) { logf_("render @%d: camera %d: %s", step, which[(size_t)(first + k)], w.errs[(size_t)k].c_str()); all_ok = false; }
            else if (stats) { stats->views += 1; stats->bytes += w.bytes[(size_t)k]; }
        }
        if (stats) { stats->transform_ms += ms; stats->entropy_ms += w.host_ms; stats->threads = std::max(stats->threads, w.threads); }
    });
    return all_ok;
}

// the PNG counterpart of render_to_jpeg: the layers whose files[l] is not empty. -> false when a file could not be deflated or written.
bool GaussianTrainerScene::Impl::render_to_png(const std::vector<int>& which, const std::vector<std::string> (&files)[3], PngStats* stats) {
    ensure_eval_ctx();
    static const int kKind[3] = {DVS_PNG_KIND_RGB8, DVS_PNG_KIND_GRAY16, DVS_PNG_KIND_GRAY8};
    static const int kType[3] = {2, 0, 0}, kDepth[3] = {8, 16, 8};
    const float scales[3] = {255.f, opt.f(gsopt::RENDER_DEPTH_SCALE), 255.f};
    constexpr size_t kCounts = DVS_PNG_ENCODE_MAX_VIEWS * sizeof(uint32_t);   // the saturation counts lead the buffer: one copy brings both
    size_t bytes_of[3] = {0, 0, 0}, per_view = 0;
    int n_layers = 0, asked[3] = {0, 0, 0};                                  // the layers asked for, in file order
    for (int l = 0; l < 3; ++l) {
        if (files[l].empty()) continue;
        if (files[l].size() != which.size()) throw std::runtime_error("render_to_png: a layer's file list does not match the cameras");
        bytes_of[l] = dvs_png_encode_bytes(kKind[l], W, H);
        if (!bytes_of[l]) throw std::runtime_error("dvs_png_encode_bytes: invalid arguments");
        per_view += bytes_of[l];
        asked[n_layers++] = l;
    }
    if (!n_layers) return true;
    const bool maps = !files[1].empty() || !files[2].empty();
    const size_t img = 3 * (size_t)W * H, map = (size_t)W * H;
    d_render_png.reserve(kCounts + (size_t)eval_views * per_view);
    if (render_png_host.size() < kCounts + (size_t)eval_views * per_view) render_png_host.resize(kCounts + (size_t)eval_views * per_view);
    if (maps) { d_render_depth.reserve((size_t)eval_views * map * sizeof(float)); d_render_alpha.reserve((size_t)eval_views * map * sizeof(float)); }
    const dvs_opts opts = eval_opts();
    char scale_text[32];
    snprintf(scale_text, sizeof scale_text, "%.9g", (double)opt.f(gsopt::RENDER_DEPTH_SCALE));
    const gspng::TextPairs depth_text = {{"depth_scale", scale_text}};
    bool all_ok = true;
    for_each_eval_pass(splats(), which, true, [&](const EvalPass& p) {
        const int first = p.first, nb = p.nb;
        if (maps) DVS_OR_THROW(dvs_raster_depth_views(eval_ctx.get(), stream.get(), &opts, d_render_depth.get(), d_render_alpha.get()));
        HIP_OR_THROW(hipMemsetAsync(d_render_png.get(), 0, kCounts, stream.get()));
        size_t layer_at[3] = {0, 0, 0}, at = kCounts;
        render_timer.begin(stream.get());
        for (int l = 0; l < 3; ++l) {
            if (files[l].empty()) continue;
            layer_at[l] = at;
            const float* images[DVS_PNG_ENCODE_MAX_VIEWS];
            uint8_t* outs[DVS_PNG_ENCODE_MAX_VIEWS];
            for (int k = 0; k < nb; ++k) {
                images[k] = l == 0 ? p.images + (size_t)k * img : (l == 1 ? d_render_depth.get() : d_render_alpha.get()) + (size_t)k * map;
                outs[k] = d_render_png.get() + at + (size_t)k * bytes_of[l];
            }
            DVS_OR_THROW(dvs_png_encode_views(stream.get(), kKind[l], W, H, scales[l], images, outs, l == 1 ? (uint32_t*)d_render_png.get() : nullptr, nb));
            at += (size_t)nb * bytes_of[l];
        }
        render_timer.end(stream.get());
        HIP_OR_THROW(hipMemcpyAsync(render_png_host.data(), d_render_png.get(), at, hipMemcpyDeviceToHost, stream.get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        const float ms = render_timer.ms();
        // task t: view t / n_layers, layer asked[t % n_layers]
        const Written w = write_files(nb * n_layers, load_threads(), "out of memory while writing the view", [&](int t, std::string* out, std::string* err) {
            const int k = t / n_layers, l = asked[t % n_layers];
            return gspng::write_png(W, H, kDepth[l], kType[l], render_png_host.data() + layer_at[l] + (size_t)k * bytes_of[l], bytes_of[l], opt.i(gsopt::RENDER_PNG_LEVEL),
                                    l == 1 ? &depth_text : nullptr, out, err);
        }, [&](int t) -> const std::string& { return files[asked[t % n_layers]][(size_t)(first + t / n_layers)]; });
        for (int k = 0; k < nb; ++k) {
            bool view_ok = true;
            for (int j = 0; j < n_layers; ++j) {
                const size_t t = (size_t)(k * n_layers + j);
                if (!w.errs[t].empty()) { logf_("render @%d: camera %d: %s", step, which[(size_t)(first + k)], w.errs[t].c_str()); all_ok = view_ok = false; }
                else if (stats) { stats->files += 1; stats->bytes += w.bytes[t]; }
            }
            if (stats && view_ok) stats->views += 1;
            if (stats && !files[1].empty()) { uint32_t c; memcpy(&c, render_png_host.data() + (size_t)k * sizeof c, sizeof c); stats->saturated += c; }
        }
        if (stats) { stats->filter_ms += ms; stats->deflate_ms += w.host_ms; stats->threads = std::max(stats->threads, w.threads); }
    });
    return all_ok;
}

// at a save, rank 0: the cameras cfg.renderViews selects, into <modelPath>_<step>_renders/
void GaussianTrainerScene::Impl::render_at_save() {
    if (!render_views || rank != 0 || !ctx) return;
    HIP_OR_THROW(hipSetDevice(device));
    std::vector<int> which;
    for (int c = 0; c < (int)cams.size(); ++c) {
        const bool test = eval_holdout > 0 && c % eval_holdout == 0;
        if (render_views & (test ? RENDER_TEST : RENDER_TRAIN)) which.push_back(c);
    }
    if (which.empty()) { logf_("render @%d: 0 views (renderViews %d selects no camera: nothing is held out)", step, render_views); return; }
    const std::string dir = save_path(step, "_renders");
    std::error_code ec;
    std::filesystem::create_directories(dir, ec);
    if (ec) { logf_("render @%d: cannot create %s: %s", step, dir.c_str(), ec.message().c_str()); return; }
    if (opt.on(gsopt::RENDER_FORMAT)) {
        static const char* const kSuffix[3] = {".png", "_depth.png", "_alpha.png"};
        std::vector<std::string> layers[3];
        for (int l = 0; l < 3; ++l)
            if (opt.i(gsopt::RENDER_LAYERS) & (1 << l)) for (int c : which) layers[l].push_back(dir + "/" + camera_name(c) + kSuffix[l]);
        PngStats st;
        render_to_png(which, layers, &st);
        logf_("render @%d: %zu views, %zu files, %zu bytes, filtering %.3f ms (device, events), deflate %.3f ms (host, %d threads, wall), %zu depth samples saturated",
              step, st.views, st.files, st.bytes, st.filter_ms, st.deflate_ms, st.threads, st.saturated);
        return;
    }
    std::vector<std::string> files;
    for (int c : which) files.push_back(dir + "/" + camera_name(c) + ".jpg");
    RenderStats st;
    render_to_jpeg(which, files, &st);
    logf_("render @%d: %zu views, %zu bytes, transform %.3f ms (device, events), entropy coding %.3f ms (host, %d threads, wall)", step, st.views,
          st.bytes, st.transform_ms, st.entropy_ms, st.threads);
}
