// trainer_dataset.cpp — load_dataset, the capture-directory loader, as a short driver over the stages of CaptureLoad.
// A capture directory is a COLMAP sparse model and its images, binary PPM, baseline JPEG or PNG (dataset_io.hpp). A JPEG is entropy-decoded
// on the host (jpeg_io.hpp, ahead of the loop by DecodeAhead) and reconstructed on the device (dvs_jpeg_reconstruct) into the same planar
// bytes a PPM is uploaded as; a PNG is inflated on the host (png_io.hpp, by the same threads) and unfiltered and expanded on the device
// (dvs_png_reconstruct) into those bytes too. Where a view's mask comes from is decided in one place, CaptureLoad::mask. The view of a
// SIMPLE_RADIAL / RADIAL / OPENCV camera is then remapped on the device into the view of the pinhole camera with the same fx, fy, cx, cy and
// size (dvs_undistort_view); the pixels without a source are blank and masked out, not cropped, so a capture with one such camera carries a
// mask on every view. Everything after that is one path. The views go up as bytes and are box-filtered on the device when maxImageWidth /
// maxImageHeight ask for it; the splats start from the sparse points (include/dvs_init.h).
#include "trainer.hpp"
#include <condition_variable>
#include <mutex>
#include <thread>
#include "jpeg_io.hpp"
#include "png_io.hpp"
#include "../../include/dvs_image.h"

namespace {
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

dvs_jpeg_desc jpeg_desc_of(const gsjpeg::Frame& f) {
    dvs_jpeg_desc d{};
    d.width = f.width; d.height = f.height; d.components = f.components; d.hs = f.hs[0]; d.vs = f.vs[0];
    for (int k = 0; k < 3; ++k) { d.blocks_w[k] = f.blocks_w[k]; d.blocks_h[k] = f.blocks_h[k]; d.offset[k] = f.offset[k]; }
    memcpy(d.quant, f.quant, sizeof d.quant);
    return d;
}

// A capture the loader does not take. Every stage reports it this way, once; load_dataset logs `load_train_data('<path>'): <what>`.
struct Refusal { std::string what; };
[[noreturn]] __attribute__((format(printf, 1, 2))) void refuse(const char* fmt, ...) {
    va_list ap, ap2;
    va_start(ap, fmt); va_copy(ap2, ap);
    std::string s((size_t)std::max(0, vsnprintf(nullptr, 0, fmt, ap)), '\0');
    va_end(ap);
    vsnprintf(s.data(), s.size() + 1, fmt, ap2);
    va_end(ap2);
    throw Refusal{std::move(s)};
}

bool is_distorted(const gsdata::Camera& c) { return c.model >= 2 && c.model <= 4; }

struct ViewLoad {                                            // image i on its way to a stored view: its camera, size, factor
    size_t i; const gsdata::Image& im; const gsdata::Camera& c;
    int w, h, d; size_t p0; bool distorted;
};
struct ViewMask {                                            // a view's mask before the undistortion: device bytes in {0, 1}, or host floats
    DevBuf<uint8_t> bytes;                                   // (uploaded when the view is stored), or neither
    const std::vector<float>* floats = nullptr;
};
}  // namespace

struct GaussianTrainerScene::Impl::CaptureLoad {
    Impl& m;
    gsdata::Dataset ds;
    // the plan
    int n_pts = 0, W0 = 0, H0 = 0, model = -1;
    bool one_model = true, distorted_models[5] = {false, false, false, false, false};
    std::vector<int> factor;
    std::vector<gsdata::ImageKind> kind;
    std::vector<gsdata::MaskKind> mask_kind;
    size_t n_distorted = 0, n_jpeg = 0, n_png = 0, n_png_masks = 0, n_alpha = 0;
    std::vector<DecodeAhead::Job> jobs;                      // (moved into `ahead`)
    // the loop's state
    std::unique_ptr<DecodeAhead> ahead;
    size_t job_at = 0;
    TimedPair decode_timer, undistort_timer;
    double recon_ms = 0, png_ms = 0, undistort_ms = 0;
    uint64_t undistort_pixels = 0;
    DevBuf<uint32_t> d_invalid;                              // pixels without a source, summed over the distorted views on the device
    std::vector<uint8_t> px, planar, mk;
    std::vector<float> mkf;

    ViewLoad view(size_t i) const {
        const gsdata::Camera& c = ds.cameras[ds.images[i].camera];
        return {i, ds.images[i], c, (int)c.width, (int)c.height, factor[i], (size_t)c.width * c.height, is_distorted(c)};
    }
    // the points and, per image, the smallest factor of {1, 2, 4, 8} that fits it into maxImageWidth x maxImageHeight; one size per run.
    // Sets m.W, m.H, m.undistorted. Everything refused here is refused before the context exists.
    void plan_sizes(const std::string& path) {
        std::string err;
        gsdata::ReadOptions read_opt;
        read_opt.accept_distorted = true;
        if (!gsdata::read_dataset(path, read_opt, &ds, &err)) refuse("%s", err.c_str());
        n_pts = (int)std::min<size_t>(ds.xyz.size() / 3, (size_t)0x7FFFFFFF);
        if (n_pts <= 0) refuse("the sparse model has no usable points (%zu dropped); initialisation without a point cloud is out of scope", ds.dropped);
        const int max_w = m.cfg.maxImageWidth > 0 ? m.cfg.maxImageWidth : 0x7FFFFFFF, max_h = m.cfg.maxImageHeight > 0 ? m.cfg.maxImageHeight : 0x7FFFFFFF;
        factor.assign(ds.images.size(), 1);
        m.undistorted = false;
        for (size_t i = 0; i < ds.images.size(); ++i) {
            const gsdata::Camera& c = ds.cameras[ds.images[i].camera];
            if (is_distorted(c)) { ++n_distorted; distorted_models[c.model] = true; m.undistorted = true; }
            const int w = (int)c.width, h = (int)c.height;
            int d = 1;
            while (d <= 8 && (w / d > max_w || h / d > max_h)) d *= 2;
            if (d > 8 || w / d <= 0 || h / d <= 0)
                refuse("image %s is %dx%d; even 1/8 of it does not fit maxImageWidth / maxImageHeight %dx%d", ds.images[i].name.c_str(), w, h, m.cfg.maxImageWidth, m.cfg.maxImageHeight);
            factor[i] = d;
            if (i == 0) { W0 = w; H0 = h; m.W = w / d; m.H = h / d; model = c.model; }
            else if (w / d != m.W || h / d != m.H)
                refuse("image %s ends up %dx%d but %s ends up %dx%d; this trainer takes one image size per run", ds.images[i].name.c_str(), w / d, h / d, ds.images[0].name.c_str(), m.W, m.H);
            one_model = one_model && c.model == model;
        }
    }

    // which file each image, and under useMask its mask, is read from; the JPEGs and PNGs among them are decoded ahead by load_threads()
    // host threads, in the order the loop takes them: an image's picture, then its mask
    void plan_files() {
        std::string file, err;
        kind.assign(ds.images.size(), gsdata::ImageKind::PPM);
        mask_kind.assign(ds.images.size(), gsdata::MaskKind::NONE);
        for (size_t i = 0; i < ds.images.size(); ++i) {
            if (!gsdata::resolve_image_kind(ds, i, &file, &kind[i], &err)) refuse("%s", err.c_str());
            if (kind[i] == gsdata::ImageKind::JPEG) { jobs.push_back({file, false}); ++n_jpeg; }
            if (kind[i] == gsdata::ImageKind::PNG) { jobs.push_back({file, true}); ++n_png; }
            if (!m.cfg.useMask) continue;
            if (!gsdata::resolve_mask(ds, i, &file, &mask_kind[i], &err)) refuse("%s", err.c_str());
            if (mask_kind[i] == gsdata::MaskKind::PNG) { jobs.push_back({file, true}); ++n_png_masks; }
        }
    }

    DecodeAhead::Result take() {                             // the next file of the ahead-decoder, which must have decoded
        DecodeAhead::Result r = ahead->take(job_at++);
        if (!r.ok) refuse("%s", r.err.c_str());
        return r;
    }
    void check_size(const ViewLoad& v, int fw, int fh, bool picture) {       // the file just taken has its camera's size
        if (fw == v.w && fh == v.h) return;
        const char* file = ahead->file(job_at - 1).c_str();
        if (picture) refuse("%s is %dx%d but its camera %u is %dx%d", file, fw, fh, v.c.id, v.w, v.h);
        refuse("%s is %dx%d but its camera is %dx%d", file, fw, fh, v.w, v.h);
    }

    void jpeg_picture(const ViewLoad& v, uint8_t* rgb) {
        const DecodeAhead::Result r = take();
        const gsjpeg::Frame& f = r.frame;
        check_size(v, f.width, f.height, true);
        const dvs_jpeg_desc desc = jpeg_desc_of(f);
        DevBuf<int16_t> d_coef(f.coef.size() * sizeof(int16_t));
        HIP_OR_THROW(hipMemcpy(d_coef.get(), f.coef.data(), f.coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        recon_ms += decode_timer.run(m.stream.get(), [&] { DVS_OR_THROW(dvs_jpeg_reconstruct(m.stream.get(), &desc, d_coef.get(), rgb)); });
    }

    // a PNG from the ahead-decoder onto the device: rgb (planar, 3 p0 bytes) and, when the file has one and `alpha` is given, its alpha plane
    void png_to_device(const gspng::Frame& f, uint8_t* rgb, DevBuf<uint8_t>* alpha) {
        const dvs_png_desc desc = png_desc_of(f);
        DevBuf<uint8_t> d_filtered(f.filtered.size());
        HIP_OR_THROW(hipMemcpy(d_filtered.get(), f.filtered.data(), f.filtered.size(), hipMemcpyHostToDevice));
        if (alpha && gspng::has_alpha(f)) alpha->alloc((size_t)f.width * f.height);
        png_ms += decode_timer.run(m.stream.get(), [&] { DVS_OR_THROW(dvs_png_reconstruct(m.stream.get(), &desc, d_filtered.get(), rgb, alpha ? alpha->get() : nullptr)); });
    }

    void png_picture(const ViewLoad& v, uint8_t* rgb, DevBuf<uint8_t>* alpha) {
        const DecodeAhead::Result r = take();
        check_size(v, r.png.width, r.png.height, true);
        if (gspng::has_alpha(r.png)) ++n_alpha;
        png_to_device(r.png, rgb, alpha);
    }

    void ppm_picture(const ViewLoad& v, uint8_t* rgb) {
        std::string err;
        if (!gsdata::read_image(ds, v.i, &px, &err)) refuse("%s", err.c_str());
        planar.resize(3 * v.p0);                                 // the file is [H][W][3], the trainer's views are planar [3][H][W]
        for (size_t q = 0; q < v.p0; ++q) for (int k = 0; k < 3; ++k) planar[(size_t)k * v.p0 + q] = px[3 * q + k];
        HIP_OR_THROW(hipMemcpy(rgb, planar.data(), 3 * v.p0, hipMemcpyHostToDevice));
    }

    // the view as planar bytes on the device; a PNG's alpha plane too, kept only where a mask is asked for
    DevBuf<uint8_t> picture(const ViewLoad& v, DevBuf<uint8_t>* alpha8) {
        DevBuf<uint8_t> full8(3 * v.p0);
        if (kind[v.i] == gsdata::ImageKind::JPEG) jpeg_picture(v, full8.get());
        else if (kind[v.i] == gsdata::ImageKind::PNG) png_picture(v, full8.get(), m.cfg.useMask ? alpha8 : nullptr);
        else ppm_picture(v, full8.get());
        return full8;
    }

    // a PNG mask (gray, or gray + alpha) reconstructed like a picture and reduced to bytes in {0, 1}, ANDed with the picture's alpha
    DevBuf<uint8_t> png_mask(const ViewLoad& v, const DevBuf<uint8_t>& alpha8) {
        const DecodeAhead::Result r = take();
        const gspng::Frame& f = r.png;
        if (f.color_type != 0 && f.color_type != 4)
            refuse("mask %s has colour type %d; a PNG mask must be grayscale or grayscale with alpha (types 0 and 4)", ahead->file(job_at - 1).c_str(), f.color_type);
        check_size(v, f.width, f.height, false);
        DevBuf<uint8_t> mask8(v.p0), gray3(3 * v.p0), mask_alpha;
        png_to_device(f, gray3.get(), &mask_alpha);
        DVS_OR_THROW(dvs_mask_combine(m.stream.get(), v.p0, gray3.get(), mask_alpha.get(), nullptr, mask8.get(), nullptr));
        if (alpha8) DVS_OR_THROW(dvs_mask_combine(m.stream.get(), v.p0, alpha8.get(), nullptr, mask8.get(), mask8.get(), nullptr));
        HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
        return mask8;
    }

    // Where a view's mask comes from (masks/, "Distorted cameras", "PNG"). > 127 of a file or of a picture's alpha trains.
    //   no useMask, pinhole capture                   nothing
    //   no useMask, capture with a distorted camera   a distorted view: nothing here (the undistortion's validity is its mask);
    //                                                 a pinhole view: all ones
    //   useMask, PNG mask file                        the file AND the picture's alpha, on the device
    //   useMask, PGM mask file or none (all ones)     AND the picture's alpha on the device when it has one; as bytes for the undistortion
    //                                                 of a distorted view; else the floats a pinhole view keeps
    ViewMask mask(const ViewLoad& v, const DevBuf<uint8_t>& alpha8) {
        ViewMask out;
        if (!m.cfg.useMask) {
            if (m.undistorted && !v.distorted) { mkf.assign(v.p0, 1.f); out.floats = &mkf; }
            return out;
        }
        if (mask_kind[v.i] == gsdata::MaskKind::PNG) { out.bytes = png_mask(v, alpha8); return out; }
        std::string err;
        if (!gsdata::read_mask(ds, v.i, &mk, &err)) refuse("%s", err.c_str());
        if (!alpha8 && !v.distorted) { mkf.assign(mk.begin(), mk.end()); out.floats = &mkf; return out; }
        out.bytes.alloc(v.p0);
        HIP_OR_THROW(hipMemcpy(out.bytes.get(), mk.data(), v.p0, hipMemcpyHostToDevice));
        if (alpha8) DVS_OR_THROW(dvs_mask_combine(m.stream.get(), v.p0, alpha8.get(), nullptr, out.bytes.get(), out.bytes.get(), nullptr));
        return out;
    }

    // -> the pinhole camera's view; *mask := valid and, with a source mask, trainable; *valid := valid alone, kept only when there is a
    // source mask and maskCarve is on (one more pass without the source mask, whose one plane of pixels is overwritten right after)
    DevBuf<uint8_t> undistort(const ViewLoad& v, DevBuf<uint8_t> full8, DevBuf<uint8_t> mask8, DevBuf<float>* mask, DevBuf<float>* valid) {
        const gsdata::Camera& c = v.c;
        const double prm[8] = {c.fx, c.fy, c.cx, c.cy, c.dist[0], c.dist[1], c.dist[2], c.dist[3]};      // the camera in OPENCV's order (absent coefficients are 0)
        dvs_undistort_desc desc;
        if (dvs_undistort_desc_from_colmap(4, prm, v.w, v.h, &desc) != DVS_OK)
            refuse("the parameters of camera %u (%s) do not round to finite fp32 values", c.id, gsdata::model_name(c.model));
        DevBuf<uint8_t> pinhole(3 * v.p0);
        mask->alloc(v.p0 * sizeof(float));
        if (mask8 && m.opt.i(gsopt::MASK_CARVE) > 0) {
            valid->alloc(v.p0 * sizeof(float));
            DVS_OR_THROW(dvs_undistort_view(m.stream.get(), &desc, 1, full8.get(), nullptr, pinhole.get(), valid->get(), nullptr));
        }
        undistort_ms += undistort_timer.run(m.stream.get(), [&] {
            DVS_OR_THROW(dvs_undistort_view(m.stream.get(), &desc, 3, full8.get(), mask8.get(), pinhole.get(), mask->get(), d_invalid.get()));
        });
        undistort_pixels += v.p0;
        return pinhole;
    }

    // box-filtered by the image's factor (rounded back to 8 bits when the views are kept as bytes) unless the bytes are the view as they
    // are; the mask as the floats a view keeps (> 127 trains; a level mask keeps the box filter's fractional weights)
    void store(const ViewLoad& v, DevBuf<uint8_t> full8, ViewMask vm, DevBuf<float> mask, DevBuf<float> valid) {
        const bool u8 = m.views_u8();
        const size_t P = (size_t)m.W * m.H;
        DevBuf<float> t;
        if (!(u8 && v.d == 1)) {
            t.alloc(3 * P * sizeof(float));
            const dvs_downsample_view dv{full8.get(), t.get()};
            DVS_OR_THROW(dvs_downsample_views(m.stream.get(), &dv, 1, 3, v.w, v.h, v.d, 1));
        }
        if (vm.bytes) {                                          // (a distorted view's mask came out of the undistortion)
            mask.alloc(v.p0 * sizeof(float));
            DVS_OR_THROW(dvs_mask_combine(m.stream.get(), v.p0, nullptr, nullptr, vm.bytes.get(), nullptr, mask.get()));
            HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
        } else if (vm.floats) {
            mask.alloc(v.p0 * sizeof(float));
            HIP_OR_THROW(hipMemcpy(mask.get(), vm.floats->data(), v.p0 * sizeof(float), hipMemcpyHostToDevice));
        }
        if (mask && v.d > 1) {
            DevBuf<float> md(P * sizeof(float));
            const dvs_downsample_view dv{mask.get(), md.get()};
            DVS_OR_THROW(dvs_downsample_views(m.stream.get(), &dv, 1, 1, v.w, v.h, v.d, 0));
            HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
            mask = std::move(md);
        }
        if (valid && v.d > 1) {                                  // (the validity plane of the mask carve: filtered like the mask)
            DevBuf<float> vd(P * sizeof(float));
            const dvs_downsample_view dv{valid.get(), vd.get()};
            DVS_OR_THROW(dvs_downsample_views(m.stream.get(), &dv, 1, 1, v.w, v.h, v.d, 0));
            HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
            valid = std::move(vd);
        }
        if (t) {
            m.store_view(std::move(t), std::move(mask));
            if (!u8) HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));         // (u8: store_view has synchronised) full8 was read until here
        } else {
            m.views.push_back(View{DevBuf<float>(), std::move(full8), std::move(mask), DevBuf<float>()});
        }
        m.views.back().valid = std::move(valid);
    }

    void camera(const ViewLoad& v) {
        float R[9];
        gsdata::rotation_of(v.im, R);
        const float t3[3] = {(float)v.im.t[0], (float)v.im.t[1], (float)v.im.t[2]};
        dvs_camera cam, camd;
        DVS_OR_THROW(dvs_make_camera_intrinsics(R, t3, v.c.fx, v.c.fy, v.c.cx, v.c.cy, v.w, v.h, &cam));
        DVS_OR_THROW(dvs_camera_downscale(&cam, v.d, &camd));
        m.cams.push_back(camd);
        m.cam_names.push_back(std::filesystem::path(v.im.name).stem().string());
    }

    void report() {
        if (m.rank != 0) return;
        const size_t n = ds.images.size();
        const int threads = m.load_threads();
        char lvl[64] = "";
        if (factor[0] > 1) snprintf(lvl, sizeof lvl, " -> %dx%d (1/%d)", m.W, m.H, factor[0]);
        logf_("dataset: %zu cameras (%s), %dx%d%s, %d points (%zu dropped)", n, one_model ? gsdata::model_name(model) : m.undistorted ? "mixed models" : "mixed pinhole models",
              W0, H0, lvl, n_pts, ds.dropped);
        if (n_jpeg)
            logf_("dataset: jpeg: %zu of %zu images, entropy decode %.3f ms (host, %d threads, wall), reconstruction %.3f ms (device, events)", n_jpeg, n,
                  ahead->wall_ms(false), threads, recon_ms);
        if (n_png + n_png_masks)
            logf_("dataset: png: %zu of %zu images, %zu masks, inflate %.3f ms (host, %d threads, wall), reconstruction %.3f ms (device, events)", n_png, n,
                  n_png_masks, ahead->wall_ms(true), threads, png_ms);
        if (n_alpha && !m.cfg.useMask)
            logf_("dataset: png: %zu of %zu images have alpha; it is ignored without useMask (with it, alpha > 127 is ANDed into the mask)", n_alpha, n);
        if (!m.undistorted) return;
        uint32_t invalid = 0;
        HIP_OR_THROW(hipMemcpy(&invalid, d_invalid.get(), sizeof invalid, hipMemcpyDeviceToHost));
        std::string names;
        for (int k = 2; k <= 4; ++k) if (distorted_models[k]) names += std::string(names.empty() ? "" : ", ") + gsdata::model_name(k);
        logf_("dataset: undistort: %zu of %zu images (%s), %.3f ms (device, events), %u of %llu pixels have no source and are masked out", n_distorted, n,
              names.c_str(), undistort_ms, invalid, (unsigned long long)undistort_pixels);
    }

    // the points, their 3-NN scales and the initial parameters, straight into the parameter arrays
    void points() {
        DevBuf<uint8_t> d_rgb((size_t)n_pts * 3 + 16);
        DevBuf<float> d_dist2((size_t)n_pts * sizeof(float) + 16);
        DevBuf<void> d_knn(dvs_knn_scratch_bytes(n_pts));
        float* const pos = m.d_param[P_POS].get();
        HIP_OR_THROW(hipMemcpy(pos, ds.xyz.data(), (size_t)n_pts * 3 * sizeof(float), hipMemcpyHostToDevice));
        HIP_OR_THROW(hipMemcpy(d_rgb.get(), ds.rgb.data(), (size_t)n_pts * 3, hipMemcpyHostToDevice));
        const auto t_init = std::chrono::steady_clock::now();
        DVS_OR_THROW(dvs_knn_mean_dist2(m.stream.get(), n_pts, pos, d_knn.get(), d_dist2.get()));
        DVS_OR_THROW(dvs_init_from_points(m.stream.get(), n_pts, pos, d_rgb.get(), d_dist2.get(), m.d_param[P_SH0].get(), m.d_param[P_OPA].get(),
                                          m.d_param[P_SCALE].get(), m.d_param[P_ROT].get()));
        HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
        if (m.rank == 0) logf_("init: 3-NN scales for %d points: %.3f ms", n_pts, ms_since(t_init));
    }
};

bool GaussianTrainerScene::Impl::load_dataset(const std::string& path) try {
    CaptureLoad L{*this};
    L.plan_sizes(path);
    sh_max = 3;
    std::vector<float> zero[6];
    for (int g = 0; g < 6; ++g) zero[g].assign((size_t)L.n_pts * kWidth[g], 0.f);
    create_context(L.n_pts, std::max(L.n_pts, cfg.capMax), zero);
    L.plan_files();
    L.ahead = std::make_unique<DecodeAhead>(std::move(L.jobs), load_threads());
    if (undistorted) {
        L.d_invalid.alloc(sizeof(uint32_t));
        HIP_OR_THROW(hipMemset(L.d_invalid.get(), 0, sizeof(uint32_t)));
    }
    for (size_t i = 0; i < L.ds.images.size(); ++i) {
        const ViewLoad v = L.view(i);
        DevBuf<uint8_t> alpha8;                                 // (read by the mask's launches until the view is stored)
        DevBuf<uint8_t> full8 = L.picture(v, &alpha8);
        ViewMask vm = L.mask(v, alpha8);
        DevBuf<float> mask, valid;
        if (v.distorted) full8 = L.undistort(v, std::move(full8), std::move(vm.bytes), &mask, &valid);
        L.store(v, std::move(full8), std::move(vm), std::move(mask), std::move(valid));
        L.camera(v);
    }
    L.report();
    L.points();
    const int n_pts = L.n_pts;
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
} catch (const Refusal& r) {
    logf_("load_train_data('%s'): %s", path.c_str(), r.what.c_str());
    return false;
}
