// trainer_step.cpp — the phases of one trainStep: plan, resolution level, render + loss + backward, gradient exchange, optimizer tail.
#include "trainer.hpp"

namespace {
constexpr float kAdamBeta1 = 0.9f, kAdamBeta2 = 0.999f, kAdamEps = 1e-15f;

__global__ void k_unpack_u8(const uint8_t* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i] * (1.0f / 255.0f);
}
// useMask (main.cpp:69-70): pixels outside the mask carry no loss gradient; mask [H*W] in {0,1}, dL planar [3,H,W]
__global__ void k_mask_mul(float* __restrict__ dL, const float* __restrict__ mask, size_t P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * P) dL[i] *= mask[i % P];
}
__global__ void k_norm2(const float* __restrict__ v2, float* __restrict__ out2, int n) {      // (x, y) -> (|v|, 0)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const float x = v2[2 * i], y = v2[2 * i + 1]; out2[2 * i] = sqrtf(x * x + y * y); out2[2 * i + 1] = 0.f; }
}
}  // namespace

// the fp32 target image of camera ci on the device (expands the 8-bit copy when packLevel has PackF32ToU8)
const float* GaussianTrainerScene::Impl::target_for(int ci) {
    if (!views_u8()) return views[(size_t)ci].f32.get();
    const size_t img = 3 * (size_t)W * H;
    hipLaunchKernelGGL(k_unpack_u8, dim3((unsigned)((img + 255) / 256)), dim3(256), 0, stream.get(), views[(size_t)ci].u8.get(), d_target_f32.get(), img);
    return d_target_f32.get();
}

// A step at another level than the one before it (the first step included): ONE stream synchronisation closes the finished level's
// wall time and opens the new one's. max_radii is in pixels of its level and starts again; grad_accum / denom are in NDC units and carry over.
void GaussianTrainerScene::Impl::enter_level(const Step& s) {
    if (s.level == cur_level) return;
    if (cur_level >= 0) {
        close_level();
        HIP_OR_THROW(hipMemsetAsync(d_max_radii.get(), 0, (size_t)cap * 4, stream.get()));
    } else {
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    }
    cur_level = s.level; level_first_step = step; level_t0 = std::chrono::steady_clock::now();
    if (rank == 0) logf_("resolution @%d: %dx%d (1/%d)", s.it, s.Wd, s.Hd, s.div);
}
void GaussianTrainerScene::Impl::close_level() {                            // (also when training ends)
    if (cur_level < 0) return;
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - level_t0).count();
    const int steps = step - level_first_step;
    if (rank == 0 && steps > 0) logf_("resolution: %d steps at %dx%d: %.4f ms/step", steps, W >> cur_level, H >> cur_level, ms / steps);
    cur_level = -1;
}

// the step's views at its level (level > 0): ONE launch for the images, one more for the masks
void GaussianTrainerScene::Impl::level_targets(const Step& s) {
    const size_t P = (size_t)s.Wd * s.Hd;
    bool masked = false;                                                     // (every view carries a mask or none does)
    dvs_downsample_view tv[DVS_DOWNSAMPLE_MAX_VIEWS] = {}, mv[DVS_DOWNSAMPLE_MAX_VIEWS] = {};
    for (int v = 0; v < vpi; ++v) {
        const size_t ci = (size_t)s.ci_all[(size_t)rank * vpi + v];
        tv[v].src = view_pixels(ci);
        tv[v].dst = d_level_targets.get() + (size_t)v * 3 * P;
        if (const float* mask = view_mask(ci)) { mv[v].src = mask; mv[v].dst = d_level_masks.get() + (size_t)v * P; masked = true; }
    }
    DVS_OR_THROW(dvs_downsample_views(stream.get(), tv, vpi, 3, W, H, s.div, views_u8() ? 1 : 0));
    if (masked) DVS_OR_THROW(dvs_downsample_views(stream.get(), mv, vpi, 1, W, H, s.div, 0));   // fractional weights at the ellipse's edge: they scale the gradient
}

GaussianTrainerScene::Impl::Step GaussianTrainerScene::Impl::plan_step() {
    Step s;
    if (next_ci.size() == (size_t)world * vpi) { s.ci_all = next_ci; next_ci.clear(); }   // (drawn by the previous, pipelined step: the same stream)
    else draw_cameras(s.ci_all);
    s.level = level_of(step); s.div = 1 << s.level; s.Wd = W / s.div; s.Hd = H / s.div;
    s.vcams = rank_cameras(s.ci_all, s.level);
    s.it = step + 1;
    s.deg = sh_degree_at(step);
    s.mcmc = mcmc();
    s.absgrad = cfg.useAbsGrad || cfg.densifyStrategy == 2;                  // ADC+ always splits on the abs-grad statistic
    const bool refining = s.it < cfg.refineStopIter;
    // densification statistics of the step's views, summed over the ranks in densify(): per view and visible
    // splat  grad_accum += |abs-grad|, denom += 1, max_radii = max
    s.want_stats = refining && !s.mcmc;
    s.refine_now = refining && s.it > cfg.warmupLength && cfg.refineEvery > 0 && s.it % cfg.refineEvery == 0;
    s.reset_now = refining && !s.mcmc && cfg.resetAlphaEvery > 0 && s.it % cfg.resetAlphaEvery == 0;
    s.prune_now = !refining && cfg.pruneStrategy > 0 && cfg.pruneInterval > 0 && s.it % cfg.pruneInterval == 0;
    s.opts.sh_degree = s.deg; s.opts.antialias = cfg.mipAntiliased ? 1 : 0; s.opts.absgrad = s.absgrad ? 1 : 0; s.opts.accumulate = 0;
    s.opts.shn_layout = DVS_SHN_TILED;
    s.opts.grad_mode = DVS_GRAD_LINEAGE;        // the backward of the lineage the reference credits (README.md:95)
    static const bool tight_tiles = env_is("DVS_TIGHT_TILES", "1");
    s.opts.tile_bounds = tight_tiles ? DVS_TILES_TIGHT : DVS_TILES_CANONICAL;   // opt-in: same images and gradients, shorter tile lists (dvs_raster.h)
    // Adam, per-group learning rates (names gs_train.cpp:52-57; position lr decays exponentially init -> final, scaled by the scene extent)
    const float t = std::min(1.0f, (float)step / (float)std::max(1, cfg.numIters));
    s.lr_pos = extent * std::exp((1.f - t) * std::log(cfg.poslrInit) + t * std::log(cfg.poslrFinal));
    const float lr[6] = {s.lr_pos, cfg.featurelr, cfg.featurelr / 20.f, cfg.opacitylr, cfg.scalinglr, cfg.rotationlr};
    // one launch per set of groups; shN chunks above the active SH degree have g = m = v = 0 (Adam is the identity there)
    for (int k = 0; k < 6; ++k)
        s.adam[k] = dvs_adam_group{d_param[k].get(), d_grad[k], d_m[k].get(), d_v[k].get(), (uint64_t)dev_floats(k), lr[k], kWidth[k],
                                   k == P_SHN ? DVS_SHN_TILED : DVS_SHN_ROWS, 0};
    s.adam[P_SHN].active_chunks = s.deg >= 3 ? 0 : (3 * ((s.deg + 1) * (s.deg + 1) - 1) + 3) / 4;
    if (s.deg == 0) s.adam[P_SHN].count = 0;
    return s;
}

// photometric loss (1-w) L1 + w (1 - SSIM), w = --ssim (main.cpp:24-25), of view v: its gradient goes straight into d_dL[v]; the loss
// sums of the step's views add up in d_loss (getCurrentLoss reports their mean)
void GaussianTrainerScene::Impl::loss_of_view(const Step& s, int v) {
    const int ci = s.ci_all[(size_t)rank * vpi + v];
    const int W = s.Wd, H = s.Hd;                                            // the step's level: everything below is per pixel of it
    const size_t img = 3 * (size_t)W * H;
    const float* target = s.level > 0 ? d_level_targets.get() + (size_t)v * img : target_for(ci);
    const float* out = d_out.get() + (size_t)v * img;
    float* dL = d_dL.get() + (size_t)v * img;
    float* const maps[3] = {d_ssim_maps[0].get(), d_ssim_maps[1].get(), d_ssim_maps[2].get()};
    const float w_ssim = maps[0] ? cfg.ssimWeight : 0.f;
    if (w_ssim > 0.f) {     // SSIM maps, then the L1 and SSIM gradients in one pass over the image
        DVS_OR_THROW(dvs_ssim_forward(stream.get(), out, target, W, H, maps[0], maps[1], maps[2], d_loss.get() + DVS_SSIM_SLOTS));
        DVS_OR_THROW(dvs_loss_l1_ssim_backward(stream.get(), out, target, W, H, maps[0], maps[1], maps[2], w_ssim, dL, d_loss.get()));
    } else {
        DVS_OR_THROW(dvs_l1_loss_grad_w(stream.get(), out, target, img, 1.f, dL, d_loss.get()));
    }
    const size_t P = (size_t)W * H;
    const float* mask = view_mask((size_t)ci);
    if (mask && s.level > 0) mask = d_level_masks.get() + (size_t)v * P;
    if (s.region_mask) mask = s.region_mask + (size_t)v * P;                // (the camera's mask x the region's hit)
    if (mask) hipLaunchKernelGGL(k_mask_mul, dim3((unsigned)((3 * P + 255) / 256)), dim3(256), 0, stream.get(), dL, mask, P);
}

// ---- focus region ----
// The box of the region: DVS_FOCUS_REGION=x0,y0,z0,x1,y1,z1 (--focusRegion), or the axis-aligned bounds of the initial centres; the
// initial rotation DVS_FOCUS_ROTATION=rx,ry,rz (--focusRotation; radians, as updateFocusRegion's), both from opt.
void GaussianTrainerScene::Impl::setup_region() {
    for (int k = 0; k < 3; ++k) { focus_lo[k] = INFINITY; focus_hi[k] = -INFINITY; }
    const std::vector<float>& p = init_host[P_POS];
    for (size_t i = 0; i + 2 < p.size(); i += 3) {
        if (!(std::isfinite(p[i]) && std::isfinite(p[i + 1]) && std::isfinite(p[i + 2]))) continue;
        for (int k = 0; k < 3; ++k) { focus_lo[k] = std::min(focus_lo[k], p[i + k]); focus_hi[k] = std::max(focus_hi[k], p[i + k]); }
    }
    for (int k = 0; k < 3; ++k) if (!(focus_hi[k] >= focus_lo[k])) focus_lo[k] = focus_hi[k] = 0.f;      // (no finite centre)
    if (opt.given[gsopt::FOCUS_REGION])
        for (int k = 0; k < 3; ++k) { focus_lo[k] = opt.f(gsopt::FOCUS_REGION, k); focus_hi[k] = opt.f(gsopt::FOCUS_REGION, 3 + k); }
    const float rot[3] = {opt.f(gsopt::FOCUS_ROTATION, 0), opt.f(gsopt::FOCUS_ROTATION, 1), opt.f(gsopt::FOCUS_ROTATION, 2)};
    const float zero[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 1.f, 1.f};
    set_region(zero, rot, one);
    region_flag_seen = cfg.enableFocusRegion;
}
// -> false (with a log line, the previous region stays) when dvs_region_from_trs refuses the vectors: a zero or non-finite scale
bool GaussianTrainerScene::Impl::set_region(const float* pos, const float* rot, const float* scale) {
    dvs_region r; float b2w[16];
    if (dvs_region_from_trs(pos, rot, scale, focus_lo, focus_hi, &r, b2w) != DVS_OK) {
        logf_("focus region: position %g,%g,%g rotation %g,%g,%g scale %g,%g,%g refused (every scale component must be finite and not zero): the "
              "previous region stays", (double)pos[0], (double)pos[1], (double)pos[2], (double)rot[0], (double)rot[1], (double)rot[2], (double)scale[0],
              (double)scale[1], (double)scale[2]);
        return false;
    }
    region = r;
    memcpy(region_b2w, b2w, sizeof b2w);
    for (int k = 0; k < 3; ++k) { focus_trs[k] = pos[k]; focus_trs[3 + k] = rot[k]; focus_trs[6 + k] = scale[k]; }
    region_dirty = true;
    return true;
}
// the masks of nb views of w x h: out[k] = in[k] x (the ray of the pixel crosses the region), in[k] = nullptr: all ones. ONE launch
// (dvs_region_mask_views) into d_region_mask; what it returns is valid until the next call.
const float* GaussianTrainerScene::Impl::region_masks(const dvs_camera* bc, const float* const* in, int nb, int w, int h) {
    if (!d_region_mask) d_region_mask.alloc((size_t)std::max(vpi, 8) * (size_t)W * H * sizeof(float) + 16);
    dvs_region_mask_view mv[DVS_REGION_MAX_VIEWS] = {};
    for (int k = 0; k < nb; ++k) { mv[k].cam = bc[k]; mv[k].in_mask = in[k]; mv[k].out = d_region_mask.get() + (size_t)k * w * h; }
    if (dvs_region_mask_views(stream.get(), mv, nb, w, h, &region) != DVS_OK) throw std::runtime_error("dvs_region_mask_views refused the step's views");
    return d_region_mask.get();
}

// forward, loss, composite backward, statistics and A9 of the step's views: ONE multi-view pass (parameters read once, one depth sort /
// scan / (view, tile) sort / composite launch for all V views, the gradient rows written once: their sum over the views), or with
// DVS_VIEWS_MODE=sequential one pass per view, gradients accumulating (the reference shape, kept as the check of the multi-view pass)
void GaussianTrainerScene::Impl::render_backward(Step& s) {
    const bool fact = exchange_factorised(), seq = sequential_views;
    const int passes = seq ? vpi : 1, pass_views = seq ? 1 : vpi;
    filter3d_refresh();                                                      // (mipFilter3d: the effective scale and opacity of this step's parameters)
    const dvs_splats sp = splats();
    const int W = s.Wd, H = s.Hd;                                            // the step's level
    const size_t img = 3 * (size_t)W * H;
    hipStream_t const st = stream.get(), cst = comm_stream.get();
    if (s.level > 0) level_targets(s);
    if (cfg.enableFocusRegion) {            // the step's masks: the camera's (at the step's level) x the region's hit, from the level's own camera
        const float* in[DVS_REGION_MAX_VIEWS] = {};
        for (int v = 0; v < vpi; ++v)
            if (const float* mask = view_mask((size_t)s.ci_all[(size_t)rank * vpi + v])) in[v] = s.level > 0 ? d_level_masks.get() + (size_t)v * W * H : mask;
        s.region_mask = region_masks(s.vcams.data(), in, vpi, W, H);
    }
    dvs_opts opts = s.opts;
    dvs_splat_grads g{};
    g.pos = d_grad[P_POS]; g.sh0 = d_grad[P_SH0]; g.shN = d_grad[P_SHN]; g.opacity = d_grad[P_OPA];
    g.scale = d_grad[P_SCALE]; g.rot = d_grad[P_ROT]; g.absgrad2d = s.absgrad ? d_absgrad.get() : nullptr;
    g.mean2d = (s.want_stats && !s.absgrad) ? d_mean2d.get() : nullptr;    // ADC without abs-grad: dL/dmean2D feeds the statistic
    if (fact) { g.sh0 = nullptr; g.shN = nullptr; }                          // (the SH rows are rebuilt after the exchange)
    const dvs_sky sky_tex = sky();
    if (sky_on) HIP_OR_THROW(hipMemsetAsync(d_sky_grad.get(), 0, sky_floats() * sizeof(float), st));
    for (int v = 0; v < passes; ++v) {                                      // v: the first view of the pass
        const dvs_camera* cam = &s.vcams[(size_t)v];
        opts.accumulate = v > 0 ? 1 : 0;
        if (seq) {
            DVS_OR_THROW(dvs_raster_forward(ctx.get(), st, &sp, cam, &opts, d_out.get() + (size_t)v * img, &fwd, nullptr));
        } else {
            DVS_OR_THROW(dvs_raster_forward_views(ctx.get(), st, &sp, cam, pass_views, &opts, d_out.get()));
            DVS_OR_THROW(dvs_get_view_state(ctx.get(), 0, &fwd));             // (view-major arrays: fwd.radii = [V][n])
        }
        if (sky_on)                                                         // out = C + final_T s; s stays for the backward
            DVS_OR_THROW(dvs_sky_forward_views(ctx.get(), st, cam, pass_views, &sky_tex, d_out.get() + (size_t)v * img, d_sky_rgb.get() + (size_t)v * img));
        for (int u = v; u < v + pass_views; ++u) loss_of_view(s, u);
        DVS_OR_THROW(dvs_raster_backward_composite(ctx.get(), st, cam, &opts, d_dL.get() + (size_t)v * img));
        if (sky_on)                                                         // the texel gradient, and the gradient through final_T into the pending rows
            DVS_OR_THROW(dvs_sky_backward_views(ctx.get(), st, cam, pass_views, &opts, &sky_tex, d_dL.get() + (size_t)v * img,
                                                d_sky_rgb.get() + (size_t)v * img, d_sky_grad.get()));
        if (fact) {
            g.dcolor = d_dcolor_scratch.get() + (size_t)v * n * 3;           // A9's own copy of the colour gradient
            DVS_OR_THROW(dvs_raster_backward_dcolor(ctx.get(), st, d_dcolor_local.get() + (size_t)v * n * 3));
        }
        if (fact && v == passes - 1) {      // all local views' colour gradients leave in ONE all-gather, under the last pass's A9
            HIP_OR_THROW(hipEventRecord(ev_dcolor.get(), st));
            HIP_OR_THROW(hipStreamWaitEvent(cst, ev_dcolor.get(), 0));
            DVS_OR_THROW(dvs_comm_all_gather_f32(comm.get(), cst, d_dcolor_local.get(), d_dcolor_all.get(), (size_t)vpi * n * 3));
        }
        if (s.want_stats && s.absgrad) {    // per view, from the composite backward's rows (before A9 consumes them): the exact single-view rule
            const float* rows = nullptr; int rf = 0;
            DVS_OR_THROW(dvs_get_bwd_intermediates(ctx.get(), &rows, &rf));
            DVS_OR_THROW(dvs_densify_accumulate_rows(st, n, pass_views, fwd.radii, rows, W, H, d_grad_accum.get(), d_denom.get(), d_max_radii.get()));
        }
        if (fact && !seq && a9_chunks > 1 && n >= 256 * a9_chunks) {
            // A9 in splat chunks: as soon as chunk k is queued its 44 B/splat of geometry gradients (four ranges of the flat buffer, one
            // grouped collective) start their all-reduce on the communication stream, under the A9 of the chunks behind it
            HIP_OR_THROW(hipEventRecord(ev_gather.get(), cst));              // (behind the colour all-gather queued above)
            s.chunk_per = ((n + a9_chunks - 1) / a9_chunks + 255) / 256 * 256;
            for (int first = 0; first < n; first += s.chunk_per, ++s.n_chunks) {
                const int count = std::min(s.chunk_per, n - first);
                const size_t k = (size_t)s.n_chunks;
                DVS_OR_THROW(dvs_raster_backward_project_chunk(ctx.get(), st, &sp, cam, &opts, &g, first, count));
                HIP_OR_THROW(hipEventRecord(ev_chunk[k].get(), st));
                HIP_OR_THROW(hipStreamWaitEvent(cst, ev_chunk[k].get(), 0));
                DVS_OR_THROW(dvs_comm_group_start(comm.get()));
                DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), cst, d_grad[P_POS] + 3 * (size_t)first, 3 * (size_t)count));
                DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), cst, d_grad[P_SCALE] + 3 * (size_t)first, 3 * (size_t)count));
                DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), cst, d_grad[P_ROT] + 4 * (size_t)first, 4 * (size_t)count));
                DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), cst, d_grad[P_OPA] + (size_t)first, (size_t)count));
                DVS_OR_THROW(dvs_comm_group_end(comm.get()));
                HIP_OR_THROW(hipEventRecord(ev_ar[k].get(), cst));
            }
        } else {
            DVS_OR_THROW(dvs_raster_backward_project(ctx.get(), st, &sp, cam, &opts, &g));
        }
        if (s.want_stats && !s.absgrad) {
            // the standard rule, threshold growGrad2d (0.0002): hypot(gx W/2, gy H/2) of the view's dL/dmean2D (pixel units) per visible
            // splat. One view per step: the signed components go to dvs_densify_accumulate as they are — it scales each by (W/2, H/2)
            // and takes the norm. The multi-view pass hands out the SUM over the views of dL/dmean2D: its norm is taken FIRST (k_norm2:
            // (|g|, 0)), so that what is accumulated, once per step for splats visible in at least one view, is |sum g| W/2 — both
            // components scaled by W/2 (documented difference for V > 1)
            if (v > 0) throw std::runtime_error("gstrain: DVS_VIEWS_MODE=sequential with useAbsGrad off needs per-view mean2d rows (use the multi-view pass)");
            const int* radii = seq || vpi == 1 ? fwd.radii : any_view_radii();
            if (vpi > 1) hipLaunchKernelGGL(k_norm2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_mean2d.get(), d_mean2d.get(), n);
            DVS_OR_THROW(dvs_densify_accumulate(st, n, radii, d_mean2d.get(), W, H, d_grad_accum.get(), d_denom.get(), d_max_radii.get()));
        }
    }
    if (visible_adam()) s.adam_gate = seq || vpi == 1 ? fwd.radii : any_view_radii();   // (sequential: the last view's — a single-view notion there)
}

// the sky texture's optimizer step: its gradient summed over the ranks (one all-reduce, on the training stream: the texture is small),
// so that the replicas keep identical textures, then plain Adam with the betas and eps of the other groups
void GaussianTrainerScene::Impl::step_sky(const Step& s) {
    if (!sky_on) return;
    if (comm) DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), stream.get(), d_sky_grad.get(), sky_floats()));
    DVS_OR_THROW(dvs_adam_step(stream.get(), d_sky.get(), d_sky_grad.get(), d_sky_m.get(), d_sky_v.get(), sky_floats(), opt.f(gsopt::SKY_LR), kAdamBeta1, kAdamBeta2,
                               kAdamEps, s.it));
}

// data parallel, over RCCL / xGMI: all-gather of the views' colour gradients + all-reduce of the geometry groups, then every
// replica rebuilds the summed SH rows from all views (factorised) — or ONE sum-all-reduce of all six groups (they share a buffer)
void GaussianTrainerScene::Impl::exchange(const Step& s, bool pipelined) {
    if (!comm) return;
    hipStream_t const st = stream.get(), cst = comm_stream.get();
    if (!factorised) { DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), st, d_grad_flat.get(), grad_floats)); return; }
    if (s.n_chunks == 0) {          // (all collectives on the communication stream, in the same order on every rank)
        HIP_OR_THROW(hipEventRecord(ev_gather.get(), cst));                  // (behind the colour all-gather)
        HIP_OR_THROW(hipEventRecord(ev_bwd.get(), st));
        HIP_OR_THROW(hipStreamWaitEvent(cst, ev_bwd.get(), 0));
        DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), cst, d_grad_flat.get(), geom_floats));
    }
    HIP_OR_THROW(hipEventRecord(ev_comm.get(), cst));
    // The SH rows need only the colour all-gather: they are rebuilt and their Adam step (sh0 + shN: 192 of the 236 B per splat) runs
    // WHILE the geometry all-reduce is still on the links; the geometry groups follow when it has landed.
    HIP_OR_THROW(hipStreamWaitEvent(st, ev_gather.get(), 0));
    std::vector<float> campos(s.ci_all.size() * 3);             // slot order of the all-gather: [rank][local view]
    for (size_t q = 0; q < s.ci_all.size(); ++q) for (int k = 0; k < 3; ++k) campos[q * 3 + k] = cams[(size_t)s.ci_all[q]].campos[k];
    DVS_OR_THROW(dvs_sh_grad_combine(ctx.get(), st, n, d_param[P_POS].get(), s.deg, (int)s.ci_all.size(), campos.data(), d_dcolor_all.get(),
                                     d_grad[P_SH0], d_grad[P_SHN], 0, DVS_SHN_TILED));
    const dvs_adam_group sh_groups[2] = {s.adam[P_SH0], s.adam[P_SHN]};
    DVS_OR_THROW(dvs_adam_step_groups(st, sh_groups, 2, kAdamBeta1, kAdamBeta2, kAdamEps, s.it, s.adam_gate, n));
    if (!pipelined) HIP_OR_THROW(hipStreamWaitEvent(st, ev_comm.get(), 0));
}

// the optimizer tail on the splats [first, first + count): MCMC regularisers, Adam on the given groups, exploration noise. All are
// element-wise, so a range is bit-identical to the whole-array calls.
void GaussianTrainerScene::Impl::finish_range(const Step& s, int first, int count, const int* groups, int n_groups, const int* gate) {
    float* const opa = d_param[P_OPA].get(); float* const scale = d_param[P_SCALE].get();
    if (f3d_on) { filter3d_chain(first, count); f3d_fresh = false; f3d_it = s.it; }         // the backward's gradients are those of the effective values; the step below changes the trained ones
    if (s.mcmc)        // opacity and scale regularisers of the MCMC strategy (0.01 each in the published rule): a function of the replicated
                       // parameters, added once (after the exchange) on every rank
        DVS_OR_THROW(dvs_mcmc_regularize_range(stream.get(), n, first, count, opa, scale, d_grad[P_OPA], d_grad[P_SCALE], 0.01f, 0.01f));
    dvs_adam_group ag[6];
    for (int k = 0; k < n_groups; ++k) {
        ag[k] = s.adam[groups[k]];
        if (ag[k].layout != DVS_SHN_ROWS) continue;                      // (the tiled shN group is only ever stepped whole: first 0, count n)
        const size_t off = (size_t)ag[k].width * (size_t)first;
        ag[k].param += off; ag[k].grad += off; ag[k].m += off; ag[k].v += off; ag[k].count = (uint64_t)ag[k].width * (uint64_t)count;
    }
    DVS_OR_THROW(dvs_adam_step_groups(stream.get(), ag, n_groups, kAdamBeta1, kAdamBeta2, kAdamEps, s.it, gate ? gate + first : nullptr, count));
    if (s.mcmc && cfg.noiselr > 0.f)      // exploration noise, scaled by the position learning rate (`noiselr`, gs_train.cpp:97)
        DVS_OR_THROW(dvs_mcmc_add_noise_range(stream.get(), n, first, count, d_param[P_POS].get(), scale, d_param[P_ROT].get(), opa,
                                              cfg.noiselr * s.lr_pos, (uint32_t)s.it));
}

// PIPELINED exchange (round 6; SURVEY 8(e) "Overlap"; DVS_EXCHANGE_PIPELINE=1, off by default until it has run on real links): the
// geometry gradients left in chunks behind A9. Here every chunk is finished as soon as ITS all-reduce has landed — regulariser,
// Adam on the four geometry groups, exploration noise, each on the chunk's splat range (all element-wise: bit-identical to the
// whole-array calls) — and then the NEXT iteration's projection (A2) of that chunk is queued: A2 is per splat, and the chunk's
// parameters are final (the SH groups were stepped in exchange(), under the all-reduces). Only the last chunk's all-reduce is exposed;
// the all-reduces of the chunks before it run under the Adam / A2 of their predecessors. Iterations that refine, reset or prune
// change the parameters after Adam: no early projection there (the next forward projects everything itself).
void GaussianTrainerScene::Impl::finish_pipelined(const Step& s) {
    const bool early = !s.refine_now && !s.reset_now && !s.prune_now && s.it < cfg.numIters && !filter3d_due(s.it);     // (a filter due at the next step changes what A2 reads)
    if (early) draw_cameras(next_ci);
    const std::vector<dvs_camera> ncams = early ? rank_cameras(next_ci, level_of(s.it)) : std::vector<dvs_camera>();   // (the NEXT step's level)
    dvs_opts nopts = s.opts;
    nopts.sh_degree = sh_degree_at(s.it);                               // (what the next trainStep will compute from step = it)
    const dvs_splats sp = splats();
    for (int k = 0; k < s.n_chunks; ++k) {
        const int first = k * s.chunk_per, count = std::min(s.chunk_per, n - first);
        HIP_OR_THROW(hipStreamWaitEvent(stream.get(), ev_ar[(size_t)k].get(), 0));
        finish_range(s, first, count, kGeomGroups, 4, nullptr);        // ungated Adam, unlike the unpipelined tail (s.adam_gate)
        if (early && f3d_on) filter3d_apply(first, count);              // what A2 of this chunk reads
        if (early) DVS_OR_THROW(dvs_raster_forward_views_prepare(ctx.get(), stream.get(), &sp, ncams.data(), vpi, &nopts, first, count));
    }
    if (early && f3d_on && s.n_chunks > 0) f3d_fresh = true;               // (the chunks cover every splat)
}
