// trainer_filter3d.cpp — the 3D smoothing filter (trainer.hpp; INTEGRATION.md "3D smoothing filter"): when the per-splat filter is computed,
// when the effective scale and opacity the renderers read are filled, the chain rule back to the trained values, the fused PLY.
#include "trainer.hpp"

// The option as it stands now (load, resetGaussian). On: the per-splat arrays at the capacity of the others and the rows of the
// full-resolution training cameras on the device; held-out cameras never count.
void GaussianTrainerScene::Impl::setup_filter3d() {
    f3d_on = opt.on(gsopt::MIP_FILTER3D);
    if (!f3d_on) return;
    f3d_dirty = true; f3d_fresh = false; f3d_it = step;
    if (f3d_cap < cap) {                                                     // with the other per-splat arrays: at their capacity, again when it grew
        d_filter.alloc((size_t)cap * sizeof(float) + 16);
        d_scale_eff.alloc((size_t)cap * 3 * sizeof(float) + 16);
        d_opacity_eff.alloc((size_t)cap * sizeof(float) + 16);
        d_f3d_scratch.alloc(16);
        f3d_cap = cap;
    }
    const std::vector<int> tc = training_cameras();
    std::vector<dvs_camera> tcams;
    for (int c : tc) tcams.push_back(cams[(size_t)c]);
    std::vector<float> rows(tcams.size() * 16);
    DVS_OR_THROW(dvs_filter3d_pack_cameras(tcams.data(), (int)tcams.size(), rows.data()));
    d_f3d_rows.alloc(rows.size() * sizeof(float));
    HIP_OR_THROW(hipMemcpy(d_f3d_rows.get(), rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    f3d_cams = (int)tcams.size();
    if (rank == 0)
        logf_("config: mipFilter3d 1: every splat is smoothed in world space by sqrt(0.2) x the smallest depth / focal length over the %d full-resolution "
              "training cameras that see it (recomputed at load, after every change of the splat set and every 100 steps); the renderers read the "
              "effective scale and opacity, the resume PLY keeps the trained ones, every other file a save writes holds the fused model; "
              "mipAntiliased %d is the method's 2D half (the paper's configuration is both)", f3d_cams, (int)cfg.mipAntiliased);
}

// the filter of the current positions into `filter` (training's d_filter, or a save's own), and rank 0's log line: one synchronous copy of
// n floats and a host selection for the median, every 100 steps or rarer
void GaussianTrainerScene::Impl::filter3d_compute(float* filter, const char* what) {
    const float ms = f3d_timer.run(stream.get(), [&] {
        DVS_OR_THROW(dvs_filter3d_compute(stream.get(), n, d_param[P_POS].get(), d_f3d_rows.get(), f3d_cams, filter, d_f3d_scratch.get()));
    });
    if (rank != 0) return;
    uint32_t h[4] = {};
    std::vector<float> f((size_t)n);
    HIP_OR_THROW(hipMemcpy(h, d_f3d_scratch.get(), sizeof h, hipMemcpyDeviceToHost));
    HIP_OR_THROW(hipMemcpy(f.data(), filter, f.size() * sizeof(float), hipMemcpyDeviceToHost));
    float lo = 0.f, mid = 0.f, hi = 0.f;
    if (n > 0) {
        std::nth_element(f.begin(), f.begin() + n / 2, f.end());
        mid = f[(size_t)n / 2];
        lo = *std::min_element(f.begin(), f.begin() + n / 2 + 1);
        hi = *std::max_element(f.begin() + n / 2, f.end());
    }
    logf_("filter3d @%d: %d splats, %u seen, filter min/median/max %.6g/%.6g/%.6g, %.3f ms%s", f3d_it, n, h[1], (double)lo, (double)mid, (double)hi,
          (double)ms, what);
}

void GaussianTrainerScene::Impl::filter3d_apply(int first, int count) {
    DVS_OR_THROW(dvs_filter3d_apply_range(stream.get(), n, first, count, d_param[P_SCALE].get(), d_param[P_OPA].get(), d_filter.get(), d_scale_eff.get(),
                                          d_opacity_eff.get()));
}

// before anything reads splats(): the filter when it is due, the effective arrays when the trained ones changed since they were filled.
// Either rewrites what a prepared projection was made from (dvs_raster.h: contents changed behind the same pointers), so that goes.
void GaussianTrainerScene::Impl::filter3d_refresh() {
    if (!f3d_on || n <= 0) return;
    const bool due = filter3d_due(f3d_it);
    if (!due && f3d_fresh) return;
    (void)dvs_raster_forward_cancel_prepared(ctx.get());
    if (due) {
        filter3d_compute(d_filter.get(), "");
        f3d_dirty = false; f3d_fresh = false; f3d_step = f3d_it;
    }
    filter3d_apply(0, n);
    f3d_fresh = true;
}

// A save exports the model fused with the filter of the positions it saves. Training's own set serves when it is that filter; else the
// filter and the effective values go into the save's own arrays (f3d_save, cleared by the save when its exports are written): what
// training reads, when it computes its filter next and what the pipelined step prepared all stay as they are. Every rank computes it
// (the call sits before the save's rank test), none exchanges anything.
void GaussianTrainerScene::Impl::filter3d_for_save() {
    f3d_save = false;
    if (!f3d_on || n <= 0) return;
    if (f3d_dirty || f3d_step == f3d_it) { filter3d_refresh(); return; }
    d_save_filter.reserve((size_t)cap * sizeof(float) + 16);
    d_save_scale.reserve((size_t)cap * 3 * sizeof(float) + 16);
    d_save_opacity.reserve((size_t)cap * sizeof(float) + 16);
    filter3d_compute(d_save_filter.get(), " (for the save; training keeps its own)");
    DVS_OR_THROW(dvs_filter3d_apply(stream.get(), n, d_param[P_SCALE].get(), d_param[P_OPA].get(), d_save_filter.get(), d_save_scale.get(), d_save_opacity.get()));
    f3d_save = true;
}

// gradients with respect to the effective scale and opacity (what the backward wrote) -> with respect to the trained ones, in place.
// Linear in the gradients and a function of the replicated parameters: after the all-reduce the ranks stay bit-identical.
void GaussianTrainerScene::Impl::filter3d_chain(int first, int count) {
    DVS_OR_THROW(dvs_filter3d_chain_range(stream.get(), n, first, count, d_param[P_SCALE].get(), d_param[P_OPA].get(), d_filter.get(), d_grad[P_SCALE],
                                          d_grad[P_OPA]));
}

// <modelPath>_<it>.fused.ply: the full PLY's wire format of the set the exports pack from (ex(): the fused scale and opacity, in the export
// frame when one is set); sh0 is invariant under both (the host copy of the save)
void GaussianTrainerScene::Impl::export_fused() {
    const auto t_start = std::chrono::steady_clock::now();
    fetch_host();
    std::vector<float> h[5];
    const size_t rows = (size_t)n * 45;
    d_xf_rows.reserve(rows * sizeof(float) + 16);
    DVS_OR_THROW(dvs_shn_relayout(ctx.get(), stream.get(), n, ex(P_SHN), d_xf_rows.get(), 0));
    const float* src[5] = {ex(P_POS), d_xf_rows.get(), ex(P_SCALE), ex(P_ROT), ex(P_OPA)};
    const size_t floats[5] = {(size_t)n * 3, rows, (size_t)n * 3, (size_t)n * 4, (size_t)n};
    for (int k = 0; k < 5; ++k) {
        h[k].resize(floats[k]);
        HIP_OR_THROW(hipMemcpyAsync(h[k].data(), src[k], floats[k] * sizeof(float), hipMemcpyDeviceToHost, stream.get()));
    }
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const std::string file = save_path(step, ".fused.ply");
    std::string err;
    if (!gsply::write_ply(file, (size_t)n, h[0].data(), host[P_SH0].data(), h[1].data(), h[4].data(), h[2].data(), h[3].data(), cfg.mipAntiliased, &err)) {
        logf_("export @%d: %s", step, err.c_str());
        return;
    }
    std::error_code ec;
    const auto bytes = std::filesystem::file_size(file, ec);
    logf_("export @%d: fused.ply %d splats, %llu bytes, %.2f ms", step, n, (unsigned long long)(ec ? 0 : bytes), ms_since(t_start));
}
