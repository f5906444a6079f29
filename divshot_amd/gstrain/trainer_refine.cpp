// trainer_refine.cpp — what changes the number of splats between two iterations: ADC / ADC+ densification, MCMC relocation, light prune,
// importance prune, focus-region prune, mask carve.
#include "trainer.hpp"

// data parallel: the densification statistics are per-view sums / maxima — make them global before a refinement decision
void GaussianTrainerScene::Impl::sync_stats() {
    if (!comm) return;
    DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), stream.get(), d_grad_accum.get(), (size_t)n));
    DVS_OR_THROW(dvs_comm_all_reduce_sum_f32(comm.get(), stream.get(), d_denom.get(), (size_t)n));
    DVS_OR_THROW(dvs_comm_all_reduce_max_i32(comm.get(), stream.get(), d_max_radii.get(), (size_t)n));
}

// the plan parameters densify() and prune_light() share; everything else starts out zero (no size limit, plain opacity of the copies)
dvs_densify_params GaussianTrainerScene::Impl::plan_params(int it) const {
    dvs_densify_params prm{};
    prm.scale_threshold = 0.01f * extent;                       // percent_dense x extent
    prm.cap_max = 0; prm.seed = (uint32_t)it; prm.shn_layout = DVS_SHN_TILED;   // no kernel cap: densify() re-plans prune-only over capMax
    return prm;
}

// plans (d_action, d_offsets) on the statistics and waits for the count of splats the plan leaves
uint64_t GaussianTrainerScene::Impl::plan(const dvs_densify_params& prm) {
    uint64_t new_n = 0;
    DVS_OR_THROW(dvs_densify_plan(stream.get(), n, d_param[P_OPA].get(), d_param[P_SCALE].get(), d_grad_accum.get(), d_denom.get(), d_max_radii.get(),
                                  &prm, d_action.get(), d_offsets.get(), d_dscratch.get(), d_newcount.get()));
    HIP_OR_THROW(hipMemcpyAsync(&new_n, d_newcount.get(), 8, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    return new_n;
}

// applies the plan to the parameter, m and v sets (old -> new) and swaps the sets. The SH tile pads of every new set are zeroed
// first; with zero_moments (densify) the whole new m and v groups are
void GaussianTrainerScene::Impl::apply_plan(const dvs_densify_params& prm, int new_n, bool zero_moments) {
    for (int set = 0; set < 3; ++set) {
        DevBuf<float>* src = set == 0 ? d_param : (set == 1 ? d_m : d_v);
        DevBuf<float>* dst = set == 0 ? d_param2 : (set == 1 ? d_m2 : d_v2);
        const float* s6[6]; float* d6[6];
        for (int g = 0; g < 6; ++g) { s6[g] = src[g].get(); d6[g] = dst[g].get(); }
        for (int g = 0; g < 6; ++g)
            if (g == P_SHN || (set > 0 && zero_moments)) HIP_OR_THROW(hipMemsetAsync(d6[g], 0, dev_floats_for(g, new_n) * sizeof(float), stream.get()));
        DVS_OR_THROW(dvs_densify_apply(stream.get(), n, d_action.get(), d_offsets.get(), &prm, set == 0 ? 0 : 1, s6, d6, new_n));
        for (int g = 0; g < 6; ++g) std::swap(src[g], dst[g]);               // (the owners: what was written is now the live set)
    }
    f3d_dirty = true;                                                        // (mipFilter3d: another splat set, another filter)
}

// densifyStrategy 1 (MCMC): dead splats are relocated onto live ones drawn ~ opacity, then the model grows by 5 % up to the cap.
// In place: no second buffer set, no host round trip.
void GaussianTrainerScene::Impl::densify_mcmc(int it) {
    dvs_mcmc_sets sets{};
    for (int g = 0; g < 6; ++g) { sets.param[g] = d_param[g].get(); sets.m[g] = d_m[g].get(); sets.v[g] = d_v[g].get(); }
    DVS_OR_THROW(dvs_mcmc_relocate(stream.get(), n, &sets, cfg.min_opacity, 2u * (uint32_t)it, DVS_SHN_TILED, d_mcmc.get(), cap, nullptr));
    const int target = std::min(cap, (int)(1.05 * (double)n));
    const int n_new = target - n;
    if (n_new > 0) {
        DVS_OR_THROW(dvs_mcmc_grow(stream.get(), n, n_new, &sets, cfg.min_opacity, 2u * (uint32_t)it + 1u, DVS_SHN_TILED, d_mcmc.get(), cap));
        if (cfg.verbose) logf_("mcmc @%d: %d -> %d splats", it, n, n + n_new);
        n += n_new;
        HIP_OR_THROW(hipMemsetAsync(d_grad[P_SHN], 0, dev_floats_for(P_SHN, cap) * sizeof(float), stream.get()));   // pad lanes of the new last tile
    }
    f3d_dirty = true;                                                        // (mipFilter3d: relocated and new splats sit elsewhere)
    host_valid = false;
}

// clone / split / prune between two iterations (densifyStrategy 0 ADC; 2 "ADC+" is served by the same rule)
void GaussianTrainerScene::Impl::densify(int it) {
    sync_stats();
    dvs_densify_params prm = plan_params(it);
    prm.grad_threshold = cfg.growGrad2d;
    prm.min_opacity = cfg.min_opacity;
    const bool after_reset = it > cfg.resetAlphaEvery;
    prm.max_world_scale = after_reset ? cfg.pruneScale3d * extent : 0.f;                     // `pruneScale3d` (fraction of the scene extent)
    prm.max_screen_radius = after_reset && it < cfg.refineScale2dStopIter                    // `pruneScale2d` (fraction of the image size)
                                ? std::max(1, (int)(cfg.pruneScale2d * (float)std::max(lw, lh))) : 0;   // (max_radii is in pixels of the level)
    prm.revised_opacity = (cfg.revisedOpacity || cfg.densifyStrategy == 2) ? 1 : 0;      // ADC+ always uses the revised opacity of the copies
    uint64_t new_n = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        new_n = plan(prm);
        if (new_n <= (uint64_t)cap) break;
        prm.grad_threshold = 3.0e38f;                            // at the cap: prune only, no growth this round
    }
    if (new_n == 0 || new_n > (uint64_t)cap) { reset_stats(); return; }
    apply_plan(prm, (int)new_n, true);
    if (cfg.verbose) {
        logf_("densify @%d: %d -> %llu splats", it, n, (unsigned long long)new_n);
        uint64_t cap_ = 0, grows_ = 0, lastT_ = 0, over_ = 0;        // the rasterizer's instance arena at this point (HBM pressure of big scenes)
        if (dvs_get_arena_info(ctx.get(), &cap_, &grows_, &lastT_, &over_) == DVS_OK)
            logf_("raster @%d: T = %llu tile instances in the last pass, instance arena %llu (enlarged %llu times), overflowed forwards %llu",
                  it, (unsigned long long)lastT_, (unsigned long long)cap_, (unsigned long long)grows_, (unsigned long long)over_);
    }
    n = (int)new_n;
    HIP_OR_THROW(hipMemsetAsync(d_grad[P_SHN], 0, dev_floats_for(P_SHN, cap) * sizeof(float), stream.get()));   // pad lanes of the new last tile
    reset_stats();
    host_valid = false;
}

// pruneStrategy > 0 ("Light Gaussian Prune" in the reference's log, screenshots/cli_example.png): after refinement has stopped, every
// pruneInterval steps splats that became transparent (opacity < pruneOpacity) or oversized (scale > pruneScale3d x extent) are removed
// and the arrays compacted; no growth. Runs replicated (deterministic) on every rank.
void GaussianTrainerScene::Impl::prune_light(int it) {
    pruning = true;
    dvs_densify_params prm = plan_params(it);
    prm.grad_threshold = 3.0e38f;                               // never clone / split
    prm.min_opacity = std::max(cfg.pruneOpacity, cfg.min_opacity);       // --minOpacity is the only opacity threshold the CLI exposes
    prm.max_world_scale = cfg.pruneScale3d * extent;
    reset_stats();
    const uint64_t new_n = plan(prm);
    if (new_n > 0 && new_n < (uint64_t)n) {
        apply_plan(prm, (int)new_n, false);
        if (cfg.verbose && rank == 0) logf_("light prune @%d: %d -> %llu splats", it, n, (unsigned long long)new_n);
        n = (int)new_n;
        HIP_OR_THROW(hipMemsetAsync(d_grad_flat.get(), 0, grad_floats * sizeof(float), stream.get()));
        host_valid = false;
    }
    pruning = false;
}

// enableFocusRegion: the splats whose centre lies outside the region go (dvs_region_plan: extents are not looked at, a NaN centre is
// outside), the arrays and both Adam moments are compacted through the plan -> apply path, the gradients and the densification
// statistics start again as after an importance prune. Called right after load, at the start of the first trainStep() after the
// region or the flag changed, before every refinement (ADC and MCMC: relocation then draws from inside splats only), at every prune
// occasion before the light prune, and before every save. A plan that would leave no splat is logged and not applied. A pure function
// of the replicated positions and the region: every rank removes the same splats, no communication.
void GaussianTrainerScene::Impl::prune_region(int it) {
    region_dirty = false;
    if (n <= 0) return;
    uint64_t new_n = 0;
    DVS_OR_THROW(dvs_region_plan(stream.get(), n, d_param[P_POS].get(), &region, d_action.get(), d_offsets.get(), d_dscratch.get(), d_newcount.get()));
    HIP_OR_THROW(hipMemcpyAsync(&new_n, d_newcount.get(), 8, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    if (new_n == 0) { if (rank == 0) logf_("region prune @%d: none of the %d splats lies inside the focus region: nothing removed", it, n); return; }
    if (new_n >= (uint64_t)n) return;
    pruning = true;
    apply_plan(plan_params(it), (int)new_n, false);
    HIP_OR_THROW(hipMemsetAsync(d_grad_flat.get(), 0, grad_floats * sizeof(float), stream.get()));
    reset_stats();
    (void)dvs_raster_forward_cancel_prepared(ctx.get());                   // (a pipelined step may have projected the next iteration's splats already)
    if (cfg.verbose && rank == 0) logf_("region prune @%d: %d -> %llu splats", it, n, (unsigned long long)new_n);
    n = (int)new_n;
    host_valid = false;
    pruning = false;
}

// importancePrune = P > 0: at every prune occasion, after the light prune, the P % of the splats that contribute least to the training
// views go. The score of a splat is its blend weight alpha T summed over the pixels of all training cameras (dvs_raster_importance_views),
// rendered through the evaluation context (for_each_eval_pass, without the sky) under the camera's mask. dvs_importance_plan keeps
// the n - n P / 100 best exactly, ties by index; the existing apply path compacts the parameters and the moments. Every rank scores
// all training cameras itself: integer scores, an exact selection, no communication — the replicas stay bit-identical.
void GaussianTrainerScene::Impl::prune_importance(int it) {
    const int P = importance_prune();
    const int new_n = n - (int)((int64_t)n * P / 100);
    if (P <= 0 || new_n >= n || new_n <= 0) return;
    pruning = true;
    ensure_eval_ctx();
    if (!d_imp_score) {
        d_imp_score.alloc((size_t)cap * sizeof(uint64_t) + 16);
        d_imp_scratch.alloc(dvs_importance_scratch_bytes(cap));
    }
    const std::vector<int> which = training_cameras();
    const dvs_opts opts = eval_opts();
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    auto t0_ = std::chrono::steady_clock::now();
    HIP_OR_THROW(hipMemsetAsync(d_imp_score.get(), 0, (size_t)n * sizeof(uint64_t), stream.get()));
    for_each_eval_pass(splats(), which, false, [&](const EvalPass& p) {
        std::vector<const float*> masks((size_t)p.nb);
        for (int k = 0; k < p.nb; ++k) masks[(size_t)k] = view_mask((size_t)p.cam[k]);
        DVS_OR_THROW(dvs_raster_importance_views(eval_ctx.get(), stream.get(), &opts, masks.data(), d_imp_score.get(), nullptr, nullptr));
    });
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const double score_ms = ms_since(t0_);
    size_t never = 0;                                                        // (for the log line only: nothing below depends on the host copy)
    if (cfg.verbose && rank == 0) {
        std::vector<uint64_t> h((size_t)n);
        HIP_OR_THROW(hipMemcpy(h.data(), d_imp_score.get(), h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        never = (size_t)std::count(h.begin(), h.end(), (uint64_t)0);
    }
    t0_ = std::chrono::steady_clock::now();
    const dvs_densify_params prm = plan_params(it);
    DVS_OR_THROW(dvs_importance_plan(stream.get(), n, d_imp_score.get(), (uint32_t)new_n, d_action.get(), d_offsets.get(), d_imp_scratch.get(),
                                     d_newcount.get()));
    apply_plan(prm, new_n, false);
    HIP_OR_THROW(hipMemsetAsync(d_grad_flat.get(), 0, grad_floats * sizeof(float), stream.get()));
    reset_stats();
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    if (cfg.verbose && rank == 0)
        logf_("importance prune @%d: %d -> %d splats, %d views, %zu never taken, score %.2f ms, select+compact %.2f ms", it, n, new_n, (int)which.size(),
              never, score_ms, ms_since(t0_));
    n = new_n;
    host_valid = false;
    pruning = false;
}

// maskCarve = T > 0 (DVS_MASK_CARVE, setMaskCarve): the splats the views' masks call background go. Every training camera is rendered
// through the evaluation context (for_each_eval_pass, without the sky) and dvs_raster_foreground_views splits each splat's blend weight
// alpha T by where it landed: on pixels with a nonzero mask (foreground) or on the others (background); a view without a mask counts as
// foreground throughout, a pixel an undistortion left blank votes for nothing when the view kept its validity plane.
// dvs_foreground_plan keeps splat i iff fg > 0 and fg (100 - T) >= bg T, the existing apply path compacts the parameters and the
// moments, the gradients and the densification statistics start again as after an importance prune. Called at every prune occasion
// before the light prune and before every save, after the focus-region prune in both places. A plan that would leave no splat is
// logged and not applied. Every rank scores all training cameras itself: integer votes, an exact rule, no communication — the
// replicas stay bit-identical.
bool GaussianTrainerScene::Impl::carve_has_masks() const {
    for (int c : training_cameras()) if (view_mask((size_t)c)) return true;
    return false;
}
bool GaussianTrainerScene::Impl::carve_has_valid() const {
    for (int c : training_cameras()) if (views[(size_t)c].valid) return true;
    return false;
}
void GaussianTrainerScene::Impl::prune_mask_carve(int it) {
    const int T = opt.i(gsopt::MASK_CARVE);
    if (T <= 0 || n <= 0 || !carve_has_masks()) return;
    pruning = true;
    ensure_eval_ctx();
    const size_t half = ((size_t)cap + 1) & ~(size_t)1;                     // (an even count: both arrays on a 16-byte boundary)
    if (!d_carve_votes) d_carve_votes.alloc(2 * half * sizeof(uint64_t) + 16);
    uint64_t* const d_fg = d_carve_votes.get();
    uint64_t* const d_bg = d_fg + half;
    const std::vector<int> which = training_cameras();
    const dvs_opts opts = eval_opts();
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    auto t0_ = std::chrono::steady_clock::now();
    HIP_OR_THROW(hipMemsetAsync(d_fg, 0, (size_t)n * sizeof(uint64_t), stream.get()));
    HIP_OR_THROW(hipMemsetAsync(d_bg, 0, (size_t)n * sizeof(uint64_t), stream.get()));
    for_each_eval_pass(splats(), which, false, [&](const EvalPass& p) {
        std::vector<const float*> fg((size_t)p.nb), valid((size_t)p.nb);
        for (int k = 0; k < p.nb; ++k) { fg[(size_t)k] = view_mask((size_t)p.cam[k]); valid[(size_t)k] = views[(size_t)p.cam[k]].valid.get(); }
        DVS_OR_THROW(dvs_raster_foreground_views(eval_ctx.get(), stream.get(), &opts, fg.data(), valid.data(), d_fg, d_bg));
    });
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    const double votes_ms = ms_since(t0_);
    size_t never = 0;                                                        // (for the log line only: nothing below depends on the host copy)
    if (cfg.verbose && rank == 0) {
        std::vector<uint64_t> hf((size_t)n), hb((size_t)n);
        HIP_OR_THROW(hipMemcpy(hf.data(), d_fg, hf.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_OR_THROW(hipMemcpy(hb.data(), d_bg, hb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < hf.size(); ++i) never += (hf[i] | hb[i]) == 0;
    }
    t0_ = std::chrono::steady_clock::now();
    uint64_t new_n = 0;
    DVS_OR_THROW(dvs_foreground_plan(stream.get(), n, d_fg, d_bg, T, d_action.get(), d_offsets.get(), d_dscratch.get(), d_newcount.get()));
    HIP_OR_THROW(hipMemcpyAsync(&new_n, d_newcount.get(), 8, hipMemcpyDeviceToHost, stream.get()));
    HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    if (new_n == 0) {
        if (rank == 0) logf_("mask carve @%d: none of the %d splats has its blend weight on the foreground (threshold %d %%): nothing removed", it, n, T);
        pruning = false;
        return;
    }
    if (new_n < (uint64_t)n) {
        apply_plan(plan_params(it), (int)new_n, false);
        HIP_OR_THROW(hipMemsetAsync(d_grad_flat.get(), 0, grad_floats * sizeof(float), stream.get()));
        reset_stats();
        (void)dvs_raster_forward_cancel_prepared(ctx.get());               // (a pipelined step may have projected the next iteration's splats already)
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    }
    if (cfg.verbose && rank == 0)
        logf_("mask carve @%d: %d -> %llu splats, %d views, %zu never taken, votes %.2f ms, plan+compact %.2f ms", it, n, (unsigned long long)new_n,
              (int)which.size(), never, votes_ms, ms_since(t0_));
    if (new_n < (uint64_t)n) { n = (int)new_n; host_valid = false; }
    pruning = false;
}
