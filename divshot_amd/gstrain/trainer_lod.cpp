// trainer_lod.cpp — level-of-detail export (trainer.hpp; INTEGRATION.md "LOD export"): at a save, for k = 1..L, the full model merged on a
// lattice of R >> (k - 1) cells (dvs_lod_merge_count / dvs_lod_merge_write, include/dvs_export.h), scored on the held-out views when
// evaluation is on, taken into the export frame when one is set, and written as <modelPath>_<it>.lod<k>.ply in the full PLY's layout.
// Rank 0, on the training stream; the training arrays and the training context are never touched.
#include "trainer.hpp"

void GaussianTrainerScene::Impl::export_lod() {
    const int L = opt.i(gsopt::EXPORT_LOD), R = opt.i(gsopt::LOD_RESOLUTION);
    if (L <= 0 || rank != 0 || !ctx || n <= 0) return;
    HIP_OR_THROW(hipSetDevice(device));
    // the box of the finite centres, from the save's host copy: a centre with a non-finite coordinate is dropped by the merge and must
    // not widen the lattice (the packers' device bounds pass would let an infinite coordinate through)
    fetch_host();
    float bounds[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; ++i) {
        const float* p = &host[P_POS][3 * (size_t)i];
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        for (int k = 0; k < 3; ++k) { bounds[k] = std::min(bounds[k], p[k]); bounds[3 + k] = std::max(bounds[3 + k], p[k]); }
    }
    d_lod_scratch.reserve(dvs_lod_scratch_bytes(n));
    const float *pos = d_param[P_POS].get(), *sh0 = d_param[P_SH0].get(), *shN = d_param[P_SHN].get(), *opa = model_ex(P_OPA),
                *scale = model_ex(P_SCALE), *rot = d_param[P_ROT].get();
    for (int k = 1; k <= L; ++k) {
        const int res = R >> (k - 1);                                        // >= 32 >> 3 = 4: what dvs_lod_lattice_for takes
        dvs_lod_lattice lat;
        if (dvs_lod_lattice_for(bounds, res, &lat) != DVS_OK) {
            logf_("lod @%d: level %d: the finite centres span no box (%.9g,%.9g,%.9g .. %.9g,%.9g,%.9g): no level is written", step, k, (double)bounds[0],
                  (double)bounds[1], (double)bounds[2], (double)bounds[3], (double)bounds[4], (double)bounds[5]);
            return;
        }
        auto t0 = std::chrono::steady_clock::now();
        uint32_t counts[2] = {0, 0};
        int rc = dvs_lod_merge_count(stream.get(), n, pos, opa, scale, rot, &lat, d_lod_scratch.get(), counts);      // (synchronises)
        if (rc != DVS_OK) throw std::runtime_error("dvs_lod_merge_count: status " + std::to_string(rc));
        const double ms_count = ms_since(t0);
        const int m = (int)counts[0];
        t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < 6; ++g) d_lod[g].reserve(dev_floats_for(g, std::max(m, 1)) * sizeof(float) + 16);
        rc = dvs_lod_merge_write(stream.get(), n, sh_max, pos, sh0, shN, opa, scale, rot, DVS_SHN_TILED, d_lod_scratch.get(), d_lod[P_POS].get(),
                                 d_lod[P_SH0].get(), d_lod[P_SHN].get(), d_lod[P_OPA].get(), d_lod[P_SCALE].get(), d_lod[P_ROT].get(), DVS_SHN_TILED);
        if (rc != DVS_OK) throw std::runtime_error("dvs_lod_merge_write: status " + std::to_string(rc));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        const double ms_merge = ms_since(t0);
        // the score, in the cameras' frame: before the export transform
        double ms_score = 0.0;
        LodScore& sc = lod_score[k - 1];
        sc.it = -1;
        if (!test_idx.empty() && m > 0) {
            if (eval_it != step) run_evaluation();                           // the full model of the same parameters: the comparison
            t0 = std::chrono::steady_clock::now();
            std::vector<double> res_views;
            score_views(splats_of(d_lod, m), res_views, sc.mean);
            sc.it = step; sc.m = m;
            ms_score = ms_since(t0);
        }
        t0 = std::chrono::steady_clock::now();
        if (xf_set && m > 0) {                                               // like every other export: in the export frame, in place
            rc = dvs_transform_splats(stream.get(), m, sh_max, &xf, xf_D, d_lod[P_POS].get(), d_lod[P_SHN].get(), DVS_SHN_TILED, d_lod[P_SCALE].get(),
                                      d_lod[P_ROT].get(), d_lod[P_POS].get(), d_lod[P_SHN].get(), d_lod[P_SCALE].get(), d_lod[P_ROT].get());
            if (rc != DVS_OK) throw std::runtime_error("dvs_transform_splats (lod): status " + std::to_string(rc));
        }
        std::vector<float> h[6];
        if (m > 0) {
            d_lod_rows.reserve((size_t)m * 45 * sizeof(float) + 16);
            DVS_OR_THROW(dvs_shn_relayout(ctx.get(), stream.get(), m, d_lod[P_SHN].get(), d_lod_rows.get(), 0));
            for (int g = 0; g < 6; ++g) {
                h[g].resize((size_t)m * kWidth[g]);
                HIP_OR_THROW(hipMemcpyAsync(h[g].data(), g == P_SHN ? d_lod_rows.get() : d_lod[g].get(), h[g].size() * sizeof(float), hipMemcpyDeviceToHost,
                                            stream.get()));
            }
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        }
        const std::string file = save_path(step, (".lod" + std::to_string(k) + ".ply").c_str());
        std::string err;
        if (!gsply::write_ply(file, (size_t)m, h[P_POS].data(), h[P_SH0].data(), h[P_SHN].data(), h[P_OPA].data(), h[P_SCALE].data(), h[P_ROT].data(),
                              cfg.mipAntiliased, &err)) {
            logf_("lod @%d: %s", step, err.c_str());
            continue;
        }
        const double ms_file = ms_since(t0);
        char score[200] = "";
        if (sc.it == step)
            snprintf(score, sizeof score, "; PSNR %.17g dB (full model %.17g dB), SSIM %.17g, L1 %.17g, score %.2f ms", sc.mean[3], eval_mean[3], sc.mean[2],
                     sc.mean[1], ms_score);
        logf_("lod @%d: level %d, lattice %dx%dx%d (resolution %d, cell %.9g): %d -> %d splats, %u dropped; count %.2f ms, merge %.2f ms, %sfile %.2f ms%s -> %s",
              step, k, lat.dims[0], lat.dims[1], lat.dims[2], res, (double)lat.cell, n, m, counts[1], ms_count, ms_merge, xf_set ? "transform + " : "", ms_file,
              score, file.c_str());
    }
}
