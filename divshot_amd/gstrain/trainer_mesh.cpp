// trainer_mesh.cpp — mesh export: the training cameras rendered through the evaluation context (for_each_eval_pass), their depth and alpha maps
// (dvs_raster_depth_views) fused into a TSDF grid and the grid's surface extracted by marching tetrahedra (include/dvs_mesh.h), written
// optionally given normals, freed of its small components (DVS_MESH_NORMALS, DVS_MESH_MIN_COMPONENT / setMeshCleanup) and decimated by
// vertex clustering (DVS_MESH_DECIMATE / setMeshDecimate) on the device, and written as a binary PLY (ply_io.hpp write_mesh_ply). Everything on the training stream; the training context is never touched.
#include "trainer.hpp"
#include "../../include/dvs_mesh.h"

namespace {
struct GridGuard {                                                           // frees the grid on every way out
    dvs_tsdf_grid g{};
    ~GridGuard() { dvs_tsdf_destroy(&g); }
};
}  // namespace

int GaussianTrainerScene::Impl::mesh_resolution() const { return env_int("DVS_MESH_RESOLUTION", cfg.meshResolution); }

// The box the grid covers: DVS_MESH_BOUNDS=x0,y0,z0,x1,y1,z1, or with enableFocusRegion the focus region's world bounds, or the box of the centres of the splats with sigmoid(opacity) >= 0.5
// cut to the cube of half-side 3 x extent about the camera centroid (extent: the scene extent the prune rules use).
bool GaussianTrainerScene::Impl::mesh_bounds(float lo[3], float hi[3]) {
    if (opt.given[gsopt::MESH_BOUNDS]) {
        for (int k = 0; k < 3; ++k) { lo[k] = opt.f(gsopt::MESH_BOUNDS, k); hi[k] = opt.f(gsopt::MESH_BOUNDS, 3 + k); }
        return true;
    }
    if (cfg.enableFocusRegion) {            // the world axis-aligned bounds of the region's eight corners
        for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
        for (int c = 0; c < 8; ++c) {
            const float b[3] = {(c & 1) ? focus_hi[0] : focus_lo[0], (c & 2) ? focus_hi[1] : focus_lo[1], (c & 4) ? focus_hi[2] : focus_lo[2]};
            for (int k = 0; k < 3; ++k) {
                const float w = region_b2w[4 * k] * b[0] + region_b2w[4 * k + 1] * b[1] + region_b2w[4 * k + 2] * b[2] + region_b2w[4 * k + 3];
                lo[k] = std::min(lo[k], w); hi[k] = std::max(hi[k], w);
            }
        }
        return hi[0] > lo[0] && hi[1] > lo[1] && hi[2] > lo[2];
    }
    fetch_host();
    double centre[3] = {0, 0, 0};
    for (const dvs_camera& c : cams) for (int k = 0; k < 3; ++k) centre[k] += c.campos[k] / (double)cams.size();
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int i = 0; i < n; ++i) {
        if (!(host[P_OPA][(size_t)i] >= 0.f)) continue;                      // sigmoid(o) >= 0.5 <=> o >= 0 (a NaN fails)
        for (int k = 0; k < 3; ++k) {
            const float p = host[P_POS][3 * (size_t)i + k];
            if (!std::isfinite(p)) continue;
            lo[k] = std::min(lo[k], p); hi[k] = std::max(hi[k], p);
        }
    }
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::max(lo[k], (float)(centre[k] - 3.0 * extent));
        hi[k] = std::min(hi[k], (float)(centre[k] + 3.0 * extent));
        if (!(hi[k] > lo[k])) return false;
    }
    return true;
}

// -> false when the grid does not fit the device or the file could not be written; throws on a failed device call. An empty box (no
// opaque splat inside the cube) gives the empty mesh. Rank 0 only.
bool GaussianTrainerScene::Impl::extract_mesh(const std::string& path, int resolution) {
    if (rank != 0 || !ctx || cams.empty()) return false;
    HIP_OR_THROW(hipSetDevice(device));
    const TrainingStatus before = status;
    status = TrainingStatus::GS2Mesh;
    struct Restore { TrainingStatus& s; TrainingStatus v; ~Restore() { s = v; } } restore{status, before};
    const int res = std::min(1024, std::max(16, resolution));
    if (res != resolution) logf_("mesh @%d: meshResolution %d clamped to %d (16..1024)", step, resolution, res);
    const auto write_ply = [&](uint32_t nv, const float* xyz, const uint8_t* rgb, uint32_t nt, const uint32_t* tri, const float* nrm) {
        std::error_code ec;
        const auto parent = std::filesystem::path(path).parent_path();
        if (!parent.empty()) std::filesystem::create_directories(parent, ec);
        std::string err;
        const bool ok = gsply::write_mesh_ply(path, nv, xyz, rgb, nt, tri, &err, nrm);
        if (!ok) logf_("mesh @%d: %s", step, err.c_str());
        return ok;
    };
    float lo[3], hi[3];
    if (!mesh_bounds(lo, hi)) {
        // nothing opaque inside the cube: the empty mesh, a valid file with zero elements, and the same log line
        static const float no_normals[3] = {0, 0, 0};                     // (zero vertices: only the header's nx ny nz)
        if (!write_ply(0, nullptr, nullptr, 0, nullptr, opt.on(gsopt::MESH_NORMALS) ? no_normals : nullptr)) return false;
        logf_("mesh @%d: 0 vertices, 0 triangles, grid 0x0x0, voxel 0, bounds %.9g,%.9g,%.9g,%.9g,%.9g,%.9g (no splat with opacity >= 0.5 within 3 x extent "
              "= %.9g of the cameras' centroid; DVS_MESH_BOUNDS sets the box), trunc 0, 0 views; render+depth 0.00 ms, fusion 0.00 ms, extraction 0.00 ms -> %s",
              step, (double)lo[0], (double)lo[1], (double)lo[2], (double)hi[0], (double)hi[1], (double)hi[2], 3.0 * (double)extent, path.c_str());
        return true;
    }
    const float longest = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    const float voxel = longest / (float)res;
    int32_t dims[3];
    for (int k = 0; k < 3; ++k) dims[k] = std::min(DVS_TSDF_MAX_DIM, std::max(2, (int)std::ceil((hi[k] - lo[k]) / voxel) + 1));
    const float trunc = opt.f(gsopt::MESH_TRUNC_VOXELS) * voxel;                  // (DVS_MESH_TRUNC_VOXELS, default 4)

    GridGuard grid;
    const int rc = dvs_tsdf_create(lo, voxel, dims, &grid.g);
    if (rc == DVS_ERR_CAPACITY) { logf_("mesh @%d: a %dx%dx%d grid (%zu bytes) does not fit the free device memory: no mesh", step, dims[0], dims[1], dims[2], dvs_tsdf_bytes(dims)); return false; }
    if (rc != DVS_OK) throw std::runtime_error("dvs_tsdf_create: status " + std::to_string(rc));

    // render + depth + fusion: a pass's depth and alpha maps from the forward for_each_eval_pass just ran, fused under the cameras' masks
    ensure_eval_ctx();
    const size_t map_bytes = (size_t)eval_views * W * H * sizeof(float);
    d_mesh_depth.reserve(map_bytes);
    d_mesh_alpha.reserve(map_bytes);
    const std::vector<int> which = training_cameras();
    const dvs_opts opts = eval_opts();
    double render_ms = 0, fuse_ms = 0;
    auto t0_ = std::chrono::steady_clock::now();                             // (a pass's forward is launched before its per_pass)
    for_each_eval_pass(splats(), which, false, [&](const EvalPass& p) {
        const float* masks[DVS_TSDF_MAX_VIEWS] = {};
        for (int k = 0; k < p.nb; ++k) masks[k] = view_mask((size_t)p.cam[k]);
        DVS_OR_THROW(dvs_raster_depth_views(eval_ctx.get(), stream.get(), &opts, d_mesh_depth.get(), d_mesh_alpha.get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        render_ms += ms_since(t0_);
        t0_ = std::chrono::steady_clock::now();
        const int ri = dvs_tsdf_integrate(stream.get(), &grid.g, p.cams, p.nb, d_mesh_depth.get(), d_mesh_alpha.get(), p.images, masks, W, H, trunc);
        if (ri != DVS_OK) throw std::runtime_error("dvs_tsdf_integrate: status " + std::to_string(ri));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
        fuse_ms += ms_since(t0_);
        t0_ = std::chrono::steady_clock::now();
    });

    // extraction, normals and clean-up when asked for, then the final arrays alone to the host
    const auto t_ex = std::chrono::steady_clock::now();
    DevBuf<void> scratch;
    scratch.alloc(dvs_mesh_scratch_bytes(dims) + 256);
    void* const sc = (void*)(((uintptr_t)scratch.get() + 255) & ~(uintptr_t)255);
    uint32_t nv = 0, nt = 0;
    const int rcount = dvs_mesh_extract_count(stream.get(), &grid.g, sc, &nv, &nt);
    if (rcount != DVS_OK) throw std::runtime_error("dvs_mesh_extract_count: status " + std::to_string(rcount));
    std::vector<float> xyz, nrm;
    std::vector<uint8_t> rgb;
    std::vector<uint32_t> tri;
    const bool want_normals = opt.on(gsopt::MESH_NORMALS);
    const uint32_t min_bp = (uint32_t)opt.i(gsopt::MESH_MIN_COMPONENT);
    bool cleaned = false;
    dvs_mesh_clean_info info{};
    double normals_ms = 0, clean_ms = 0, decimate_ms = 0;
    const int decimate = opt.i(gsopt::MESH_DECIMATE);
    bool decimated = false;
    dvs_mesh_decimate_info dinfo{};
    uint32_t dec_v0 = 0, dec_t0 = 0;
    if (nv > 0 && nt > 0) {
        DevBuf<float> d_xyz, d_nrm, c_xyz, c_nrm, m_xyz, m_nrm; DevBuf<uint8_t> d_rgb, c_rgb, m_rgb; DevBuf<uint32_t> d_tri, c_tri, m_tri;
        d_xyz.alloc((size_t)nv * 3 * sizeof(float)); d_rgb.alloc((size_t)nv * 3); d_tri.alloc((size_t)nt * 3 * sizeof(uint32_t));
        const int rw = dvs_mesh_extract_write(stream.get(), &grid.g, sc, d_xyz.get(), d_rgb.get(), d_tri.get());
        if (rw != DVS_OK) throw std::runtime_error("dvs_mesh_extract_write: status " + std::to_string(rw));
        const float *f_xyz = d_xyz.get(), *f_nrm = nullptr; const uint8_t* f_rgb = d_rgb.get(); const uint32_t* f_tri = d_tri.get();   // the final arrays
        if (want_normals) {
            d_nrm.alloc((size_t)nv * 3 * sizeof(float));
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));                // (the timers' boundary; only when normals are asked for)
            const auto t_n = std::chrono::steady_clock::now();
            const int rn = dvs_mesh_extract_normals(stream.get(), &grid.g, sc, d_nrm.get());
            if (rn != DVS_OK) throw std::runtime_error("dvs_mesh_extract_normals: status " + std::to_string(rn));
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
            normals_ms = ms_since(t_n);
            f_nrm = d_nrm.get();
        }
        if (min_bp > 0) {
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
            const auto t_c = std::chrono::steady_clock::now();
            DevBuf<void> cscratch;
            cscratch.alloc(dvs_mesh_clean_scratch_bytes(nv, nt) + 256);
            void* const cs = (void*)(((uintptr_t)cscratch.get() + 255) & ~(uintptr_t)255);
            const int rc_ = dvs_mesh_clean_count(stream.get(), nv, d_tri.get(), nt, min_bp, cs, &info);
            if (rc_ != DVS_OK) throw std::runtime_error("dvs_mesh_clean_count: status " + std::to_string(rc_));
            c_xyz.alloc(std::max<size_t>(1, info.kept_vertices) * 3 * sizeof(float)); c_rgb.alloc(std::max<size_t>(1, info.kept_vertices) * 3);
            c_tri.alloc(std::max<size_t>(1, info.kept_triangles) * 3 * sizeof(uint32_t));
            if (want_normals) c_nrm.alloc(std::max<size_t>(1, info.kept_vertices) * 3 * sizeof(float));
            const int rcw = dvs_mesh_clean_write(stream.get(), nv, d_xyz.get(), d_rgb.get(), f_nrm, d_tri.get(), nt, cs, c_xyz.get(), c_rgb.get(),
                                                 want_normals ? c_nrm.get() : nullptr, c_tri.get());
            if (rcw != DVS_OK) throw std::runtime_error("dvs_mesh_clean_write: status " + std::to_string(rcw));
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
            clean_ms = ms_since(t_c);
            cleaned = true;
            nv = info.kept_vertices; nt = info.kept_triangles;
            f_xyz = c_xyz.get(); f_rgb = c_rgb.get(); f_tri = c_tri.get(); f_nrm = want_normals ? c_nrm.get() : nullptr;
        }
        if (decimate > 0) {
            // last: vertex clustering on the voxel lattice shifted by half a voxel (the grid's own planes, where the vertices of axis
            // edges lie, are then no cell faces), `decimate` voxels per cell and axis
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
            const auto t_d = std::chrono::steady_clock::now();
            const float cell = (float)decimate * voxel;
            float origin[3]; int32_t ncell[3];
            for (int k = 0; k < 3; ++k) { origin[k] = lo[k] - 0.5f * voxel; ncell[k] = (dims[k] + decimate - 1) / decimate; }
            DevBuf<void> dscratch;
            dscratch.alloc(dvs_mesh_decimate_scratch_bytes(nv, nt) + 256);
            void* const ds = (void*)(((uintptr_t)dscratch.get() + 255) & ~(uintptr_t)255);
            const int rdc = dvs_mesh_decimate_count(stream.get(), nv, f_xyz, f_tri, nt, origin, cell, ncell, ds, &dinfo);
            if (rdc != DVS_OK) throw std::runtime_error("dvs_mesh_decimate_count: status " + std::to_string(rdc));
            m_xyz.alloc(std::max<size_t>(1, dinfo.out_vertices) * 3 * sizeof(float)); m_rgb.alloc(std::max<size_t>(1, dinfo.out_vertices) * 3);
            m_tri.alloc(std::max<size_t>(1, dinfo.out_triangles) * 3 * sizeof(uint32_t));
            if (want_normals) m_nrm.alloc(std::max<size_t>(1, dinfo.out_vertices) * 3 * sizeof(float));
            const int rdw = dvs_mesh_decimate_write(stream.get(), nv, f_xyz, f_rgb, f_nrm, f_tri, nt, ds, m_xyz.get(), m_rgb.get(),
                                                    want_normals ? m_nrm.get() : nullptr, m_tri.get());
            if (rdw != DVS_OK) throw std::runtime_error("dvs_mesh_decimate_write: status " + std::to_string(rdw));
            HIP_OR_THROW(hipStreamSynchronize(stream.get()));
            decimate_ms = ms_since(t_d);
            decimated = true;
            dec_v0 = nv; dec_t0 = nt;
            nv = dinfo.out_vertices; nt = dinfo.out_triangles;
            f_xyz = m_xyz.get(); f_rgb = m_rgb.get(); f_tri = m_tri.get(); f_nrm = want_normals ? m_nrm.get() : nullptr;
        }
        xyz.resize((size_t)nv * 3); rgb.resize((size_t)nv * 3); tri.resize((size_t)nt * 3);
        if (want_normals) nrm.resize((size_t)nv * 3);
        if (nv > 0 && xf_set) {                                              // the export frame, in place on the final arrays (they are this call's own): the model files' frame
            const int rt = dvs_transform_points(stream.get(), (int)nv, &xf, f_xyz, f_nrm, const_cast<float*>(f_xyz), const_cast<float*>(f_nrm));
            if (rt != DVS_OK) throw std::runtime_error("dvs_transform_points: status " + std::to_string(rt));
        }
        if (nv > 0) {
            HIP_OR_THROW(hipMemcpyAsync(xyz.data(), f_xyz, xyz.size() * sizeof(float), hipMemcpyDeviceToHost, stream.get()));
            HIP_OR_THROW(hipMemcpyAsync(rgb.data(), f_rgb, rgb.size(), hipMemcpyDeviceToHost, stream.get()));
            if (want_normals) HIP_OR_THROW(hipMemcpyAsync(nrm.data(), f_nrm, nrm.size() * sizeof(float), hipMemcpyDeviceToHost, stream.get()));
        }
        if (nt > 0) HIP_OR_THROW(hipMemcpyAsync(tri.data(), f_tri, tri.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream.get()));
        HIP_OR_THROW(hipStreamSynchronize(stream.get()));
    } else { nv = 0; nt = 0; }
    const double extract_ms = ms_since(t_ex) - normals_ms - clean_ms - decimate_ms;        // (count, write and the copies to the host, as before)
    char extras[512] = "";
    if (cleaned)
        snprintf(extras, sizeof extras, ", cleanup: %u of %u components kept (largest %u triangles, min %g %%), %.2f ms", info.kept_components,
                 info.n_components, info.largest, min_bp / 100.0, clean_ms);
    if (want_normals) snprintf(extras + strlen(extras), sizeof extras - strlen(extras), ", normals %.2f ms", normals_ms);
    if (decimated)
        snprintf(extras + strlen(extras), sizeof extras - strlen(extras), ", decimate: %d voxels per cell, %u -> %u vertices, %u -> %u triangles (%u degenerate, "
                 "%u duplicate), %.2f ms", decimate, dec_v0, nv, dec_t0, nt, dinfo.n_degenerate, dinfo.n_duplicate, decimate_ms);

    if (!write_ply(nv, xyz.data(), rgb.data(), nt, tri.data(), want_normals ? nrm.data() : nullptr)) return false;
    logf_("mesh @%d: %u vertices, %u triangles, grid %dx%dx%d, voxel %.9g, bounds %.9g,%.9g,%.9g,%.9g,%.9g,%.9g, trunc %.9g, %d views; render+depth %.2f ms, "
          "fusion %.2f ms, extraction %.2f ms%s%s -> %s", step, nv, nt, dims[0], dims[1], dims[2], (double)voxel, (double)lo[0], (double)lo[1], (double)lo[2],
          (double)(lo[0] + (dims[0] - 1) * voxel), (double)(lo[1] + (dims[1] - 1) * voxel), (double)(lo[2] + (dims[2] - 1) * voxel), (double)trunc,
          (int)which.size(), render_ms, fuse_ms, extract_ms, extras,
          xf_set ? "; grid, voxel and bounds are those of the extraction, in the training frame: the vertices and normals are written in the export frame" : "", path.c_str());
    return true;
}
