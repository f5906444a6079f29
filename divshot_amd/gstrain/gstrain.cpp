// gstrain.cpp — MI355X-native `libgstrain.so`: the plugin DIVSHOT's hosts dlopen (PluginManager::ensure_plugin_loaded
// ("gstrain"), application/diverseshot-cli/source/gs_train.cpp:16-23 -> diverse/diverse_base/source/core/plugin.cpp:74,89)
// and drive through nine C symbols (gs_train.cpp:24,105-109,144-150,178) plus the two every plugin exports
// (plugin.cpp:89-111). The reference's implementation is closed source (README.md:46); this one keeps its call
// sequence and ownership rules (scene allocated/freed by the plugin, config copied, bool from load_train_data) and
// puts the MI355X rasterizer (include/dvs_raster.h) at the centre of train_step():
//     sample camera -> dvs_raster_forward -> (1-w) L1 + w (1-SSIM) loss gradient -> dvs_raster_backward -> fused Adam -> step++
// -> every refineEvery steps the densification strategy (0 ADC clone / split / prune, 1 MCMC relocation + growth, 2 ADC+), the
// opacity reset every resetAlphaEvery steps, a light prune pass every pruneInterval steps after refinement has stopped.
// With WORLD_SIZE > 1 (one process per GPU, launched with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT) the step is
// data parallel: every rank holds a replica, renders its own camera of the iteration, the gradient rows are summed
// with ONE RCCL all-reduce over xGMI (include/dvs_comm.h), the densification statistics likewise before each refinement, and the
// optimizer / densifier run replicated and deterministic so that the replicas stay bit-identical.
// With resolutionSchedule > 0 the first steps train coarse to fine: on box-filtered views of 1/2^k the size, through level cameras.
// load_train_data accepts a capture directory (a COLMAP sparse model plus PPM or baseline JPEG images: dataset_io.hpp; views of
// SIMPLE_RADIAL / RADIAL / OPENCV cameras are undistorted on the device, include/dvs_image.h; the splats start from the sparse points,
// include/dvs_init.h) or a synthetic-scene spec. Out of scope: PNG and progressive-JPEG
// decoding, fisheye / FULL_OPENCV / FOV camera models, training for mesh export with the normal-consistency loss, the 2DGS model type
// (mesh export itself — depth maps, TSDF fusion, marching tetrahedra — is trainer_mesh.cpp). Every GaussianTrainConfig field the hosts set is either
// honoured or named in the one-time "ignored" line of report_config().
#include "trainer.hpp"

GaussianTrainerScene::GaussianTrainerScene(const GaussianTrainConfig& cfg, int loadItr) : impl_(new Impl()) {
    Impl& m = *impl_;
    m.cfg = cfg;
    m.loadItr = loadItr;
    m.opt = gsopt::read_env([](const std::string& line) { logf_("%s", line.c_str()); });     // before any setter can be called: a setter wins
    m.device = env_int("LOCAL_RANK", 0);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw std::runtime_error("gstrain: no HIP device visible (this plugin has no CPU fallback)");
    m.device %= count;
    HIP_OR_THROW(hipSetDevice(m.device));
    hipStream_t stream = nullptr;
    HIP_OR_THROW(hipStreamCreate(&stream));
    m.stream.reset(stream);
    // data parallel when launched as one process per GPU (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT); DVS_FORCE_COMM=1 runs the
    // collectives on a 1-rank communicator too (single-GPU proof of the RCCL path)
    const int world = env_int("WORLD_SIZE", 1);
    if (world > 1 || env_is("DVS_FORCE_COMM", "1")) {
        m.comm.reset(dvs_comm_create(m.device, env_int("RANK", 0), std::max(1, world), nullptr, 0));
        if (!m.comm) throw std::runtime_error(std::string("gstrain: dvs_comm_create failed: ") + dvs_last_error());
        m.rank = dvs_comm_rank(m.comm.get()); m.world = dvs_comm_world(m.comm.get());
        m.factorised = !env_is("DVS_EXCHANGE", "allreduce");
        logf_("rank %d of %d on device %d: %s communicator up, gradient exchange: %s", m.rank, m.world, m.device,
              env_is("DVS_COMM_BACKEND", "tcp") ? "host-staged TCP (TEST backend)" : "RCCL",
              m.factorised ? "factorised (all-gather of colour gradients + all-reduce of 44 B/splat)" : "all-reduce of all rows");
    }
}
GaussianTrainerScene::~GaussianTrainerScene() = default;

bool GaussianTrainerScene::loadTrainData(const std::string& path) {
    Impl& m = *impl_;
    try {
        HIP_OR_THROW(hipSetDevice(m.device));
        const bool synthetic = path.rfind("synthetic", 0) == 0;
        std::error_code ec;
        if (synthetic || std::filesystem::is_directory(path, ec)) {
            if (!(synthetic ? m.load_synthetic(path) : m.load_dataset(path))) { m.status = TrainingStatus::Loading_Failed; return false; }
            m.status = TrainingStatus::Preprocess_Done;
            focus_region_rotation.x = m.focus_trs[3]; focus_region_rotation.y = m.focus_trs[4]; focus_region_rotation.z = m.focus_trs[5];   // (DVS_FOCUS_ROTATION)
            trainSetup();
            return true;
        }
        logf_("load_train_data('%s'): not a directory; give a capture directory (sparse/0/ or sparse/ with cameras, images, points3D as .bin or .txt, and images/ "
              "as binary PPM) or a 'synthetic:N=..,W=..,H=..,cams=..,sh=..,seed=..' spec", path.c_str());
    } catch (const std::exception& e) {
        logf_("load_train_data failed: %s", e.what());
    }
    m.status = TrainingStatus::Loading_Failed;
    return false;
}

void GaussianTrainerScene::trainSetup() {
    impl_->t0 = std::chrono::steady_clock::now();
    impl_->status = TrainingStatus::Training;
    curIteration = impl_->step;
}

void GaussianTrainerScene::trainStep() {
    Impl& m = *impl_;
    if (!m.ctx || m.cams.empty()) throw std::runtime_error("trainStep before loadTrainData");
    HIP_OR_THROW(hipSetDevice(m.device));
    // focus region: the editor flips the flag in the config itself, so a change shows only here. While the flag is off both tests are
    // false and nothing happens; the prune runs before plan_step(), which takes the arrays' addresses and the splat count.
    if (m.cfg.enableFocusRegion != m.region_flag_seen) { m.region_flag_seen = m.cfg.enableFocusRegion; m.region_dirty = true; }
    if (m.cfg.enableFocusRegion && m.region_dirty) m.prune_region(m.step + 1);
    Impl::Step s = m.plan_step();
    if (m.res_every > 0) m.enter_level(s);
    m.lw = s.Wd; m.lh = s.Hd;
    HIP_OR_THROW(hipMemsetAsync(m.d_loss.get(), 0, 2 * DVS_SSIM_SLOTS * sizeof(float), m.stream.get()));
    m.render_backward(s);
    const bool pipelined = m.pipeline && s.n_chunks > 0;
    m.exchange(s, pipelined);
    if (pipelined) m.finish_pipelined(s);
    else if (m.exchange_factorised()) m.finish_range(s, 0, m.n, kGeomGroups, 4, s.adam_gate);     // (the SH groups were stepped in exchange())
    else m.finish_range(s, 0, m.n, kAllGroups, 6, s.adam_gate);
    m.step_sky(s);                                                          // (nothing when enableBg is off)
    if (s.refine_now) {
        if (m.cfg.enableFocusRegion) m.prune_region(s.it);                   // (MCMC: relocation draws from inside splats only)
        if (s.mcmc) m.densify_mcmc(s.it); else m.densify(s.it);
    }
    if (s.reset_now)
        DVS_OR_THROW(dvs_reset_opacity(m.stream.get(), m.n, m.d_param[P_OPA].get(), 0.01f, m.d_m[P_OPA].get(), m.d_v[P_OPA].get()));
    if (s.prune_now) {
        if (m.cfg.enableFocusRegion) m.prune_region(s.it);
        m.prune_mask_carve(s.it);                                            // (nothing when maskCarve is 0)
        m.prune_light(s.it);
        m.prune_importance(s.it);                                            // (nothing when importancePrune is 0)
        pruenIteraions.push_back(s.it);
    }
    // same line the editor logs (application/editor/source/editor.cpp:1554), every 100 steps as there unless DVS_LOSS_EVERY said otherwise at load
    if (m.cfg.verbose && m.rank == 0 && (m.step % m.loss_every == 0))
        logf_("Iteraions %d, loss : %f", m.step, (double)getCurrentLoss());
    m.step = s.it;
    curIteration = s.it;
    m.host_valid = false;
    if (m.step >= m.cfg.numIters) { m.status = TrainingStatus::Training_Done; m.close_level(); }
    if (m.eval_every > 0 && m.step % m.eval_every == 0) m.evaluate(false);
}

void GaussianTrainerScene::saveGaussianModel() {
    Impl& m = *impl_;
    if (m.cfg.enableFocusRegion && m.ctx) m.prune_region(m.step);           // what is written holds inside splats only (every rank: the replicas stay identical)
    if (m.ctx) m.prune_mask_carve(m.step);                                  // (nothing when maskCarve is 0; every rank, like the region prune)
    struct SaveSet { bool& in_use; ~SaveSet() { in_use = false; } } save_set{m.f3d_save};      // the save's own fused set belongs to this save alone
    if (m.ctx) m.filter3d_for_save();                                       // (nothing when mipFilter3d is 0: the exports below pack the model fused at the saved positions)
    // the replicas are identical: one file — unless DVS_SAVE_ALL_RANKS=1 asks every rank for its own (<model>_<it>.ply.rank<r>), which
    // is how the two-rank test checks that they ARE identical, bit for bit
    static const bool all_ranks = env_is("DVS_SAVE_ALL_RANKS", "1");
    if (m.rank != 0 && !all_ranks) return;
    const auto t_save = std::chrono::steady_clock::now();
    m.fetch_host();
    const std::string file = m.model_file(m.step) + (m.rank != 0 ? ".rank" + std::to_string(m.rank) : std::string());
    std::error_code ec;
    const auto parent = std::filesystem::path(file).parent_path();
    if (!parent.empty()) std::filesystem::create_directories(parent, ec);
    std::string err;
    if (!gsply::write_ply(file, (size_t)m.n, m.host[0].data(), m.host[1].data(), m.host[2].data(), m.host[3].data(), m.host[4].data(),
                          m.host[5].data(), m.cfg.mipAntiliased, &err))
        logf_("save_splat_model: %s", err.c_str());
    else if (m.cfg.verbose) logf_("saved %d splats to %s", m.n, file.c_str());
    m.save_sky();                                                           // <modelPath>_<it>.sky[.rank<r>] (enableBg on)
    if (m.rank == 0 && m.export_formats()) {                                // the comparison for the compact exports' lines below
        std::error_code fec;
        const auto ply_bytes = std::filesystem::file_size(file, fec);
        logf_("export @%d: ply %d splats, %llu bytes, %.2f ms", m.step, m.n, (unsigned long long)(fec ? 0 : ply_bytes), ms_since(t_save));
    }
    if (m.rank == 0 && m.export_formats()) {
        struct Done { bool& filled; ~Done() { filled = false; } } done{m.xf_filled};      // the transformed set belongs to this save alone
        if (m.xf_set) m.fill_transformed();                                  // (an export transform is set: the exports below pack from it)
        for (int format : {(int)Impl::EXPORT_COMPRESSED, (int)Impl::EXPORT_SPLAT, (int)Impl::EXPORT_SPZ, (int)Impl::EXPORT_REDUCED, (int)Impl::EXPORT_TRANSFORMED, (int)Impl::EXPORT_FUSED})
            if (m.export_formats() & format) m.export_model(format);
    }
    if (m.rank == 0 && m.opt.i(gsopt::EXPORT_LOD) > 0) m.export_lod();                  // <modelPath>_<it>.lod<k>.ply (DVS_EXPORT_LOD / setLodExport)
    m.evaluate(true);                                                       // <modelPath>_<it>_eval.json beside the PLY (rank 0, evaluation on)
    m.render_at_save();                                                     // <modelPath>_<it>_renders/*.jpg (rank 0, renderViews on)
    if (m.rank == 0 && m.mesh_resolution() > 0 && m.status == TrainingStatus::Training_Done)
        m.extract_mesh(m.mesh_file(m.step), m.mesh_resolution());           // <modelPath>_<it>_mesh.ply (the finished model only)
}

// export_mesh() / exportMesh(""): <modelPath>_<it>_mesh.ply when meshResolution (DVS_MESH_RESOLUTION) > 0, else today's log line and no
// file; exportMesh(path): that file, at resolution 256 when the field is 0.
void GaussianTrainerScene::exportMesh(const std::string& path) {
    Impl& m = *impl_;
    const int res = m.mesh_resolution();
    if (path.empty() && res <= 0) { logf_("export_mesh: mesh extraction is outside this build's scope"); return; }
    m.extract_mesh(path.empty() ? m.mesh_file(m.step) : path, res > 0 ? res : 256);
}
// The editor's switches for what the extension variables set for the CLI (ext_options.hpp): they write the fields the environment
// filled when the scene was made, so once called they win over it; an argument outside the row's bounds is reported and replaced.
void GaussianTrainerScene::setMeshCleanup(float minComponentPercent, bool normals) {
    Impl& m = *impl_;
    const float p = std::isfinite(minComponentPercent) ? std::min(100.0f, std::max(0.0f, minComponentPercent)) : 0.0f;
    m.opt.set(gsopt::MESH_MIN_COMPONENT, (double)std::lround((double)p * 100.0));
    m.opt.set(gsopt::MESH_NORMALS, normals);
}
void GaussianTrainerScene::setMeshDecimate(int factor) {
    Impl& m = *impl_;
    if (!gsopt::admits(gsopt::MESH_DECIMATE, factor)) { logf_("setMeshDecimate: %d is not 0 (off) or a factor 2..16: decimation is off", factor); factor = 0; }
    m.opt.set(gsopt::MESH_DECIMATE, factor);
}
void GaussianTrainerScene::setLodExport(int levels, int resolution) {
    Impl& m = *impl_;
    if (!gsopt::admits(gsopt::EXPORT_LOD, levels)) { logf_("setLodExport: %d is not a number of levels 0 (off) .. 4: LOD export is off", levels); levels = 0; }
    if (!gsopt::admits(gsopt::LOD_RESOLUTION, resolution)) { logf_("setLodExport: %d is not a resolution 32..1024: 256 is used", resolution); resolution = 256; }
    m.opt.set(gsopt::EXPORT_LOD, levels); m.opt.set(gsopt::LOD_RESOLUTION, resolution);
    if (levels > 0 && m.rank == 0) logf_("config: lodExport %d levels, resolution %d (setLodExport)", levels, resolution);
}
void GaussianTrainerScene::setMaskCarve(int percent) {
    Impl& m = *impl_;
    if (!gsopt::admits(gsopt::MASK_CARVE, percent)) { logf_("setMaskCarve: %d is not a percentage 0 (off) .. 100: the mask carve is off", percent); percent = 0; }
    m.opt.set(gsopt::MASK_CARVE, percent);
    m.report_mask_carve("setMaskCarve");
}
void GaussianTrainerScene::setMipFilter3d(bool on) {
    Impl& m = *impl_;
    m.opt.set(gsopt::MIP_FILTER3D, on);
    if (m.rank == 0) logf_("config: mipFilter3d %d (setMipFilter3d): in force from the next loadTrainData / resetGaussian", (int)on);
}
void GaussianTrainerScene::setReducedExport(float shCullThreshold, bool halfFloat) {
    Impl& m = *impl_;
    if (!gsopt::admits(gsopt::SH_CULL_THRESHOLD, shCullThreshold)) { logf_("setReducedExport: the threshold %g is not a number >= 0: 0.01 is used", (double)shCullThreshold); shCullThreshold = 0.01f; }
    m.opt.set(gsopt::SH_CULL_THRESHOLD, shCullThreshold); m.opt.set(gsopt::REDUCED_HALF, halfFloat);
}
// The editor's "export apply transform": what DVS_EXPORT_TRANSFORM / DVS_EXPORT_ORIENT set for the CLI. The last call wins.
bool GaussianTrainerScene::setExportTransform(const dvs_types::Vec3& position, const dvs_types::Vec3& rotationEulerRad, float scale) {
    Impl& m = *impl_;
    const float t[3] = {position.x, position.y, position.z}, e[3] = {rotationEulerRad.x, rotationEulerRad.y, rotationEulerRad.z};
    dvs_similarity sim;
    if (dvs_similarity_from_trs(t, e, scale, &sim) != DVS_OK) {
        logf_("setExportTransform: position (%g, %g, %g), rotation (%g, %g, %g), scale %g refused (finite numbers, scale > 0): the export frame stays as it was",
              (double)t[0], (double)t[1], (double)t[2], (double)e[0], (double)e[1], (double)e[2], (double)scale);
        return false;
    }
    char how[200];
    snprintf(how, sizeof how, "setExportTransform(T(%g, %g, %g) R(%g, %g, %g rad, Rz Ry Rx) S(%g))", (double)t[0], (double)t[1], (double)t[2], (double)e[0],
             (double)e[1], (double)e[2], (double)scale);
    if (!m.set_export_transform(sim, how)) return false;
    m.report_export_transform();
    return true;
}
bool GaussianTrainerScene::setExportOrientation(const std::string& axis) {
    Impl& m = *impl_;
    if (m.cams.empty()) { logf_("setExportOrientation before loadTrainData: there are no cameras yet"); return false; }
    if (!m.set_export_orientation(axis.c_str(), "setExportOrientation")) return false;
    m.report_export_transform();
    return true;
}
void GaussianTrainerScene::clearExportTransform() { impl_->xf_set = false; }
void GaussianTrainerScene::exportSparsePointCloud(const std::string& path) {
    Impl& m = *impl_;
    m.fetch_host();
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { logf_("exportSparsePointCloud: cannot open %s", path.c_str()); return; }
    fprintf(f, "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n", m.n);
    for (int i = 0; i < m.n; ++i) fprintf(f, "%g %g %g\n", m.host[P_POS][3 * i], m.host[P_POS][3 * i + 1], m.host[P_POS][3 * i + 2]);
    fclose(f);
}
void GaussianTrainerScene::saveCameraDatas(const std::string& path) {
    Impl& m = *impl_;
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { logf_("saveCameraDatas: cannot open %s", path.c_str()); return; }
    for (size_t c = 0; c < m.cams.size(); ++c) {
        const dvs_camera& k = m.cams[c];
        fprintf(f, "%zu %d %d %g %g %g %g %g", c, k.width, k.height, k.focal_x, k.focal_y, k.campos[0], k.campos[1], k.campos[2]);
        for (int e = 0; e < 16; ++e) fprintf(f, " %g", k.view[e]);
        fputc('\n', f);
    }
    fclose(f);
}
bool GaussianTrainerScene::isTerminate() const { return impl_->terminate; }
void GaussianTrainerScene::terminate() { impl_->terminate = true; }
bool GaussianTrainerScene::isPruningSplat() const { return impl_->pruning; }
void GaussianTrainerScene::resetGaussian() {
    Impl& m = *impl_;
    if (!m.ctx || m.init_host[P_OPA].empty()) return;
    HIP_OR_THROW(hipSetDevice(m.device));
    HIP_OR_THROW(hipStreamSynchronize(m.stream.get()));
    m.n = (int)m.init_host[P_OPA].size();
    for (int g = 0; g < 6; ++g) {
        const size_t bytes = m.dev_floats_for(g, m.cap) * sizeof(float);
        for (DevBuf<float>* p : {&m.d_param[g], &m.d_m[g], &m.d_v[g]}) HIP_OR_THROW(hipMemset(p->get(), 0, bytes));
        m.upload(g, m.init_host[g]);
    }
    HIP_OR_THROW(hipMemset(m.d_grad_flat.get(), 0, m.grad_floats * sizeof(float)));
    if (m.sky_on) for (DevBuf<float>* b : {&m.d_sky, &m.d_sky_m, &m.d_sky_v}) HIP_OR_THROW(hipMemset(b->get(), 0, m.sky_floats() * sizeof(float)));
    m.reset_stats();
    m.step = 0; curIteration = 0; pruenIteraions.clear();
    m.eval_it = -1;
    m.region_dirty = true;                                                  // (the initial splats are all back: the next step prunes them again)
    m.setup_filter3d();                                                     // (what setMipFilter3d said since; on: the filter of the initial splats at the next use)
    m.cur_level = -1; m.lw = m.W; m.lh = m.H;
    m.host_valid = false;
    (void)dvs_raster_forward_cancel_prepared(m.ctx.get());          // (a pipelined step may have projected the next iteration's splats already)
    m.status = TrainingStatus::Training;
    m.t0 = std::chrono::steady_clock::now();
}
void GaussianTrainerScene::setDensifyStrategy(int strategy) { impl_->cfg.densifyStrategy = std::min(2, std::max(0, strategy)); impl_->report_config(); }
void GaussianTrainerScene::setModelPath(const std::string& path) {
    const int before = impl_->export_formats();
    impl_->cfg.modelPath = path;
    if (impl_->export_formats() != before) impl_->report_config();         // the editor's "Splat Format" arrives as the suffix of the path
}
void GaussianTrainerScene::updateFocusRegion(const dvs_types::Vec3& position, const dvs_types::Vec3& rotation, const dvs_types::Vec3& scale) {
    // F = T(position) R(rotation) S(scale), the editor's own maths::Transform (include/dvs_region.h); a zero scale component is refused with
    // a log line and the previous region stays, in the public fields too. The next trainStep() prunes to the new region.
    const float pos[3] = {position.x, position.y, position.z}, rot[3] = {rotation.x, rotation.y, rotation.z}, sc[3] = {scale.x, scale.y, scale.z};
    if (!impl_->set_region(pos, rot, sc)) return;
    focus_region_position = position; focus_region_rotation = rotation; focus_region_scale = scale;
}
// (lo, hi) of the region in ITS OWN coordinates and F, box-local -> world: the editor draws F applied to the box's twelve edges
// (scene_view_panel.cpp:1393-1415)
std::pair<dvs_types::Vec3, dvs_types::Vec3> GaussianTrainerScene::getFocusRegion() const {
    dvs_types::Vec3 a{}, b{};
    a.x = impl_->focus_lo[0]; a.y = impl_->focus_lo[1]; a.z = impl_->focus_lo[2];
    b.x = impl_->focus_hi[0]; b.y = impl_->focus_hi[1]; b.z = impl_->focus_hi[2];
    return {a, b};
}
dvs_types::Mat4 GaussianTrainerScene::getFocusRegionTransform() const {
    dvs_types::Mat4 F{};
    float* o = reinterpret_cast<float*>(&F);
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 4; ++r) o[c * 4 + r] = impl_->region_b2w[r * 4 + c];      // column-major
    return F;
}
std::string GaussianTrainerScene::getCurrentTrainingPhaseName() const {
    switch (impl_->status) {
        case TrainingStatus::Loading_Prepare: return "Loading";
        case TrainingStatus::Colmap_Sfm: return "SfM";
        case TrainingStatus::Preprocess_Done: return "Preprocess done";
        case TrainingStatus::Training: return impl_->pruning ? "Pruning" : "Training";
        case TrainingStatus::Training_Done: return "Done";
        case TrainingStatus::Loading_Failed: return "Failed";
        default: return "GS2Mesh";
    }
}
float GaussianTrainerScene::getProgressOnCurrentPhase() const {
    return impl_->cfg.numIters > 0 ? std::min(1.f, (float)impl_->step / (float)impl_->cfg.numIters) : 0.f;
}
double GaussianTrainerScene::getEstimateTrainingTime() const {
    const double el = getTrainingElpasedTime();
    return impl_->step > 0 ? el / impl_->step * std::max(0, impl_->cfg.numIters - impl_->step) : 0.0;
}
dvs_types::Mat4 GaussianTrainerScene::getCameraProjection(int i) const {
    // perspective projection of the training camera (column-major, OpenGL clip conventions as the editor's Frustum expects)
    dvs_types::Mat4 P{};
    float* o = reinterpret_cast<float*>(&P);
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    if (i < 0 || i >= (int)impl_->cams.size()) return P;
    const dvs_camera& k = impl_->cams[i];
    const float zn = 0.2f, zf = 100.f;
    o[0] = 1.f / k.tan_fovx; o[5] = 1.f / k.tan_fovy; o[10] = -(zf + zn) / (zf - zn); o[11] = -1.f; o[14] = -2.f * zf * zn / (zf - zn);
    return P;
}
dvs_types::Quat GaussianTrainerScene::getCameraRotation(int i) const {
    dvs_types::Quat q{};
    if (i < 0 || i >= (int)impl_->cams.size()) return q;
    const float* v = impl_->cams[i].view;          // view[c*4+r]: world -> camera; rotation R[r][c] = v[c*4+r]; camera -> world = R^T
    const float R[3][3] = {{v[0], v[1], v[2]}, {v[4], v[5], v[6]}, {v[8], v[9], v[10]}};      // R^T rows
    const float tr = R[0][0] + R[1][1] + R[2][2];
    float w, x, y, z;
    if (tr > 0.f) { const float s = std::sqrt(tr + 1.f) * 2.f; w = 0.25f * s; x = (R[2][1] - R[1][2]) / s; y = (R[0][2] - R[2][0]) / s; z = (R[1][0] - R[0][1]) / s; }
    else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) { const float s = std::sqrt(1.f + R[0][0] - R[1][1] - R[2][2]) * 2.f; w = (R[2][1] - R[1][2]) / s; x = 0.25f * s; y = (R[0][1] + R[1][0]) / s; z = (R[0][2] + R[2][0]) / s; }
    else if (R[1][1] > R[2][2]) { const float s = std::sqrt(1.f + R[1][1] - R[0][0] - R[2][2]) * 2.f; w = (R[0][2] - R[2][0]) / s; x = (R[0][1] + R[1][0]) / s; y = 0.25f * s; z = (R[1][2] + R[2][1]) / s; }
    else { const float s = std::sqrt(1.f + R[2][2] - R[0][0] - R[1][1]) * 2.f; w = (R[1][0] - R[0][1]) / s; x = (R[0][2] + R[2][0]) / s; y = (R[1][2] + R[2][1]) / s; z = 0.25f * s; }
    float* o = reinterpret_cast<float*>(&q);
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
    return q;
}
dvs_types::Vec3 GaussianTrainerScene::getCameraPos(int i) const {
    dvs_types::Vec3 p{};
    if (i < 0 || i >= (int)impl_->cams.size()) return p;
    float* o = reinterpret_cast<float*>(&p);
    for (int k = 0; k < 3; ++k) o[k] = impl_->cams[i].campos[k];
    return p;
}
const std::vector<float>& GaussianTrainerScene::getPoints3D(int) { return impl_->init_host[P_POS]; }
bool is_device_support_gstrain() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return false;
    hipDeviceProp_t pr;
    return hipGetDeviceProperties(&pr, 0) == hipSuccess && strstr(pr.gcnArchName, "gfx95") != nullptr;
}
bool is_driver_support() { int v = 0; return hipRuntimeGetVersion(&v) == hipSuccess && v > 0; }
bool GaussianTrainerScene::isTrain() const { return impl_->training; }
void GaussianTrainerScene::startTrain() { impl_->training = true; }
void GaussianTrainerScene::pauseTrain() { impl_->training = false; }
int GaussianTrainerScene::getCurrentIterations() const { return impl_->step; }
float GaussianTrainerScene::getCurrentLoss() {
    Impl& m = *impl_;
    if (m.d_loss && m.stream) {
        float h[2 * DVS_SSIM_SLOTS] = {0.f};
        (void)hipStreamSynchronize(m.stream.get());
        (void)hipMemcpy(h, m.d_loss.get(), sizeof h, hipMemcpyDeviceToHost);
        const float w = m.d_ssim_maps[0] ? m.cfg.ssimWeight : 0.f;
        double l1 = 0, ssim_sum = 0;
        for (int k = 0; k < DVS_SSIM_SLOTS; ++k) { l1 += h[k]; ssim_sum += h[DVS_SSIM_SLOTS + k]; }
        const double nv = (double)m.vpi;                                  // the sums cover the step's views: report their mean
        m.last_loss = (float)(l1 / nv) + (w > 0.f ? w * (1.f - (float)(ssim_sum / nv / (3.0 * m.lw * m.lh))) : 0.f);
    }
    return m.last_loss;
}
int& GaussianTrainerScene::maxIteriaons() { return impl_->cfg.numIters; }
GaussianTrainConfig& GaussianTrainerScene::getTrainConfig() { return impl_->cfg; }
GaussianTrainerScene::TrainingStatus GaussianTrainerScene::getCurrentTrainingStatus() const { return impl_->status; }
void GaussianTrainerScene::setTrainingStatus(TrainingStatus s) { impl_->status = s; }
double GaussianTrainerScene::getTrainingElpasedTime() const {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - impl_->t0).count();
}
int GaussianTrainerScene::getNumGaussians() const { return impl_->n; }
int GaussianTrainerScene::getNumCameras() const { return (int)impl_->cams.size(); }
int GaussianTrainerScene::getCurrentDownscale() const { return 1 << impl_->level_of(impl_->step); }
int GaussianTrainerScene::getNumTestCameras() const { return (int)impl_->test_idx.size(); }
bool GaussianTrainerScene::evaluateTestSet() { return impl_->evaluate(false, true); }
double GaussianTrainerScene::getTestPSNR() const { return impl_->eval_mean[3]; }
double GaussianTrainerScene::getTestSSIM() const { return impl_->eval_mean[2]; }
double GaussianTrainerScene::getTestL1() const { return impl_->eval_mean[1]; }
bool GaussianTrainerScene::renderCameraToJpeg(int camera, const std::string& path) {
    Impl& m = *impl_;
    try {
        if (!m.ctx || camera < 0 || camera >= (int)m.cams.size() || path.empty()) return false;
        HIP_OR_THROW(hipSetDevice(m.device));
        return m.render_to_jpeg({camera}, {path}, nullptr);
    } catch (const std::exception& e) {
        logf_("renderCameraToJpeg(%d, '%s') failed: %s", camera, path.c_str(), e.what());
    } catch (...) {
        logf_("renderCameraToJpeg(%d, '%s') failed: unknown exception", camera, path.c_str());
    }
    return false;
}
bool GaussianTrainerScene::renderCameraToPng(int camera, const std::string& path, int layer) {
    Impl& m = *impl_;
    try {
        if (!m.ctx || camera < 0 || camera >= (int)m.cams.size() || path.empty()) return false;
        if (layer != gsopt::LAYER_COLOR && layer != gsopt::LAYER_DEPTH && layer != gsopt::LAYER_ALPHA) return false;
        HIP_OR_THROW(hipSetDevice(m.device));
        std::vector<std::string> files[3];
        files[layer == gsopt::LAYER_COLOR ? 0 : layer == gsopt::LAYER_DEPTH ? 1 : 2] = {path};
        return m.render_to_png({camera}, files, nullptr);
    } catch (const std::exception& e) {
        logf_("renderCameraToPng(%d, '%s', %d) failed: %s", camera, path.c_str(), layer, e.what());
    } catch (...) {
        logf_("renderCameraToPng(%d, '%s', %d) failed: unknown exception", camera, path.c_str(), layer);
    }
    return false;
}
const std::vector<float>& GaussianTrainerScene::getGaussianPositionCpu() { impl_->fetch_host(); return impl_->host[P_POS]; }
const std::vector<float>& GaussianTrainerScene::getGaussianSH0Cpu() { impl_->fetch_host(); return impl_->host[P_SH0]; }
const std::vector<float>& GaussianTrainerScene::getGaussianSHNCpu() { impl_->fetch_host(); return impl_->host[P_SHN]; }
const std::vector<float>& GaussianTrainerScene::getGaussianOpcaitiesCpu() { impl_->fetch_host(); return impl_->host[P_OPA]; }
const std::vector<float>& GaussianTrainerScene::getGaussianScalingsCpu() { impl_->fetch_host(); return impl_->host[P_SCALE]; }
const std::vector<float>& GaussianTrainerScene::getGaussianRotationsCpu() { impl_->fetch_host(); return impl_->host[P_ROT]; }

// ---- C symbols -------------------------------------------------------------------------------------------
extern "C" {
__attribute__((visibility("default"))) void gstrain_init() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) logf_("gstrain_init: no HIP device visible");
    else logf_("gstrain_init: %d MI355X-class device(s), rasterizer '%s'", count, dvs_version());
}
__attribute__((visibility("default"))) void* create_splat(const GaussianTrainConfig& config, int loadItr) {
    try { return new GaussianTrainerScene(config, loadItr); }
    catch (const std::exception& e) { logf_("create_splat: %s", e.what()); return nullptr; }
}
// The hosts have no try/catch around these dlsym'd calls (gs_train.cpp:152-179): nothing may escape across the C boundary. A
// failure is logged, the scene is marked Loading_Failed / finished (so that the host's loop `get_cur_step >= maxIteration` ends).
#define GSTRAIN_GUARD(name_, scene, body)                                                                        \
    try { body; } catch (const std::exception& e) {                                                               \
        logf_("%s failed: %s", name_, e.what());                                                                    \
        if (scene) { scene->setTrainingStatus(GaussianTrainerScene::TrainingStatus::Loading_Failed); scene->terminate(); } \
    } catch (...) { logf_("%s failed: unknown exception", name_); if (scene) scene->terminate(); }
__attribute__((visibility("default"))) bool load_train_data(GaussianTrainerScene* scene, const std::string& path) {
    bool ok = false;
    GSTRAIN_GUARD("load_train_data", scene, ok = scene && scene->loadTrainData(path));
    return ok;
}
__attribute__((visibility("default"))) void train_step(GaussianTrainerScene* scene) {
    if (!scene || scene->isTerminate()) return;
    GSTRAIN_GUARD("train_step", scene, scene->trainStep());
}
__attribute__((visibility("default"))) int get_cur_step(GaussianTrainerScene* scene) {
    if (!scene) return 0;
    // after a fatal error the step counter reports "done" so that the host's `while (get_cur_step < maxIteration)` loop terminates
    return scene->isTerminate() ? std::max(scene->getCurrentIterations(), scene->maxIteriaons()) : scene->getCurrentIterations();
}
__attribute__((visibility("default"))) void save_splat_model(GaussianTrainerScene* scene) {
    if (!scene) return;
    GSTRAIN_GUARD("save_splat_model", scene, scene->saveGaussianModel());
}
__attribute__((visibility("default"))) void export_mesh(GaussianTrainerScene* scene) { if (scene) { GSTRAIN_GUARD("export_mesh", scene, scene->exportMesh("")); } }
__attribute__((visibility("default"))) void delete_splat(GaussianTrainerScene* scene) { try { delete scene; } catch (...) { logf_("delete_splat failed"); } }
__attribute__((visibility("default"))) void gstrain_destroy() {}
__attribute__((visibility("default"))) const char* get_description() { return "gstrain: MI355X-native Gaussian-splat trainer (divshot_amd)"; }
__attribute__((visibility("default"))) void* create_instance() { return nullptr; }

// plain-C helpers so the PLY wire format can be tested from Python without a GPU (tests/test_ply.py)
__attribute__((visibility("default"))) int gstrain_write_ply(const char* path, uint64_t n, const float* pos, const float* sh0,
                                                              const float* shN, const float* opacity, const float* scale,
                                                              const float* rot, int antialiased) {
    std::string err;
    return gsply::write_ply(path, (size_t)n, pos, sh0, shN, opacity, scale, rot, antialiased != 0, &err) ? 0 : 1;
}
__attribute__((visibility("default"))) int64_t gstrain_read_ply(const char* path, float* pos, float* sh0, float* shN, float* opacity,
                                                                float* scale, float* rot, uint64_t capacity) {
    std::vector<float> a, b, c, d, e, f;
    std::string err;
    if (!gsply::read_ply(path, a, b, c, d, e, f, &err)) return -1;
    const uint64_t n = d.size();
    if (pos && n <= capacity) {
        memcpy(pos, a.data(), a.size() * 4); memcpy(sh0, b.data(), b.size() * 4); memcpy(shN, c.data(), c.size() * 4);
        memcpy(opacity, d.data(), d.size() * 4); memcpy(scale, e.data(), e.size() * 4); memcpy(rot, f.data(), f.size() * 4);
    }
    return (int64_t)n;
}
}
