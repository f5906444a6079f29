// diverseshot_cli.cpp — this build's counterpart of DIVSHOT's `diverseshot-cli` host: same flags and defaults
// (application/diverseshot-cli/source/main.cpp:9-70), same plugin loading (dlopen of "libgstrain.so" next to the
// executable, RTLD_LAZY|RTLD_LOCAL — diverse/diverse_base/source/core/plugin.cpp:74,89; symbols via dlsym, plugin.cpp:153-167)
// and the same call order as train_gaussian() (application/diverseshot-cli/source/gs_train.cpp:7-181):
//   gstrain_init -> create_splat -> load_train_data (false => exit(-1)) -> { get_cur_step, train_step }* with a progress line
//   every 500 steps and save_splat_model every 10000 steps once i > resetAlphaEvery -> [export_mesh] -> save_splat_model ->
//   delete_splat -> gstrain_destroy.
// The reference's own gs_train.cpp cannot be compiled here (it needs the closed header and <format>);
// CLI11 / indicators / spdlog are replaced by a few lines of standard C++.
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <map>
#include <string>
#include "../../include/gaussian_trainer_scene.hpp"
#include "ext_options.hpp"

static std::map<std::string, std::string> g_opts = {
    // flag -> default (main.cpp:12-70)
    {"maxImageWidth", "2048"}, {"maxImageHeight", "2048"}, {"inputPath", ""}, {"ssim", "0.2"}, {"outputPath", "../out_put/iteration"},
    {"modelType", "0"}, {"densifyStrategy", "1"}, {"maxIteration", "30000"}, {"progressTrain", "1"}, {"load_itr", "-1"},
    {"absgrad", "1"}, {"growGrad2d", "0.0002"}, {"warmupLength", "500"}, {"refineEvery", "100"}, {"resetAlphaEvery", "3000"},
    {"refineStopIter", "15000"}, {"refineScale2dStopIter", "15000"}, {"minOpacity", "0.005"}, {"pruneEvery", "70000"},
    {"pruneStrategy", "1"}, {"revisedOpacity", "1"}, {"mipAntiliased", "0"}, {"packLevel", "1"}, {"exportMesh", "0"},
    {"noiselr", "100000"}, {"useMask", "0"}, {"eval", "0"},
    {"viewsPerIter", "1"},        // extension of this build: cameras per train_step as one multi-view pass (BASELINE config C4: 8)
    // extensions of this build: --eval holds out every 8th camera (0, 8, ...) as the test set; --evalHoldout K chooses the modulus
    // (-1 = not given; it wins over --eval), --evalEvery N also scores the test set every N steps (it is always scored at a save)
    {"evalHoldout", "-1"}, {"evalEvery", "0"},
    // the reference's config field resolutionSchedule (its CLI has no flag for it; the editor sets 3000) and this build's numDownscales:
    // coarse-to-fine training, start at 1/2^K of the image size and double every N steps (0 = off)
    {"resolutionSchedule", "0"}, {"numDownscales", "2"},
    // extension of this build: compact formats every save writes beside the full PLY: compressed | splat | compressed,splat
    // (<outputPath>_<it>.compressed.ply / .splat); empty = none, unless --outputPath itself ends in .compressed.ply / .splat
    {"exportFormat", ""},
    // extension of this build: a switch, every save also writes <outputPath>_<it>.spz (the compact format that keeps the SH bands above 0;
    // with --eval its decoded model is scored on the held-out views too); also on when --outputPath itself ends in .spz
    {"exportSpz", "0"},
    // extension of this build: --exportFormat also takes reduced (<outputPath>_<it>.reduced.ply: per-splat SH degree, k-means codebooks; also
    // on when --outputPath ends in .reduced.ply). --cullSH 1 lets a splat drop the SH bands that change its colour by at most
    // --cullSHThreshold (default 0.01) from every training camera; --reducedHalf 1 writes half-float positions
    {"cullSH", "0"}, {"cullSHThreshold", "0.01"}, {"reducedHalf", "0"},
    // the config fields pruneScale3d / pruneScale2d (the reference's CLI has no flag for them): after the first opacity reset a refinement
    // also prunes splats larger than this fraction of the scene extent / whose screen radius exceeds this fraction of the image size
    {"pruneScale3d", "0.1"}, {"pruneScale2d", "0.15"},
    // extension of this build: every save also writes rendered views as JPEG files to <outputPath>_<it>_renders/: --renderViews test (the
    // held-out cameras of --eval) | train | all; --renderQuality 1..100; --renderSampling 420 | 444
    {"renderViews", ""}, {"renderQuality", "90"}, {"renderSampling", "420"},
    // extension of this build: --renderFormat jpg | png writes those views as lossless PNG files instead; with png, --renderLayers
    // color[,depth][,alpha] adds <name>_depth.png (16-bit gray: depth x --renderDepthScale, 0 = no depth) and <name>_alpha.png (8-bit
    // gray). The config struct has no room left: when given they are handed to the plugin as DVS_RENDER_FORMAT / DVS_RENDER_LAYERS (the
    // sum of 1 color, 2 depth, 4 alpha) / DVS_RENDER_DEPTH_SCALE.
    {"renderFormat", "jpg"}, {"renderLayers", "color"}, {"renderDepthScale", "1000"},
    // the reference's config field meshResolution (its CLI has no flag for it): > 0 = the final save also writes <outputPath>_<it>_mesh.ply,
    // the surface extracted on a grid of that many voxels along its longest side (16..1024). --exportMesh keeps the reference's meaning.
    {"meshResolution", "0"},
    // extension of this build: --importancePrune P (0..90) removes, at every prune occasion (--pruneStrategy > 0, every --pruneEvery steps after
    // --refineStopIter) and after the light prune, the P % of the splats that contribute least to the training views; 0 = off
    {"importancePrune", "0"},
    // extensions of this build, for the mesh --meshResolution writes: --meshMinComponent P (percent, 0..100, at most two decimals) drops the
    // connected components with fewer than P % of the largest one's triangles; --meshNormals 1 adds nx ny nz, the TSDF gradient's unit
    // normals. The config struct has no room left: when given they are handed to the plugin as DVS_MESH_MIN_COMPONENT / DVS_MESH_NORMALS.
    {"meshMinComponent", "0"}, {"meshNormals", "0"},
    // extension of this build: --meshDecimate F (0 = off, or 2..16) decimates that mesh last, by vertex clustering: all vertices inside a cell
    // of F voxels of the extraction grid per axis become one. Handed to the plugin as DVS_MESH_DECIMATE, like the two above.
    {"meshDecimate", "0"},
    // the reference's config field enableBg ("Create Sky Model"; its CLI has no flag for it): --enableBg 1 trains an equirectangular sky
    // texture behind the splats and writes <outputPath>_<it>.sky at every save. --skyResolution Hs (default 128, clamped to 16..1024) is the
    // texture's height, its width 2 Hs; the config struct has no room left: it is handed to the plugin as DVS_SKY_RESOLUTION.
    {"enableBg", "0"}, {"skyResolution", "128"},
    // the reference's config field enableFocusRegion (its CLI has no flag for it; the editor's "Focus Region"): --enableFocusRegion 1 keeps and
    // trains only the splats inside an oriented box. --focusRegion x0,y0,z0,x1,y1,z1 is the box (default: the bounds of the initial splat
    // centres), --focusRotation rx,ry,rz turns it about the origin (Euler angles in radians, as the editor's). The config struct has no room
    // left: the two are handed to the plugin as DVS_FOCUS_REGION / DVS_FOCUS_ROTATION.
    {"enableFocusRegion", "0"}, {"focusRegion", ""}, {"focusRotation", ""},
    // extension of this build (the editor's "export apply transform"): every file a save writes but the resume PLY, and the mesh, in a chosen
    // frame. --exportTransform tx,ty,tz,rx,ry,rz,s: p' = s R p + t, Euler angles in radians (R = Rz Ry Rx), s > 0. --exportOrient +y (or -y,
    // +x, -x, +z, -z): turn the cameras' mean up vector onto that axis and centre their centroid. One of the two at most. --exportFormat
    // takes `transformed` with either: <outputPath>_<it>.transformed.ply, the full PLY in that frame (implied when no other format is
    // selected). The config struct has no room left: they are handed to the plugin as DVS_EXPORT_TRANSFORM / DVS_EXPORT_ORIENT.
    {"exportTransform", ""}, {"exportOrient", ""},
    // extension of this build: --exportLod L (0 = off .. 4): every save also writes <outputPath>_<it>.lod<k>.ply, k = 1..L, the model with the
    // splats of every cell of a lattice merged into one (moment-matched, on the GPU); --lodResolution R (32..1024) is level 1's cell count
    // along the longest side, level k has R >> (k - 1). Handed to the plugin as DVS_EXPORT_LOD / DVS_LOD_RESOLUTION, like the mesh flags.
    {"exportLod", "0"}, {"lodResolution", "256"},
    // extension of this build: --maskCarve T (0 = off .. 100) removes, at every prune occasion and before every save, the splats whose blend
    // weight over the training views landed on background pixels of the masks (--useMask 1): a splat stays iff fg > 0 and
    // fg (100 - T) >= bg T. The config struct has no room left: it is handed to the plugin as DVS_MASK_CARVE.
    {"maskCarve", "0"},
    // extension of this build: --mipFilter3d 1 trains with the 3D smoothing filter of Mip-Splatting: every splat is low-pass filtered in world
    // space by the highest rate at which a training camera samples it (recomputed at load, after every change of the splat set, and every 100
    // steps). Independent of --mipAntiliased, the method's 2D half; the paper's configuration is both. Every file a save writes but the resume
    // PLY holds the fused (filtered) model; --exportFormat takes `fused` with it: <outputPath>_<it>.fused.ply, the full PLY of that model (implied
    // when no other format is selected). The config struct has no room left: it is handed to the plugin as DVS_MIP_FILTER3D.
    {"mipFilter3d", "0"}};
static std::map<std::string, bool> g_given;

static bool as_bool(const std::string& v) { return v == "1" || v == "true" || v == "True" || v == "on"; }

template <class F> static F sym(void* h, const char* name, bool required = true) {
    void* p = dlsym(h, name);
    if (!p && required) { std::cerr << "can't find " << name << " symbol\n"; exit(-1); }
    return reinterpret_cast<F>(p);
}

int main(int argc, const char* argv[]) {
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);      // dmabuf IPC for RCCL between the ranks' processes; read when the HSA runtime starts (first HIP call)
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--help" || a == "-h") {
            std::cout << "gaussian_train (divshot_amd counterpart of diverseshot-cli)\nflags:";
            for (auto& kv : g_opts) std::cout << " --" << kv.first << " [" << kv.second << "]";
            std::cout << "\n--inputPath accepts synthetic:N=..,W=..,H=..,cams=..,sh=..,seed=..\n";
            return 0;
        }
        if (a == "--version") { std::cout << "1.0.0\n"; return 0; }
        if (a.rfind("--", 0) != 0) { std::cout << "Command Line Error: unexpected argument " << a << "\n"; return 1; }
        a = a.substr(2);
        std::string val;
        size_t eq = a.find('=');
        if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        else if (a == "eval" || a == "exportSpz") val = "1";
        else if (i + 1 < argc) val = argv[++i];
        if (!g_opts.count(a)) { std::cout << "Command Line Error: unknown flag --" << a << "\n"; return 1; }   // config_extras_mode::error
        g_opts[a] = val;
        g_given[a] = true;
    }
    // the extension options the config struct has no room for (ext_options.hpp): a given flag's value is checked against its table row
    // and handed to the plugin in the row's environment variable, before the plugin is loaded
    int layers = gsopt::LAYER_COLOR;
    for (int id = 0; id < gsopt::N_OPTIONS; ++id) {
        const gsopt::Row& r = gsopt::row((gsopt::Id)id);
        if (!r.flag || !g_given.count(r.flag)) continue;
        std::string v = g_opts[r.flag];
        double parsed[8];
        if ((r.flag_to_var && !r.flag_to_var(v, &v)) || !gsopt::parse(r, v.c_str(), parsed)) { std::cout << gsopt::cli_error(r, g_opts[r.flag]) << "\n"; return 1; }
        setenv(r.var, v.c_str(), 1);
        if (id == gsopt::RENDER_LAYERS) layers = (int)parsed[0];
    }
    for (const char* flag : {"cullSH", "enableBg", "enableFocusRegion"})
        if (g_opts[flag] != "0" && g_opts[flag] != "1") { std::cout << "Command Line Error: --" << flag << " takes 0 or 1, not '" << g_opts[flag] << "'\n"; return 1; }
    // the rules across options
    if (gsopt::layers_need_png(layers, g_opts["renderFormat"] == "png")) {
        std::cout << "Command Line Error: --renderLayers takes depth or alpha only with --renderFormat png (JPEG files carry colour alone), not '" << g_opts["renderLayers"] << "'\n";
        return 1;
    }
    const bool export_frame = g_given.count("exportTransform") || g_given.count("exportOrient");
    if (gsopt::two_export_frames(g_given.count("exportTransform"), g_given.count("exportOrient"))) { std::cout << "Command Line Error: --exportTransform and --exportOrient exclude each other\n"; return 1; }
    if (gsopt::transformed_needs_frame(g_opts["exportFormat"], export_frame)) { std::cout << "Command Line Error: --exportFormat transformed needs --exportTransform or --exportOrient\n"; return 1; }
    if (gsopt::fused_needs_filter(g_opts["exportFormat"], g_opts["mipFilter3d"] == "1")) { std::cout << "Command Line Error: --exportFormat fused needs --mipFilter3d 1\n"; return 1; }
    // plugin: "libgstrain.so" next to the executable (plugin.cpp:74 builds parent_path / "lib<name>.so")
    std::error_code ec;
    auto exe = std::filesystem::read_symlink("/proc/self/exe", ec);
    const std::string plugin_path = (exe.parent_path() / "libgstrain.so").string();
    void* h = dlopen(plugin_path.c_str(), RTLD_LAZY | RTLD_LOCAL);
    if (!h) { std::cerr << "Failed to load library or its dependencies : " << plugin_path << " : " << dlerror() << "\ncreate plugin failed\n"; exit(-1); }
    (void)sym<const char* (*)()>(h, "get_description", false);
    (void)sym<void* (*)()>(h, "create_instance", false);
    typedef void (*voidFunc)();
    auto gsplat_init = sym<voidFunc>(h, "gstrain_init");
    gsplat_init();

    const std::string source_path = g_opts["inputPath"];
    const int max_iteraion = atoi(g_opts["maxIteration"].c_str());
    const int load_itr = atoi(g_opts["load_itr"].c_str());
    auto start = std::chrono::high_resolution_clock::now();
    GaussianTrainConfig train_config;                       // field-by-field, as gs_train.cpp:50-103
    train_config.sourcePath = source_path;
    train_config.growGrad2d = (float)atof(g_opts["growGrad2d"].c_str());
    train_config.warmupLength = atoi(g_opts["warmupLength"].c_str());
    train_config.refineEvery = atoi(g_opts["refineEvery"].c_str());
    train_config.resetAlphaEvery = atoi(g_opts["resetAlphaEvery"].c_str());
    train_config.refineStopIter = atoi(g_opts["refineStopIter"].c_str());
    train_config.revisedOpacity = as_bool(g_opts["revisedOpacity"]);
    train_config.refineScale2dStopIter = atoi(g_opts["refineScale2dStopIter"].c_str());
    train_config.ssimWeight = (float)atof(g_opts["ssim"].c_str());
    train_config.modelPath = g_opts["outputPath"];
    train_config.modelType = atoi(g_opts["modelType"].c_str());
    train_config.densifyStrategy = atoi(g_opts["densifyStrategy"].c_str());
    train_config.progressiveTrain = as_bool(g_opts["progressTrain"]);
    train_config.useAbsGrad = as_bool(g_opts["absgrad"]);
    train_config.pruneInterval = atoi(g_opts["pruneEvery"].c_str());
    train_config.pruneStrategy = atoi(g_opts["pruneStrategy"].c_str());
    train_config.pruneScale3d = (float)atof(g_opts["pruneScale3d"].c_str());
    train_config.pruneScale2d = (float)atof(g_opts["pruneScale2d"].c_str());
    train_config.mipAntiliased = as_bool(g_opts["mipAntiliased"]);
    train_config.maxImageHeight = atoi(g_opts["maxImageHeight"].c_str());
    train_config.maxImageWidth = atoi(g_opts["maxImageWidth"].c_str());
    train_config.exportMesh = as_bool(g_opts["exportMesh"]);
    train_config.useMask = as_bool(g_opts["useMask"]);
    train_config.numIters = max_iteraion;
    if (g_opts.count("viewsPerIter")) train_config.viewsPerIter = atoi(g_opts["viewsPerIter"].c_str());   // extension of this build (config C4)
    train_config.evalHoldout = atoi(g_opts["evalHoldout"].c_str()) >= 0 ? atoi(g_opts["evalHoldout"].c_str()) : (as_bool(g_opts["eval"]) ? 8 : 0);
    train_config.evalEvery = atoi(g_opts["evalEvery"].c_str());
    train_config.resolutionSchedule = atoi(g_opts["resolutionSchedule"].c_str());
    train_config.numDownscales = atoi(g_opts["numDownscales"].c_str());
    for (size_t at = 0; at < g_opts["exportFormat"].size();) {
        const std::string& v = g_opts["exportFormat"];
        const size_t comma = std::min(v.find(',', at), v.size());
        const std::string tok = v.substr(at, comma - at);
        if (tok == "compressed") train_config.exportFormats |= 1;
        else if (tok == "splat") train_config.exportFormats |= 2;
        else if (tok == "reduced") train_config.exportFormats |= 8;
        else if (tok == "transformed") train_config.exportFormats |= 16;     // (refused above without an export frame)
        else if (tok == "fused") train_config.exportFormats |= 32;           // (refused above without --mipFilter3d 1)
        else { std::cout << "Command Line Error: --exportFormat takes compressed, splat, reduced, transformed, fused or a comma-separated list of them, not '" << tok << "'\n"; return 1; }
        at = comma + 1;
    }
    if (as_bool(g_opts["exportSpz"])) train_config.exportFormats |= 4;
    train_config.cullSH = as_bool(g_opts["cullSH"]);
    {
        const std::string &rv = g_opts["renderViews"], &rs = g_opts["renderSampling"];
        const int q = atoi(g_opts["renderQuality"].c_str());
        if (rv == "test") train_config.renderViews = 1;
        else if (rv == "train") train_config.renderViews = 2;
        else if (rv == "all") train_config.renderViews = 3;
        else if (!rv.empty()) { std::cout << "Command Line Error: --renderViews takes test, train or all, not '" << rv << "'\n"; return 1; }
        if (rs != "420" && rs != "444") { std::cout << "Command Line Error: --renderSampling takes 420 or 444, not '" << rs << "'\n"; return 1; }
        if (q < 1 || q > 100) { std::cout << "Command Line Error: --renderQuality takes 1..100, not '" << g_opts["renderQuality"] << "'\n"; return 1; }
        train_config.renderSampling = rs == "444" ? 1 : 0;
        train_config.renderQuality = (uint8_t)q;
    }
    train_config.meshResolution = atoi(g_opts["meshResolution"].c_str());
    if (train_config.meshResolution < 0) { std::cout << "Command Line Error: --meshResolution takes 0 (off) or a grid resolution, not '" << g_opts["meshResolution"] << "'\n"; return 1; }
    {
        const std::string& ip = g_opts["importancePrune"];
        const bool digits = !ip.empty() && ip.size() <= 2 && ip.find_first_not_of("0123456789") == std::string::npos;
        if (!digits || atoi(ip.c_str()) > 90) { std::cout << "Command Line Error: --importancePrune takes an integer 0..90, not '" << ip << "'\n"; return 1; }
        train_config.importancePrune = (uint8_t)atoi(ip.c_str());
    }
    train_config.enableBg = g_opts["enableBg"] == "1";
    train_config.enableFocusRegion = g_opts["enableFocusRegion"] == "1";
    train_config.normalConsistencyLoss = false;
    if (train_config.exportMesh) { train_config.normalConsistencyLoss = true; train_config.useMask = true; }
    train_config.verbose = true;
    train_config.capMax = 3000000;
    const int packLevel = atoi(g_opts["packLevel"].c_str());
    train_config.packLevel = packLevel == 0 ? 0 : (packLevel == 1 ? (int)GSPackLevel::PackF32ToU8 : (int)(GSPackLevel::PackF32ToU8 | GSPackLevel::PackTileID));
    train_config.noiselr = (float)atof(g_opts["noiselr"].c_str());
    train_config.bestQuality = true;

    typedef void* (*createFunc)(const GaussianTrainConfig& config, int loadItr);
    auto create_splat = sym<createFunc>(h, "create_splat");
    auto scene = (GaussianTrainerScene*)create_splat(train_config, load_itr);
    if (!scene) { std::cout << "create_splat failed\n"; exit(-1); }
    typedef bool (*loadDataFunc)(GaussianTrainerScene* scene, const std::string& path);
    auto loadData = sym<loadDataFunc>(h, "load_train_data");
    if (!loadData(scene, source_path)) { std::cout << "load data failed!, please check source_path \n"; exit(-1); }
    std::cout << "Training [Preprocess done]\n";

    typedef void (*SceneParamFunc)(GaussianTrainerScene* scene);
    auto train_step = sym<SceneParamFunc>(h, "train_step");
    auto save_splat_model = sym<SceneParamFunc>(h, "save_splat_model");
    auto export_mesh = sym<SceneParamFunc>(h, "export_mesh");
    auto delete_splat = sym<SceneParamFunc>(h, "delete_splat");
    typedef int (*IntReturnFunc)(GaussianTrainerScene* scene);
    auto get_cur_step = sym<IntReturnFunc>(h, "get_cur_step");
    auto loop_start = std::chrono::high_resolution_clock::now();
    const int first = get_cur_step(scene);
    while (true) {
        auto i = get_cur_step(scene);
        if (i >= max_iteraion) break;
        train_step(scene);
        if (i % 500 == 0) {
            const double el = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - loop_start).count();
            printf("Training [%3d%%] train step : %d/%d  (%.1f it/s)\n", (int)((i / (float)max_iteraion) * 100), i, max_iteraion,
                   i > first ? (i - first) / el : 0.0);
            fflush(stdout);
        }
        if (i > train_config.resetAlphaEvery && i % 10000 == 0) save_splat_model(scene);
    }
    std::cout << "Training [100%] Train Done\n";
    if (train_config.exportMesh) export_mesh(scene);
    auto end = std::chrono::high_resolution_clock::now();
    std::cout << "train cost time : " << std::chrono::duration_cast<std::chrono::seconds>(end - start).count() << " seconds\n";
    save_splat_model(scene);
    delete_splat(scene);
    auto gstrain_destroy = sym<voidFunc>(h, "gstrain_destroy");
    gstrain_destroy();
    return 0;
}
