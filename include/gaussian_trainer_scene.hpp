// gaussian_trainer_scene.hpp — reconstruction of the header DIVSHOT's hosts compile against
// (`#include <gaussian_trainer_scene.hpp>` at application/diverseshot-cli/source/gs_train.cpp:3 and the editor;
// the original ships only with the closed `gstrain` plugin). Field names, types and defaults are
// the ones the in-tree callers use:
//   GaussianTrainConfig fields  gs_train.cpp:50-103, editor.cpp:1750-1961,2000-2020, inspector_panel.cpp:778-925
//   defaults                    application/diverseshot-cli/source/main.cpp:12-70 (CLI defaults)
//   GSPackLevel bit flags       gs_train.cpp:89-96
//   GaussianTrainerScene surface editor.cpp:1413-1654,2023-2035; inspector_panel.cpp:765-1000
// Because the config crosses dlsym() by const reference and carries std::string members, host and plugin must be
// built against THIS header with the same C++ standard library (SURVEY.md §7 "ABI of GaussianTrainConfig").
#pragma once
// GSTRAIN_API marks what libgstrain.so exports: the class the editor constructs itself (editor.cpp:2023
// add_component<GaussianTrainerScene>(trainConfig, -1)) with its CPU getters (editor.cpp:1459-1473), the two free probes
// (editor.cpp:1534,1539) and the C symbols the CLI resolves by dlsym. Everything else in the plugin is built -fvisibility=hidden.
#ifndef GSTRAIN_API
#define GSTRAIN_API __attribute__((visibility("default")))
#endif
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

enum GSPackLevel : int { PackF32ToU8 = 1, PackTileID = 2 };   // bit flags (gs_train.cpp:91-96)

// The editor passes glm values through a few members (editor.cpp:852-856, inspector_panel.cpp:909-933). This header does not depend on
// glm: the PODs below are layout-compatible with glm::vec3 / glm::quat (x, y, z, w order) / glm::mat4 (column-major); a host that has
// glm can build with -DDVS_TRAINER_USE_GLM and gets the glm types themselves.
#ifdef DVS_TRAINER_USE_GLM
#include <glm/glm.hpp>
#include <glm/gtc/quaternion.hpp>
namespace dvs_types { using Vec3 = glm::vec3; using Quat = glm::quat; using Mat4 = glm::mat4; }
#else
namespace dvs_types {
struct Vec3 { float x = 0.f, y = 0.f, z = 0.f; };
struct Quat { float x = 0.f, y = 0.f, z = 0.f, w = 1.f; };
struct Mat4 { float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; };     // column-major
}
#endif

struct GaussianTrainConfig {
    std::string sourcePath, modelPath = "../out_put/iteration", cameraPosePath, pointCloudPath;
    int numIters = 30000;                 // --maxIteration (main.cpp:19)
    int modelType = 0;                    // 0 = 3DGS (2DGS etc. are out of scope)
    int densifyStrategy = 1;              // 0 ADC / 1 MCMC / 2 ADC+ (main.cpp:20,29)
    int warmupLength = 500, refineEvery = 100, resetAlphaEvery = 3000, refineStopIter = 15000;   // main.cpp:47-48
    int refineScale2dStopIter = 15000, pruneInterval = 70000, pruneStrategy = 1;
    int maxImageWidth = 2048, maxImageHeight = 2048, maxImageCount = 0;
    int capMax = 3000000;                 // gs_train.cpp:89
    int packLevel = PackF32ToU8;          // main.cpp:52 (--packLevel 1)
    int meshResolution = 0, resolutionSchedule = 0, cameraModel = 0, datasetType = 0, quality = 0, mapperType = 0;
    int videoStrategy = 0, videoFps = 0;
    float growGrad2d = 0.0002f;           // main.cpp:46
    float ssimWeight = 0.2f;              // main.cpp:24
    float noiselr = 1e5f;                 // main.cpp:67
    float poslrInit = 0.00016f, poslrFinal = 0.0000016f, rotationlr = 0.001f;       // main.cpp:31 (the commented-out defaults of the CLI)
    float scalinglr = 0.005f;             // NOT main.cpp:31's commented 0.001: the CLI never passes it (main.cpp:35, gs_train.cpp:35,55 are commented out), so
                                          // the closed trainer's own default applies, which the tree does not show; this build keeps the lineage's published
                                          // 0.005 (with 0.001 the splits of an ADC refinement take ~5x longer to settle: tests/test_plugin.py's 8-view run)
    float featurelr = 0.0025f, opacitylr = 0.05f;
    float min_opacity = 0.005f, pruneOpacity = 0.005f, pruneScale3d = 0.1f, pruneScale2d = 0.15f;
    bool progressiveTrain = true, useAbsGrad = true, revisedOpacity = true, mipAntiliased = false;
    bool exportMesh = false, normalConsistencyLoss = false, useMask = false, verbose = true, bestQuality = false;
    bool enableBg = false, enableFocusRegion = false, cullSH = false, singleCamera = false, outputSparsePoints = false;
    bool visibleAdam = false, pixelGradScale = false;
    // extension of this build (not a field of the reference's struct; appended last, default = the reference's behaviour): cameras
    // rendered per trainStep() and GPU as ONE multi-view pass (BASELINE.json config C4: 8). Their gradients are summed — one
    // optimizer step per trainStep, as after that many accumulated single-view steps. The environment variable DVS_VIEWS_PER_ITER
    // overrides it (the reference's hosts do not know the field).
    int viewsPerIter = 1;
    // extension of this build, appended the same way (0 / 0 = the reference's behaviour: every camera trains, nothing is evaluated).
    // evalHoldout = K > 0: camera i is a TEST camera iff i % K == 0 (K = 8 is the lineage's usual hold-out); trainStep draws from the
    // other cameras only, and the test cameras are rendered and scored (PSNR / SSIM / L1, include/dvs_train.h dvs_image_metrics_views)
    // after every saveGaussianModel() and every evalEvery steps (0 = only when saving). The environment variables DVS_EVAL_HOLDOUT /
    // DVS_EVAL_EVERY override them (the reference's hosts do not know the fields).
    int evalHoldout = 0;
    int evalEvery = 0;
    // extension of this build, appended the same way: the number of levels of the coarse-to-fine schedule that the reference's field
    // resolutionSchedule (above; 0 = off, the editor's dataset import sets 3000: editor.cpp:2016) turns on. With S = resolutionSchedule > 0
    // and K = numDownscales the step after `step` completed ones trains at level k = max(K - step / S, 0): on the training views
    // box-filtered by 2^k (W / 2^k x H / 2^k, floor) through the cameras of dvs_camera_downscale — the published rule of the lineage:
    // start at 1/2^K, double every S steps. K is clamped at load to 3 and so that the smaller image side stays >= 16 pixels. Saved
    // models and the held-out evaluation are always at full resolution. DVS_RESOLUTION_SCHEDULE / DVS_NUM_DOWNSCALES override the two.
    int numDownscales = 2;
    // extension of this build, appended the same way (0 = the reference's behaviour: saveGaussianModel() writes the full PLY only). Bit
    // flags of the viewer's compact formats that every saveGaussianModel() writes BESIDE <modelPath>_<it>.ply (which stays the resume
    // format): 1 = <modelPath>_<it>.compressed.ply (chunked, quantised: 16 B per splat + 48 B per 256), 2 = <modelPath>_<it>.splat
    // (32 B per splat), 4 = <modelPath>_<it>.spz (version 3, gzipped, 20 + 3 dim B per splat: keeps the SH bands above 0). Packed on the
    // device from the trained arrays (include/dvs_export.h); only the packed payload crosses to the host.
    // 8 = <modelPath>_<it>.reduced.ply (per-splat SH degree with cullSH, twenty 256-entry k-means codebooks, 17..68 B per splat).
    // The editor passes its "Splat Format" choice only as the suffix of modelPath (editor.cpp:1886-1904, 2024): while this field is 0 a
    // modelPath ending in ".compressed.ply" / ".splat" / ".spz" / ".reduced.ply" turns on the matching bit. DVS_EXPORT_FORMATS overrides the field.
    int exportFormats = 0;
    // extension of this build, appended the same way (0 = the reference's behaviour: a save writes no picture). renderViews: bit 1 = the
    // test cameras (evalHoldout), bit 2 = the training cameras; at every saveGaussianModel() they are rendered with the evaluation's
    // options (full SH degree, mipAntiliased) and written as baseline JPEG files <modelPath>_<it>_renders/<image stem>.jpg (cam_%04d.jpg for
    // a synthetic scene): the forward DCT and quantisation run on the device (include/dvs_image.h dvs_jpeg_encode_views), only the
    // coefficients cross to the host, which Huffman-codes them. renderQuality: the IJG quality 1..100; renderSampling: 0 = 4:2:0,
    // 1 = 4:4:4. DVS_RENDER_VIEWS / DVS_RENDER_QUALITY / DVS_RENDER_SAMPLING override them. The three are bytes: they sit in what was
    // the struct's tail padding behind exportFormats, so sizeof(GaussianTrainConfig) is what it was.
    uint8_t renderViews = 0;
    uint8_t renderQuality = 90;
    uint8_t renderSampling = 0;
    // extension of this build, the last free byte of that tail padding (0 = the reference's behaviour: the light prune alone).
    // importancePrune = P in 1..90: at every prune occasion (pruneStrategy > 0, every pruneInterval steps after refineStopIter; there is
    // no second schedule), after the light prune, the P % of the splats that contribute least to the training views are removed. The
    // score of a splat is its blend weight alpha T summed over every pixel of every training camera (dvs_raster_importance_views,
    // dvs_raster.h), so a splat hidden behind others in every view goes first whatever its opacity. Values above 90 are clamped.
    // DVS_IMPORTANCE_PRUNE overrides the field.
    uint8_t importancePrune = 0;
};

class GSTRAIN_API GaussianTrainerScene {
public:
    enum class TrainingStatus { Loading_Prepare, Colmap_Sfm, Preprocess_Done, Training, Training_Done, Loading_Failed, GS2Mesh };

    GaussianTrainerScene(const GaussianTrainConfig& cfg, int loadItr);
    ~GaussianTrainerScene();
    GaussianTrainerScene(const GaussianTrainerScene&) = delete;
    GaussianTrainerScene& operator=(const GaussianTrainerScene&) = delete;

    bool loadTrainData(const std::string& path);     // accepts "synthetic:N=..,W=..,H=..,cams=..,sh=..,seed=.." 
    void trainSetup();
    void trainStep();                                 // one iteration: sample camera -> raster fwd -> loss -> raster bwd -> Adam
    void saveGaussianModel();                         // PLY at modelPath (external/tinygsplat/tiny_gsplat.cpp:168-241 layout)
    void exportMesh(const std::string& path);         // <path> ("": <modelPath>_<it>_mesh.ply, only when meshResolution > 0): INTEGRATION.md "Mesh export"
    // mesh clean-up (extension of this build; INTEGRATION.md "Mesh export"): components with fewer than minComponentPercent % (0..100, two
    // decimals count; 0 = off) of the largest component's triangles are dropped before the mesh is written, and `normals` adds the
    // TSDF gradient's unit normals nx ny nz to the file. Wins over DVS_MESH_MIN_COMPONENT / DVS_MESH_NORMALS once called.
    void setMeshCleanup(float minComponentPercent, bool normals);
    // mesh decimation (extension of this build; INTEGRATION.md "Mesh export"): factor 2..16 merges, last before the mesh is written, all
    // vertices inside a cell of factor^3 voxels of the extraction grid into one (vertex clustering on the device); 0 = off, any other
    // value is reported and counts as 0. Wins over DVS_MESH_DECIMATE once called.
    void setMeshDecimate(int factor);
    // level-of-detail export (extension of this build; INTEGRATION.md "LOD export"): levels = L in 1..4 makes every save also write
    // <modelPath>_<it>.lod<k>.ply, k = 1..L — the full model's splats merged per cell of a lattice with resolution >> (k - 1) cells
    // (resolution 32..1024) along the longest side of the model's box, moment-matched on the device; 0 = off. A value outside these
    // ranges is reported and counts as 0 / 256. Wins over DVS_EXPORT_LOD / DVS_LOD_RESOLUTION once called.
    void setLodExport(int levels, int resolution);
    // mask carve (extension of this build; INTEGRATION.md "Mask carve"): percent = T in 1..100 removes, at every prune occasion and before
    // every save, the splats whose blend weight over the training views landed on background pixels of the views' masks: a splat stays
    // iff fg > 0 and fg (100 - T) >= bg T, with fg / bg its weight on pixels with a nonzero / zero mask. Needs views loaded with useMask;
    // 0 = off, any other value is reported and counts as 0. Wins over DVS_MASK_CARVE once called. Turned on after the load of a capture
    // with distorted cameras, the pixels the undistortion left blank count as background (at load their validity is kept apart).
    void setMaskCarve(int percent);
    // 3D smoothing filter (extension of this build; INTEGRATION.md "3D smoothing filter"): the world-space half of Mip-Splatting — the
    // rasterizer reads every splat convolved with the Gaussian of the highest rate at which a training camera samples it; every file a
    // save writes but the resume PLY holds that fused model, <modelPath>_<it>.fused.ply (exportFormats bit 32) its full PLY. Takes effect
    // at the next loadTrainData / resetGaussian. Wins over DVS_MIP_FILTER3D once called. Independent of mipAntiliased, the 2D half.
    void setMipFilter3d(bool on);
    // the .reduced.ply export (extension of this build; exportFormats bit 8, INTEGRATION.md "Compact exports"): the colour a splat may lose
    // when cullSH lowers its SH degree (>= 0, default 0.01) and whether positions are written as half floats. Once called it wins over
    // DVS_SH_CULL_THRESHOLD / DVS_REDUCED_HALF.
    void setReducedExport(float shCullThreshold, bool halfFloat);
    // export frame (extension of this build, the editor's "export apply transform"; INTEGRATION.md "Export frame"): every file a save writes
    // but the resume PLY <modelPath>_<it>.ply, and the mesh, are written under p' = scale R p + position, R = Rz Ry Rx of rotationEulerRad
    // (radians; the focus region's convention). setExportOrientation("+y" | "-y" | "+x" | ...) derives R and the translation from the
    // training cameras instead: their mean image-up vector turned onto the axis, their centroid moved to the origin, scale 1 (after
    // loadTrainData). false = refused with a log line, the frame stays as it was. The last call wins, also over DVS_EXPORT_TRANSFORM /
    // DVS_EXPORT_ORIENT; clearExportTransform() goes back to the training frame.
    bool setExportTransform(const dvs_types::Vec3& position, const dvs_types::Vec3& rotationEulerRad, float scale);
    bool setExportOrientation(const std::string& axis);
    void clearExportTransform();
    void exportSparsePointCloud(const std::string& path);   // editor.cpp:3535 — writes the splat centres as an ASCII PLY point cloud
    void saveCameraDatas(const std::string& path);          // editor.cpp:3512 — one line per camera: centre, view matrix, intrinsics
    bool isTrain() const;
    void startTrain();
    void pauseTrain();
    bool isTerminate() const;                         // editor.cpp:1603: the training thread leaves its loop when this is set
    void terminate();
    bool isPruningSplat() const;                      // editor.cpp:1551: true while a post-refinement prune pass is running
    void resetGaussian();                             // inspector_panel.cpp:837,861,883,1017: back to the initial splats, step 0
    void setDensifyStrategy(int strategy);            // inspector_panel.cpp:789 (0 ADC / 1 MCMC / 2 ADC+)
    void setModelPath(const std::string& path);       // editor.cpp:2024
    void updateFocusRegion(const dvs_types::Vec3& position, const dvs_types::Vec3& rotation, const dvs_types::Vec3& scale);   // inspector_panel.cpp:933
    // The focus region (config enableFocusRegion; INTEGRATION.md "Focus region"): (lo, hi) of the box in its own coordinates — fixed at load
    // to the bounds of the initial splat centres, or what DVS_FOCUS_REGION says — and F = T(position) R(rotation) S(scale), box -> world, of
    // the last updateFocusRegion() that was accepted (rotation: Euler angles in radians, R = Rz Ry Rx, as the editor's maths::Transform:
    // diverse/source/maths/transform.cpp:129). The editor draws F applied to the box (scene_view_panel.cpp:1393-1415). While the flag is
    // on the trainer keeps the splats whose centre p has lo <= F^-1 p <= hi and trains on the pixels whose ray crosses the box.
    std::pair<dvs_types::Vec3, dvs_types::Vec3> getFocusRegion() const;     // scene_view_panel.cpp:1393
    dvs_types::Mat4 getFocusRegionTransform() const;                        // scene_view_panel.cpp:1394
    std::string getCurrentTrainingPhaseName() const;  // inspector_panel.cpp:997
    float getProgressOnCurrentPhase() const;          // inspector_panel.cpp:999, scene_view_panel.cpp:1022 (0..1)
    double getEstimateTrainingTime() const;           // inspector_panel.cpp:998: remaining seconds at the current rate
    dvs_types::Mat4 getCameraProjection(int i) const; // editor.cpp:852-856: training cameras for the frustum gizmos
    dvs_types::Quat getCameraRotation(int i) const;
    dvs_types::Vec3 getCameraPos(int i) const;
    const std::vector<float>& getPoints3D(int i);     // editor.cpp:1523: xyz of the initial point cloud (here: the initial splat centres)
    int  getCurrentIterations() const;
    float getCurrentLoss();                           // synchronises the training stream
    int& maxIteriaons();
    GaussianTrainConfig& getTrainConfig();
    TrainingStatus getCurrentTrainingStatus() const;
    void setTrainingStatus(TrainingStatus s);
    double getTrainingElpasedTime() const;
    int getNumGaussians() const;
    int getNumCameras() const;                        // all cameras, held-out ones included
    int getCurrentDownscale() const;                  // 1, 2, 4 or 8: the divisor of the image size the next trainStep() trains at (1 when resolutionSchedule is 0)
    // held-out evaluation (extension of this build; config evalHoldout / evalEvery)
    int getNumTestCameras() const;                    // 0 when evaluation is off
    bool evaluateTestSet();                           // renders and scores the test cameras now, synchronises; false when evaluation is off
    double getTestPSNR() const;                       // means over the test cameras of the last evaluation, NaN before the first
    double getTestSSIM() const;
    double getTestL1() const;
    // rendered views (extension of this build): camera i (any camera, held out or not) rendered now from the current parameters with the
    // evaluation's options and written to `path` as a baseline JPEG at the config's renderQuality / renderSampling; synchronises.
    // false for a bad index, before loadTrainData, or when the file cannot be written; nothing is thrown.
    bool renderCameraToJpeg(int camera, const std::string& path);
    // the same as a PNG file (INTEGRATION.md "Rendered views"): layer 1 = colour (8-bit RGB, lossless: the JPEG's quantisation of the
    // render), 2 = depth (16-bit gray, depth x DVS_RENDER_DEPTH_SCALE, default 1000; 0 = no depth; a tEXt chunk depth_scale), 4 = alpha
    // (8-bit gray); the sky is in neither of the last two. Same contract; false also for another layer value.
    bool renderCameraToPng(int camera, const std::string& path, int layer);
    // trainer -> viewer hand-off (editor.cpp:1459-1473 -> GaussianModel::update_from_cpu, gaussian_model.cpp:43-68)
    const std::vector<float>& getGaussianPositionCpu();
    const std::vector<float>& getGaussianSH0Cpu();
    const std::vector<float>& getGaussianSHNCpu();
    const std::vector<float>& getGaussianOpcaitiesCpu();
    const std::vector<float>& getGaussianScalingsCpu();
    const std::vector<float>& getGaussianRotationsCpu();

    // public fields the editor touches
    bool ShowTrainView = false;
    int curIteration = 0;
    std::vector<int> pruenIteraions;
    dvs_types::Vec3 focus_region_position, focus_region_rotation, focus_region_scale{1.f, 1.f, 1.f};   // editor.cpp:1486-1487

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// free functions the editor calls before it starts training (editor.cpp:1534,1539)
GSTRAIN_API bool is_device_support_gstrain();     // a gfx950-class HIP device is visible
GSTRAIN_API bool is_driver_support();             // the HIP runtime initialises

// C symbols the hosts resolve with dlsym (gs_train.cpp:24,105-109,144-150,178; plugin.cpp:89-111)
extern "C" {
GSTRAIN_API void  gstrain_init();
GSTRAIN_API void* create_splat(const GaussianTrainConfig& config, int loadItr);
GSTRAIN_API bool  load_train_data(GaussianTrainerScene* scene, const std::string& path);
GSTRAIN_API void  train_step(GaussianTrainerScene* scene);
GSTRAIN_API int   get_cur_step(GaussianTrainerScene* scene);
GSTRAIN_API void  save_splat_model(GaussianTrainerScene* scene);
GSTRAIN_API void  export_mesh(GaussianTrainerScene* scene);
GSTRAIN_API void  delete_splat(GaussianTrainerScene* scene);
GSTRAIN_API void  gstrain_destroy();
GSTRAIN_API const char* get_description();
GSTRAIN_API void* create_instance();
}
