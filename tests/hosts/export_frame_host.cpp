// export_frame_host.cpp — a host that links libgstrain directly, as the editor does, and drives the export frame through the class
// methods (the editor's "export apply transform"): setExportTransform, setExportOrientation, clearExportTransform. Built and run by
// tests/test_gpu_transform_methods.py (-m gpu). It trains a few steps once and saves the same parameters three times:
//   <dir>/a_<it>.ply + a_<it>.transformed.ply   after setExportTransform(T(0.5, -1, 2) R(0.3, -0.7, 1.1) S(2.5))
//   <dir>/b_<it>.ply + b_<it>.transformed.ply   after setExportOrientation("+y")
//   <dir>/c_<it>.ply alone                        after clearExportTransform()
// and prints what each call returned.
//
// usage: export_frame_host <synthetic spec> <directory> <iterations>
#include <gaussian_trainer_scene.hpp>
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s <synthetic spec> <directory> <iterations>\n", argv[0]); return 2; }
    const std::string spec = argv[1], dir = argv[2];
    const int iters = atoi(argv[3]);
    if (!is_driver_support() || !is_device_support_gstrain()) { fprintf(stderr, "export_frame_host: no supported device\n"); return 3; }
    GaussianTrainConfig cfg;
    cfg.numIters = iters; cfg.densifyStrategy = 0; cfg.warmupLength = 5; cfg.refineEvery = 1000; cfg.refineStopIter = 100000;
    cfg.progressiveTrain = false; cfg.ssimWeight = 0.2f; cfg.capMax = 200000; cfg.verbose = false;
    GaussianTrainerScene gs(cfg, -1);
    gs.setModelPath(dir + "/a");
    const bool early = gs.setExportOrientation("+y");                      // no cameras yet: refused
    if (!gs.loadTrainData(spec)) { fprintf(stderr, "export_frame_host: loadTrainData failed\n"); return 4; }
    gs.trainSetup();
    for (int i = 0; i < iters && !gs.isTerminate(); ++i) gs.trainStep();
    dvs_types::Vec3 t, e;
    t.x = 0.5f; t.y = -1.f; t.z = 2.f; e.x = 0.3f; e.y = -0.7f; e.z = 1.1f;
    const bool set = gs.setExportTransform(t, e, 2.5f);
    gs.saveGaussianModel();
    gs.setModelPath(dir + "/b");
    const bool orient = gs.setExportOrientation("+y");
    const bool bad_scale = gs.setExportTransform(t, e, 0.f);               // refused: the +y frame stays
    const bool bad_axis = gs.setExportOrientation("up");
    gs.saveGaussianModel();
    gs.setModelPath(dir + "/c");
    gs.clearExportTransform();
    gs.saveGaussianModel();
    printf("export_frame_host: early %d set %d orient %d bad_scale %d bad_axis %d iterations %d cameras %d\n", (int)early, (int)set, (int)orient,
           (int)bad_scale, (int)bad_axis, gs.getCurrentIterations(), gs.getNumCameras());
    return gs.isTerminate() ? 6 : 0;
}
