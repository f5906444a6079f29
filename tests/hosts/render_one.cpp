// render_one.cpp — a host that links libgstrain directly (as editor_like.cpp does) and asks the trainer for pictures through the class:
// GaussianTrainerScene::renderCameraToJpeg. It loads a synthetic scene, trains a few steps, renders camera 1 to <out>, then asks for
// camera -1, for a camera past the last one and for a file in a directory that does not exist: each of those must come back false
// without anything thrown. Built and run by tests/test_gpu_render_views.py (-m gpu).
//
// usage: render_one <synthetic spec> <iterations> <out.jpg>
#include <gaussian_trainer_scene.hpp>
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s <synthetic spec> <iterations> <out.jpg>\n", argv[0]); return 2; }
    if (!is_driver_support() || !is_device_support_gstrain()) { fprintf(stderr, "render_one: no supported device\n"); return 3; }
    GaussianTrainConfig cfg;
    cfg.numIters = atoi(argv[2]);
    cfg.verbose = false;
    cfg.capMax = 20000;
    cfg.renderQuality = 95;
    cfg.renderSampling = 1;
    GaussianTrainerScene scene(cfg, -1);
    const bool before_load = scene.renderCameraToJpeg(0, argv[3]);
    if (!scene.loadTrainData(argv[1])) { fprintf(stderr, "render_one: loadTrainData failed\n"); return 4; }
    for (int i = 0; i < cfg.numIters && !scene.isTerminate(); ++i) scene.trainStep();
    const bool ok = scene.renderCameraToJpeg(1, argv[3]);
    const bool negative = scene.renderCameraToJpeg(-1, argv[3]);
    const bool past = scene.renderCameraToJpeg(scene.getNumCameras(), argv[3]);
    const bool no_dir = scene.renderCameraToJpeg(1, std::string(argv[3]) + ".missing/dir/x.jpg");
    scene.trainStep();                                      // training goes on after a render
    printf("render_one: before_load %d, camera 1 %d, camera -1 %d, past the end %d, missing directory %d, iterations %d, terminated %d\n", (int)before_load,
           (int)ok, (int)negative, (int)past, (int)no_dir, scene.getCurrentIterations(), (int)scene.isTerminate());
    return 0;
}
