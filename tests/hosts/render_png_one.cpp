// render_png_one.cpp — a host that links libgstrain directly (as render_one.cpp does) and asks the trainer for PNG pictures through the
// class: GaussianTrainerScene::renderCameraToPng. It loads a synthetic scene, trains a few steps, renders camera 1 as colour, depth and
// alpha to <stem>_1.png, <stem>_2.png, <stem>_4.png, then asks for camera -1, a camera past the last one, the layers 0, 3 and 8 and a
// file in a directory that does not exist: each of those must come back false without anything thrown. Built and run by
// tests/test_gpu_render_png.py (-m gpu).
//
// usage: render_png_one <synthetic spec> <iterations> <stem>
#include <gaussian_trainer_scene.hpp>
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s <synthetic spec> <iterations> <stem>\n", argv[0]); return 2; }
    if (!is_driver_support() || !is_device_support_gstrain()) { fprintf(stderr, "render_png_one: no supported device\n"); return 3; }
    GaussianTrainConfig cfg;
    cfg.numIters = atoi(argv[2]);
    cfg.verbose = false;
    cfg.capMax = 20000;
    GaussianTrainerScene scene(cfg, -1);
    const std::string stem = argv[3];
    const bool before_load = scene.renderCameraToPng(0, stem + "_early.png", 1);
    if (!scene.loadTrainData(argv[1])) { fprintf(stderr, "render_png_one: loadTrainData failed\n"); return 4; }
    for (int i = 0; i < cfg.numIters && !scene.isTerminate(); ++i) scene.trainStep();
    int ok = 0;
    for (int layer : {1, 2, 4}) ok += scene.renderCameraToPng(1, stem + "_" + std::to_string(layer) + ".png", layer) ? layer : 0;
    const bool negative = scene.renderCameraToPng(-1, stem + "_bad.png", 1);
    const bool past = scene.renderCameraToPng(scene.getNumCameras(), stem + "_bad.png", 1);
    int bad_layers = 0;
    for (int layer : {0, 3, 8, -1}) bad_layers += scene.renderCameraToPng(1, stem + "_bad.png", layer) ? 1 : 0;
    const bool no_dir = scene.renderCameraToPng(1, stem + ".missing/dir/x.png", 1);
    scene.trainStep();                                      // training goes on after a render
    printf("render_png_one: before_load %d, layers written %d, camera -1 %d, past the end %d, bad layers %d, missing directory %d, iterations %d, terminated %d\n",
           (int)before_load, ok, (int)negative, (int)past, bad_layers, (int)no_dir, scene.getCurrentIterations(), (int)scene.isTerminate());
    return 0;
}
