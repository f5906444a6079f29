// dataset_capi.cpp — plain-C entry points of the dataset reader (dataset_io.hpp) in libgsplyio.so, the host-only library of
// ply_capi.cpp, so that the reader can be tested from Python without a GPU or the HIP runtime. Every call returns 0 on success; a
// failure leaves its message (NUL-terminated, cut to `cap`) in `err`.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "dataset_io.hpp"

namespace {
int report(bool ok, const std::string& msg, char* err, int cap) {
    if (!ok && err && cap > 0) { strncpy(err, msg.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
    return ok ? 0 : 1;
}
}  // namespace

#define GSDATA_API extern "C" __attribute__((visibility("default")))

GSDATA_API void* gstrain_dataset_open(const char* path, char* err, int cap) {
    gsdata::Dataset* d = new gsdata::Dataset();
    std::string msg;
    if (!path || !gsdata::read_dataset(path, d, &msg)) { report(false, path ? msg : "NULL path", err, cap); delete d; return nullptr; }
    return d;
}
// flags: bit 0 = accept the distorted models SIMPLE_RADIAL, RADIAL and OPENCV (gsdata::ReadOptions::accept_distorted)
GSDATA_API void* gstrain_dataset_open_ex(const char* path, uint32_t flags, char* err, int cap) {
    gsdata::Dataset* d = new gsdata::Dataset();
    gsdata::ReadOptions opt;
    opt.accept_distorted = (flags & 1u) != 0;
    std::string msg;
    if (!path || !gsdata::read_dataset(path, opt, d, &msg)) { report(false, path ? msg : "NULL path", err, cap); delete d; return nullptr; }
    return d;
}
GSDATA_API void gstrain_dataset_close(void* h) { delete (gsdata::Dataset*)h; }
// counts[5] = {cameras, images, points, dropped points, 1 if the model was read from .bin files}
GSDATA_API int gstrain_dataset_counts(const void* h, uint64_t* counts) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !counts) return 1;
    counts[0] = d->cameras.size(); counts[1] = d->images.size(); counts[2] = d->xyz.size() / 3; counts[3] = d->dropped; counts[4] = d->binary ? 1 : 0;
    return 0;
}
// ints[4] = {camera id, model id, width, height}, params[4] = {fx, fy, cx, cy}
GSDATA_API int gstrain_dataset_camera(const void* h, uint64_t index, uint64_t* ints, double* params) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !ints || !params || index >= d->cameras.size()) return 1;
    const gsdata::Camera& c = d->cameras[index];
    ints[0] = c.id; ints[1] = (uint64_t)c.model; ints[2] = c.width; ints[3] = c.height;
    params[0] = c.fx; params[1] = c.fy; params[2] = c.cx; params[3] = c.cy;
    return 0;
}
// k[4] = {k1, k2, p1, p2} of camera `index` (zeros for a pinhole model)
GSDATA_API int gstrain_dataset_camera_distortion(const void* h, uint64_t index, double* k) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !k || index >= d->cameras.size()) return 1;
    for (int i = 0; i < 4; ++i) k[i] = d->cameras[index].dist[i];
    return 0;
}
// image `index` in name order: ints[3] = {image id, camera id, index of its camera}, pose[7] = {qw, qx, qy, qz, tx, ty, tz},
// rot[9] = the world -> camera rotation the trainer uses, row-major
GSDATA_API int gstrain_dataset_image(const void* h, uint64_t index, uint64_t* ints, double* pose, float* rot, char* name, int name_cap) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !ints || !pose || !rot || !name || name_cap <= 0 || index >= d->images.size()) return 1;
    const gsdata::Image& im = d->images[index];
    if (im.name.size() + 1 > (size_t)name_cap) return 1;
    ints[0] = im.id; ints[1] = im.camera_id; ints[2] = im.camera;
    for (int k = 0; k < 4; ++k) pose[k] = im.q[k];
    for (int k = 0; k < 3; ++k) pose[4 + k] = im.t[k];
    gsdata::rotation_of(im, rot);
    memcpy(name, im.name.c_str(), im.name.size() + 1);
    return 0;
}
GSDATA_API int gstrain_dataset_points(const void* h, float* xyz, uint8_t* rgb) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !xyz || !rgb) return 1;
    if (!d->xyz.empty()) { memcpy(xyz, d->xyz.data(), d->xyz.size() * sizeof(float)); memcpy(rgb, d->rgb.data(), d->rgb.size()); }
    return 0;
}
// the file image `index` is read from (NUL-terminated into `file`) and whether it is decoded as a JPEG
GSDATA_API int gstrain_dataset_resolve_image(const void* h, uint64_t index, char* file, int file_cap, int* is_jpeg, char* err, int cap) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !file || file_cap <= 0 || !is_jpeg) return report(false, "NULL argument", err, cap);
    std::string path, msg;
    bool jpeg = false;
    if (!gsdata::resolve_image(*d, (size_t)index, &path, &jpeg, &msg)) return report(false, msg, err, cap);
    if (path.size() + 1 > (size_t)file_cap) return report(false, "path longer than the buffer", err, cap);
    memcpy(file, path.c_str(), path.size() + 1);
    *is_jpeg = jpeg ? 1 : 0;
    return 0;
}
// the same with the kind told apart: *kind = 0 PPM, 1 JPEG, 2 PNG (gsdata::resolve_image_kind)
GSDATA_API int gstrain_dataset_resolve_image_kind(const void* h, uint64_t index, char* file, int file_cap, int* kind, char* err, int cap) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !file || file_cap <= 0 || !kind) return report(false, "NULL argument", err, cap);
    std::string path, msg;
    gsdata::ImageKind k = gsdata::ImageKind::PPM;
    if (!gsdata::resolve_image_kind(*d, (size_t)index, &path, &k, &msg)) return report(false, msg, err, cap);
    if (path.size() + 1 > (size_t)file_cap) return report(false, "path longer than the buffer", err, cap);
    memcpy(file, path.c_str(), path.size() + 1);
    *kind = (int)k;
    return 0;
}
// the mask file of image `index` under --useMask: *kind = 0 none (file = ""), 1 PGM, 2 PNG (gsdata::resolve_mask)
GSDATA_API int gstrain_dataset_resolve_mask(const void* h, uint64_t index, char* file, int file_cap, int* kind, char* err, int cap) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !file || file_cap <= 0 || !kind) return report(false, "NULL argument", err, cap);
    std::string path, msg;
    gsdata::MaskKind k = gsdata::MaskKind::NONE;
    if (!gsdata::resolve_mask(*d, (size_t)index, &path, &k, &msg)) return report(false, msg, err, cap);
    if (path.size() + 1 > (size_t)file_cap) return report(false, "path longer than the buffer", err, cap);
    memcpy(file, path.c_str(), path.size() + 1);
    *kind = (int)k;
    return 0;
}
// rgb [H][W][3] of the image's camera size; mask (nullable) [H][W] in {0, 1}
GSDATA_API int gstrain_dataset_read_image(const void* h, uint64_t index, uint8_t* rgb, uint8_t* mask, char* err, int cap) {
    const gsdata::Dataset* d = (const gsdata::Dataset*)h;
    if (!d || !rgb) return report(false, "NULL argument", err, cap);
    std::vector<uint8_t> px;
    std::string msg;
    if (!gsdata::read_image(*d, (size_t)index, &px, &msg)) return report(false, msg, err, cap);
    memcpy(rgb, px.data(), px.size());
    if (mask) {
        if (!gsdata::read_mask(*d, (size_t)index, &px, &msg)) return report(false, msg, err, cap);
        memcpy(mask, px.data(), px.size());
    }
    return 0;
}
