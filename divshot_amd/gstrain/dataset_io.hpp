// dataset_io.hpp — reader of the capture format the lineage trains from: a COLMAP sparse model (cameras / images / points3D, binary or
// text) plus its images. Host only, no GPU dependency; every malformed input is a `false` with a message, never a crash and
// never an allocation sized by an unchecked count field.
//   <path>/sparse/0/ (tried first) or <path>/sparse/: cameras, images, points3D as .bin (preferred) or .txt
//   <path>/images/<name>: binary PPM (P6, maxval 255), or baseline JPEG when the file's extension is .jpg / .jpeg in any case (decoded by
//                         jpeg_io.hpp + dvs_jpeg_reconstruct, not here), or PNG when it is .png in any case (png_io.hpp +
//                         dvs_png_reconstruct, not here); a name whose file is absent is retried with its extension replaced
//                         by .ppm, then .jpg, .jpeg, .JPG, .JPEG, .png, .PNG
//   <path>/masks/<stem>.pgm (P5, maxval 255): > 127 is trainable; then masks/<stem>.png, then masks/<image name>.png (gray or gray+alpha,
//                         read by the trainer's loader, not here); no file means all ones
// Camera models: SIMPLE_PINHOLE and PINHOLE by default — anything else is refused with the hint to undistort the capture first (the
// lineage's own requirement). With ReadOptions::accept_distorted also SIMPLE_RADIAL, RADIAL and OPENCV, whose coefficients come back
// in Camera::dist: the trainer's loader undistorts their views on the device (include/dvs_image.h: dvs_undistort_view). The fisheye
// models, FULL_OPENCV and FOV stay refused either way: they need atan or a division, and a pinhole target suits no wide fisheye.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gsdata {

struct Camera {
    uint32_t id = 0;
    int model = 0;                       // COLMAP model id: 0 SIMPLE_PINHOLE, 1 PINHOLE; with accept_distorted also 2 SIMPLE_RADIAL, 3 RADIAL, 4 OPENCV
    uint64_t width = 0, height = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0;
    double dist[4] = {0, 0, 0, 0};       // k1, k2, p1, p2 (the coefficients a model lacks are 0)
};
struct Image {
    uint32_t id = 0, camera_id = 0;
    double q[4] = {1, 0, 0, 0};          // qvec (w, x, y, z), world -> camera
    double t[3] = {0, 0, 0};             // tvec, world -> camera
    std::string name;
    size_t camera = 0;                   // index into Dataset::cameras
};
struct Dataset {
    std::string root, sparse_dir;
    bool binary = false;
    std::vector<Camera> cameras;
    std::vector<Image> images;           // ordered by name (a hold-out by index splits as the lineage does)
    std::vector<float> xyz;              // [points][3]
    std::vector<uint8_t> rgb;            // [points][3]
    size_t dropped = 0;                  // points with a non-finite coordinate, not in xyz / rgb
};

const char* model_name(int model);      // "SIMPLE_PINHOLE", "PINHOLE", ... ("?" outside COLMAP's list)

// the sparse model under `path`; images and masks are read one by one with the calls below
bool read_dataset(const std::string& path, Dataset* out, std::string* err);
struct ReadOptions {
    bool accept_distorted = false;      // also read SIMPLE_RADIAL, RADIAL and OPENCV cameras (fx, fy, cx, cy and dist)
};
bool read_dataset(const std::string& path, const ReadOptions& opt, Dataset* out, std::string* err);
// the file of image `index` and whether it is a JPEG: an existing <name> is a JPEG by its extension (.jpg / .jpeg, any case) and a PPM
// otherwise; an absent one is retried as <stem>.ppm, then <stem>.jpg, .jpeg, .JPG, .JPEG
bool resolve_image(const Dataset& d, size_t index, std::string* file, bool* is_jpeg, std::string* err);
// the same with PNG told apart (resolve_image is a wrapper over this one and calls a PNG "not a JPEG", as it always did): an existing
// <name> is a PNG when its extension is .png in any case; an absent one is retried in the order above, then as <stem>.png, <stem>.PNG
enum class ImageKind { PPM = 0, JPEG = 1, PNG = 2 };
bool resolve_image_kind(const Dataset& d, size_t index, std::string* file, ImageKind* kind, std::string* err);
// the mask file of image `index`, the first that exists of masks/<stem>.pgm, masks/<stem>.png, masks/<image name>.png (COLMAP's own
// convention); NONE with an empty `file` when there is none, which means all ones
enum class MaskKind { NONE = 0, PGM = 1, PNG = 2 };
bool resolve_mask(const Dataset& d, size_t index, std::string* file, MaskKind* kind, std::string* err);
// image `index` as interleaved 8-bit RGB [H][W][3]; its size must equal its camera's (PPM only: <name>, else <stem>.ppm)
bool read_image(const Dataset& d, size_t index, std::vector<uint8_t>* rgb, std::string* err);
// its mask as [H][W] bytes in {0, 1}; all ones when <root>/masks/<stem>.pgm does not exist
bool read_mask(const Dataset& d, size_t index, std::vector<uint8_t>* mask, std::string* err);
// world -> camera rotation of an image, row-major [9], from the normalised qvec
void rotation_of(const Image& im, float R[9]);

// binary PNM (P6: channels = 3, P5: channels = 1; maxval 255)
bool read_pnm(const std::string& file, int channels, int* width, int* height, std::vector<uint8_t>* pixels, std::string* err);

}  // namespace gsdata
