// jpeg_capi.cpp — plain-C entry points of the JPEG coefficient decoder (jpeg_io.hpp) in libgsplyio.so, the host-only library of
// ply_capi.cpp and dataset_capi.cpp, so that the decoder can be tested from Python without a GPU or the HIP runtime. Every call returns
// 0 on success; a failure of gstrain_jpeg_open leaves its message (NUL-terminated, cut to `cap`) in `err`.
#include <cstdint>
#include <cstring>
#include <string>
#include "jpeg_io.hpp"

#define GSJPEG_API extern "C" __attribute__((visibility("default")))

GSJPEG_API void* gstrain_jpeg_open(const char* file, char* err, int cap) {
    gsjpeg::Frame* f = new gsjpeg::Frame();
    std::string msg = "NULL path";
    if (!file || !gsjpeg::decode_coefficients(file, f, &msg)) {
        if (err && cap > 0) { strncpy(err, msg.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
        delete f;
        return nullptr;
    }
    return f;
}
GSJPEG_API void gstrain_jpeg_close(void* h) { delete (gsjpeg::Frame*)h; }
// ints[15] = {width, height, components, hs[3], vs[3], blocks_w[3], blocks_h[3]}, quant[3][64] in natural order,
// offsets[4] = {offset[3] in coefficients, their total count}
GSJPEG_API int gstrain_jpeg_info(const void* h, int32_t* ints, uint16_t* quant, uint64_t* offsets) {
    const gsjpeg::Frame* f = (const gsjpeg::Frame*)h;
    if (!f || !ints || !quant || !offsets) return 1;
    ints[0] = f->width; ints[1] = f->height; ints[2] = f->components;
    for (int k = 0; k < 3; ++k) { ints[3 + k] = f->hs[k]; ints[6 + k] = f->vs[k]; ints[9 + k] = f->blocks_w[k]; ints[12 + k] = f->blocks_h[k]; offsets[k] = f->offset[k]; }
    offsets[3] = f->coef.size();
    memcpy(quant, f->quant, sizeof f->quant);
    return 0;
}
GSJPEG_API int gstrain_jpeg_coefficients(const void* h, int16_t* out) {
    const gsjpeg::Frame* f = (const gsjpeg::Frame*)h;
    if (!f || !out) return 1;
    memcpy(out, f->coef.data(), f->coef.size() * sizeof(int16_t));
    return 0;
}
