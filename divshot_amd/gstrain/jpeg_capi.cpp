// jpeg_capi.cpp — plain-C entry points of the JPEG coefficient decoder (jpeg_io.hpp) and encoder (jpeg_write.hpp, at the end) in libgsplyio.so, the host-only library of
// ply_capi.cpp and dataset_capi.cpp, so that the decoder can be tested from Python without a GPU or the HIP runtime. Every call returns
// 0 on success; a failure of gstrain_jpeg_open leaves its message (NUL-terminated, cut to `cap`) in `err`.
#include <cstdint>
#include <cstring>
#include <exception>
#include <string>
#include "jpeg_io.hpp"
#include "jpeg_write.hpp"

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

// ---- the encoder (jpeg_write.hpp) ----
// A frame's pieces in, a JFIF byte stream out: ints[15], quant[3][64] and offsets[4] exactly as gstrain_jpeg_info hands them out
// (offsets[3] = the number of values `coef` holds). Returns a handle (NULL with a message in `err` when the frame is refused);
// gstrain_jpeg_encoded_size / _bytes read it, gstrain_jpeg_encoded_free releases it.
// Nothing is thrown across the boundary: an allocation failure is a NULL with its message like any other refusal.
static void put_err(char* err, int cap, const char* msg) { if (err && cap > 0) { strncpy(err, msg, (size_t)cap - 1); err[cap - 1] = 0; } }
GSJPEG_API void* gstrain_jpeg_encode(const int32_t* ints, const uint16_t* quant, const uint64_t* offsets, const int16_t* coef, char* err, int cap) {
    if (!ints || !quant || !offsets || !coef) { put_err(err, cap, "jpeg encode: a NULL argument"); return nullptr; }
    std::string* out = nullptr;
    try {
        out = new std::string();
        std::string msg;
        int hs[3], vs[3], bw[3], bh[3];
        for (int k = 0; k < 3; ++k) { hs[k] = ints[3 + k]; vs[k] = ints[6 + k]; bw[k] = ints[9 + k]; bh[k] = ints[12 + k]; }
        if (gsjpeg::encode_coefficients(ints[0], ints[1], ints[2], hs, vs, (const uint16_t(*)[64])quant, bw, bh, offsets, coef, offsets[3], out, &msg)) return out;
        put_err(err, cap, msg.c_str());
    } catch (const std::exception& e) {
        put_err(err, cap, e.what());
    } catch (...) {
        put_err(err, cap, "jpeg encode: unknown exception");
    }
    delete out;
    return nullptr;
}
GSJPEG_API uint64_t gstrain_jpeg_encoded_size(const void* h) { return h ? ((const std::string*)h)->size() : 0; }
GSJPEG_API int gstrain_jpeg_encoded_bytes(const void* h, uint8_t* dst) {
    if (!h || !dst) return 1;
    const std::string* v = (const std::string*)h;
    memcpy(dst, v->data(), v->size());
    return 0;
}
GSJPEG_API void gstrain_jpeg_encoded_free(void* h) { delete (std::string*)h; }
// the same as gstrain_jpeg_open over bytes in memory (what the encoder returned), so that a round trip needs no file
GSJPEG_API void* gstrain_jpeg_open_memory(const uint8_t* data, uint64_t size, char* err, int cap) {
    if (!data) { put_err(err, cap, "NULL data"); return nullptr; }
    gsjpeg::Frame* f = nullptr;
    try {
        f = new gsjpeg::Frame();
        std::string msg;
        if (gsjpeg::decode_coefficients(data, (size_t)size, "memory", f, &msg)) return f;
        put_err(err, cap, msg.c_str());
    } catch (const std::exception& e) {
        put_err(err, cap, e.what());
    } catch (...) {
        put_err(err, cap, "jpeg decode: unknown exception");
    }
    delete f;
    return nullptr;
}
