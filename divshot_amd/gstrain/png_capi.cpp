// png_capi.cpp — plain-C entry points of the PNG host half (png_io.hpp) in libgsplyio.so, the host-only library of ply_capi.cpp,
// dataset_capi.cpp and jpeg_capi.cpp, so that it can be tested from Python without a GPU or the HIP runtime. Every call returns 0 on
// success; a failure of gstrain_png_open / _open_memory is a NULL with its message (NUL-terminated, cut to `cap`) in `err`. Nothing is
// thrown across the boundary: an allocation failure is a NULL with its message like any other refusal.
#include <cstdint>
#include <cstring>
#include <exception>
#include <string>
#include "png_io.hpp"

#define GSPNG_API extern "C" __attribute__((visibility("default")))

namespace {
void put_err(char* err, int cap, const char* msg) { if (err && cap > 0) { strncpy(err, msg, (size_t)cap - 1); err[cap - 1] = 0; } }

template <class Decode> void* open_with(const Decode& decode, char* err, int cap) {
    gspng::Frame* f = nullptr;
    try {
        f = new gspng::Frame();
        std::string msg;
        if (decode(f, &msg)) return f;
        put_err(err, cap, msg.c_str());
    } catch (const std::exception& e) {
        put_err(err, cap, e.what());
    } catch (...) {
        put_err(err, cap, "png decode: unknown exception");
    }
    delete f;
    return nullptr;
}
}  // namespace

GSPNG_API void* gstrain_png_open(const char* file, char* err, int cap) {
    if (!file) { put_err(err, cap, "NULL path"); return nullptr; }
    return open_with([&](gspng::Frame* f, std::string* msg) { return gspng::decode_filtered(file, f, msg); }, err, cap);
}
GSPNG_API void* gstrain_png_open_memory(const uint8_t* data, uint64_t size, char* err, int cap) {
    if (!data) { put_err(err, cap, "NULL data"); return nullptr; }
    return open_with([&](gspng::Frame* f, std::string* msg) { return gspng::decode_filtered(data, (size_t)size, "memory", f, msg); }, err, cap);
}
GSPNG_API void gstrain_png_close(void* h) { delete (gspng::Frame*)h; }
// ints[5] = {width, height, bit depth, colour type, 1 if there is a colour key}, key[3], palette[256][4] (RGBA),
// *filtered_bytes = height * (1 + rowbytes)
GSPNG_API int gstrain_png_info(const void* h, int32_t* ints, uint16_t* key, uint8_t* palette, uint64_t* filtered_bytes) {
    const gspng::Frame* f = (const gspng::Frame*)h;
    if (!f || !ints || !key || !palette || !filtered_bytes) return 1;
    ints[0] = f->width; ints[1] = f->height; ints[2] = f->bit_depth; ints[3] = f->color_type; ints[4] = f->has_key ? 1 : 0;
    for (int k = 0; k < 3; ++k) key[k] = f->key[k];
    memcpy(palette, f->palette, sizeof f->palette);
    *filtered_bytes = f->filtered.size();
    return 0;
}
GSPNG_API int gstrain_png_filtered(const void* h, uint8_t* out) {
    const gspng::Frame* f = (const gspng::Frame*)h;
    if (!f || !out) return 1;
    memcpy(out, f->filtered.data(), f->filtered.size());
    return 0;
}
