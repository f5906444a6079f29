// png_capi.cpp — plain-C entry points of the PNG host halves (png_io.hpp: the decoder, and the writer as gstrain_png_write) in libgsplyio.so, the host-only library of ply_capi.cpp,
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
// gspng::write_png: ints[5] = {width, height, bit depth, colour type, zlib level}; keys / texts: n_text NUL-terminated strings each (NULL
// with n_text = 0). *out_size = the file's bytes; they are copied to `out` when it is not NULL (a NULL `out` only asks for the size) and
// must then fit `cap`. -> 0, or 1 with the writer's message in `err` and *out_size = 0.
GSPNG_API int gstrain_png_write(const int32_t* ints, const uint8_t* filtered, uint64_t filtered_bytes, const char* const* keys, const char* const* texts,
                                int n_text, uint8_t* out, uint64_t cap, uint64_t* out_size, char* err, int err_cap) {
    if (out_size) *out_size = 0;
    if (!ints || !out_size || n_text < 0 || (n_text > 0 && (!keys || !texts))) { put_err(err, err_cap, "NULL argument"); return 1; }
    try {
        gspng::TextPairs text;
        for (int k = 0; k < n_text; ++k) {
            if (!keys[k] || !texts[k]) { put_err(err, err_cap, "NULL tEXt string"); return 1; }
            text.emplace_back(keys[k], texts[k]);
        }
        std::string file, msg;
        if (!gspng::write_png(ints[0], ints[1], ints[2], ints[3], filtered, (size_t)filtered_bytes, ints[4], &text, &file, &msg)) { put_err(err, err_cap, msg.c_str()); return 1; }
        if (out && file.size() > cap) { put_err(err, err_cap, ("a buffer of " + std::to_string(cap) + " bytes for a file of " + std::to_string(file.size())).c_str()); return 1; }
        if (out) memcpy(out, file.data(), file.size());
        *out_size = file.size();
        return 0;
    } catch (const std::exception& e) {
        put_err(err, err_cap, e.what());
    } catch (...) {
        put_err(err, err_cap, "png write: unknown exception");
    }
    return 1;
}
GSPNG_API int gstrain_png_filtered(const void* h, uint8_t* out) {
    const gspng::Frame* f = (const gspng::Frame*)h;
    if (!f || !out) return 1;
    memcpy(out, f->filtered.data(), f->filtered.size());
    return 0;
}
