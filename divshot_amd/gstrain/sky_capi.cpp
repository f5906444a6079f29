// sky_capi.cpp — plain-C entry points of the sky texture file's reader and writer (sky_io.hpp) in libgsplyio.so, the host-only library, so
// that the format can be tested from Python without a GPU. 0 on success; a failure leaves its message (NUL-terminated, cut to `cap`) in `err`.
#include <cstring>
#include <exception>
#include "sky_io.hpp"

#define GSSKY_API extern "C" __attribute__((visibility("default")))

static int report(const std::string& msg, char* err, int cap) {
    if (err && cap > 0) { strncpy(err, msg.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
    return 1;
}
GSSKY_API int gstrain_sky_write(const char* file, uint32_t width, uint32_t height, const float* texels, char* err, int cap) {
    std::string msg = "NULL path";
    try {
        if (file && gssky::write_sky(file, width, height, texels, &msg)) return 0;
    } catch (const std::exception& e) { msg = e.what(); }
    return report(msg, err, cap);
}
// texels == NULL: only the size is returned (dims[2] = {width, height}); else `capacity` floats are available at texels
GSSKY_API int gstrain_sky_read(const char* file, uint32_t* dims, float* texels, uint64_t capacity, char* err, int cap) {
    std::string msg = "NULL argument";
    try {
        std::vector<float> t;
        if (file && dims && gssky::read_sky(file, &dims[0], &dims[1], &t, &msg)) {
            if (!texels) return 0;
            if (capacity < t.size()) return report("capacity too small", err, cap);
            memcpy(texels, t.data(), t.size() * sizeof(float));
            return 0;
        }
    } catch (const std::exception& e) { msg = e.what(); }
    return report(msg, err, cap);
}
