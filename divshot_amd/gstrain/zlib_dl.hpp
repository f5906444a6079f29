// zlib_dl.hpp — zlib, resolved at run time: dlopen("libz.so.1"), no link-time dependency and no zlib header (the gzFile handle is opaque, the
// z_stream is restated below). ONE loader for its users: ply_io.cpp writes .spz through gzopen / gzwrite / gzclose, png_io.cpp inflates
// IDAT streams through inflateInit_ / inflate / inflateEnd and deflates them (write_png) through deflateInit_ / deflate / deflateEnd. api() loads the library once (thread-safe) and never unloads it; when the
// library or one of the symbols is missing, Api::err names it and every pointer is to be left alone.
#pragma once
#include <dlfcn.h>
#include <cstdint>
#include <string>

namespace gszlib {

struct Stream {                           // z_stream of zlib 1.x, field for field
    const uint8_t* next_in; unsigned avail_in; unsigned long total_in;
    uint8_t* next_out; unsigned avail_out; unsigned long total_out;
    const char* msg; void* state;
    void* zalloc; void* zfree; void* opaque;
    int data_type; unsigned long adler; unsigned long reserved;
};
constexpr int kOk = 0, kStreamEnd = 1, kBufError = -5, kNoFlush = 0, kFinish = 4;

struct Api {
    void* (*gzopen)(const char*, const char*) = nullptr;
    int (*gzwrite)(void*, const void*, unsigned) = nullptr;
    int (*gzclose)(void*) = nullptr;
    const char* (*zlibVersion)() = nullptr;
    int (*inflateInit_)(Stream*, const char*, int) = nullptr;
    int (*inflate)(Stream*, int) = nullptr;
    int (*inflateEnd)(Stream*) = nullptr;
    int (*deflateInit_)(Stream*, int, const char*, int) = nullptr;
    int (*deflate)(Stream*, int) = nullptr;
    int (*deflateEnd)(Stream*) = nullptr;
    std::string err;
    Api() {
        void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) { err = std::string("cannot dlopen libz.so.1: ") + dlerror(); return; }
#define GSZLIB_SYM(field) field = (decltype(field))dlsym(h, #field); if (!field) { err = "libz.so.1 lacks " #field; return; }
        GSZLIB_SYM(gzopen) GSZLIB_SYM(gzwrite) GSZLIB_SYM(gzclose) GSZLIB_SYM(zlibVersion) GSZLIB_SYM(inflateInit_) GSZLIB_SYM(inflate) GSZLIB_SYM(inflateEnd)
        GSZLIB_SYM(deflateInit_) GSZLIB_SYM(deflate) GSZLIB_SYM(deflateEnd)
#undef GSZLIB_SYM
    }
};

inline const Api& api() {
    static const Api z;                   // (initialised once, thread-safe)
    return z;
}

}  // namespace gszlib
