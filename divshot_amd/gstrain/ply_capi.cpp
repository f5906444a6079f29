// ply_capi.cpp — libgsplyio.so: plain-C entry points of the compact-format file writers (ply_io.hpp), in a host-only library of their
// own so that the wire formats can be tested from Python without a GPU or the HIP runtime. libgstrain.so links the same ply_io.cpp
// and keeps its pinned set of exported symbols.
#include <cstdint>
#include <string>
#include "ply_io.hpp"

extern "C" {
__attribute__((visibility("default"))) int gstrain_write_compressed_ply(const char* path, uint64_t n, const float* chunks, const uint32_t* verts,
                                                                         int antialiased) {
    std::string err;
    return gsply::write_compressed_ply(path, (size_t)n, chunks, verts, antialiased != 0, &err) ? 0 : 1;
}
__attribute__((visibility("default"))) int gstrain_write_splat(const char* path, uint64_t n, const uint8_t* bytes) {
    std::string err;
    return gsply::write_splat(path, (size_t)n, bytes, &err) ? 0 : 1;
}
}
