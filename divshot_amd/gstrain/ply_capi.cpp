// ply_capi.cpp — libgsplyio.so: plain-C entry points of the compact-format file writers (ply_io.hpp), in a host-only library of their
// own so that the wire formats can be tested from Python without a GPU or the HIP runtime. libgstrain.so links the same ply_io.cpp
// and keeps its pinned set of exported symbols.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
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
// `packed`: the six sections at layout->off[k]; on failure the message goes to err_out (when given, NUL-terminated, at most err_cap bytes)
__attribute__((visibility("default"))) int gstrain_write_spz(const char* path, uint64_t n, int sh_degree, int antialiased, const uint8_t* packed,
                                                              const dvs_spz_layout* layout, char* err_out, uint64_t err_cap) {
    std::string err;
    if (gsply::write_spz(path, (size_t)n, sh_degree, antialiased != 0, packed, *layout, &err)) return 0;
    if (err_out && err_cap > 0) { const size_t k = std::min<size_t>(err.size(), (size_t)err_cap - 1); memcpy(err_out, err.data(), k); err_out[k] = 0; }
    return 1;
}
// `payload`: the payload_bytes bytes that follow end_header (dvs_pack_reduced); layout or payload may be NULL: refused with a message
__attribute__((visibility("default"))) int gstrain_write_reduced_ply(const char* path, const dvs_reduced_layout* layout, const uint8_t* payload,
                                                                      uint64_t payload_bytes, char* err_out, uint64_t err_cap) {
    std::string err;
    if (gsply::write_reduced_ply(path, layout, payload, payload_bytes, &err)) return 0;
    if (err_out && err_cap > 0) { const size_t k = std::min<size_t>(err.size(), (size_t)err_cap - 1); memcpy(err_out, err.data(), k); err_out[k] = 0; }
    return 1;
}
__attribute__((visibility("default"))) int gstrain_write_mesh_ply(const char* path, uint64_t n_vertices, const float* xyz, const uint8_t* rgb,
                                                                   uint64_t n_triangles, const uint32_t* tri, char* err_out, uint64_t err_cap) {
    std::string err;
    if (gsply::write_mesh_ply(path, (size_t)n_vertices, xyz, rgb, (size_t)n_triangles, tri, &err)) return 0;
    if (err_out && err_cap > 0) { const size_t k = std::min<size_t>(err.size(), (size_t)err_cap - 1); memcpy(err_out, err.data(), k); err_out[k] = 0; }
    return 1;
}
// ... with vertex normals ([n_vertices][3]; NULL = the call above)
__attribute__((visibility("default"))) int gstrain_write_mesh_ply_normals(const char* path, uint64_t n_vertices, const float* xyz, const float* normals,
                                                                           const uint8_t* rgb, uint64_t n_triangles, const uint32_t* tri, char* err_out,
                                                                           uint64_t err_cap) {
    std::string err;
    if (gsply::write_mesh_ply(path, (size_t)n_vertices, xyz, rgb, (size_t)n_triangles, tri, &err, normals)) return 0;
    if (err_out && err_cap > 0) { const size_t k = std::min<size_t>(err.size(), (size_t)err_cap - 1); memcpy(err_out, err.data(), k); err_out[k] = 0; }
    return 1;
}
// gsply::read_ply of a full PLY (the resume file, .transformed.ply): -> the splat count, or -1 when the file is refused; the six arrays are
// filled (shN coefficient-major [n][45]) when pos is given and n <= capacity
__attribute__((visibility("default"))) int64_t gstrain_host_read_ply(const char* path, float* pos, float* sh0, float* shN, float* opacity, float* scale,
                                                                      float* rot, uint64_t capacity) {
    std::vector<float> a, b, c, d, e, f;
    std::string err;
    if (!gsply::read_ply(path, a, b, c, d, e, f, &err)) return -1;
    const uint64_t n = d.size();
    if (pos && n <= capacity) {
        memcpy(pos, a.data(), a.size() * 4); memcpy(sh0, b.data(), b.size() * 4); memcpy(shN, c.data(), c.size() * 4);
        memcpy(opacity, d.data(), d.size() * 4); memcpy(scale, e.data(), e.size() * 4); memcpy(rot, f.data(), f.size() * 4);
    }
    return (int64_t)n;
}
}
