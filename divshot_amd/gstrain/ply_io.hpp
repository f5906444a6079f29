// ply_io.hpp — the splat .ply wire format DIVSHOT's viewer loads (external/tinygsplat/tiny_gsplat.cpp:168-241 save,
// :632-722 load; RichPoint external/tinygsplat/tiny_gsplat.hpp:262-269): binary_little_endian, per vertex 59 floats
//   x y z | f_dc_0..2 | f_rest_0..44 | opacity | scale_0..2 | rot_0..3          (236 bytes, no normals)
// with f_rest CHANNEL-major on disk ([c*15 + j], tiny_gsplat.cpp:231-236) while the in-memory shN block is
// coefficient-major [j*3 + c] (gaussian_model.cpp:163-167) — the writer/reader transposes.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/dvs_export.h"

namespace gsply {
bool write_ply(const std::string& path, size_t n, const float* pos, const float* sh0, const float* shN, const float* opacity,
               const float* scale, const float* rot, bool antialiased, std::string* err);
bool read_ply(const std::string& path, std::vector<float>& pos, std::vector<float>& sh0, std::vector<float>& shN,
              std::vector<float>& opacity, std::vector<float>& scale, std::vector<float>& rot, std::string* err);
// The viewer's two compact formats, written from payloads packed on the device (include/dvs_export.h):
// the chunked, quantised PLY with the header of tiny_gsplat.cpp:371-391 — `element chunk` ceil(n / 256) rows of 12 floats, then
// `element vertex` n records of 4 uints (packed_position, packed_rotation, packed_scale, packed_color) — read by load_compress_ply
// (tiny_gsplat.cpp:766-815); and the headerless .splat file of 32-byte records (tiny_gsplat.cpp:243-291).
bool write_compressed_ply(const std::string& path, size_t n, const float* chunks, const uint32_t* verts, bool antialiased, std::string* err);
bool write_splat(const std::string& path, size_t n, const uint8_t* bytes, std::string* err);
// .spz version 3 (external/spz/src/load-spz.cc serializePackedGaussians / saveSpz): through gzip, the 16-byte header — magic 0x5053474e,
// version 3, numPoints, shDegree, fractionalBits 12, flags (bit 0: antialiased), reserved 0 — then the six sections of the buffer
// dvs_pack_spz filled, bytes[k] bytes from off[k] each. zlib is resolved at run time (dlopen of libz.so.1: gzopen / gzwrite /
// gzclose); without it the call fails with a message naming the library or the symbol.
bool write_spz(const std::string& path, size_t n, int sh_degree, bool antialiased, const uint8_t* packed, const dvs_spz_layout& layout,
               std::string* err);
// .reduced.ply, quantised (tiny_gsplat.cpp save_reduced_ply with quantised = true, read by load_reduced_ply): the header — `element
// vertex <count>` four times, one block per SH degree 0..3, each with `property float|f16 x y z` and its `property u8` ids (f_dc_0..2,
// f_rest_0..3 coeffs - 1, opacity, scale_0..2, rot_0..3), then `element cook_center 256` with the 20 float columns — and the payload
// dvs_pack_reduced filled, layout->total bytes. An empty block keeps its header lines. Refused, with a message and nothing written: a
// NULL layout or payload, a layout that is not the one its counts and half imply, no splats, payload_bytes != layout->total.
bool write_reduced_ply(const std::string& path, const dvs_reduced_layout* layout, const uint8_t* payload, uint64_t payload_bytes, std::string* err);
// The extracted surface (include/dvs_mesh.h): binary_little_endian PLY, `element vertex` x y z float + red green blue uchar (15 bytes),
// `element face` with `property list uchar uint vertex_indices` (13 bytes per triangle). An empty mesh is a valid file with zero
// elements. Refused, with a message, when an index is >= n_vertices (nothing is written then). With `normals` ([n_vertices][3]) the
// vertex carries nx ny nz float between z and red (27 bytes); without them the file is what it always was.
bool write_mesh_ply(const std::string& path, size_t n_vertices, const float* xyz, const uint8_t* rgb, size_t n_triangles, const uint32_t* tri,
                    std::string* err, const float* normals = nullptr);
}
