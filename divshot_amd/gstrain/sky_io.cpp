// sky_io.cpp — reader and writer of the sky texture file (sky_io.hpp).
#include "sky_io.hpp"
#include <cstdio>
#include <cstring>

namespace gssky {
namespace {
const char kMagic[8] = {'D', 'V', 'S', 'S', 'K', 'Y', '1', '\0'};
bool fail(std::string* err, const std::string& what) { if (err) *err = what; return false; }
void put_u32(unsigned char* p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (unsigned char)(v >> (8 * k)); }
uint32_t get_u32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
bool shape_ok(uint32_t width, uint32_t height) { return height >= 2 && height <= kMaxHeight && width == 2 * height; }
}  // namespace

bool write_sky(const std::string& file, uint32_t width, uint32_t height, const float* texels, std::string* err) {
    if (!texels || !shape_ok(width, height)) return fail(err, "sky texture must have 2 <= height <= 4096 and width == 2 * height");
    const size_t count = (size_t)width * height * 3;
    std::vector<unsigned char> buf(16 + count * 4);
    memcpy(buf.data(), kMagic, 8);
    put_u32(buf.data() + 8, width); put_u32(buf.data() + 12, height);
    for (size_t i = 0; i < count; ++i) { uint32_t bits; memcpy(&bits, &texels[i], 4); put_u32(buf.data() + 16 + 4 * i, bits); }
    FILE* f = fopen(file.c_str(), "wb");
    if (!f) return fail(err, "cannot open " + file + " for writing");
    const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0 || !ok) return fail(err, "cannot write " + file);
    return true;
}

bool read_sky(const std::string& file, uint32_t* width, uint32_t* height, std::vector<float>* texels, std::string* err) {
    if (!width || !height || !texels) return fail(err, "null argument");
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return fail(err, "cannot open " + file);
    unsigned char head[16];
    if (fread(head, 1, 16, f) != 16) { fclose(f); return fail(err, file + ": shorter than the 16-byte header"); }
    if (memcmp(head, kMagic, 8) != 0) { fclose(f); return fail(err, file + ": not a sky texture (wrong magic)"); }
    const uint32_t w = get_u32(head + 8), h = get_u32(head + 12);
    if (!shape_ok(w, h)) { fclose(f); return fail(err, file + ": header says " + std::to_string(w) + " x " + std::to_string(h) + " (needs width == 2 * height, 2 <= height <= 4096)"); }
    const size_t bytes = (size_t)w * h * 3 * 4;
    std::vector<unsigned char> buf(bytes + 1);                             // one more: a longer file is refused too
    const size_t got = fread(buf.data(), 1, bytes + 1, f);
    fclose(f);
    if (got != bytes)
        return fail(err, file + ": the header says " + std::to_string(bytes) + " bytes of texels, the file holds " + (got > bytes ? "more" : std::to_string(got)));
    texels->resize((size_t)w * h * 3);
    for (size_t i = 0; i < texels->size(); ++i) { const uint32_t bits = get_u32(buf.data() + 4 * i); memcpy(&(*texels)[i], &bits, 4); }
    *width = w; *height = h;
    return true;
}
}  // namespace gssky
