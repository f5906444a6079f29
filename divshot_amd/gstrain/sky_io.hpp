// sky_io.hpp — the sky texture file <modelPath>_<it>.sky (host only, no HIP): a 16-byte header — the magic "DVSSKY1\0", uint32 width,
// uint32 height, little-endian — followed by height * width * 3 little-endian fp32 values, row-major [height][width][3].
// width == 2 * height (equirectangular), 2 <= height <= 4096. A file whose size contradicts its header is refused.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace gssky {
constexpr uint32_t kMaxHeight = 4096;
bool write_sky(const std::string& file, uint32_t width, uint32_t height, const float* texels, std::string* err);
bool read_sky(const std::string& file, uint32_t* width, uint32_t* height, std::vector<float>* texels, std::string* err);
}  // namespace gssky
