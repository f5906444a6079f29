// jpeg_io.hpp — the serial half of baseline JPEG decoding: marker parsing and Huffman entropy decoding, file -> quantised DCT
// coefficients. Host only, no GPU dependency, no library; a pure function without mutable globals or statics, so any number of threads
// may decode different files at once. The parallel half (dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB) is
// dvs_jpeg_reconstruct (include/dvs_image.h); tests/jpeg_ref.py restates both.
//   Accepted: SOF0 / SOF1 with 8-bit samples (baseline / extended sequential Huffman), 8- or 16-bit DQT, DRI with RST0-7, optimised
//             Huffman tables, ONE interleaved scan; grayscale, or YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1.
//   Rejected with a message that names the kind: progressive, arithmetic, lossless, hierarchical, 12-bit, 4 components, RGB (Adobe
//             transform 0), multi-scan sequential, other sampling factors, missing tables, a side of 0 or above 65500.
//   EXIF orientation is ignored, as COLMAP ignores it: the pixels come out as stored.
// The file is read whole and parsed through a bounds-checked cursor; every segment length is compared with the bytes left before it is
// used. The coefficient array is sized from the validated width, height and sampling factors, capped at kMaxCoefficients, and refused
// when the bytes left in the file could not hold that many blocks (a block takes at least 2 bits). Every malformed input is a `false`
// with a message, never a crash.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gsjpeg {

constexpr uint32_t kMaxSide = 65500;
constexpr uint64_t kMaxCoefficients = 1ull << 29;   // int16 values = 1 GiB: 178 Mpixel at 4:4:4, 357 Mpixel at 4:2:0

struct Frame {
    int width = 0, height = 0, components = 0;       // components: 1 (grayscale) or 3 (Y, Cb, Cr)
    int hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};        // sampling factors (a grayscale file's are normalised to 1x1)
    uint16_t quant[3][64] = {};                      // per component, natural (de-zigzagged) order: index = 8 v + u
    int blocks_w[3] = {0, 0, 0}, blocks_h[3] = {0, 0, 0};   // blocks per row / per column, padded to whole MCUs
    uint64_t offset[3] = {0, 0, 0};                  // first coefficient of the component in `coef`; multiples of 8 (16 bytes)
    std::vector<int16_t> coef;                       // component-major, block-row-major, 64 natural-order coefficients per block
};

bool decode_coefficients(const std::string& file, Frame* out, std::string* err);
// the same over bytes already in memory; `name` prefixes the messages
bool decode_coefficients(const uint8_t* data, size_t size, const std::string& name, Frame* out, std::string* err);

}  // namespace gsjpeg
