// png_io.hpp — the serial halves of PNG decoding and (write_png, further down) encoding. Decoding: chunk parsing and inflate, file -> FILTERED scanlines (the inflated IDAT stream exactly
// as stored: per row one filter byte and rowbytes = ceil(W * channels * depth / 8) bytes). Host only, no GPU dependency; a pure function
// without mutable globals, so any number of threads may decode different files at once. The parallel half (the five filters, sample
// expansion, palette, transparency) is dvs_png_reconstruct (include/dvs_image.h); tests/png_ref.py restates both.
//   Accepted: non-interlaced PNG of every legal (colour type, bit depth) pair: gray 1/2/4/8/16, RGB 8/16, palette 1/2/4/8, gray+alpha
//             8/16, RGBA 8/16; any number of consecutive IDAT chunks, split anywhere; tRNS as the palette's alpha table or as the colour
//             key of types 0 and 2; every ancillary chunk is skipped (gAMA, sRGB, iCCP, the APNG chunks: the default image is decoded).
//   Refused with a message that names the kind: a wrong signature, a chunk CRC that does not match (the CRC-32 table is this file's),
//             a first chunk other than IHDR, an illegal type / depth pair, a side of 0 or above 65500, Adam7 interlacing, a compression
//             or filter method other than 0, an unknown critical chunk, type 3 without PLTE, a PLTE whose length is no multiple of 3 or
//             beyond 256 entries, a tRNS longer than the palette or of the wrong length for types 0 and 2, tRNS on types 4 and 6, IDAT
//             chunks that are not consecutive, no IDAT, no IEND, an inflate error, an inflated stream shorter or longer than
//             H * (1 + rowbytes), a scanline whose filter byte is above 4 (so that the device never has to refuse).
//   zlib is resolved at run time (zlib_dl.hpp); without it the file is refused with the message that names the library or the symbol.
// The file is read whole and parsed through a bounds-checked cursor; every chunk length is compared with the bytes left before it is
// used. `filtered` is sized from the validated header and refused before it is allocated when the IDAT bytes could not inflate to that
// much (deflate expands at most 1032 : 1). Every malformed input is a `false` with a message, never a crash.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace gspng {

constexpr uint32_t kMaxSide = 65500;

struct Frame {
    int width = 0, height = 0, bit_depth = 0, color_type = 0;
    uint8_t palette[256][4] = {};         // RGBA; entries the file does not give are opaque black
    bool has_key = false;                 // tRNS on type 0 (key[0]) or type 2 (key[0..2]), at the file's depth
    uint16_t key[3] = {0, 0, 0};
    std::vector<uint8_t> filtered;        // exactly height * (1 + rowbytes) bytes
};

// samples per pixel of a colour type (0 for a type PNG does not have)
int channels_of(int color_type);
// bytes of one scanline without its filter byte; 0 for an illegal type / depth pair or a side outside 1..kMaxSide
size_t row_bytes(int width, int bit_depth, int color_type);
// true when reconstruction yields an alpha plane that is not 255 everywhere by definition: types 4 and 6, a colour key, a palette tRNS
bool has_alpha(const Frame& f);

bool decode_filtered(const std::string& file, Frame* out, std::string* err);
// the same over bytes already in memory; `name` prefixes the messages
bool decode_filtered(const uint8_t* data, size_t size, const std::string& name, Frame* out, std::string* err);

// The serial half of PNG ENCODING, the mirror image of decode_filtered: a filtered stream (what dvs_png_encode_views writes: per row one
// filter byte 0..4 and rowbytes bytes) -> a whole PNG file in *out: the signature, IHDR, one tEXt chunk per (keyword, text) pair of
// `text` (nullable), the zlib stream of `filtered` at `level` 0..9 in IDAT chunks of at most kMaxIdat bytes, IEND; CRCs from this
// file's table, deflate through zlib_dl.hpp. A pure function without statics: any number of threads may write different files at once.
// Refused with a message in *err and *out left empty: a NULL filtered or out, an illegal type / depth pair, a side outside 1..kMaxSide,
// a size other than height * (1 + rowbytes), a filter byte above 4, a level outside 0..9, a keyword that is not 1..79 Latin-1
// characters (32..126 and 161..255, no space at either end, no two spaces in a row) or a text with a NUL in it, zlib missing.
constexpr size_t kMaxIdat = 1u << 20;
using TextPairs = std::vector<std::pair<std::string, std::string>>;
bool write_png(int width, int height, int bit_depth, int color_type, const uint8_t* filtered, size_t size, int level, const TextPairs* text,
               std::string* out, std::string* err);

// the five filters undone in place by a plain loop, one thread: what the device half replaces (png_check times it)
void unfilter_host(const Frame& f, uint8_t* filtered);

}  // namespace gspng
