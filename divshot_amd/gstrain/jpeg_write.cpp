// jpeg_write.cpp — see jpeg_write.hpp
#include "jpeg_write.hpp"
#include <cstring>

namespace gsjpeg {
namespace {
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K, tables K.3 - K.6: code counts per length 1..16, then the symbols in code order
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

struct Codes { uint16_t code[256]; uint8_t len[256]; };        // len 0: the table has no code for the symbol
void make_codes(const uint8_t bits[16], const uint8_t* vals, Codes* c) {
    memset(c, 0, sizeof *c);
    unsigned code = 0, k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < bits[length - 1]; ++i) { c->code[vals[k]] = (uint16_t)code++; c->len[vals[k]] = (uint8_t)length; ++k; }
        code <<= 1;
    }
}

struct Bits {
    std::string& out;
    uint64_t acc = 0;
    int n = 0;
    void put(unsigned value, int count) {                      // count <= 27
        acc = (acc << count) | (value & ((1u << count) - 1u));
        n += count;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            out.push_back((char)b);
            if (b == 0xFF) out.push_back((char)0);
            n -= 8;
        }
    }
    void flush() { if (n) put((1u << (8 - n)) - 1u, 8 - n); }
};
inline int category(int v) { unsigned a = (unsigned)(v < 0 ? -v : v); int s = 0; while (a) { ++s; a >>= 1; } return s; }
inline void put8(std::string& o, unsigned v) { o.push_back((char)(uint8_t)v); }
inline void put16(std::string& o, unsigned v) { put8(o, v >> 8); put8(o, v); }
void put_dht(std::string& o, int tc_th, const uint8_t bits[16], const uint8_t* vals, int n) {
    put8(o, 0xFF); put8(o, 0xC4); put16(o, (unsigned)(2 + 1 + 16 + n));
    put8(o, (unsigned)tc_th);
    o.append((const char*)bits, 16);
    o.append((const char*)vals, (size_t)n);
}
bool fail(std::string* err, const std::string& msg) { if (err) *err = msg; return false; }
}  // namespace

bool encode_coefficients(int width, int height, int components, const int hs[3], const int vs[3], const uint16_t quant[3][64],
                         const int blocks_w[3], const int blocks_h[3], const uint64_t offset[3], const int16_t* coef, uint64_t n_coef,
                         std::string* out, std::string* err) {
    if (!hs || !vs || !quant || !blocks_w || !blocks_h || !offset || !coef || !out) return fail(err, "jpeg encode: a NULL argument");
    if (width < 1 || height < 1 || (uint32_t)width > kMaxSide || (uint32_t)height > kMaxSide)
        return fail(err, "jpeg encode: image size " + std::to_string(width) + "x" + std::to_string(height) + " (a side of 0 or above 65500)");
    if (components != 1 && components != 3) return fail(err, "jpeg encode: " + std::to_string(components) + " components; only grayscale and YCbCr");
    const int H = hs[0], V = vs[0];
    const bool sampling = components == 1 ? (H == 1 && V == 1)
                                          : ((H == 1 && V == 1) || (H == 2 && (V == 1 || V == 2))) && hs[1] == 1 && vs[1] == 1 && hs[2] == 1 && vs[2] == 1;
    if (!sampling) return fail(err, "jpeg encode: sampling factors; only luma 1x1, 2x1, 2x2 with chroma 1x1");
    const int mx = (width + 8 * H - 1) / (8 * H), my = (height + 8 * V - 1) / (8 * V);
    for (int c = 0; c < components; ++c) {
        if (blocks_w[c] != mx * hs[c] || blocks_h[c] != my * vs[c])
            return fail(err, "jpeg encode: component " + std::to_string(c) + " has " + std::to_string(blocks_w[c]) + "x" + std::to_string(blocks_h[c]) +
                                 " blocks, the size and sampling ask for " + std::to_string(mx * hs[c]) + "x" + std::to_string(my * vs[c]));
        const uint64_t need = (uint64_t)blocks_w[c] * (uint64_t)blocks_h[c] * 64;
        if (offset[c] > n_coef || need > n_coef - offset[c])
            return fail(err, "jpeg encode: component " + std::to_string(c) + " needs " + std::to_string(need) + " coefficients from offset " +
                                 std::to_string(offset[c]) + ", the array holds " + std::to_string(n_coef));
        for (int k = 0; k < 64; ++k)
            if (quant[c][k] < 1 || quant[c][k] > 255)
                return fail(err, "jpeg encode: quantiser " + std::to_string(quant[c][k]) + " of component " + std::to_string(c) + " (a baseline table holds 1..255)");
    }
    // quantiser table ids: 0 for Y, 1 for Cb, and for Cr table 1 when it equals Cb's (a frame of the device's encoder: two DQT), else 2
    const int tq[3] = {0, 1, components == 3 && memcmp(quant[2], quant[1], sizeof quant[2]) != 0 ? 2 : 1};
    const int n_tables = components == 1 ? 1 : tq[2] + 1;
    std::string& o = *out;
    o.clear();
    o.reserve(1024 + (size_t)(n_coef / 4));
    put8(o, 0xFF); put8(o, 0xD8);
    const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    o.append((const char*)app0, 18);
    for (int t = 0; t < n_tables; ++t) {
        int c = 0;
        while (tq[c] != t) ++c;
        put8(o, 0xFF); put8(o, 0xDB); put16(o, 67); put8(o, (unsigned)t);
        for (int k = 0; k < 64; ++k) put8(o, quant[c][kZigzag[k]]);
    }
    put8(o, 0xFF); put8(o, 0xC0); put16(o, (unsigned)(8 + 3 * components)); put8(o, 8);
    put16(o, (unsigned)height); put16(o, (unsigned)width); put8(o, (unsigned)components);
    for (int c = 0; c < components; ++c) { put8(o, (unsigned)(c + 1)); put8(o, (unsigned)((hs[c] << 4) | vs[c])); put8(o, (unsigned)tq[c]); }
    put_dht(o, 0x00, kDcLumaBits, kDcVals, 12);
    put_dht(o, 0x10, kAcLumaBits, kAcLumaVals, 162);
    put_dht(o, 0x01, kDcChromaBits, kDcVals, 12);
    put_dht(o, 0x11, kAcChromaBits, kAcChromaVals, 162);
    put8(o, 0xFF); put8(o, 0xDA); put16(o, (unsigned)(6 + 2 * components)); put8(o, (unsigned)components);
    for (int c = 0; c < components; ++c) { put8(o, (unsigned)(c + 1)); put8(o, c ? 0x11 : 0x00); }
    put8(o, 0); put8(o, 63); put8(o, 0);

    Codes dc[2], ac[2];
    make_codes(kDcLumaBits, kDcVals, &dc[0]); make_codes(kDcChromaBits, kDcVals, &dc[1]);
    make_codes(kAcLumaBits, kAcLumaVals, &ac[0]); make_codes(kAcChromaBits, kAcChromaVals, &ac[1]);
    Bits bits{o};
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < mx * my; ++m) {
        const int my_ = m / mx, mx_ = m - my_ * mx;
        for (int c = 0; c < components; ++c) {
            const Codes &d = dc[c ? 1 : 0], &a = ac[c ? 1 : 0];
            for (int by = 0; by < vs[c]; ++by)
                for (int bx = 0; bx < hs[c]; ++bx) {
                    const int16_t* const b = coef + offset[c] + ((uint64_t)(my_ * vs[c] + by) * (uint64_t)blocks_w[c] + (uint64_t)(mx_ * hs[c] + bx)) * 64;
                    if (b[0] < -1023 || b[0] > 1023)          // (so that every DC difference fits the 11 bits of the largest category)
                        return o.clear(), fail(err, "jpeg encode: a DC coefficient of " + std::to_string(b[0]) + " (this encoder carries -1023..1023)");
                    const int diff = (int)b[0] - pred[c];
                    pred[c] = b[0];
                    int s = category(diff);
                    bits.put(d.code[s], d.len[s]);
                    if (s) bits.put((unsigned)(diff < 0 ? diff - 1 : diff), s);
                    int run = 0;
                    for (int k = 1; k < 64; ++k) {
                        const int v = b[kZigzag[k]];
                        if (v == 0) { ++run; continue; }
                        for (; run >= 16; run -= 16) bits.put(a.code[0xF0], a.len[0xF0]);
                        s = category(v);
                        if (s > 10) return o.clear(), fail(err, "jpeg encode: an AC coefficient of " + std::to_string(v) + " (a baseline Huffman stream carries -1023..1023)");
                        const int sym = (run << 4) | s;
                        bits.put(a.code[sym], a.len[sym]);
                        bits.put((unsigned)(v < 0 ? v - 1 : v), s);
                        run = 0;
                    }
                    if (run) bits.put(a.code[0], a.len[0]);
                }
        }
    }
    bits.flush();
    put8(o, 0xFF); put8(o, 0xD9);
    return true;
}

bool encode_coefficients(const Frame& f, std::string* out, std::string* err) {
    return encode_coefficients(f.width, f.height, f.components, f.hs, f.vs, f.quant, f.blocks_w, f.blocks_h, f.offset, f.coef.data(), f.coef.size(), out, err);
}

}  // namespace gsjpeg
