// png_write_check.cpp — the PNG writer (png_io.hpp write_png) as a host program, built with -fsanitize=address,undefined (Makefile target
// png_write_check_asan): filtered streams of the three kinds dvs_png_encode_views writes (RGB8, GRAY8, GRAY16) at several sizes and zlib
// levels go through write_png and come back through decode_filtered byte for byte; a stream above 1 MiB at level 0 must split into
// several IDAT chunks; every refusal of the writer is gone through and must leave a message and an empty output. Exit status 0 = all
// held. Never loaded into Python, never run on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "png_io.hpp"

namespace {
int failures = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what.c_str()); ++failures; }
}

// any bytes with filter bytes 0..4 make a valid filtered stream
std::vector<uint8_t> stream_of(int w, int h, int depth, int type, uint32_t seed) {
    const size_t rb = gspng::row_bytes(w, depth, type);
    std::vector<uint8_t> s((size_t)h * (1 + rb));
    uint32_t x = seed * 2654435761u + 1u;
    for (size_t i = 0; i < s.size(); ++i) {
        x = x * 1664525u + 1013904223u;
        // smooth enough to deflate, rough enough to need more than one code
        s[i] = i % (1 + rb) == 0 ? (uint8_t)((x >> 24) % 5) : (uint8_t)((x >> 28) + (i & 31));
    }
    return s;
}

int count_chunks(const std::string& file, const char* type, size_t* largest) {
    int n = 0;
    size_t at = 8;
    if (largest) *largest = 0;
    while (at + 12 <= file.size()) {
        const uint8_t* p = (const uint8_t*)file.data() + at;
        const size_t len = (size_t)p[0] << 24 | (size_t)p[1] << 16 | (size_t)p[2] << 8 | (size_t)p[3];
        if (memcmp(p + 4, type, 4) == 0) { ++n; if (largest && len > *largest) *largest = len; }
        at += 12 + len;
    }
    return n;
}

void round_trip(int w, int h, int depth, int type, int level, const gspng::TextPairs* text) {
    const std::string what = std::to_string(w) + "x" + std::to_string(h) + " type " + std::to_string(type) + " depth " + std::to_string(depth) + " level " + std::to_string(level);
    const std::vector<uint8_t> s = stream_of(w, h, depth, type, (uint32_t)(w * 31 + h * 7 + depth + level));
    std::string file, err;
    expect(gspng::write_png(w, h, depth, type, s.data(), s.size(), level, text, &file, &err), what + ": write_png refused: " + err);
    gspng::Frame f;
    expect(gspng::decode_filtered((const uint8_t*)file.data(), file.size(), "memory", &f, &err), what + ": decode_filtered refused: " + err);
    expect(f.width == w && f.height == h && f.bit_depth == depth && f.color_type == type, what + ": header differs");
    expect(f.filtered == s, what + ": the stream differs");
    size_t largest = 0;
    expect(count_chunks(file, "IDAT", &largest) >= 1 && largest <= gspng::kMaxIdat, what + ": IDAT chunks");
    expect(count_chunks(file, "tEXt", nullptr) == (text ? (int)text->size() : 0), what + ": tEXt chunks");
    expect(count_chunks(file, "IHDR", nullptr) == 1 && count_chunks(file, "IEND", nullptr) == 1, what + ": IHDR / IEND");
}

void refused(const char* what, int w, int h, int depth, int type, const uint8_t* s, size_t size, int level, const gspng::TextPairs* text, bool null_out = false) {
    std::string file = "left over", err;
    const bool ok = gspng::write_png(w, h, depth, type, s, size, level, text, null_out ? nullptr : &file, &err);
    expect(!ok, std::string(what) + ": accepted");
    expect(!err.empty(), std::string(what) + ": no message");
    expect(null_out || file.empty(), std::string(what) + ": output not empty");
}
}  // namespace

int main() {
    const int kinds[3][2] = {{2, 8}, {0, 8}, {0, 16}};                       // (colour type, depth) of RGB8, GRAY8, GRAY16
    const int sizes[][2] = {{1, 1}, {3, 2}, {17, 5}, {64, 48}, {257, 9}, {1030, 3}, {40, 1}};
    const gspng::TextPairs text = {{"depth_scale", "1000"}, {"Software", "gstrain"}};
    for (const auto& k : kinds)
        for (const auto& sz : sizes)
            for (int level : {0, 1, 6, 9}) round_trip(sz[0], sz[1], k[1], k[0], level, level == 6 ? &text : nullptr);
    {   // above 1 MiB at level 0: several IDAT chunks, none above the limit
        const int w = 700, h = 520;
        const std::vector<uint8_t> s = stream_of(w, h, 8, 2, 99);
        std::string file, err;
        expect(s.size() > gspng::kMaxIdat, "the large stream is large");
        expect(gspng::write_png(w, h, 8, 2, s.data(), s.size(), 0, nullptr, &file, &err), "large: " + err);
        size_t largest = 0;
        expect(count_chunks(file, "IDAT", &largest) >= 2 && largest <= gspng::kMaxIdat, "large: not split");
        gspng::Frame f;
        expect(gspng::decode_filtered((const uint8_t*)file.data(), file.size(), "memory", &f, &err) && f.filtered == s, "large: round trip " + err);
    }
    // the refusals
    const std::vector<uint8_t> s = stream_of(5, 4, 8, 2, 1);
    refused("NULL stream", 5, 4, 8, 2, nullptr, s.size(), 6, nullptr);
    refused("NULL output", 5, 4, 8, 2, s.data(), s.size(), 6, nullptr, true);
    refused("type 2 at depth 4", 5, 4, 4, 2, s.data(), s.size(), 6, nullptr);
    refused("type 5", 5, 4, 8, 5, s.data(), s.size(), 6, nullptr);
    refused("width 0", 0, 4, 8, 2, s.data(), s.size(), 6, nullptr);
    refused("height 65501", 5, 65501, 8, 2, s.data(), s.size(), 6, nullptr);
    refused("a byte short", 5, 4, 8, 2, s.data(), s.size() - 1, 6, nullptr);
    refused("a byte long", 5, 3, 8, 2, s.data(), 3 * 16 + 1, 6, nullptr);
    { std::vector<uint8_t> b = s; b[2 * 16] = 5; refused("filter byte 5", 5, 4, 8, 2, b.data(), b.size(), 6, nullptr); }
    refused("level -1", 5, 4, 8, 2, s.data(), s.size(), -1, nullptr);
    refused("level 10", 5, 4, 8, 2, s.data(), s.size(), 10, nullptr);
    for (const std::string& key : {std::string(), std::string(80, 'k'), std::string(" lead"), std::string("trail "), std::string("two  spaces"), std::string("tab\there"),
                                   std::string("nul\0in", 6), std::string("\x7f"), std::string("\xa0")}) {
        const gspng::TextPairs bad = {{key, "v"}};
        refused(("keyword '" + key + "'").c_str(), 5, 4, 8, 2, s.data(), s.size(), 6, &bad);
    }
    { const gspng::TextPairs bad = {{"key", std::string("a\0b", 3)}}; refused("NUL in the text", 5, 4, 8, 2, s.data(), s.size(), 6, &bad); }
    { const gspng::TextPairs ok = {{std::string(79, 'k'), ""}, {"caf\xe9 one", "v"}}; round_trip(5, 4, 8, 2, 6, &ok); }
    if (failures) { fprintf(stderr, "png_write_check: %d check(s) failed\n", failures); return 1; }
    printf("png_write_check: all round trips and refusals held\n");
    return 0;
}
