// png_check.cpp — the PNG host half (png_io.hpp) as a host program, for the build under the address and undefined-behaviour sanitizers
// (make png_check_asan): never loaded into Python, never run on a GPU. Without arguments it builds small PNGs in memory (stored
// deflate blocks, so no compressor is needed), decodes them, goes through the refusal list of png_io.hpp and times the plain host
// unfiltering loop on one 1920x1080 RGB8 stream (one thread: the figure DESIGN.md sets beside the device's); with file arguments it
// decodes those and times their unfiltering.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "png_io.hpp"

namespace {
typedef std::vector<uint8_t> Bytes;

uint32_t crc_of(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}
void be32(Bytes* b, uint32_t v) { for (int k = 3; k >= 0; --k) b->push_back((uint8_t)(v >> (8 * k))); }
void chunk(Bytes* b, const char* type, const Bytes& body, bool break_crc = false) {
    be32(b, (uint32_t)body.size());
    const size_t at = b->size();
    b->insert(b->end(), type, type + 4);
    b->insert(b->end(), body.begin(), body.end());
    be32(b, crc_of(b->data() + at, body.size() + 4) ^ (break_crc ? 1u : 0u));
}
Bytes zlib_stored(const Bytes& raw) {
    Bytes z = {0x78, 0x01};
    size_t at = 0;
    do {
        const size_t n = std::min<size_t>(raw.size() - at, 65535);
        z.push_back(at + n == raw.size() ? 1 : 0);
        z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8)); z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
        z.insert(z.end(), raw.begin() + (ptrdiff_t)at, raw.begin() + (ptrdiff_t)(at + n));
        at += n;
    } while (at < raw.size());
    uint32_t a = 1, b = 0;
    for (uint8_t v : raw) { a = (a + v) % 65521; b = (b + a) % 65521; }
    be32(&z, b << 16 | a);
    return z;
}
Bytes ihdr(uint32_t w, uint32_t h, int depth, int type, int comp = 0, int filt = 0, int lace = 0) {
    Bytes b;
    be32(&b, w); be32(&b, h);
    b.push_back((uint8_t)depth); b.push_back((uint8_t)type); b.push_back((uint8_t)comp); b.push_back((uint8_t)filt); b.push_back((uint8_t)lace);
    return b;
}
const Bytes kSig = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

Bytes stream_for(int w, int h, int depth, int type, uint32_t seed) {
    const size_t rb = gspng::row_bytes(w, depth, type);
    Bytes raw((size_t)h * (rb + 1));
    for (size_t i = 0; i < raw.size(); ++i) { seed = seed * 1664525u + 1013904223u; raw[i] = (uint8_t)(seed >> 24); }
    for (int y = 0; y < h; ++y) raw[(size_t)y * (rb + 1)] = (uint8_t)((y + seed) % 5);
    return raw;
}
// a whole file: IHDR, optional PLTE / tRNS, IDAT split into pieces of `split` bytes (0 = one chunk), IEND
Bytes file_for(int w, int h, int depth, int type, const Bytes& raw, const Bytes& plte = Bytes(), const Bytes& trns = Bytes(), size_t split = 0) {
    Bytes f = kSig;
    chunk(&f, "IHDR", ihdr((uint32_t)w, (uint32_t)h, depth, type));
    chunk(&f, "gAMA", Bytes{0, 0, 0xB1, 0x8F});
    if (!plte.empty()) chunk(&f, "PLTE", plte);
    if (!trns.empty()) chunk(&f, "tRNS", trns);
    const Bytes z = zlib_stored(raw);
    if (split == 0) chunk(&f, "IDAT", z);
    else for (size_t at = 0; at < z.size(); at += split) chunk(&f, "IDAT", Bytes(z.begin() + (ptrdiff_t)at, z.begin() + (ptrdiff_t)std::min(z.size(), at + split)));
    chunk(&f, "IEND", Bytes());
    return f;
}

int failures = 0;
void expect_ok(const char* what, const Bytes& file, const Bytes& raw) {
    gspng::Frame f;
    std::string err;
    if (!gspng::decode_filtered(file.data(), file.size(), what, &f, &err)) { printf("FAIL %s: refused: %s\n", what, err.c_str()); ++failures; return; }
    if (f.filtered != raw) { printf("FAIL %s: the filtered bytes differ\n", what); ++failures; return; }
    printf("ok   %s: %dx%d depth %d type %d, %zu bytes\n", what, f.width, f.height, f.bit_depth, f.color_type, f.filtered.size());
}
void expect_refused(const char* what, const Bytes& file, const char* word) {
    gspng::Frame f;
    std::string err;
    if (gspng::decode_filtered(file.data(), file.size(), "memory", &f, &err)) { printf("FAIL %s: accepted\n", what); ++failures; return; }
    if (err.find(word) == std::string::npos) { printf("FAIL %s: the message lacks '%s': %s\n", what, word, err.c_str()); ++failures; return; }
    printf("ok   %s: %s\n", what, err.c_str());
}
double time_unfilter(gspng::Frame& f) {
    const auto t0 = std::chrono::steady_clock::now();
    gspng::unfilter_host(f, f.filtered.data());
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int k = 1; k < argc; ++k) {
            gspng::Frame f;
            std::string err;
            if (!gspng::decode_filtered(argv[k], &f, &err)) { printf("refused: %s\n", err.c_str()); ++failures; continue; }
            const double ms = time_unfilter(f);
            printf("%s: %dx%d depth %d type %d%s, %zu filtered bytes, host unfiltering %.3f ms (one thread)\n", argv[k], f.width, f.height, f.bit_depth,
                   f.color_type, gspng::has_alpha(f) ? ", alpha" : "", f.filtered.size(), ms);
        }
        return failures ? 1 : 0;
    }
    static const int pairs[15][2] = {{0, 1}, {0, 2}, {0, 4}, {0, 8}, {0, 16}, {2, 8}, {2, 16}, {3, 1}, {3, 2}, {3, 4}, {3, 8}, {4, 8}, {4, 16}, {6, 8}, {6, 16}};
    const Bytes plte3 = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    for (const auto& p : pairs)
        for (size_t split : {(size_t)0, (size_t)1, (size_t)7}) {
            const Bytes raw = stream_for(37, 29, p[1], p[0], 5u + (uint32_t)p[0] * 16u + (uint32_t)p[1]);
            char what[64];
            snprintf(what, sizeof what, "type %d depth %d split %zu", p[0], p[1], split);
            expect_ok(what, file_for(37, 29, p[1], p[0], raw, p[0] == 3 ? plte3 : Bytes(), p[0] == 3 ? Bytes{9, 8} : Bytes(), split), raw);
        }
    const Bytes raw = stream_for(5, 3, 8, 2, 1);
    const Bytes z = zlib_stored(raw);
    const auto build = [&](const Bytes& head, const std::vector<std::pair<const char*, Bytes>>& chunks) {
        Bytes f = kSig;
        chunk(&f, "IHDR", head);
        for (const auto& c : chunks) chunk(&f, c.first, c.second);
        return f;
    };
    const Bytes good_head = ihdr(5, 3, 8, 2);
    { Bytes f = file_for(5, 3, 8, 2, raw); f[0] = 0x88; expect_refused("signature", f, "signature"); }
    { Bytes f = kSig; chunk(&f, "IHDR", good_head, true); chunk(&f, "IDAT", z); chunk(&f, "IEND", Bytes()); expect_refused("crc", f, "CRC"); }
    { Bytes f = kSig; chunk(&f, "gAMA", Bytes{0, 0, 0, 1}); chunk(&f, "IHDR", good_head); expect_refused("first chunk", f, "not IHDR"); }
    expect_refused("type/depth", build(ihdr(5, 3, 4, 2), {{"IDAT", z}, {"IEND", {}}}), "illegal");
    expect_refused("zero side", build(ihdr(0, 3, 8, 2), {{"IDAT", z}, {"IEND", {}}}), "image size");
    expect_refused("large side", build(ihdr(65501, 3, 8, 2), {{"IDAT", z}, {"IEND", {}}}), "image size");
    expect_refused("interlace", build(ihdr(5, 3, 8, 2, 0, 0, 1), {{"IDAT", z}, {"IEND", {}}}), "Adam7");
    expect_refused("compression", build(ihdr(5, 3, 8, 2, 1), {{"IDAT", z}, {"IEND", {}}}), "compression method");
    expect_refused("filter method", build(ihdr(5, 3, 8, 2, 0, 1), {{"IDAT", z}, {"IEND", {}}}), "filter method");
    expect_refused("critical chunk", build(good_head, {{"ABCD", {1}}, {"IDAT", z}, {"IEND", {}}}), "critical");
    expect_refused("no PLTE", build(ihdr(5, 3, 8, 3), {{"IDAT", z}, {"IEND", {}}}), "without a PLTE");
    expect_refused("PLTE % 3", build(ihdr(5, 3, 8, 3), {{"PLTE", {1, 2, 3, 4}}, {"IDAT", z}, {"IEND", {}}}), "multiple of 3");
    expect_refused("PLTE > 256", build(ihdr(5, 3, 8, 3), {{"PLTE", Bytes(771, 0)}, {"IDAT", z}, {"IEND", {}}}), "more than 256");
    expect_refused("tRNS > PLTE", build(ihdr(5, 3, 8, 3), {{"PLTE", plte3}, {"tRNS", {1, 2, 3, 4}}, {"IDAT", z}, {"IEND", {}}}), "longer than the palette");
    expect_refused("tRNS length", build(good_head, {{"tRNS", {0, 1}}, {"IDAT", z}, {"IEND", {}}}), "wrong length");
    expect_refused("tRNS on type 6", build(ihdr(5, 3, 8, 6), {{"tRNS", {0, 1}}, {"IDAT", z}, {"IEND", {}}}), "alpha channel");
    expect_refused("IDAT gap", build(good_head, {{"IDAT", Bytes(z.begin(), z.begin() + 5)}, {"tEXt", {'a', 0, 'b'}}, {"IDAT", Bytes(z.begin() + 5, z.end())}, {"IEND", {}}}), "not consecutive");
    expect_refused("no IDAT", build(good_head, {{"IEND", {}}}), "no IDAT");
    expect_refused("no IEND", build(good_head, {{"IDAT", z}}), "IEND");
    { Bytes bad = z; bad[2] = 7; expect_refused("inflate", build(good_head, {{"IDAT", bad}, {"IEND", {}}}), "inflate error"); }
    expect_refused("short", build(good_head, {{"IDAT", zlib_stored(Bytes(raw.begin(), raw.end() - 1))}, {"IEND", {}}}), "shorter");
    { Bytes more = raw; more.push_back(0); expect_refused("long", build(good_head, {{"IDAT", zlib_stored(more)}, {"IEND", {}}}), "longer"); }
    { Bytes five = raw; five[16] = 5; expect_refused("filter byte", build(good_head, {{"IDAT", zlib_stored(five)}, {"IEND", {}}}), "filter type"); }
    for (size_t cut = 0; cut < 60; ++cut) {                                  // every truncation of a good file is a refusal, not a crash
        const Bytes f = file_for(5, 3, 8, 2, raw);
        gspng::Frame out;
        std::string err;
        if (cut < f.size() && gspng::decode_filtered(f.data(), f.size() - 1 - cut, "cut", &out, &err)) { printf("FAIL truncation by %zu accepted\n", cut + 1); ++failures; }
    }
    {
        gspng::Frame f;
        f.width = 1920; f.height = 1080; f.bit_depth = 8; f.color_type = 2;
        f.filtered = stream_for(1920, 1080, 8, 2, 77);
        printf("host unfiltering of one 1920x1080 RGB8 stream (filters cycling 0..4, one thread): %.3f ms\n", time_unfilter(f));
    }
    printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
