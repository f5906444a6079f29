// sky_check.cpp — the sky texture file's reader and writer as a stand-alone host program (what a sanitizer build runs: `make sky_check_asan`):
// textures of several sizes round-tripped bit for bit, and truncated, over-long, wrong-magic and wrong-shape files refused. With file
// arguments it reads those instead and prints their size or the refusal. Exit status 0 when everything went as it must.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>
#include "sky_io.hpp"

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++bad; } }

static void rewrite(const std::string& file, const std::vector<unsigned char>& bytes) {
    FILE* f = fopen(file.c_str(), "wb");
    if (f) { fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) {
            uint32_t w = 0, h = 0; std::vector<float> t; std::string err;
            if (gssky::read_sky(argv[i], &w, &h, &t, &err)) printf("%s: %u x %u\n", argv[i], w, h);
            else { printf("%s: refused: %s\n", argv[i], err.c_str()); ++bad; }
        }
        return bad ? 1 : 0;
    }
    const char* tmp = getenv("TMPDIR");
    const std::string file = std::string(tmp ? tmp : "/tmp") + "/sky_check_" + std::to_string((long)getpid()) + ".sky";
    for (uint32_t h : {2u, 16u, 128u}) {
        const uint32_t w = 2 * h;
        std::vector<float> tex((size_t)w * h * 3);
        uint32_t s = 12345u + h;
        for (float& v : tex) { s = s * 1664525u + 1013904223u; uint32_t bits = (s >> 9) | 0x3F000000u; memcpy(&v, &bits, 4); }
        std::string err;
        expect(gssky::write_sky(file, w, h, tex.data(), &err), "write");
        uint32_t rw = 0, rh = 0; std::vector<float> back;
        expect(gssky::read_sky(file, &rw, &rh, &back, &err) && rw == w && rh == h && back.size() == tex.size() &&
               memcmp(back.data(), tex.data(), tex.size() * 4) == 0, "round trip");
        std::vector<unsigned char> bytes(16 + tex.size() * 4);
        FILE* f = fopen(file.c_str(), "rb");
        expect(f && fread(bytes.data(), 1, bytes.size(), f) == bytes.size(), "reread");
        if (f) fclose(f);
        std::vector<unsigned char> cut(bytes.begin(), bytes.end() - 5);
        rewrite(file, cut); expect(!gssky::read_sky(file, &rw, &rh, &back, &err), "truncated file refused");
        cut.assign(bytes.begin(), bytes.begin() + 9);
        rewrite(file, cut); expect(!gssky::read_sky(file, &rw, &rh, &back, &err), "truncated header refused");
        std::vector<unsigned char> more(bytes); more.push_back(0);
        rewrite(file, more); expect(!gssky::read_sky(file, &rw, &rh, &back, &err), "over-long file refused");
        std::vector<unsigned char> magic(bytes); magic[6] = '2';
        rewrite(file, magic); expect(!gssky::read_sky(file, &rw, &rh, &back, &err), "wrong magic refused");
        std::vector<unsigned char> shape(bytes); shape[8] = (unsigned char)(w - 1);
        rewrite(file, shape); expect(!gssky::read_sky(file, &rw, &rh, &back, &err), "width != 2 * height refused");
        expect(!gssky::write_sky(file, w + 1, h, tex.data(), &err) && !gssky::write_sky(file, 2, 1, tex.data(), &err), "bad shapes not written");
    }
    remove(file.c_str());
    printf("sky_check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
