// jpeg_write_check.cpp — a stand-alone host program over the JPEG entropy coder (jpeg_write.hpp) and decoder (jpeg_io.hpp): it builds
// synthetic frames — sizes 1x1, 8x8, 17x1, 37x29, 40x24 at 4:4:4 and 4:2:0; all-zero blocks, a single last coefficient (a run of 62
// zeros: three ZRL), +-1023 everywhere, DC alternating +-1023, pseudo-random sparse coefficients — encodes each, decodes the bytes
// and compares every field; then the frames the encoder must refuse (a coefficient of 1024, block counts that are not the size's, a
// short coefficient array, a quantiser of 0, NULLs). One line per case, "ok ..." or "FAILED ...". The exit status is the number of
// failures; a crash or a sanitizer report is the other thing a caller looks for. Built with -fsanitize=address,undefined by
// `make jpeg_write_check_asan` and run as an ordinary host program.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "jpeg_write.hpp"

namespace {
gsjpeg::Frame make_frame(int W, int H, int s) {
    gsjpeg::Frame f;
    f.width = W; f.height = H; f.components = 3;
    f.hs[0] = f.vs[0] = s;
    const int mx = (W + 8 * s - 1) / (8 * s), my = (H + 8 * s - 1) / (8 * s);
    uint64_t total = 0;
    for (int c = 0; c < 3; ++c) {
        f.blocks_w[c] = mx * f.hs[c]; f.blocks_h[c] = my * f.vs[c]; f.offset[c] = total;
        total += (uint64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
        for (int k = 0; k < 64; ++k) f.quant[c][k] = (uint16_t)(1 + (k * 7 + c * 3) % 255);
    }
    f.coef.assign(total, 0);
    return f;
}
bool same(const gsjpeg::Frame& a, const gsjpeg::Frame& b) {
    if (a.width != b.width || a.height != b.height || a.components != b.components || a.coef != b.coef) return false;
    for (int c = 0; c < 3; ++c)
        if (a.hs[c] != b.hs[c] || a.vs[c] != b.vs[c] || a.blocks_w[c] != b.blocks_w[c] || a.blocks_h[c] != b.blocks_h[c] || a.offset[c] != b.offset[c] ||
            memcmp(a.quant[c], b.quant[c], sizeof a.quant[c]) != 0) return false;
    return true;
}
}  // namespace

int main() {
    int failures = 0;
    const int sizes[5][2] = {{1, 1}, {8, 8}, {17, 1}, {37, 29}, {40, 24}};
    const char* kinds[5] = {"zero", "last", "extreme", "dc_alternating", "random"};
    for (const auto& wh : sizes)
        for (int s = 1; s <= 2; ++s)
            for (int kind = 0; kind < 5; ++kind) {
                gsjpeg::Frame f = make_frame(wh[0], wh[1], s);
                uint64_t rng = 0x9E3779B97F4A7C15ull + (uint64_t)kind * 977 + (uint64_t)wh[0] * 31 + (uint64_t)s;
                for (size_t i = 0; i < f.coef.size(); ++i) {
                    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
                    const size_t k = i & 63, blk = i >> 6;
                    int v = 0;
                    if (kind == 1) v = k == 63 ? -3 : 0;
                    else if (kind == 2) v = (rng & 1) ? 1023 : -1023;
                    else if (kind == 3) v = k == 0 ? ((blk & 1) ? -1023 : 1023) : 0;
                    else if (kind == 4) v = k == 0 ? (int)(rng % 121) - 60 : (rng >> 8) % 4 == 0 ? (int)((rng >> 16) % 2047) - 1023 : 0;
                    f.coef[i] = (int16_t)v;
                }
                std::string bytes;
                std::string err;
                gsjpeg::Frame g;
                const bool ok = gsjpeg::encode_coefficients(f, &bytes, &err) && gsjpeg::decode_coefficients((const uint8_t*)bytes.data(), bytes.size(), "memory", &g, &err) && same(f, g);
                printf("%s %dx%d %dx%d %s: %zu bytes%s%s\n", ok ? "ok" : "FAILED", wh[0], wh[1], s, s, kinds[kind], bytes.size(), err.empty() ? "" : ": ", err.c_str());
                failures += ok ? 0 : 1;
            }
    // refusals: each must come back false with a message
    struct Case { const char* name; gsjpeg::Frame f; };
    std::vector<Case> bad;
    { gsjpeg::Frame f = make_frame(40, 24, 2); f.coef[5] = 1024; bad.push_back({"ac_1024", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 2); f.coef[64] = -1024; bad.push_back({"dc_-1024", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 2); f.blocks_w[1] += 1; bad.push_back({"block_count", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 2); f.coef.resize(f.coef.size() - 1); bad.push_back({"short_array", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 2); f.offset[2] = ~0ull - 7; bad.push_back({"offset_overflow", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 1); f.quant[0][3] = 0; bad.push_back({"quant_0", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 1); f.quant[2][63] = 256; bad.push_back({"quant_256", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 1); f.components = 2; bad.push_back({"two_components", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 1); f.hs[0] = 3; bad.push_back({"sampling_3x1", f}); }
    { gsjpeg::Frame f = make_frame(40, 24, 1); f.width = 0; bad.push_back({"width_0", f}); }
    for (Case& c : bad) {
        std::string bytes;
        std::string err;
        const bool refused = !gsjpeg::encode_coefficients(c.f, &bytes, &err) && !err.empty();
        printf("%s refuses %s: %s\n", refused ? "ok" : "FAILED", c.name, err.c_str());
        failures += refused ? 0 : 1;
    }
    {
        gsjpeg::Frame f = make_frame(8, 8, 1);
        std::string bytes;
        std::string err;
        const bool a = !gsjpeg::encode_coefficients(f, nullptr, &err) && !err.empty();
        const bool b = !gsjpeg::encode_coefficients(8, 8, 3, f.hs, f.vs, f.quant, f.blocks_w, f.blocks_h, f.offset, nullptr, 192, &bytes, &err);
        const bool c = !gsjpeg::encode_coefficients(f, nullptr, nullptr);
        printf("%s refuses NULLs\n", a && b && c ? "ok" : "FAILED");
        failures += a && b && c ? 0 : 1;
    }
    printf("%d failures\n", failures);
    return failures;
}
