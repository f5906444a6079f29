// reduced_check.cpp — gsply::write_reduced_ply as a stand-alone host program (what a sanitizer build runs: `make reduced_check_asan`):
// payloads of several block mixes and both position widths written and read back — the header's counts, the position type and the
// payload byte for byte — and a NULL layout or payload, a layout that its counts do not imply, an empty model, a payload of the wrong
// length and an unwritable path refused with a message. Exit status 0 when everything went as it must.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>
#include "ply_io.hpp"

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++bad; } }

// the layout the header defines (dvs_reduced_layout_for lives in the device library; this program links no HIP)
static dvs_reduced_layout layout_for(const uint32_t counts[4], int half) {
    dvs_reduced_layout L;
    memset(&L, 0, sizeof L);
    uint64_t o = 0;
    for (int d = 0; d < 4; ++d) {
        L.count[d] = counts[d]; L.off[d] = o;
        L.stride[d] = (uint64_t)(half ? 6 : 12) + 3 + 3 * (uint64_t)((d + 1) * (d + 1) - 1) + 8;
        o += L.count[d] * L.stride[d];
    }
    L.table_off = o; L.total = o + 20 * 256 * 4; L.half = half;
    return L;
}

static std::vector<unsigned char> slurp(const std::string& file) {
    std::vector<unsigned char> b;
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return b;
    unsigned char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}

int main() {
    const char* tmp = getenv("TMPDIR");
    const std::string file = std::string(tmp ? tmp : "/tmp") + "/reduced_check_" + std::to_string((long)getpid()) + ".reduced.ply";
    const uint32_t mixes[5][4] = {{1, 0, 0, 0}, {0, 0, 0, 1}, {3, 5, 7, 11}, {100, 0, 37, 0}, {0, 2000, 0, 1}};
    for (const auto& counts : mixes)
        for (int half = 0; half < 2; ++half) {
            const dvs_reduced_layout L = layout_for(counts, half);
            std::vector<uint8_t> payload(L.total);
            uint32_t s = 777u + counts[2] + (uint32_t)half;
            for (uint8_t& v : payload) { s = s * 1664525u + 1013904223u; v = (uint8_t)(s >> 24); }
            std::string err;
            expect(gsply::write_reduced_ply(file, &L, payload.data(), payload.size(), &err), "write");
            const std::vector<unsigned char> raw = slurp(file);
            const std::string text(raw.begin(), raw.end());
            const size_t end = text.find("end_header\n");
            expect(end != std::string::npos, "header ends");
            if (end == std::string::npos) continue;
            const size_t body = end + 11;
            expect(raw.size() - body == payload.size() && memcmp(raw.data() + body, payload.data(), payload.size()) == 0, "payload round trip");
            size_t at = 0;
            for (int d = 0; d < 4; ++d) {
                const std::string want = "element vertex " + std::to_string(counts[d]) + "\nproperty " + (half ? "f16" : "float") + " x\n";
                at = text.find(want, at);
                expect(at != std::string::npos && at < end, "block header");
                if (at == std::string::npos) break;
                at += want.size();
            }
            expect(text.find("element cook_center 256\nproperty float f_dc\n") < end, "table header");
            // refusals: nothing may be written
            remove(file.c_str());
            expect(!gsply::write_reduced_ply(file, nullptr, payload.data(), payload.size(), &err) && !err.empty(), "NULL layout refused");
            expect(!gsply::write_reduced_ply(file, &L, nullptr, payload.size(), &err), "NULL payload refused");
            expect(!gsply::write_reduced_ply(file, &L, payload.data(), payload.size() - 1, &err), "short payload refused");
            expect(!gsply::write_reduced_ply(file, &L, payload.data(), payload.size() + 1, &err), "long payload refused");
            dvs_reduced_layout M = L; M.count[1] += 1;
            expect(!gsply::write_reduced_ply(file, &M, payload.data(), payload.size(), &err), "counts that do not match the offsets refused");
            M = L; M.stride[3] -= 1;
            expect(!gsply::write_reduced_ply(file, &M, payload.data(), payload.size(), &err), "wrong stride refused");
            M = L; M.half = 2;
            expect(!gsply::write_reduced_ply(file, &M, payload.data(), payload.size(), &err), "half = 2 refused");
            M = L; M.table_off += 4;
            expect(!gsply::write_reduced_ply(file, &M, payload.data(), payload.size(), &err), "moved table refused");
            expect(slurp(file).empty(), "a refused call writes nothing");
            expect(!gsply::write_reduced_ply(file + "/no/such/dir.ply", &L, payload.data(), payload.size(), &err) && err.find("cannot open") == 0,
                   "unwritable path refused");
        }
    const uint32_t none[4] = {0, 0, 0, 0};
    const dvs_reduced_layout E = layout_for(none, 0);
    std::vector<uint8_t> table(E.total);
    std::string err;
    expect(!gsply::write_reduced_ply(file, &E, table.data(), table.size(), &err), "empty model refused");
    remove(file.c_str());
    printf("reduced_check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
