// jpeg_io.cpp — see jpeg_io.hpp. ITU-T T.81: B.1 - B.2 (markers and segments), C (Huffman table construction), F.2.2 (sequential
// Huffman decoding). The byte buffer is only ever indexed below a length that was compared first.
#include "jpeg_io.hpp"
#include <cerrno>
#include <cstdio>
#include <cstring>

namespace gsjpeg {
namespace {

bool fail(std::string* err, const std::string& msg) { if (err) *err = msg; return false; }
std::string num(uint64_t v) { return std::to_string(v); }
std::string hex2(unsigned v) { char b[8]; snprintf(b, sizeof b, "%02X", v & 255u); return b; }

const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool present = false;
    int32_t mincode[17] = {}, maxcode[17] = {};      // maxcode[l] = -1: no code of length l
    int valptr[17] = {};
    uint8_t symbols[256] = {};
    uint16_t fast[512] = {};                         // by the next 9 bits: (length << 8) | symbol, 0 = longer than 9 bits or no code
    // counts[16], then the symbols; false when the counts exceed the code space
    bool build(const uint8_t* counts, const uint8_t* syms, int total) {
        memcpy(symbols, syms, (size_t)total);
        memset(fast, 0, sizeof fast);
        int32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            valptr[len] = k; mincode[len] = code;
            for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
                if (len <= 9 && code < (1 << len)) {
                    const int first = code << (9 - len);
                    for (int j = 0; j < (1 << (9 - len)); ++j) fast[first + j] = (uint16_t)((len << 8) | symbols[k]);
                }
            }
            if (code > (1 << len)) return false;
            maxcode[len] = counts[len - 1] ? code - 1 : -1;
            code <<= 1;
        }
        present = true;
        return true;
    }
};

// entropy-coded bytes with FF00 unstuffed. Past a marker or the end of the buffer zero bits are handed out and counted in `fake` (they
// are always the youngest bits of `acc`); `bad` turns true when one of them is consumed.
struct Bits {
    const uint8_t* d; size_t pos, end;
    uint64_t acc = 0; int n = 0, fake = 0; bool bad = false;
    Bits(const uint8_t* data, size_t at, size_t size) : d(data), pos(at), end(size) {}
    void fill() {
        while (n <= 56) {
            uint64_t b = 0;
            if (pos < end && d[pos] != 0xFF) b = d[pos++];
            else if (pos + 1 < end && d[pos + 1] == 0) { b = 0xFF; pos += 2; }
            else fake += 8;
            acc = (acc << 8) | b; n += 8;
        }
    }
    uint32_t peek(int k) { if (n < k) fill(); return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1u); }       // 1 <= k <= 16
    void drop(int k) { n -= k; if (n < fake) bad = true; }
    uint32_t get(int k) { if (k == 0) return 0; const uint32_t v = peek(k); drop(k); return v; }
    // -> the symbol, or -1 for a code that is not in the table
    int symbol(const Huff& h) {
        const uint32_t look = peek(16);
        const uint16_t f = h.fast[look >> 7];
        if (f) { drop(f >> 8); return f & 255; }
        for (int len = 1; len <= 16; ++len) {
            const int32_t code = (int32_t)(look >> (16 - len));
            if (h.maxcode[len] >= 0 && code >= h.mincode[len] && code <= h.maxcode[len]) { drop(len); return h.symbols[h.valptr[len] + code - h.mincode[len]]; }
        }
        drop(16);
        return -1;
    }
    // the bits up to the byte boundary are padding; whole bytes left over, or anything but RST<expect> next, is an error
    bool restart(int expect) {
        const int real = n - fake;
        if (real < 0 || real / 8) return false;
        acc = 0; n = 0; fake = 0;
        while (pos + 1 < end && d[pos] == 0xFF && d[pos + 1] == 0xFF) ++pos;
        if (!(pos + 1 < end && d[pos] == 0xFF && d[pos + 1] == 0xD0 + expect)) return false;
        pos += 2;
        return true;
    }
    bool finish() const { const int real = n - fake; return !(real < 0 || real / 8); }
};

int extend(uint32_t v, int t) { return t && v < (1u << (t - 1)) ? (int)v - (1 << t) + 1 : (int)v; }

struct SofComp { uint8_t id, h, v, tq; };

bool read_file(const std::string& file, std::vector<uint8_t>* out, std::string* err) {
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return fail(err, "cannot open " + file + ": " + strerror(errno));
    uint8_t chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) out->insert(out->end(), chunk, chunk + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    return bad ? fail(err, "short read of " + file) : true;
}
}  // namespace

bool decode_coefficients(const std::string& file, Frame* out, std::string* err) {
    std::vector<uint8_t> buf;
    if (!read_file(file, &buf, err)) return false;
    return decode_coefficients(buf.data(), buf.size(), file, out, err);
}

bool decode_coefficients(const uint8_t* d, size_t size, const std::string& name, Frame* out, std::string* err) {
    *out = Frame();
    const std::string hint = "; re-save the image as a baseline JPEG (or convert it to PPM)";
    auto bad = [&](const std::string& msg) { return fail(err, name + ": " + msg); };
    if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return bad("not a JPEG file (no SOI marker)");
    size_t pos = 2;
    struct Quant { bool present = false; uint16_t v[64] = {}; } qt[4];
    std::vector<Huff> dc(4), ac(4);
    bool have_sof = false, have_scan = false;
    int width = 0, height = 0, ncomp = 0;
    SofComp comps[3] = {};
    unsigned restart_interval = 0;
    int adobe_transform = -1;
    for (;;) {
        if (pos >= size) return bad(std::string("truncated: the file ends before ") + (have_scan ? "the EOI marker" : "a scan"));
        if (d[pos] != 0xFF) return bad("a marker is expected at byte " + num(pos));
        while (pos < size && d[pos] == 0xFF) ++pos;
        if (pos >= size) return bad("truncated: the file ends inside a marker");
        const unsigned m = d[pos++];
        if (m == 0xD9) {
            if (!have_scan) return bad("no scan before the EOI marker");
            return true;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0x00) return bad("a marker is expected at byte " + num(pos - 2));
        if (size - pos < 2) return bad("truncated: the file ends inside a segment length");
        const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
        if (L < 2 || L > size - pos)
            return bad("truncated or corrupt: segment length " + num(L) + " of marker FF" + hex2(m) + " overruns the file (" + num(size - pos) + " bytes left)");
        const uint8_t* seg = d + pos + 2;
        const size_t sl = L - 2;
        pos += L;
        if (have_scan) {
            if (m == 0xDA) return bad("multi-scan sequential JPEG: a second scan" + hint);
            continue;
        }
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return bad("a second frame header");
            if (sl < 6) return bad("truncated frame header");
            if (seg[0] != 8) return bad(num(seg[0]) + "-bit JPEG (12-bit is not decoded); only 8-bit" + hint);
            const unsigned h = ((unsigned)seg[1] << 8) | seg[2], w = ((unsigned)seg[3] << 8) | seg[4], n = seg[5];
            if (w == 0 || h == 0 || w > kMaxSide || h > kMaxSide) return bad("image size " + num(w) + "x" + num(h) + " (a side of 0 or above 65500)");
            if (n != 1 && n != 3) return bad(num(n) + " components (4 = CMYK / YCCK); only grayscale and YCbCr" + hint);
            if (sl != 6 + 3 * (size_t)n) return bad("frame header length does not match its component count");
            for (unsigned k = 0; k < n; ++k) {
                comps[k] = SofComp{seg[6 + 3 * k], (uint8_t)(seg[7 + 3 * k] >> 4), (uint8_t)(seg[7 + 3 * k] & 15), seg[8 + 3 * k]};
                if (comps[k].tq > 3 || comps[k].h < 1 || comps[k].h > 4 || comps[k].v < 1 || comps[k].v > 4)
                    return bad("bad sampling factors or quantiser table id in the frame header");
            }
            if (n == 3) {
                const int lh = comps[0].h, lv = comps[0].v;
                const bool luma_ok = (lh == 1 && lv == 1) || (lh == 2 && lv == 1) || (lh == 2 && lv == 2);
                if (!luma_ok || comps[1].h != 1 || comps[1].v != 1 || comps[2].h != 1 || comps[2].v != 1) {
                    std::string s;
                    for (unsigned k = 0; k < 3; ++k) s += (k ? " " : "") + num(comps[k].h) + "x" + num(comps[k].v);
                    return bad("sampling factors " + s + "; only luma 1x1, 2x1, 2x2 with chroma 1x1" + hint);
                }
            } else {
                comps[0].h = comps[0].v = 1;
            }
            width = (int)w; height = (int)h; ncomp = (int)n; have_sof = true;
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            const char* kind = m == 0xC2 ? "progressive" : m == 0xC3 || m == 0xC7 ? "lossless" : m == 0xC5 ? "hierarchical"
                             : m == 0xC6 ? "hierarchical progressive" : "arithmetic-coded";
            return bad(std::string(kind) + " JPEG (SOF" + num(m - 0xC0) + ")" + hint);
        } else if (m == 0xCC) {
            return bad("arithmetic-coded JPEG (DAC)" + hint);
        } else if (m == 0xDB) {
            size_t at = 0;
            while (at < sl) {
                const unsigned pq = seg[at] >> 4, tq = seg[at] & 15;
                const size_t need = pq == 1 ? 128 : 64;
                if (pq > 1 || tq > 3 || need > sl - at - 1) return bad("malformed DQT segment");
                for (int k = 0; k < 64; ++k)
                    qt[tq].v[kZigzag[k]] = pq ? (uint16_t)(((unsigned)seg[at + 1 + 2 * k] << 8) | seg[at + 2 + 2 * k]) : seg[at + 1 + k];
                qt[tq].present = true;
                at += 1 + need;
            }
        } else if (m == 0xC4) {
            size_t at = 0;
            while (at < sl) {
                if (sl - at < 17) return bad("malformed DHT segment");
                const unsigned tc = seg[at] >> 4, th = seg[at] & 15;
                size_t total = 0;
                for (int k = 0; k < 16; ++k) total += seg[at + 1 + k];
                if (tc > 1 || th > 3) return bad("malformed DHT segment");
                if (total > 256 || total > sl - at - 17) return bad("a Huffman table whose counts overrun its segment");
                if (!(tc ? ac : dc)[th].build(seg + at + 1, seg + at + 17, (int)total))
                    return bad("a Huffman table is over-subscribed (its counts overrun the code space)");
                at += 17 + total;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return bad("malformed DRI segment");
            restart_interval = ((unsigned)seg[0] << 8) | seg[1];
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe_transform = seg[11];
        } else if (m == 0xDC) {
            return bad("DNL segment (image height defined after the scan)" + hint);
        } else if (m == 0xDA) {
            if (!have_sof) return bad("a scan before the frame header");
            const size_t n = (size_t)ncomp;
            if (sl < 1 || sl != 4 + 2 * (size_t)seg[0]) return bad("malformed scan header");
            if (seg[0] != n) return bad("multi-scan sequential JPEG: a scan of " + num(seg[0]) + " of the " + num(n) + " components" + hint);
            if (n == 3 && adobe_transform == 0) return bad("RGB JPEG (Adobe transform 0); only grayscale and YCbCr" + hint);
            const Huff* tdc[3] = {}; const Huff* tac[3] = {};
            for (size_t k = 0; k < n; ++k) {
                if (seg[1 + 2 * k] != comps[k].id) return bad("the scan's components are not in frame order");
                const unsigned td = seg[2 + 2 * k] >> 4, ta = seg[2 + 2 * k] & 15;
                if (td > 3 || ta > 3 || !dc[td].present || !ac[ta].present) return bad("missing Huffman table (DC " + num(td) + " / AC " + num(ta) + ")");
                if (!qt[comps[k].tq].present) return bad("missing quantiser table " + num(comps[k].tq));
                tdc[k] = &dc[td]; tac[k] = &ac[ta];
            }
            if (seg[1 + 2 * n] != 0 || seg[2 + 2 * n] != 63 || seg[3 + 2 * n] != 0) return bad("progressive scan parameters in a sequential JPEG");
            Frame& f = *out;
            f.width = width; f.height = height; f.components = ncomp;
            int hmax = 1, vmax = 1;
            for (size_t k = 0; k < n; ++k) { f.hs[k] = comps[k].h; f.vs[k] = comps[k].v; hmax = hmax > f.hs[k] ? hmax : f.hs[k]; vmax = vmax > f.vs[k] ? vmax : f.vs[k]; }
            const int mx = (width + 8 * hmax - 1) / (8 * hmax), my = (height + 8 * vmax - 1) / (8 * vmax);       // <= 8188 each
            uint64_t total = 0;
            for (size_t k = 0; k < n; ++k) {
                f.blocks_w[k] = mx * f.hs[k]; f.blocks_h[k] = my * f.vs[k];
                memcpy(f.quant[k], qt[comps[k].tq].v, sizeof f.quant[k]);
                f.offset[k] = total;
                total += (uint64_t)f.blocks_w[k] * (uint64_t)f.blocks_h[k] * 64;
            }
            if (total > kMaxCoefficients) return bad("image too large: " + num(total) + " coefficients (the cap is 2^29)");
            if (total / 64 > 4 * (uint64_t)(size - pos)) return bad("truncated scan: " + num(size - pos) + " bytes cannot hold " + num(total / 64) + " blocks");
            f.coef.assign((size_t)total, 0);
            Bits bits(d, pos, size);
            // an error met after the data ran out is reported as the truncation it is
            auto in_scan = [&](const char* msg) { return bad(bits.bad ? "truncated scan: the entropy-coded data ends before the last block" : msg); };
            int pred[3] = {0, 0, 0};
            unsigned count = 0;
            const int64_t mcus = (int64_t)mx * my;
            for (int64_t mcu = 0; mcu < mcus; ++mcu) {
                if (restart_interval && mcu && mcu % restart_interval == 0) {
                    if (!bits.restart((int)(count & 7))) return bad("missing or wrong restart marker (RST" + num(count & 7) + " expected after MCU " + num((uint64_t)mcu) + ")");
                    ++count;
                    pred[0] = pred[1] = pred[2] = 0;
                }
                const int my_ = (int)(mcu / mx), mx_ = (int)(mcu % mx);
                for (size_t k = 0; k < n; ++k)
                    for (int by = 0; by < f.vs[k]; ++by)
                        for (int bx = 0; bx < f.hs[k]; ++bx) {
                            int16_t* const blk = f.coef.data() + f.offset[k] +
                                                 ((uint64_t)(my_ * f.vs[k] + by) * (uint64_t)f.blocks_w[k] + (uint64_t)(mx_ * f.hs[k] + bx)) * 64;
                            const int t = bits.symbol(*tdc[k]);
                            if (t < 0) return in_scan("a Huffman code that is not in the table");
                            if (t > 15) return in_scan("bad DC size category");
                            pred[k] += extend(bits.get(t), t);
                            if (pred[k] < -32768 || pred[k] > 32767) return in_scan("DC coefficient out of the 16-bit range");
                            blk[0] = (int16_t)pred[k];
                            int i = 1;
                            while (i < 64) {
                                const int rs = bits.symbol(*tac[k]);
                                if (rs < 0) return in_scan("a Huffman code that is not in the table");
                                const int r = rs >> 4, s = rs & 15;
                                if (s == 0) {
                                    if (r == 15) { i += 16; if (i > 64) return in_scan("a zero run past coefficient 63"); continue; }
                                    if (r == 0) break;
                                    return in_scan("an end-of-band run in a sequential scan");
                                }
                                i += r;
                                if (i > 63) return in_scan("a zero run past coefficient 63");
                                blk[kZigzag[i]] = (int16_t)extend(bits.get(s), s);
                                ++i;
                            }
                            if (bits.bad) return in_scan("");
                        }
            }
            if (!bits.finish()) return bad("bytes after the last block of the scan where a marker belongs");
            pos = bits.pos;
            have_scan = true;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

}  // namespace gsjpeg
