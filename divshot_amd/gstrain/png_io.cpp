// png_io.cpp — see png_io.hpp. The file is read whole (its size is the file system's, not a field's) and parsed through a bounds-checked
// cursor: every chunk length is compared with the bytes that are left before anything is sized by it.
#include "png_io.hpp"
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include "zlib_dl.hpp"

namespace gspng {
namespace {

bool fail(std::string* err, const std::string& msg) { if (err) *err = msg; return false; }

// CRC-32 of the PNG specification (polynomial 0xEDB88320, reflected), table built at compile time
struct CrcTable {
    uint32_t t[256];
    constexpr CrcTable() : t() {
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
    }
};
constexpr CrcTable kCrc;
uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = kCrc.t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

struct Cursor {                          // big-endian fields out of a byte buffer; every read is checked against the bytes left
    const uint8_t* p; size_t left;
    bool u32(uint32_t* v) {
        if (left < 4) return false;
        *v = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
        p += 4; left -= 4;
        return true;
    }
    bool skip(size_t k) { if (k > left) return false; p += k; left -= k; return true; }
};

bool read_file(const std::string& file, std::vector<uint8_t>* out, std::string* err) {
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return fail(err, "cannot open " + file + ": " + strerror(errno));
    out->clear();
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(err, "cannot read " + file);
    return true;
}

bool legal_pair(int type, int depth) {
    switch (type) {
        case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
        case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
        case 2: case 4: case 6: return depth == 8 || depth == 16;
        default: return false;
    }
}
uint16_t be16(const uint8_t* p) { return (uint16_t)((uint16_t)p[0] << 8 | p[1]); }

}  // namespace

int channels_of(int color_type) {
    switch (color_type) { case 0: case 3: return 1; case 4: return 2; case 2: return 3; case 6: return 4; default: return 0; }
}

size_t row_bytes(int width, int bit_depth, int color_type) {
    if (width < 1 || (uint32_t)width > kMaxSide || !legal_pair(color_type, bit_depth)) return 0;
    return ((size_t)width * (size_t)channels_of(color_type) * (size_t)bit_depth + 7) / 8;
}

bool has_alpha(const Frame& f) {
    if (f.color_type == 4 || f.color_type == 6 || f.has_key) return true;
    if (f.color_type == 3) for (int k = 0; k < 256; ++k) if (f.palette[k][3] != 255) return true;
    return false;
}

bool decode_filtered(const std::string& file, Frame* out, std::string* err) {
    std::vector<uint8_t> b;
    if (!read_file(file, &b, err)) return false;
    return decode_filtered(b.data(), b.size(), file, out, err);
}

bool decode_filtered(const uint8_t* data, size_t size, const std::string& name, Frame* out, std::string* err) {
    *out = Frame();
    for (int k = 0; k < 256; ++k) out->palette[k][3] = 255;
    const auto bad = [&](const std::string& what) { return fail(err, name + ": " + what); };
    static const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (!data || size < 8 || memcmp(data, kSig, 8) != 0) return bad("not a PNG file (wrong signature)");
    Cursor c{data + 8, size - 8};
    bool seen_ihdr = false, seen_plte = false, seen_trns = false, seen_iend = false, idat_open = false, idat_closed = false;
    int palette_entries = 0;
    std::vector<uint8_t> idat;           // the IDAT payloads one after the other: never more than the file holds
    while (!seen_iend) {
        uint32_t len = 0, type = 0, crc = 0;
        if (!c.u32(&len)) return bad(seen_ihdr ? "truncated: the file ends without an IEND chunk" : "truncated before the IHDR chunk");
        const uint8_t* const type_at = c.p;
        if (!c.u32(&type)) return bad("truncated inside a chunk header (no IEND chunk)");
        const std::string tname((const char*)type_at, 4);
        if (len > 0x7FFFFFFFu || (size_t)len + 4 > c.left) return bad("truncated: chunk " + tname + " claims " + std::to_string(len) + " bytes, " + std::to_string(c.left) + " are left (no IEND chunk)");
        const uint8_t* const body = c.p;
        c.skip(len);
        c.u32(&crc);
        if (crc32(type_at, (size_t)len + 4) != crc) return bad("chunk " + tname + " fails its CRC check");
        if (!seen_ihdr) {
            if (tname != "IHDR") return bad("the first chunk is " + tname + ", not IHDR");
            if (len != 13) return bad("IHDR of " + std::to_string(len) + " bytes");
            Cursor h{body, 13};
            uint32_t w = 0, hgt = 0;
            h.u32(&w); h.u32(&hgt);
            const int depth = h.p[0], ctype = h.p[1], comp = h.p[2], filt = h.p[3], lace = h.p[4];
            if (w == 0 || hgt == 0 || w > kMaxSide || hgt > kMaxSide) return bad("image size " + std::to_string(w) + "x" + std::to_string(hgt) + " (a side must be 1.." + std::to_string(kMaxSide) + ")");
            if (!legal_pair(ctype, depth)) return bad("illegal colour type / bit depth pair " + std::to_string(ctype) + " / " + std::to_string(depth));
            if (comp != 0) return bad("compression method " + std::to_string(comp) + " (only 0 exists)");
            if (filt != 0) return bad("filter method " + std::to_string(filt) + " (only 0 exists)");
            if (lace == 1) return bad("Adam7 interlaced PNG is not supported: write the file without interlacing");
            if (lace != 0) return bad("interlace method " + std::to_string(lace));
            out->width = (int)w; out->height = (int)hgt; out->bit_depth = depth; out->color_type = ctype;
            seen_ihdr = true;
            continue;
        }
        if (tname == "IHDR") return bad("a second IHDR chunk");
        if (idat_open && tname != "IDAT") { idat_open = false; idat_closed = true; }
        if (tname == "IDAT") {
            if (idat_closed) return bad("IDAT chunks are not consecutive");
            if (out->color_type == 3 && !seen_plte) return bad("palette image (colour type 3) without a PLTE chunk");
            idat_open = true;
            idat.insert(idat.end(), body, body + len);
        } else if (tname == "PLTE") {
            if (seen_plte) return bad("a second PLTE chunk");
            if (idat_closed || seen_trns) return bad("PLTE after IDAT or tRNS");
            if (len % 3 != 0 || len == 0) return bad("PLTE length " + std::to_string(len) + " is not a multiple of 3");
            if (len > 768) return bad("PLTE has " + std::to_string(len / 3) + " entries, more than 256");
            palette_entries = (int)len / 3;
            if (out->color_type == 3)
                for (int k = 0; k < palette_entries; ++k) for (int j = 0; j < 3; ++j) out->palette[k][j] = body[3 * k + j];
            seen_plte = true;
        } else if (tname == "tRNS") {
            if (seen_trns) return bad("a second tRNS chunk");
            if (idat_closed) return bad("tRNS after IDAT");
            seen_trns = true;
            if (out->color_type == 4 || out->color_type == 6) return bad("tRNS in an image that has an alpha channel (colour type " + std::to_string(out->color_type) + ")");
            if (out->color_type == 3) {
                if (!seen_plte) return bad("tRNS before PLTE");
                if ((int)len > palette_entries) return bad("tRNS has " + std::to_string(len) + " entries, longer than the palette's " + std::to_string(palette_entries));
                for (uint32_t k = 0; k < len; ++k) out->palette[k][3] = body[k];
            } else {
                const uint32_t want = out->color_type == 0 ? 2 : 6;
                if (len != want) return bad("tRNS of " + std::to_string(len) + " bytes, wrong length for colour type " + std::to_string(out->color_type) + " (" + std::to_string(want) + ")");
                out->has_key = true;
                for (uint32_t k = 0; k < want / 2; ++k) out->key[k] = be16(body + 2 * k);
            }
        } else if (tname == "IEND") {
            seen_iend = true;
        } else if (!(type_at[0] & 0x20)) {
            return bad("unknown critical chunk " + tname);
        }                                                                    // every other ancillary chunk is skipped
    }
    if (idat.empty() && !idat_open && !idat_closed) return bad("no IDAT chunk");
    const size_t rowbytes = row_bytes(out->width, out->bit_depth, out->color_type);
    const uint64_t expected = (uint64_t)out->height * (1 + (uint64_t)rowbytes);
    if (expected > ((uint64_t)idat.size() + 1) * 1032) return bad("the inflated stream is shorter than the " + std::to_string(expected) + " bytes of the image: " + std::to_string(idat.size()) + " IDAT bytes cannot hold them");
    const gszlib::Api& z = gszlib::api();
    if (!z.err.empty()) return bad("PNG needs zlib: " + z.err);
    out->filtered.resize((size_t)expected + 1);                              // one more, to see a stream that goes on
    gszlib::Stream s;
    memset(&s, 0, sizeof s);
    if (z.inflateInit_(&s, z.zlibVersion(), (int)sizeof s) != gszlib::kOk) return bad("inflate error: inflateInit failed");
    size_t in_at = 0, out_at = 0;
    int rc = gszlib::kOk;
    for (;;) {
        const size_t in_part = std::min<size_t>(idat.size() - in_at, 1u << 30), out_part = std::min<size_t>(out->filtered.size() - out_at, 1u << 30);
        s.next_in = idat.data() + in_at; s.avail_in = (unsigned)in_part;
        s.next_out = out->filtered.data() + out_at; s.avail_out = (unsigned)out_part;
        rc = z.inflate(&s, gszlib::kNoFlush);
        in_at += in_part - s.avail_in; out_at += out_part - s.avail_out;
        if (rc == gszlib::kStreamEnd) break;
        if (rc != gszlib::kOk && rc != gszlib::kBufError) break;
        if (out_at == out->filtered.size()) break;                           // longer than the image
        if (in_at == idat.size()) break;                                     // the input ran out before the stream ended
        if (in_part - s.avail_in == 0 && out_part - s.avail_out == 0) break; // no progress
    }
    const std::string zmsg = s.msg ? s.msg : "";
    z.inflateEnd(&s);
    if (out_at > expected) return bad("the inflated stream is longer than the " + std::to_string(expected) + " bytes of the image");
    if (rc != gszlib::kStreamEnd && rc != gszlib::kOk && rc != gszlib::kBufError) return bad("inflate error " + std::to_string(rc) + (zmsg.empty() ? "" : ": " + zmsg));
    if (rc != gszlib::kStreamEnd) return bad("inflate error: the zlib stream ends before it is complete (" + std::to_string(out_at) + " of " + std::to_string(expected) + " bytes)");
    if (out_at < expected) return bad("the inflated stream is shorter than the image: " + std::to_string(out_at) + " of " + std::to_string(expected) + " bytes");
    out->filtered.resize((size_t)expected);
    for (int y = 0; y < out->height; ++y) {
        const uint8_t ft = out->filtered[(size_t)y * (1 + rowbytes)];
        if (ft > 4) return bad("scanline " + std::to_string(y) + " has the unknown filter type " + std::to_string(ft));
    }
    return true;
}

namespace {
void put_u32(std::string* s, uint32_t v) { const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v}; s->append(b, 4); }
// one chunk appended to *s: length, type, body, CRC over type and body
void put_chunk(std::string* s, const char type[4], const uint8_t* body, size_t n) {
    put_u32(s, (uint32_t)n);
    const size_t at = s->size();
    s->append(type, 4);
    if (n) s->append((const char*)body, n);
    put_u32(s, crc32((const uint8_t*)s->data() + at, n + 4));
}
bool keyword_ok(const std::string& k) {
    if (k.empty() || k.size() > 79 || k.front() == ' ' || k.back() == ' ') return false;
    for (size_t i = 0; i < k.size(); ++i) {
        const uint8_t ch = (uint8_t)k[i];
        if (!((ch >= 32 && ch <= 126) || ch >= 161)) return false;
        if (ch == ' ' && k[i + 1] == ' ') return false;                      // (the last character is no space: i + 1 is inside)
    }
    return true;
}
}  // namespace

bool write_png(int width, int height, int bit_depth, int color_type, const uint8_t* filtered, size_t size, int level, const TextPairs* text,
               std::string* out, std::string* err) {
    if (!out) return fail(err, "write_png: NULL output");
    out->clear();
    if (!filtered) return fail(err, "write_png: NULL filtered stream");
    if (!legal_pair(color_type, bit_depth)) return fail(err, "write_png: illegal colour type / bit depth pair " + std::to_string(color_type) + " / " + std::to_string(bit_depth));
    if (width < 1 || height < 1 || (uint32_t)width > kMaxSide || (uint32_t)height > kMaxSide)
        return fail(err, "write_png: image size " + std::to_string(width) + "x" + std::to_string(height) + " (a side must be 1.." + std::to_string(kMaxSide) + ")");
    const size_t rowbytes = row_bytes(width, bit_depth, color_type);
    const uint64_t expected = (uint64_t)height * (1 + (uint64_t)rowbytes);
    if ((uint64_t)size != expected) return fail(err, "write_png: a filtered stream of " + std::to_string(size) + " bytes, the image takes " + std::to_string(expected));
    for (int y = 0; y < height; ++y)
        if (filtered[(size_t)y * (1 + rowbytes)] > 4) return fail(err, "write_png: scanline " + std::to_string(y) + " has the unknown filter type " + std::to_string(filtered[(size_t)y * (1 + rowbytes)]));
    if (level < 0 || level > 9) return fail(err, "write_png: zlib level " + std::to_string(level) + " (0..9)");
    if (text)
        for (const auto& kv : *text) {
            if (!keyword_ok(kv.first)) return fail(err, "write_png: a tEXt keyword must be 1..79 Latin-1 characters without leading, trailing or doubled spaces");
            if (kv.second.find('\0') != std::string::npos) return fail(err, "write_png: the tEXt text of '" + kv.first + "' holds a NUL");
        }
    const gszlib::Api& z = gszlib::api();
    if (!z.err.empty()) return fail(err, "write_png: PNG needs zlib: " + z.err);

    std::string file;
    static const char kSig[8] = {(char)0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    file.append(kSig, 8);
    const uint32_t w = (uint32_t)width, h = (uint32_t)height;
    const uint8_t ihdr[13] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8),
                              (uint8_t)h, (uint8_t)bit_depth, (uint8_t)color_type, 0, 0, 0};
    put_chunk(&file, "IHDR", ihdr, 13);
    if (text)
        for (const auto& kv : *text) {
            std::string body = kv.first;
            body.push_back('\0');
            body += kv.second;
            put_chunk(&file, "tEXt", (const uint8_t*)body.data(), body.size());
        }
    gszlib::Stream s;
    memset(&s, 0, sizeof s);
    if (z.deflateInit_(&s, level, z.zlibVersion(), (int)sizeof s) != gszlib::kOk) return fail(err, "write_png: deflateInit failed");
    std::vector<uint8_t> part(kMaxIdat);                                     // one IDAT body at a time
    size_t in_at = 0;
    int rc = gszlib::kOk;
    for (;;) {
        const size_t in_part = std::min<size_t>(size - in_at, 1u << 30);
        const bool last = in_at + in_part == size;
        s.next_in = filtered + in_at; s.avail_in = (unsigned)in_part;
        s.next_out = part.data(); s.avail_out = (unsigned)part.size();
        rc = z.deflate(&s, last ? gszlib::kFinish : gszlib::kNoFlush);
        in_at += in_part - s.avail_in;
        const size_t made = part.size() - s.avail_out;
        if (rc != gszlib::kOk && rc != gszlib::kStreamEnd && rc != gszlib::kBufError) break;
        if (made) put_chunk(&file, "IDAT", part.data(), made);
        if (rc == gszlib::kStreamEnd) break;
        if (made == 0 && in_part - s.avail_in == 0) break;                   // no progress
    }
    z.deflateEnd(&s);
    if (rc != gszlib::kStreamEnd) return fail(err, "write_png: deflate error " + std::to_string(rc));
    put_chunk(&file, "IEND", nullptr, 0);
    out->swap(file);
    return true;
}

void unfilter_host(const Frame& f, uint8_t* filtered) {
    const size_t rb = row_bytes(f.width, f.bit_depth, f.color_type), stride = rb + 1;
    const size_t bpp = std::max<size_t>(1, (size_t)channels_of(f.color_type) * (size_t)f.bit_depth / 8);
    for (int y = 0; y < f.height; ++y) {
        uint8_t* const row = filtered + (size_t)y * stride + 1;
        const uint8_t* const up = y ? row - stride : nullptr;
        const int ft = row[-1];
        for (size_t x = 0; x < rb; ++x) {
            const int a = x >= bpp ? row[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int pred = 0;
            if (ft == 1) pred = a;
            else if (ft == 2) pred = b;
            else if (ft == 3) pred = (a + b) >> 1;
            else if (ft == 4) {
                const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
                pred = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
            }
            row[x] = (uint8_t)(row[x] + pred);
        }
    }
}

}  // namespace gspng
