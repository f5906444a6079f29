// dataset_io.cpp — see dataset_io.hpp. The binary files are read whole (their size is the file system's, not a field's) and parsed
// through a bounds-checked cursor: every count is compared with the bytes that are left before anything is sized by it.
#include "dataset_io.hpp"
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <map>

namespace gsdata {
namespace {
namespace fs = std::filesystem;

bool fail(std::string* err, const std::string& msg) { if (err) *err = msg; return false; }

const char* const kModels[] = {"SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
                               "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"};
const int kModelParams[] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12};
constexpr int kNumModels = 11;
constexpr uint64_t kMaxSide = 1u << 16;                    // an image side beyond this is a corrupt field, not a photograph

// the reader that takes pinhole models only (the default) and the one that also takes the three models the loader undistorts
std::string undistort_hint(const std::string& model, bool accept_distorted = false) {
    if (accept_distorted)
        return "camera model " + model + " is not supported: SIMPLE_PINHOLE and PINHOLE are read as they are, SIMPLE_RADIAL, RADIAL and OPENCV "
               "are undistorted by the loader; undistort a capture of any other model first (colmap image_undistorter)";
    return "camera model " + model + " is not supported: only SIMPLE_PINHOLE and PINHOLE are; undistort the capture first "
           "(colmap image_undistorter), as the lineage requires";
}

bool read_file(const std::string& file, std::vector<uint8_t>* out, std::string* err) {
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return fail(err, "cannot open " + file + ": " + strerror(errno));
    std::error_code ec;
    const uintmax_t size = fs::file_size(file, ec);
    if (ec) { fclose(f); return fail(err, "cannot size " + file); }
    out->resize((size_t)size);
    const size_t got = size ? fread(out->data(), 1, (size_t)size, f) : 0;
    fclose(f);
    if (got != (size_t)size) return fail(err, "short read of " + file);
    return true;
}

struct Cursor {                          // little-endian fields out of a byte buffer; ok turns false at the first overrun and stays false
    const uint8_t* p; size_t left; bool ok = true;
    Cursor(const std::vector<uint8_t>& b) : p(b.data()), left(b.size()) {}
    bool take(void* dst, size_t k) {
        if (!ok || k > left) { ok = false; memset(dst, 0, k); return false; }
        memcpy(dst, p, k); p += k; left -= k;
        return true;
    }
    bool skip(uint64_t k) {
        if (!ok || k > left) { ok = false; return false; }
        p += k; left -= (size_t)k;
        return true;
    }
    template <class T> T get() { T v; take(&v, sizeof v); return v; }
};

bool model_accepted(int model, bool accept_distorted) { return model <= 1 || (accept_distorted && model <= 4); }

bool finish_camera(Camera& c, const double* prm, const std::string& where, bool accept_distorted, std::string* err) {
    if (c.model < 0 || c.model >= kNumModels) return fail(err, where + ": unknown camera model id " + std::to_string(c.model));
    if (!model_accepted(c.model, accept_distorted)) return fail(err, where + ": " + undistort_hint(kModels[c.model], accept_distorted));
    if (c.width == 0 || c.height == 0 || c.width > kMaxSide || c.height > kMaxSide)
        return fail(err, where + ": camera " + std::to_string(c.id) + " has size " + std::to_string(c.width) + "x" + std::to_string(c.height));
    if (c.model == 0 || c.model == 2 || c.model == 3) { c.fx = c.fy = prm[0]; c.cx = prm[1]; c.cy = prm[2]; }      // f cx cy [k1 [k2]]
    else { c.fx = prm[0]; c.fy = prm[1]; c.cx = prm[2]; c.cy = prm[3]; }                                           // fx fy cx cy [k1 k2 p1 p2]
    if (c.model == 2 || c.model == 3) { c.dist[0] = prm[3]; if (c.model == 3) c.dist[1] = prm[4]; }
    if (c.model == 4) for (int k = 0; k < 4; ++k) c.dist[k] = prm[4 + k];
    if (!(c.fx > 0) || !(c.fy > 0) || !std::isfinite(c.fx) || !std::isfinite(c.fy) || !std::isfinite(c.cx) || !std::isfinite(c.cy))
        return fail(err, where + ": camera " + std::to_string(c.id) + " has a focal length or principal point that is not a positive / finite number");
    for (double k : c.dist)
        if (!std::isfinite(k)) return fail(err, where + ": camera " + std::to_string(c.id) + " has a distortion coefficient that is not a finite number");
    return true;
}

void add_point(Dataset* d, const double xyz[3], const uint8_t rgb[3]) {
    const float f[3] = {(float)xyz[0], (float)xyz[1], (float)xyz[2]};
    if (!std::isfinite(f[0]) || !std::isfinite(f[1]) || !std::isfinite(f[2])) { ++d->dropped; return; }
    d->xyz.insert(d->xyz.end(), f, f + 3);
    d->rgb.insert(d->rgb.end(), rgb, rgb + 3);
}

// ---- binary ----
bool cameras_bin(const std::string& file, bool accept_distorted, Dataset* d, std::string* err) {
    std::vector<uint8_t> buf;
    if (!read_file(file, &buf, err)) return false;
    Cursor c(buf);
    const uint64_t count = c.get<uint64_t>();
    if (!c.ok) return fail(err, file + ": truncated (no camera count)");
    if (count > c.left / 48) return fail(err, file + ": camera count " + std::to_string(count) + " overruns the file");
    for (uint64_t i = 0; i < count; ++i) {
        Camera cam;
        cam.id = c.get<uint32_t>(); cam.model = c.get<int32_t>(); cam.width = c.get<uint64_t>(); cam.height = c.get<uint64_t>();
        if (!c.ok) return fail(err, file + ": truncated in camera record " + std::to_string(i));
        if (cam.model < 0 || cam.model >= kNumModels) return fail(err, file + ": unknown camera model id " + std::to_string(cam.model));
        double prm[12] = {0};
        c.take(prm, sizeof(double) * (size_t)kModelParams[cam.model]);
        if (!c.ok) return fail(err, file + ": truncated in the parameters of camera record " + std::to_string(i));
        if (!finish_camera(cam, prm, file, accept_distorted, err)) return false;
        d->cameras.push_back(cam);
    }
    if (c.left) return fail(err, file + ": " + std::to_string(c.left) + " bytes after the last camera record");
    return true;
}

bool images_bin(const std::string& file, Dataset* d, std::string* err) {
    std::vector<uint8_t> buf;
    if (!read_file(file, &buf, err)) return false;
    Cursor c(buf);
    const uint64_t count = c.get<uint64_t>();
    if (!c.ok) return fail(err, file + ": truncated (no image count)");
    if (count > c.left / 73) return fail(err, file + ": image count " + std::to_string(count) + " overruns the file");   // 64 + the NUL of a name + 8
    for (uint64_t i = 0; i < count; ++i) {
        Image im;
        im.id = c.get<uint32_t>();
        c.take(im.q, sizeof im.q); c.take(im.t, sizeof im.t);
        im.camera_id = c.get<uint32_t>();
        if (!c.ok) return fail(err, file + ": truncated in image record " + std::to_string(i));
        const void* nul = memchr(c.p, 0, c.left);
        if (!nul) return fail(err, file + ": the name of image record " + std::to_string(i) + " is not terminated");
        im.name.assign((const char*)c.p, (const char*)nul);
        c.skip(im.name.size() + 1);
        const uint64_t n2d = c.get<uint64_t>();
        if (!c.ok) return fail(err, file + ": truncated in image record " + std::to_string(i));
        if (n2d > c.left / 24) return fail(err, file + ": the 2D point count " + std::to_string(n2d) + " of image record " + std::to_string(i) + " overruns the file");
        c.skip(n2d * 24);
        d->images.push_back(im);
    }
    if (c.left) return fail(err, file + ": " + std::to_string(c.left) + " bytes after the last image record");
    return true;
}

bool points_bin(const std::string& file, Dataset* d, std::string* err) {
    std::vector<uint8_t> buf;
    if (!read_file(file, &buf, err)) return false;
    Cursor c(buf);
    const uint64_t count = c.get<uint64_t>();
    if (!c.ok) return fail(err, file + ": truncated (no point count)");
    if (count > c.left / 51) return fail(err, file + ": point count " + std::to_string(count) + " overruns the file");    // 8 + 24 + 3 + 8 + 8
    d->xyz.reserve((size_t)count * 3); d->rgb.reserve((size_t)count * 3);
    for (uint64_t i = 0; i < count; ++i) {
        double xyz[3]; uint8_t rgb[3];
        c.skip(8); c.take(xyz, sizeof xyz); c.take(rgb, 3); c.skip(8);
        const uint64_t track = c.get<uint64_t>();
        if (!c.ok) return fail(err, file + ": truncated in point record " + std::to_string(i));
        if (track > c.left / 8) return fail(err, file + ": the track length " + std::to_string(track) + " of point record " + std::to_string(i) + " overruns the file");
        c.skip(track * 8);
        add_point(d, xyz, rgb);
    }
    if (c.left) return fail(err, file + ": " + std::to_string(c.left) + " bytes after the last point record");
    return true;
}

// ---- text ----
struct Lines {                           // the lines of a text file; `all` keeps empty lines too (images.txt: an image without 2D points)
    std::vector<std::string> v;
    bool load(const std::string& file, std::string* err) {
        std::vector<uint8_t> buf;
        if (!read_file(file, &buf, err)) return false;
        size_t at = 0;
        while (at < buf.size()) {
            const void* nl = memchr(buf.data() + at, '\n', buf.size() - at);
            const size_t end = nl ? (size_t)((const uint8_t*)nl - buf.data()) : buf.size();
            std::string line((const char*)buf.data() + at, end - at);
            if (!line.empty() && line.back() == '\r') line.pop_back();
            v.push_back(line);
            at = end + 1;
        }
        return true;
    }
};
bool blank(const std::string& s) { return s.find_first_not_of(" \t") == std::string::npos; }
bool comment(const std::string& s) { const size_t k = s.find_first_not_of(" \t"); return k != std::string::npos && s[k] == '#'; }
std::vector<std::string> tokens(const std::string& s) {
    std::vector<std::string> t;
    size_t at = 0;
    while ((at = s.find_first_not_of(" \t", at)) != std::string::npos) {
        const size_t end = std::min(s.find_first_of(" \t", at), s.size());
        t.push_back(s.substr(at, end - at));
        at = end;
    }
    return t;
}
bool to_double(const std::string& s, double* v) { char* e = nullptr; errno = 0; *v = strtod(s.c_str(), &e); return !s.empty() && e == s.c_str() + s.size(); }
bool to_u64(const std::string& s, uint64_t* v) {
    if (s.empty() || s[0] == '-' || s[0] == '+') return false;
    char* e = nullptr; errno = 0; *v = strtoull(s.c_str(), &e, 10);
    return e == s.c_str() + s.size() && errno == 0;
}

bool cameras_txt(const std::string& file, bool accept_distorted, Dataset* d, std::string* err) {
    Lines L;
    if (!L.load(file, err)) return false;
    for (size_t ln = 0; ln < L.v.size(); ++ln) {
        if (blank(L.v[ln]) || comment(L.v[ln])) continue;
        const std::vector<std::string> t = tokens(L.v[ln]);
        const std::string where = file + ":" + std::to_string(ln + 1);
        if (t.size() < 4) return fail(err, where + ": a camera line needs CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]");
        Camera cam;
        uint64_t id = 0;
        if (!to_u64(t[0], &id) || id > 0xFFFFFFFFull || !to_u64(t[2], &cam.width) || !to_u64(t[3], &cam.height)) return fail(err, where + ": bad camera id or size");
        cam.id = (uint32_t)id;
        cam.model = -1;
        for (int m = 0; m < kNumModels; ++m) if (t[1] == kModels[m]) cam.model = m;
        if (cam.model < 0) return fail(err, where + ": unknown camera model " + t[1]);
        if (!model_accepted(cam.model, accept_distorted)) return fail(err, where + ": " + undistort_hint(t[1], accept_distorted));
        if (t.size() != 4 + (size_t)kModelParams[cam.model]) return fail(err, where + ": " + t[1] + " takes " + std::to_string(kModelParams[cam.model]) + " parameters");
        double prm[12] = {0};
        for (int k = 0; k < kModelParams[cam.model]; ++k) if (!to_double(t[4 + (size_t)k], &prm[k])) return fail(err, where + ": bad camera parameter");
        if (!finish_camera(cam, prm, where, accept_distorted, err)) return false;
        d->cameras.push_back(cam);
    }
    return true;
}

bool images_txt(const std::string& file, Dataset* d, std::string* err) {
    Lines L;
    if (!L.load(file, err)) return false;
    size_t ln = 0;
    while (ln < L.v.size()) {
        if (blank(L.v[ln]) || comment(L.v[ln])) { ++ln; continue; }
        const std::vector<std::string> t = tokens(L.v[ln]);
        const std::string where = file + ":" + std::to_string(ln + 1);
        if (t.size() < 10) return fail(err, where + ": an image line needs IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME");
        Image im;
        uint64_t id = 0, cam = 0;
        if (!to_u64(t[0], &id) || id > 0xFFFFFFFFull || !to_u64(t[8], &cam) || cam > 0xFFFFFFFFull) return fail(err, where + ": bad image or camera id");
        im.id = (uint32_t)id; im.camera_id = (uint32_t)cam;
        for (int k = 0; k < 4; ++k) if (!to_double(t[1 + (size_t)k], &im.q[k])) return fail(err, where + ": bad qvec");
        for (int k = 0; k < 3; ++k) if (!to_double(t[5 + (size_t)k], &im.t[k])) return fail(err, where + ": bad tvec");
        im.name = t[9];
        for (size_t k = 10; k < t.size(); ++k) im.name += " " + t[k];       // (a name with blanks)
        d->images.push_back(im);
        ln += 2;                                                            // the line of 2D points (possibly empty) belongs to the image
    }
    return true;
}

bool points_txt(const std::string& file, Dataset* d, std::string* err) {
    Lines L;
    if (!L.load(file, err)) return false;
    for (size_t ln = 0; ln < L.v.size(); ++ln) {
        if (blank(L.v[ln]) || comment(L.v[ln])) continue;
        const std::vector<std::string> t = tokens(L.v[ln]);
        const std::string where = file + ":" + std::to_string(ln + 1);
        if (t.size() < 8) return fail(err, where + ": a point line needs POINT3D_ID X Y Z R G B ERROR TRACK[]");
        double xyz[3]; uint8_t rgb[3];
        for (int k = 0; k < 3; ++k) if (!to_double(t[1 + (size_t)k], &xyz[k])) return fail(err, where + ": bad coordinate");
        for (int k = 0; k < 3; ++k) {
            uint64_t c = 0;
            if (!to_u64(t[4 + (size_t)k], &c) || c > 255) return fail(err, where + ": bad colour");
            rgb[k] = (uint8_t)c;
        }
        add_point(d, xyz, rgb);
    }
    return true;
}

bool path_exists(const fs::path& p) { std::error_code ec; return fs::exists(p, ec); }

// header of a binary PNM: magic, width, height, maxval, each followed by white space; '#' starts a comment up to the end of the line
bool pnm_number(const std::vector<uint8_t>& b, size_t* at, uint64_t* v) {
    for (;;) {
        while (*at < b.size() && (b[*at] == ' ' || b[*at] == '\t' || b[*at] == '\n' || b[*at] == '\r')) ++*at;
        if (*at < b.size() && b[*at] == '#') { while (*at < b.size() && b[*at] != '\n') ++*at; continue; }
        break;
    }
    size_t digits = 0;
    *v = 0;
    while (*at < b.size() && b[*at] >= '0' && b[*at] <= '9' && digits < 10) { *v = *v * 10 + (uint64_t)(b[*at] - '0'); ++*at; ++digits; }
    return digits > 0 && digits < 10;
}
}  // namespace

const char* model_name(int model) { return model >= 0 && model < kNumModels ? kModels[model] : "?"; }

bool read_pnm(const std::string& file, int channels, int* width, int* height, std::vector<uint8_t>* pixels, std::string* err) {
    std::vector<uint8_t> b;
    if (!read_file(file, &b, err)) return false;
    const char want = channels == 3 ? '6' : '5';
    if (b.size() < 2 || b[0] != 'P' || b[1] != (uint8_t)want)
        return fail(err, file + ": not a binary " + (channels == 3 ? "PPM (P6)" : "PGM (P5)") + " file; JPEG and PNG are not decoded here, convert the images to PPM");
    size_t at = 2;
    uint64_t w = 0, h = 0, maxval = 0;
    if (!pnm_number(b, &at, &w) || !pnm_number(b, &at, &h) || !pnm_number(b, &at, &maxval)) return fail(err, file + ": truncated or malformed PNM header");
    if (maxval != 255) return fail(err, file + ": maxval " + std::to_string(maxval) + " (only 255 is supported)");
    if (at >= b.size() || !(b[at] == ' ' || b[at] == '\t' || b[at] == '\n' || b[at] == '\r')) return fail(err, file + ": malformed PNM header");
    ++at;
    if (w == 0 || h == 0 || w > kMaxSide || h > kMaxSide) return fail(err, file + ": image size " + std::to_string(w) + "x" + std::to_string(h));
    const uint64_t need = w * h * (uint64_t)channels;
    if (need > b.size() - at) return fail(err, file + ": truncated: " + std::to_string(b.size() - at) + " pixel bytes of " + std::to_string(need));
    pixels->assign(b.begin() + (ptrdiff_t)at, b.begin() + (ptrdiff_t)(at + need));
    *width = (int)w; *height = (int)h;
    return true;
}

bool read_dataset(const std::string& path, Dataset* d, std::string* err) { return read_dataset(path, ReadOptions(), d, err); }

bool read_dataset(const std::string& path, const ReadOptions& opt, Dataset* d, std::string* err) {
    *d = Dataset();
    d->root = path;
    std::error_code ec;
    if (!fs::is_directory(path, ec)) return fail(err, path + " is not a directory");
    for (const char* sub : {"sparse/0", "sparse"}) {
        const fs::path dir = fs::path(path) / sub;
        for (int bin = 1; bin >= 0 && d->sparse_dir.empty(); --bin) {
            const char* ext = bin ? ".bin" : ".txt";
            if (path_exists(dir / (std::string("cameras") + ext)) && path_exists(dir / (std::string("images") + ext)) && path_exists(dir / (std::string("points3D") + ext))) {
                d->sparse_dir = dir.string(); d->binary = bin != 0;
            }
        }
        if (!d->sparse_dir.empty()) break;
    }
    if (d->sparse_dir.empty())
        return fail(err, "no COLMAP sparse model under " + path + ": cameras, images and points3D (.bin or .txt) are looked for in sparse/0/, then sparse/");
    if (!fs::is_directory(fs::path(path) / "images", ec)) return fail(err, "no images/ directory under " + path);
    const std::string base = d->sparse_dir + "/", ext = d->binary ? ".bin" : ".txt";
    if (!(d->binary ? cameras_bin(base + "cameras" + ext, opt.accept_distorted, d, err) : cameras_txt(base + "cameras" + ext, opt.accept_distorted, d, err))) return false;
    if (!(d->binary ? images_bin(base + "images" + ext, d, err) : images_txt(base + "images" + ext, d, err))) return false;
    if (!(d->binary ? points_bin(base + "points3D" + ext, d, err) : points_txt(base + "points3D" + ext, d, err))) return false;
    if (d->cameras.empty()) return fail(err, d->sparse_dir + ": no cameras");
    if (d->images.empty()) return fail(err, d->sparse_dir + ": no images");
    std::map<uint32_t, size_t> by_id;
    for (size_t k = 0; k < d->cameras.size(); ++k) by_id[d->cameras[k].id] = k;
    for (Image& im : d->images) {
        const auto it = by_id.find(im.camera_id);
        if (it == by_id.end()) return fail(err, d->sparse_dir + ": image " + im.name + " refers to the unknown camera id " + std::to_string(im.camera_id));
        im.camera = it->second;
        const double qq = im.q[0] * im.q[0] + im.q[1] * im.q[1] + im.q[2] * im.q[2] + im.q[3] * im.q[3];
        if (!(qq > 0) || !std::isfinite(qq) || !std::isfinite(im.t[0]) || !std::isfinite(im.t[1]) || !std::isfinite(im.t[2]))
            return fail(err, d->sparse_dir + ": image " + im.name + " has a pose that is not finite");
        if (im.name.empty() || im.name.find("..") != std::string::npos) return fail(err, d->sparse_dir + ": bad image name '" + im.name + "'");
    }
    std::stable_sort(d->images.begin(), d->images.end(), [](const Image& a, const Image& b) { return a.name < b.name; });
    return true;
}

void rotation_of(const Image& im, float R[9]) {
    const double n = std::sqrt(im.q[0] * im.q[0] + im.q[1] * im.q[1] + im.q[2] * im.q[2] + im.q[3] * im.q[3]);
    const double w = im.q[0] / n, x = im.q[1] / n, y = im.q[2] / n, z = im.q[3] / n;
    const double r[9] = {1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z,     2 * z * x + 2 * w * y,
                         2 * x * y + 2 * w * z,     1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                         2 * z * x - 2 * w * y,     2 * y * z + 2 * w * x,     1 - 2 * x * x - 2 * y * y};
    for (int k = 0; k < 9; ++k) R[k] = (float)r[k];
}

bool resolve_image_kind(const Dataset& d, size_t index, std::string* file, ImageKind* kind, std::string* err) {
    if (index >= d.images.size()) return fail(err, "image index out of range");
    const fs::path named = fs::path(d.root) / "images" / d.images[index].name;
    *kind = ImageKind::PPM;
    if (path_exists(named)) {
        std::string ext = named.extension().string();
        for (char& c : ext) c = (char)tolower((unsigned char)c);
        if (ext == ".jpg" || ext == ".jpeg") *kind = ImageKind::JPEG;
        else if (ext == ".png") *kind = ImageKind::PNG;
        *file = named.string();
        return true;
    }
    for (const char* ext : {".ppm", ".jpg", ".jpeg", ".JPG", ".JPEG", ".png", ".PNG"}) {
        fs::path alt = named;
        alt.replace_extension(ext);
        if (path_exists(alt)) { *kind = ext[1] == 'p' && ext[2] == 'p' ? ImageKind::PPM : (ext[1] == 'j' || ext[1] == 'J') ? ImageKind::JPEG : ImageKind::PNG; *file = alt.string(); return true; }
    }
    fs::path ppm = named;
    ppm.replace_extension(".ppm");
    const std::string stem = named.stem().string();
    return fail(err, "image " + named.string() + " does not exist (nor " + ppm.filename().string() + "); JPEG and PNG are not decoded here, convert the images to PPM" +
                         " — nor is there a JPEG for the loader to decode under " + stem + ".jpg, " + stem + ".jpeg, " + stem + ".JPG or " + stem + ".JPEG" +
                         ", nor a PNG under " + stem + ".png or " + stem + ".PNG");
}

// the resolver from before PNG was read: a PNG file is reported as it always was, as a file that is not a JPEG
bool resolve_image(const Dataset& d, size_t index, std::string* file, bool* is_jpeg, std::string* err) {
    ImageKind kind = ImageKind::PPM;
    *is_jpeg = false;
    if (!resolve_image_kind(d, index, file, &kind, err)) return false;
    *is_jpeg = kind == ImageKind::JPEG;
    return true;
}

bool resolve_mask(const Dataset& d, size_t index, std::string* file, MaskKind* kind, std::string* err) {
    if (index >= d.images.size()) return fail(err, "image index out of range");
    const std::string& name = d.images[index].name;
    fs::path pgm = fs::path(d.root) / "masks" / name, png = pgm;
    pgm.replace_extension(".pgm");
    png.replace_extension(".png");
    const fs::path full = fs::path(d.root) / "masks" / (name + ".png");
    file->clear();
    *kind = MaskKind::NONE;
    if (path_exists(pgm)) { *kind = MaskKind::PGM; *file = pgm.string(); }
    else if (path_exists(png)) { *kind = MaskKind::PNG; *file = png.string(); }
    else if (path_exists(full)) { *kind = MaskKind::PNG; *file = full.string(); }
    return true;
}

bool read_image(const Dataset& d, size_t index, std::vector<uint8_t>* rgb, std::string* err) {
    if (index >= d.images.size()) return fail(err, "image index out of range");
    const Image& im = d.images[index];
    const Camera& cam = d.cameras[im.camera];
    fs::path file = fs::path(d.root) / "images" / im.name;
    if (!path_exists(file)) {
        fs::path alt = file;
        alt.replace_extension(".ppm");
        if (!path_exists(alt))
            return fail(err, "image " + file.string() + " does not exist (nor " + alt.filename().string() + "); JPEG and PNG are not decoded here, convert the images to PPM");
        file = alt;
    }
    int w = 0, h = 0;
    if (!read_pnm(file.string(), 3, &w, &h, rgb, err)) return false;
    if ((uint64_t)w != cam.width || (uint64_t)h != cam.height)
        return fail(err, file.string() + " is " + std::to_string(w) + "x" + std::to_string(h) + " but its camera " + std::to_string(cam.id) + " is " +
                             std::to_string(cam.width) + "x" + std::to_string(cam.height));
    return true;
}

bool read_mask(const Dataset& d, size_t index, std::vector<uint8_t>* mask, std::string* err) {
    if (index >= d.images.size()) return fail(err, "image index out of range");
    const Image& im = d.images[index];
    const Camera& cam = d.cameras[im.camera];
    fs::path file = fs::path(d.root) / "masks" / im.name;
    file.replace_extension(".pgm");
    if (!path_exists(file)) { mask->assign((size_t)(cam.width * cam.height), 1); return true; }
    int w = 0, h = 0;
    if (!read_pnm(file.string(), 1, &w, &h, mask, err)) return false;
    if ((uint64_t)w != cam.width || (uint64_t)h != cam.height)
        return fail(err, file.string() + " is " + std::to_string(w) + "x" + std::to_string(h) + " but its camera is " + std::to_string(cam.width) + "x" +
                             std::to_string(cam.height));
    for (uint8_t& m : *mask) m = m > 127 ? 1 : 0;
    return true;
}

}  // namespace gsdata
