// ext_options.cpp — see ext_options.hpp: the table, the parsers, the two messages.
#include "ext_options.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "export_frame.hpp"

namespace gsopt {
namespace {
// --renderLayers color[,depth][,alpha] -> the sum DVS_RENDER_LAYERS carries: each name once, in this order, color first
bool layers_to_sum(const std::string& lay, std::string* sum) {
    int bits = 0;
    bool ok = !lay.empty();
    for (size_t at = 0; ok && at <= lay.size();) {
        const size_t comma = std::min(lay.find(',', at), lay.size());
        const std::string name = lay.substr(at, comma - at);
        const int bit = name == "color" ? LAYER_COLOR : name == "depth" ? LAYER_DEPTH : name == "alpha" ? LAYER_ALPHA : 0;
        ok = bit > bits;                                                     // (unknown: 0; repeated or out of order: not above what came before)
        bits |= bit;
        at = comma + 1;
    }
    ok = ok && (bits & LAYER_COLOR);
    if (ok) *sum = std::to_string(bits);
    return ok;
}

const char kBox[] = "x0,y0,z0,x1,y1,z1 with x1 > x0, y1 > y0, z1 > z0";
const char kPositive[] = "a finite number > 0";
const char kSwitch[] = "0 or 1";
#define U(digits, lo, hi, also) UINT, digits, lo, hi, also, 0, ANY, false, nullptr
#define F(n, pred, inf_ok) FLOATS, 0, 0, 0, -1, n, pred, inf_ok, nullptr
#define K(kind, words) kind, 0, 0, 0, -1, 0, ANY, false, words
const Row kRows[N_OPTIONS] = {
    // id                 flag                var                        grammar                      default  prefix             takes
    {MESH_MIN_COMPONENT, "meshMinComponent", "DVS_MESH_MIN_COMPONENT", K(PERCENT, nullptr),           0,       "mesh",            "a percentage 0..100 with at most two decimals"},
    {MESH_NORMALS,       "meshNormals",      "DVS_MESH_NORMALS",       K(BOOL01, nullptr),            0,       "mesh",            kSwitch},
    {MESH_DECIMATE,      "meshDecimate",     "DVS_MESH_DECIMATE",      U(2, 2, 16, 0),                0,       "mesh",            "0 (off) or an integer 2..16"},
    {MESH_BOUNDS,        nullptr,            "DVS_MESH_BOUNDS",        F(6, BOX, false),              0,       "mesh",            kBox},
    {MESH_TRUNC_VOXELS,  nullptr,            "DVS_MESH_TRUNC_VOXELS",  F(1, LAST_GT0, false),         4,       "mesh",            kPositive},
    {RENDER_FORMAT,      "renderFormat",     "DVS_RENDER_FORMAT",      K(WORD, "jpg|png"),            0,       "render",          "jpg or png"},
    {RENDER_LAYERS,      "renderLayers",     "DVS_RENDER_LAYERS",      U(1, 1, 7, -1),                1,       "render",          "a sum 1..7 of 1 (color), 2 (depth), 4 (alpha)",
                                                                                                                                   layers_to_sum, "color[,depth][,alpha]"},
    {RENDER_DEPTH_SCALE, "renderDepthScale", "DVS_RENDER_DEPTH_SCALE", F(1, LAST_GT0, false),         1000,    "render",          kPositive},
    {RENDER_PNG_LEVEL,   nullptr,            "DVS_RENDER_PNG_LEVEL",   U(1, 0, 9, -1),                6,       "render",          "a zlib level 0..9"},
    {EXPORT_LOD,         "exportLod",        "DVS_EXPORT_LOD",         U(4, 0, 4, -1),                0,       "lod",             "a number of levels 0 (off) .. 4"},
    {LOD_RESOLUTION,     "lodResolution",    "DVS_LOD_RESOLUTION",     U(4, 32, 1024, -1),            256,     "lod",             "a resolution 32..1024"},
    {MASK_CARVE,         "maskCarve",        "DVS_MASK_CARVE",         U(3, 0, 100, -1),              0,       "mask carve",      "a percentage 0 (off) .. 100"},
    {SH_CULL_THRESHOLD,  "cullSHThreshold",  "DVS_SH_CULL_THRESHOLD",  F(1, LAST_GE0, true),          0.01f,   "reduced",         "a number >= 0"},
    {REDUCED_HALF,       "reducedHalf",      "DVS_REDUCED_HALF",       K(BOOL01, nullptr),            0,       "reduced",         kSwitch},
    {SKY_RESOLUTION,     "skyResolution",    "DVS_SKY_RESOLUTION",     U(5, 0, 99999, -1),            128,     "sky",             "a texture height (16..1024)"},      // (clamped where it is used)
    {SKY_LR,             nullptr,            "DVS_SKY_LR",             F(1, LAST_GT0, false),         0.01f,   "sky",             kPositive},
    {FOCUS_REGION,       "focusRegion",      "DVS_FOCUS_REGION",       F(6, BOX, false),              0,       "focus region",    kBox},
    {FOCUS_ROTATION,     "focusRotation",    "DVS_FOCUS_ROTATION",     F(3, ANY, false),              0,       "focus region",    "rx,ry,rz (radians)"},
    {EXPORT_TRANSFORM,   "exportTransform",  "DVS_EXPORT_TRANSFORM",   F(7, LAST_GT0, false),         0,       "exportTransform", "tx,ty,tz,rx,ry,rz,s with finite numbers and s > 0"},
    {EXPORT_ORIENT,      "exportOrient",     "DVS_EXPORT_ORIENT",      K(AXIS, nullptr),              0,       "exportTransform", "one of +x -x +y -y +z -z"},
    {MIP_FILTER3D,       "mipFilter3d",      "DVS_MIP_FILTER3D",       K(BOOL01, nullptr),            0,       "filter3d",        kSwitch},
};
#undef U
#undef F
#undef K

// the 1..cap digits at `c` (none at all too when may_be_empty) -> their value, `c` left behind them; -1: none, or more than cap
long digits_of(const char*& c, int cap, bool may_be_empty = false) {
    long v = 0;
    int nd = 0;
    for (; *c >= '0' && *c <= '9'; ++c, ++nd) {
        if (nd == cap) return -1;
        v = v * 10 + (*c - '0');
    }
    return nd > 0 || may_be_empty ? v : -1;
}
bool in_bounds(const Row& r, double x) { return (x >= r.lo && x <= r.hi) || (r.also >= 0 && x == r.also); }
bool holds(const Row& r, const double* v) {
    for (int k = 0; k < r.n; ++k) if (!r.inf_ok && !std::isfinite(v[k])) return false;
    switch (r.pred) {
        case LAST_GT0: return v[r.n - 1] > 0;
        case LAST_GE0: return v[r.n - 1] >= 0;
        case BOX: return v[3] > v[0] && v[4] > v[1] && v[5] > v[2];
        default: return true;
    }
}
}  // namespace

const Row& row(Id id) { return kRows[id]; }
const Row* find(const char* name) {
    for (const Row& r : kRows)
        if (name && ((r.flag && !strcmp(name, r.flag)) || !strcmp(name, r.var))) return &r;
    return nullptr;
}

bool parse(const Row& r, const char* text, double out[8]) {
    if (!text) return false;
    for (int k = 0; k < 8; ++k) out[k] = 0.0;
    const char* c = text;
    switch (r.kind) {
        case UINT: {
            const long v = digits_of(c, r.digits);
            out[0] = (double)v;
            return v >= 0 && !*c && in_bounds(r, out[0]);
        }
        case PERCENT: {
            const long whole = digits_of(c, 3);
            long frac = 0;
            if (whole >= 0 && *c == '.') {
                const char* const f0 = ++c;
                frac = digits_of(c, 2, true);
                if (c - f0 == 1) frac *= 10;                                 // (one decimal: tenths)
            }
            out[0] = (double)(whole * 100 + frac);
            return whole >= 0 && frac >= 0 && !*c && out[0] <= 10000;
        }
        case BOOL01:
            out[0] = text[0] == '1';
            return (text[0] == '0' || text[0] == '1') && !text[1];
        case FLOATS:
            for (int k = 0; k < r.n; ++k) {
                char* end = nullptr;
                out[k] = (double)strtof(c, &end);
                if (end == c || *end != (k + 1 < r.n ? ',' : 0)) return false;
                c = end + 1;
            }
            return holds(r, out);
        case WORD: {
            const size_t len = strlen(text);
            int index = 0;
            for (const char* w = r.words; w; ++index) {
                const char* const bar = strchr(w, '|');
                if ((bar ? (size_t)(bar - w) : strlen(w)) == len && !strncmp(w, text, len)) { out[0] = index; return true; }
                w = bar ? bar + 1 : nullptr;
            }
            return false;
        }
        case AXIS: return gsframe::parse_axis(text, out);
    }
    return false;
}

bool admits(Id id, double x) {
    const Row& r = kRows[id];
    return r.kind == FLOATS ? r.n == 1 && holds(r, &x) : r.kind == UINT ? x == std::floor(x) && in_bounds(r, x) : x == 0 || x == 1;
}

std::string cli_error(const Row& r, const std::string& v) {
    return std::string("Command Line Error: --") + r.flag + " takes " + (r.flag_takes ? r.flag_takes : r.takes) + ", not '" + v + "'";
}
std::string env_error(const Row& r, const char* text) { return std::string(r.prefix) + ": " + r.var + "='" + text + "' is not " + r.takes + ": ignored"; }

ExtOptions::ExtOptions() : v{}, given{} {
    for (const Row& r : kRows) v[r.id][0] = r.def;
}
ExtOptions read_env(const std::function<void(const std::string&)>& log) {
    ExtOptions o;
    for (const Row& r : kRows) {
        const char* e = getenv(r.var);
        double out[8];
        if (!e) continue;
        if (!parse(r, e, out)) { log(env_error(r, e)); continue; }
        memcpy(o.v[r.id], out, sizeof out);
        o.given[r.id] = true;
        o.text[r.id] = e;
    }
    return o;
}

namespace {
bool lists(const std::string& formats, const char* token) {                  // `token` is one of the comma list's entries
    for (size_t at = 0; at < formats.size();) {
        const size_t comma = std::min(formats.find(',', at), formats.size());
        if (formats.compare(at, comma - at, token) == 0) return true;
        at = comma + 1;
    }
    return false;
}
}  // namespace
bool transformed_needs_frame(const std::string& formats, bool frame) { return !frame && lists(formats, "transformed"); }
bool fused_needs_filter(const std::string& formats, bool filter3d) { return !filter3d && lists(formats, "fused"); }
}  // namespace gsopt
