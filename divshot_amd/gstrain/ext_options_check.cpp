// ext_options_check.cpp — the extension options' table (ext_options.hpp) as a host program for the address and undefined-behaviour
// sanitizers (Makefile: ext_options_check_asan; never loaded into Python, never run on a GPU): every row under its variable's and its
// flag's name against the boundary, sign, trailing-text, digit-count, nan / inf and field-count probes of tests/test_ext_options.py,
// then over-long inputs (4 KiB of digits, 1000 commas, 4 KiB without a comma), both messages for them, the setters' bounds, and
// read_env over an environment in which every variable is malformed. Exit status 0 = every probe came out as written here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ext_options.hpp"

namespace {
int failures = 0;
void expect(bool ok, const char* what, const std::string& detail) {
    if (!ok) { ++failures; fprintf(stderr, "FAILED %s: %.80s\n", what, detail.c_str()); }
}
// `text` against the row found by `name`, the way the CLI (a flag) or read_env (a variable) treats it
bool takes(const char* name, const std::string& text) {
    const gsopt::Row* r = gsopt::find(name);
    if (!r) { expect(false, "no such row", name); return false; }
    std::string v = text;
    double out[8];
    const bool as_flag = r->flag && !strcmp(name, r->flag);
    const bool ok = (!as_flag || !r->flag_to_var || r->flag_to_var(v, &v)) && gsopt::parse(*r, v.c_str(), out);
    const std::string msg = as_flag ? gsopt::cli_error(*r, text) : gsopt::env_error(*r, text.c_str());     // built either way: it reads the text too
    expect(msg.find(text) != std::string::npos, "message quotes the text", name);
    return ok;
}
struct Probe { const char* name; std::vector<const char*> yes, no; };
}  // namespace

int main() {
    const std::vector<const char*> box_yes = {"0,0,0,1,1,1", "-3,-2.5,2,3,2.5,8", "+0,0,0,+1,1,1"},
                                   box_no = {"0,0,0,0,1,1", "0,0,0,1,1", "0,0,0,1,1,1,1", "0,0,0,1,1,1x", "0,0,0,1,1,1,", "0,0,0,inf,inf,inf", "nan,0,0,1,1,1"},
                                   rate_yes = {"0.05", "4", "1e38", "+5"}, rate_no = {"0", "-1", "-0", "x", "0.05x", "nan", "inf", "1e60", "1e-60", "1,2"},
                                   switch_yes = {"0", "1"}, switch_no = {"2", "+1", "-1", "1x", "01", "yes"};
    const std::vector<Probe> probes = {
        {"DVS_MESH_MIN_COMPONENT", {"0", "100", "12.5", "12.", "100.00", "007"}, {"100.01", "101", "+5", "-1", "5x", "1000", "12.345", ".5"}},
        {"DVS_MESH_NORMALS", switch_yes, switch_no}, {"DVS_REDUCED_HALF", switch_yes, switch_no}, {"DVS_MIP_FILTER3D", switch_yes, switch_no},
        {"DVS_MESH_DECIMATE", {"0", "2", "16", "8", "02"}, {"1", "17", "+2", "-2", "2x", "016"}},
        {"DVS_MESH_BOUNDS", box_yes, box_no}, {"DVS_FOCUS_REGION", box_yes, box_no},
        {"DVS_MESH_TRUNC_VOXELS", rate_yes, rate_no}, {"DVS_SKY_LR", rate_yes, rate_no}, {"DVS_RENDER_DEPTH_SCALE", rate_yes, rate_no},
        {"DVS_RENDER_FORMAT", {"jpg", "png"}, {"bmp", "JPG", "jpg ", "jpg|png", "pn"}},
        {"DVS_RENDER_LAYERS", {"1", "7", "3"}, {"0", "8", "+3", "3x", "03", "color"}},
        {"renderLayers", {"color", "color,depth", "color,alpha", "color,depth,alpha"}, {"depth", "color,", ",color", "color,color", "color,alpha,depth", "colour", "3"}},
        {"DVS_RENDER_PNG_LEVEL", {"0", "9", "6"}, {"10", "+6", "-1", "6x", "06"}},
        {"DVS_EXPORT_LOD", {"0", "4", "0004"}, {"5", "+1", "-1", "1x", "00001", "two"}},
        {"DVS_LOD_RESOLUTION", {"32", "1024", "256"}, {"31", "1025", "+64", "64x", "00064"}},
        {"DVS_MASK_CARVE", {"0", "100", "50", "050"}, {"101", "+50", "-1", "50x", "0100", "fifty"}},
        {"DVS_SH_CULL_THRESHOLD", {"0", "0.01", "-0", "inf", "1e60"}, {"-0.01", "0.01x", "nan", "-inf", "1,2"}},
        {"DVS_SKY_RESOLUTION", {"0", "99999", "128", "00128"}, {"+128", "-1", "128x", "100000", "abc"}},
        {"DVS_FOCUS_ROTATION", {"0,0,0", "0.1,-0.2,3"}, {"0,0", "0,0,0,0", "0,0,0x", "nan,0,0", "0,inf,0"}},
        {"DVS_EXPORT_TRANSFORM", {"0,0,0,0,0,0,1", "0.5,-1,2,0.1,0.2,0.3,2.5"}, {"0,0,0,0,0,0", "0,0,0,0,0,0,0", "0,0,0,0,0,0,1,5", "0,0,0,0,0,0,1x", "nan,0,0,0,0,0,1", "0,0,0,0,0,0,inf"}},
        {"DVS_EXPORT_ORIENT", {"+x", "-x", "+y", "-y", "+z", "-z"}, {"up", "y", "+w", "+yy", "++"}},
    };
    for (const Probe& p : probes) {
        const gsopt::Row* r = gsopt::find(p.name);
        const char* flag = r && r->flag && !r->flag_to_var && strcmp(p.name, r->flag) ? r->flag : nullptr;     // the same spelling under the flag's name
        for (const char* v : p.yes) { expect(takes(p.name, v), p.name, v); if (flag) expect(takes(flag, v), flag, v); }
        for (const char* v : p.no) { expect(!takes(p.name, v), p.name, v); if (flag) expect(!takes(flag, v), flag, v); }
    }
    // over-long and unterminated-looking inputs, every row under both names
    std::string ones;
    for (int k = 0; k < 1000; ++k) ones += "1,";
    const std::vector<std::string> longs = {"", std::string(4096, '9'), std::string(1000, ','), ones, ones + "1", std::string(4096, 'x'), "0." + std::string(4096, '0'),
                                            std::string(4096, ' '), "color" + std::string(2000, ','), std::string(4095, '1') + "."};
    for (int id = 0; id < gsopt::N_OPTIONS; ++id) {
        const gsopt::Row& r = gsopt::row((gsopt::Id)id);
        for (const std::string& v : longs) {
            const bool number = !v.empty() && v.find_first_not_of("0123456789.") == std::string::npos;     // huge or long-winded: a row of one number may take it
            if (!number || r.kind != gsopt::FLOATS || r.n != 1) { expect(!takes(r.var, v), r.var, v); if (r.flag) expect(!takes(r.flag, v), r.flag, v); }
            else (void)takes(r.var, v);
        }
    }
    expect(takes("DVS_SH_CULL_THRESHOLD", std::string(4096, '9')) && !takes("DVS_SKY_LR", std::string(4096, '9')), "4 KiB of digits as a number", "inf");
    expect(!gsopt::find("") && !gsopt::find(nullptr) && !gsopt::find("DVS_MESH_RESOLUTION") && !gsopt::find(std::string(4096, 'D').c_str()), "find", "unknown names");
    // the setters' bounds
    using namespace gsopt;
    expect(admits(MESH_DECIMATE, 0) && admits(MESH_DECIMATE, 2) && admits(MESH_DECIMATE, 16) && !admits(MESH_DECIMATE, 1) && !admits(MESH_DECIMATE, 17) && !admits(MESH_DECIMATE, -1), "admits", "decimate");
    expect(admits(EXPORT_LOD, 0) && admits(EXPORT_LOD, 4) && !admits(EXPORT_LOD, 5) && !admits(EXPORT_LOD, -1) && admits(LOD_RESOLUTION, 32) && admits(LOD_RESOLUTION, 1024) &&
           !admits(LOD_RESOLUTION, 31) && !admits(LOD_RESOLUTION, 1025), "admits", "lod");
    expect(admits(MASK_CARVE, 0) && admits(MASK_CARVE, 100) && !admits(MASK_CARVE, 101) && !admits(MASK_CARVE, -1), "admits", "mask carve");
    expect(admits(SH_CULL_THRESHOLD, 0) && admits(SH_CULL_THRESHOLD, INFINITY) && !admits(SH_CULL_THRESHOLD, -0.5) && !admits(SH_CULL_THRESHOLD, NAN), "admits", "threshold");
    // read_env: every variable malformed -> one line each, every value at its default; then every variable well-formed
    const ExtOptions defaults;
    for (int id = 0; id < N_OPTIONS; ++id) setenv(row((Id)id).var, id % 2 ? "x" : "", 1);
    std::vector<std::string> lines;
    ExtOptions o = read_env([&](const std::string& line) { lines.push_back(line); });
    expect(lines.size() == (size_t)N_OPTIONS, "read_env", "one line per malformed variable");
    for (int id = 0; id < N_OPTIONS; ++id) {
        expect(!o.given[id] && !memcmp(o.v[id], defaults.v[id], sizeof o.v[id]) && o.text[id].empty(), "read_env default", row((Id)id).var);
        expect(lines.size() == (size_t)N_OPTIONS && lines[(size_t)id] == env_error(row((Id)id), id % 2 ? "x" : ""), "read_env line", row((Id)id).var);
    }
    expect(o.i(LOD_RESOLUTION) == 256 && o.i(SKY_RESOLUTION) == 128 && o.f(SKY_LR) == 0.01f && o.f(SH_CULL_THRESHOLD) == 0.01f && o.f(MESH_TRUNC_VOXELS) == 4.0f &&
           o.f(RENDER_DEPTH_SCALE) == 1000.0f && o.i(RENDER_PNG_LEVEL) == 6 && o.i(RENDER_LAYERS) == LAYER_COLOR && !o.on(RENDER_FORMAT), "defaults", "values");
    for (const Probe& p : probes) if (!strncmp(p.name, "DVS_", 4)) setenv(p.name, p.yes.back(), 1);
    lines.clear();
    o = read_env([&](const std::string& line) { lines.push_back(line); });
    expect(lines.empty(), "read_env", "no line for well-formed values");
    for (int id = 0; id < N_OPTIONS; ++id) expect(o.given[id] && o.text[id] == getenv(row((Id)id).var), "read_env given", row((Id)id).var);
    expect(o.i(MASK_CARVE) == 50 && o.f(MESH_BOUNDS, 3) == 1.0f && o.f(EXPORT_TRANSFORM, 6) == 2.5f && o.f(EXPORT_ORIENT, 2) == -1.0f && o.on(RENDER_FORMAT), "read_env", "values");
    expect(layers_need_png(3, false) && !layers_need_png(3, true) && !layers_need_png(1, false) && two_export_frames(true, true) && !two_export_frames(true, false) &&
           transformed_needs_frame("splat,transformed", false) && !transformed_needs_frame("splat,transformed", true) && !transformed_needs_frame("splat,transformedx", false) &&
           !transformed_needs_frame("", false) && transformed_needs_frame(std::string(1000, ',') + "transformed", false) && fused_needs_filter("splat,fused", false) &&
           !fused_needs_filter("splat,fused", true) && !fused_needs_filter("fusedx", false) && !fused_needs_filter("", false), "rules", "across options");
    printf("ext_options_check: %s (%d failed)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
