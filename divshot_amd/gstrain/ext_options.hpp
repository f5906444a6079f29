// ext_options.hpp — the extension options GaussianTrainConfig has no room for (INTEGRATION.md "Extension options"): ONE table row per
// option says its CLI flag, its environment variable, its grammar and bounds, its default, and the phrase both messages are built from.
// The CLI (diverseshot_cli.cpp) checks a flag's value against the row and hands it to the plugin in the variable; the plugin reads every
// variable once (read_env) into ExtOptions; the setters of GaussianTrainerScene check their arguments against the same bounds (admits)
// and write the same struct. Host only: no HIP, no trainer state. To add an option: one Id, one row in ext_options.cpp.
#pragma once
#include <functional>
#include <string>

namespace gsopt {
enum Id {
    MESH_MIN_COMPONENT, MESH_NORMALS, MESH_DECIMATE, MESH_BOUNDS, MESH_TRUNC_VOXELS,
    RENDER_FORMAT, RENDER_LAYERS, RENDER_DEPTH_SCALE, RENDER_PNG_LEVEL,
    EXPORT_LOD, LOD_RESOLUTION, MASK_CARVE, SH_CULL_THRESHOLD, REDUCED_HALF, SKY_RESOLUTION, SKY_LR,
    FOCUS_REGION, FOCUS_ROTATION, EXPORT_TRANSFORM, EXPORT_ORIENT, MIP_FILTER3D, N_OPTIONS
};
// What a value looks like, each parser written once (ext_options.cpp):
//   UINT     1..digits decimal digits and nothing else, lo..hi or the one extra value `also` (-1: none)          -> out[0]
//   PERCENT  digits[.digits]: at most 3 before and 2 after the point, 0..100                                      -> out[0] in 1/100 percent
//   BOOL01   0 | 1                                                                                                -> out[0]
//   FLOATS   n numbers (strtof) separated by commas, nothing behind them; finite unless `inf_ok`; then `pred`     -> out[0..n)
//   WORD     one of `words` ("a|b|c")                                                                             -> out[0] = its index
//   AXIS     what gsframe::parse_axis accepts (+x -x +y -y +z -z)                                                 -> out[0..3) = the unit axis
enum Kind { UINT, PERCENT, BOOL01, FLOATS, WORD, AXIS };
enum Pred { ANY, LAST_GT0, LAST_GE0, BOX };            // the last number > 0 / >= 0; n = 6: out[3 + k] > out[k] on every axis
struct Row {
    Id id;
    const char* flag;                                  // without the dashes; nullptr: the option has no flag (environment only)
    const char* var;
    Kind kind;
    int digits; double lo, hi, also;                   // UINT
    int n; Pred pred; bool inf_ok;                     // FLOATS
    const char* words;                                 // WORD
    double def;                                        // out[0] while nothing is given (0 for the rows that are off until given)
    const char* prefix;                                // of the plugin's log line
    const char* takes;                                 // "--<flag> takes <takes>, not '<v>'" / "<prefix>: <VAR>='<v>' is not <takes>: ignored"
    // only where the flag spells the value differently (--renderLayers color,depth <-> DVS_RENDER_LAYERS=3): flag text -> variable text
    // (false: not of the flag's grammar) and the flag's own phrase
    bool (*flag_to_var)(const std::string& flag_text, std::string* var_text);
    const char* flag_takes;
};
const Row& row(Id id);
const Row* find(const char* flag_or_var);              // by flag name (no dashes) or variable name; nullptr: neither
bool parse(const Row& r, const char* text, double out[8]);
bool admits(Id id, double value);                      // a setter's argument against the row's bounds (UINT, BOOL01, a FLOATS row with n = 1)
std::string cli_error(const Row& r, const std::string& flag_text);      // "Command Line Error: --<flag> takes ..., not '...'"
std::string env_error(const Row& r, const char* text);                  // "<prefix>: <VAR>='...' is not ...: ignored"

// The effective values, in the parsers' output form. given[id]: the environment or a setter supplied it (the rows whose default is
// "none": the two boxes, the export frame); text[id]: as the environment spelled it (the export frame's log line quotes it).
struct ExtOptions {
    double v[N_OPTIONS][8];
    bool given[N_OPTIONS];
    std::string text[N_OPTIONS];
    ExtOptions();                                      // every row's default
    int i(Id id) const { return (int)v[id][0]; }
    bool on(Id id) const { return v[id][0] != 0.0; }
    float f(Id id, int k = 0) const { return (float)v[id][k]; }
    void set(Id id, double value) { v[id][0] = value; given[id] = true; }
};
// Every row's variable, once: a value of the row's grammar is taken, any other is reported through `log` (env_error) and leaves the default.
ExtOptions read_env(const std::function<void(const std::string&)>& log);

// ---- rules across options: true = broken; each caller words its own message ----
enum { LAYER_COLOR = 1, LAYER_DEPTH = 2, LAYER_ALPHA = 4 };               // DVS_RENDER_LAYERS is their sum
inline bool layers_need_png(int layers, bool png) { return layers != LAYER_COLOR && !png; }     // JPEG files carry colour alone
inline bool two_export_frames(bool transform, bool orient) { return transform && orient; }       // one export frame at most
bool transformed_needs_frame(const std::string& export_formats, bool frame);                    // `transformed` in the comma list, no frame
bool fused_needs_filter(const std::string& export_formats, bool filter3d);                      // `fused` in the comma list, mipFilter3d off
}  // namespace gsopt
