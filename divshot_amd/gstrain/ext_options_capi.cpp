// ext_options_capi.cpp — the extension options' table (ext_options.hpp) as one plain-C entry point of libgsplyio.so, the host-only
// library of png_capi.cpp and its neighbours, so that every row's grammar and both messages can be tested from Python without a GPU.
#include <cstring>
#include <exception>
#include "ext_options.hpp"

// `name_or_var`: a flag's name without the dashes (the text is then the flag's: --renderLayers color,depth) or a variable's name.
// -> 0: the text is of the row's grammar, out[8] holds what the parser made of it; 1: it is not, and `err` (NUL-terminated, cut to `cap`)
// holds the message of that spelling — the CLI's for a flag, the plugin's log line for a variable; -1: no such row, or a NULL argument.
extern "C" __attribute__((visibility("default"))) int gstrain_ext_option_check(const char* name_or_var, const char* text, double out[8], char* err, int cap) {
    if (err && cap > 0) err[0] = 0;
    try {
        const gsopt::Row* r = gsopt::find(name_or_var);
        if (!r || !text || !out) return -1;
        const bool as_flag = r->flag && !strcmp(name_or_var, r->flag);
        std::string v = text;
        if ((!as_flag || !r->flag_to_var || r->flag_to_var(v, &v)) && gsopt::parse(*r, v.c_str(), out)) return 0;
        const std::string msg = as_flag ? gsopt::cli_error(*r, text) : gsopt::env_error(*r, text);
        if (err && cap > 0) { strncpy(err, msg.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
        return 1;
    } catch (const std::exception&) {
        return -1;
    }
}
