// jpeg_check.cpp — a stand-alone host program over the JPEG coefficient decoder (jpeg_io.hpp): decodes every file given on the command
// line and prints one line per file — "ok <width> <height> <components>" or "rejected: <message>". The exit status is always 0: a
// crash or a sanitizer report is what a caller looks for. Built with -fsanitize=address,undefined by `make jpeg_check_asan` and by
// tests/test_jpeg_format.py: the decoder's rejections run under the sanitizers as an ordinary host program.
#include <cstdio>
#include <string>
#include "jpeg_io.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        gsjpeg::Frame f;
        std::string err;
        if (gsjpeg::decode_coefficients(argv[a], &f, &err)) printf("ok %d %d %d\n", f.width, f.height, f.components);
        else printf("rejected: %s\n", err.empty() ? "(no message)" : err.c_str());
    }
    return 0;
}
