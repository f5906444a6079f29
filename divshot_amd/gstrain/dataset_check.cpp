// dataset_check.cpp — a stand-alone host program over the dataset reader (dataset_io.hpp): reads every capture directory given on the
// command line, with every image and mask, and prints one line per directory — "ok <cameras> <images> <points> <dropped>" or
// "rejected: <message>". A leading --distorted argument reads with ReadOptions::accept_distorted. Exit status 0 when every directory was read or rejected with a message. Built with
// -fsanitize=address,undefined by tests/test_dataset_io.py and by `make dataset_check_asan`: the reader's rejections run under the
// sanitizers as an ordinary host program.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "dataset_io.hpp"

int main(int argc, char** argv) {
    int bad = 0, first = 1;
    gsdata::ReadOptions opt;
    if (argc > 1 && !strcmp(argv[1], "--distorted")) { opt.accept_distorted = true; first = 2; }
    for (int a = first; a < argc; ++a) {
        gsdata::Dataset d;
        std::string err;
        bool ok = gsdata::read_dataset(argv[a], opt, &d, &err);
        std::vector<uint8_t> px;
        for (size_t i = 0; ok && i < d.images.size(); ++i) ok = gsdata::read_image(d, i, &px, &err) && gsdata::read_mask(d, i, &px, &err);
        if (ok) printf("ok %zu %zu %zu %zu\n", d.cameras.size(), d.images.size(), d.xyz.size() / 3, d.dropped);
        else if (!err.empty()) printf("rejected: %s\n", err.c_str());
        else { printf("FAILED WITHOUT A MESSAGE: %s\n", argv[a]); bad = 1; }
    }
    return bad;
}
