// check.hpp -- TEST INFRASTRUCTURE: what the drivers of the sanitizer build (tests/asan/*_check.cpp) share.  A driver defines
// CHECK_PROGRAM, the name its messages begin with, before it includes this file, and ends with its "<name>: N failures" line.
#pragma once
#include <cstdio>
#include <string>

#include "lightdock_hip.h"

#ifndef CHECK_PROGRAM
#error "define CHECK_PROGRAM before including check.hpp"
#endif

static int failures = 0;
#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) {                                                                                             \
            std::fprintf(stderr, CHECK_PROGRAM ": %s failed at line %d (%s)\n", #cond, __LINE__, ld_last_error()); \
            failures++;                                                                                            \
        }                                                                                                          \
    } while (0)

inline void put(const std::string &path, const std::string &text) {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (f) {
        std::fwrite(text.data(), 1, text.size(), f);
        std::fclose(f);
    }
}

// An ATOM record of exactly 54 columns, then `rest` (the columns after the coordinates, a line end).
inline std::string atom_line(int serial, const char *name, const char *res, char chain, int res_seq, double x, double y, double z,
                             const char *rest = "") {
    char buf[128];
    std::snprintf(buf, sizeof buf, "ATOM  %5d %-4s %3s %c%4d    %8.3f%8.3f%8.3f%s", serial, name, res, chain, res_seq, x, y, z, rest);
    return buf;
}
