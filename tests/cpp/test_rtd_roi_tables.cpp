// Stand-alone driver of rtd::roiMarginTables (raytracedicom_amd/csrc/rtd_roi_tables.hpp): margins in mm -> the cost tables of
// rtd_roi_margin. tests/test_roi_ops_reference.py builds it (also with -fsanitize=address,undefined), runs it on the CPU and compares
// what it prints with the numpy restatement.
//   test_rtd_roi_tables CASE...      CASE = sx sy sz m-x m+x m-y m+y m-z m+z swap   (floats as strtof reads them, hex floats included)
// Per case one line "ok l-x l+x l-y l+y l-z l+z" and three lines with the costs c[-l-] .. c[+l+] of the axis as hex floats, or one
// line "refused <reason>". Exit code 0 unless the command line is malformed (2).
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "rtd_roi_tables.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 1) % 10 != 0) { std::fprintf(stderr, "usage: %s (sx sy sz m-x m+x m-y m+y m-z m+z swap)...\n", argv[0]); return 2; }
    for (int c = 1; c < argc; c += 10) {
        float v[9];
        for (int i = 0; i < 9; ++i) {
            char* end = nullptr;
            v[i] = std::strtof(argv[c + i], &end);
            if (end == argv[c + i] || *end) { std::fprintf(stderr, "not a number: %s\n", argv[c + i]); return 2; }
        }
        const bool swap = std::atoi(argv[c + 9]) != 0;
        auto t = std::make_unique<rtd::RoiTables>();                   // (on the heap: the sanitizer watches both ends of it)
        if (const char* why = rtd::roiMarginTables(v, v + 3, swap, *t)) { std::printf("refused %s\n", why); continue; }
        std::printf("ok");
        for (int i = 0; i < 6; ++i) std::printf(" %d", t->len[i]);
        std::printf("\n");
        for (int a = 0; a < 3; ++a) {
            for (int d = -t->len[2 * a]; d <= t->len[2 * a + 1]; ++d) std::printf("%s%a", d == -t->len[2 * a] ? "" : " ", (double)t->cost[a][rtd::kRoiTableMax + d]);
            std::printf("\n");
        }
        // everything outside the table must read +inf: the kernels rely on nothing there, but a later reader might
        for (int a = 0; a < 3; ++a)
            for (int d = -rtd::kRoiTableMax; d <= rtd::kRoiTableMax; ++d)
                if ((d < -t->len[2 * a] || d > t->len[2 * a + 1]) && !(t->cost[a][rtd::kRoiTableMax + d] > 3.0e38f)) { std::printf("bad entry outside the table\n"); return 1; }
    }
    return 0;
}
