// rtd_roi_tables.hpp — margins in mm -> the per-axis cost tables of rtd_roi_margin (include/rtd.h). Plain host
// code without a HIP dependency: rtd_roi_ops_host.hpp uses it, and tests/cpp/test_rtd_roi_tables.cpp compiles it alone.
//   c_a[0] = 0; for d = 1, 2, ... on a side with margin m > 0: q = (double(d) * double(s_a)) / double(m), c = float(q * q); the side
//   holds d while c <= 1.0f and ends at the first d where that fails; a side with m == 0 holds only d = 0.
// Every operation is rounded on its own (the engine and the driver are built without contraction; there is no a * b + c here anyway).
#pragma once

#include <cmath>
#include <limits>

namespace rtd {

constexpr int kRoiTableMax = 127;                    // the farthest d a side may hold

struct RoiTables {
    int len[6];                                      // the farthest d of the side: (-x, +x, -y, +y, -z, +z)
    float cost[3][2 * kRoiTableMax + 1];             // cost[a][kRoiTableMax + d]; +inf outside the table
};

// 0, or the reason of the refusal (a string literal). With `swapSides` the two sides of every axis change places: the tables of the
// expansion of the complement that a contraction is.
inline const char* roiMarginTables(const float spacing_mm[3], const float margin_mm[6], bool swapSides, RoiTables& t) {
    if (!spacing_mm || !margin_mm) return "null pointer";
    for (int a = 0; a < 3; ++a)
        if (!(spacing_mm[a] > 0.0f) || !std::isfinite(spacing_mm[a])) return "a spacing is not positive and finite";
    for (int i = 0; i < 6; ++i)
        if (!(margin_mm[i] >= 0.0f) || !std::isfinite(margin_mm[i])) return "a margin is negative or not finite";
    for (int a = 0; a < 3; ++a) {
        for (int i = 0; i < 2 * kRoiTableMax + 1; ++i) t.cost[a][i] = std::numeric_limits<float>::infinity();
        t.cost[a][kRoiTableMax] = 0.0f;
        const double s = (double)spacing_mm[a];
        for (int side = 0; side < 2; ++side) {       // 0: d < 0, 1: d > 0
            const double m = (double)margin_mm[2 * a + (swapSides ? 1 - side : side)];
            int d = 1;
            if (m > 0.0) {
                for (;; ++d) {
                    const double q = ((double)d * s) / m;
                    const float c = (float)(q * q);
                    if (!(c <= 1.0f)) break;
                    if (d > kRoiTableMax) return "a table side holds more than 127 entries";
                    t.cost[a][side ? kRoiTableMax + d : kRoiTableMax - d] = c;
                }
            }
            t.len[2 * a + side] = d - 1;
        }
    }
    return nullptr;
}

}  // namespace rtd
