// rtd_dij_compact_rules.hpp — the decisions of the compact dose-influence form that are plain arithmetic on a few integers: a
// column's scale from the bits of its largest |v|, what the build refuses, which forward trees exist and when the 16-bit offsets of
// the CSC side fit. Plain C++17 (tests/cpp/test_rtd_dij_compact.cpp compiles it alone); under hipcc the functions are also device
// functions, so the kernel that writes the scales (k_dijc_scales, rtd_dij_compact.hpp) and the host share one text.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define RTD_DIJC_FN __host__ __device__ inline
#else
#define RTD_DIJC_FN inline
#endif

namespace rtd {

constexpr unsigned kDijcErrNotFinite = 1, kDijcErrTiny = 2;           // the build's refusal flags
constexpr unsigned kDijcInfBits = 0x7f800000u;                        // |v| bits at or above: not finite
constexpr unsigned kDijcTinyBits = (127u - 100u) << 23;               // 2^-100: a column maximum below it (and not 0) is refused
constexpr size_t kDijcMaxSpots = 65536;                               // 16-bit columns
constexpr unsigned kDijcMaxOffset = 65535;                            // 16-bit offsets

// The bits of the scale s_j of a column whose largest |v| has the bits maxBits; *err gets the flags the column raises.
// m = 1.f 2^(E - 127) = 0.1f 2^(E - 126): frexp's exponent is e = E - 126, s = 2^(e - 15) has the exponent field E - 14.
// An empty or all-zero column: 1.0f. A refused column: 1.0f too (the build is dropped).
RTD_DIJC_FN unsigned dijcScaleBits(unsigned maxBits, unsigned* err) {
    const unsigned one = 127u << 23;
    *err = 0;
    if (maxBits == 0) return one;
    if (maxBits >= kDijcInfBits) { *err = kDijcErrNotFinite; return one; }
    if (maxBits < kDijcTinyBits) { *err = kDijcErrTiny; return one; }
    return ((maxBits >> 23) - 14u) << 23;
}
// The bits of 1 / s for a scale s = 2^k: the exponent mirrored, no division (both are normal numbers for every scale above).
RTD_DIJC_FN unsigned dijcInvScaleBits(unsigned scaleBits) { return (254u << 23) - scaleBits; }

inline bool dijcSpotsFit(size_t nSpots) { return nSpots <= kDijcMaxSpots; }
inline bool dijcTreeAllowed(int lanes, int per) { return (lanes == 16 || lanes == 32) && (per == 1 || per == 2 || per == 4); }
inline bool dijcOffsetsFit(unsigned largestOffset) { return largestOffset <= kDijcMaxOffset; }
// What the build answers to the flags read from the device (nullptr: nothing to refuse).
inline const char* dijcRefusal(unsigned flags) {
    if (flags & kDijcErrNotFinite) return "a value of the matrix is not finite";
    if (flags & kDijcErrTiny) return "a column's largest value lies below 2^-100";
    return nullptr;
}

}  // namespace rtd
