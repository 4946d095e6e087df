// Stand-alone driver of the compact stage of rtd::FieldMatrix (raytracedicom_amd/csrc/rtd_field_matrix.hpp) and of the host rules of
// the compact dose-influence form (rtd_dij_compact_rules.hpp). tests/test_dij_compact_reference.py builds it (also with
// -fsanitize=address,undefined) and runs it on the CPU.
//
// Part 1 walks the events of rtd_field_dose_influence_compact in the order the engine reports them and checks every query and every
// element count of the buffer table after each: a build, the companion side sized after the scan, the wide rows, a refused build,
// the release of the plain form, and the next computation that takes everything with it.
// Part 2 checks the rules: a column's scale from the bits of its largest |v| against frexp, the refusals (a value that is not
// finite, a maximum below 2^-100, 65 537 spots), the trees that exist, the offsets that fit.
// Prints "ok <checks>"; the first failing check prints its line and exits with 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "rtd_dij_compact_rules.hpp"
#include "rtd_field_matrix.hpp"

namespace {

long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

unsigned bitsOf(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
float floatOf(unsigned u) { float x; std::memcpy(&x, &u, 4); return x; }

constexpr size_t kSpots = 12;

void computeMatrix(rtd::FieldMatrix& m, size_t nnz) {
    const int own[6] = {1, 2, 3, 8, 9, 10};
    m.computeBegins();
    m.stagingSized(1 << 10);
    m.resultSized(nnz, own);
    m.computeFinished(std::vector<int>(kSpots, 0));
}
void prepare(rtd::FieldMatrix& m, size_t rows, size_t chunks) { m.companionSized(rtd::DijBox{1, 2, 3, 8, 8, 8}, rows, chunks); }

void walkMatrix() {
    rtd::FieldMatrix m;
    // nothing yet: no compact form, nothing listed
    CHECK(!m.compact() && !m.plainReleased());
    CHECK(m.compactSpots(kSpots) == 0 && m.compactCscEntries() == 0 && m.compactCscOffsets() == 0 && m.compactCscGroups() == 0);
    CHECK(m.compactRowPtrs() == 0 && m.compactCompanionEntries() == 0);
    computeMatrix(m, 1000);
    prepare(m, 512, 14);
    const unsigned epoch = m.epoch();
    CHECK(m.hasMatrix() && m.prepared() && !m.compact() && !m.isCompactOf(epoch));
    CHECK(m.resultRows() == 1000 && m.resultValues() == 1000 && m.companionEntries() == 1000);
    // a build at 16 lanes, 4 entries: the first class is listed, the companion side after the scan
    m.compactBegins(16, 4, 14 * 32);
    CHECK(!m.compact() && m.compactLanes() == 16 && m.compactPer() == 4 && m.compactRowBits() == 16 && m.compactGroups() == 14 * 32);
    CHECK(m.compactSpots(kSpots) == kSpots && m.compactCscEntries() == 1000 && m.compactCscOffsets() == 1000 && m.compactCscGroups() == 14 * 32);
    CHECK(m.compactRowPtrs() == 513 && m.compactCompanionEntries() == 0);
    m.compactCompanionSized(1200);
    CHECK(m.compactCompanionEntries() == 1200 && m.compactEntries() == 1200 && !m.compact());
    m.compactBuilt();
    CHECK(m.compact() && m.isCompactOf(epoch) && !m.isCompactOf(epoch + 1) && m.isMatrixOf(epoch, 14));
    // a second build, one entry per lane: no row pointers of its own; a group too wide: no offsets
    m.compactBegins(32, 1, 14 * 32);
    CHECK(!m.compact() && m.compactRowPtrs() == 0 && m.compactCompanionEntries() == 0);
    m.compactRowsStayWide();
    CHECK(m.compactRowBits() == 32 && m.compactCscOffsets() == 0 && m.compactCscEntries() == 1000);
    m.compactCompanionSized(1000);
    m.compactBuilt();
    CHECK(m.compact() && m.compactLanes() == 32 && m.compactPer() == 1);
    // released with wide rows: the rows stay listed, the values and the companion's bulk go, the LET values too
    m.letSized(); m.letComputed(7);
    CHECK(m.letValid(true, 7) && m.letEntries() == 1000);
    m.plainReleasedNow(12345);
    CHECK(m.plainReleased() && m.releasedBytes() == 12345 && m.compact() && m.hasMatrix() && m.prepared());
    CHECK(m.resultRows() == 1000 && m.resultValues() == 0 && m.companionEntries() == 0 && m.companionRowPtrs() == 513);
    CHECK(m.companionChunkFirsts(kSpots) == kSpots + 1 && m.companionChunks() == 14);
    CHECK(!m.letValid(true, 7) && m.letEntries() == 0 && m.letDepths() == 0);
    CHECK(!m.isMatrixOf(epoch, 14) && m.isCompactOf(epoch));       // nobody's who reads the plain form; still the compact optimiser's
    // the next computation: the compact form is no longer valid once it begins, and gone with the result's size
    m.computeBegins();
    CHECK(!m.compact() && !m.isCompactOf(epoch) && m.plainReleased());
    const int own[6] = {0, 0, 0, 3, 3, 3};
    m.resultSized(10, own);
    CHECK(!m.plainReleased() && m.compactSpots(kSpots) == 0 && m.compactCscEntries() == 0 && m.compactCompanionEntries() == 0);
    CHECK(m.resultRows() == 10 && m.resultValues() == 10);
    m.computeFinished(std::vector<int>(kSpots, 0));
    CHECK(m.hasMatrix() && !m.prepared() && !m.compact());
    // released with narrow rows: the rows go too
    prepare(m, 27, 12);
    m.compactBegins(16, 2, 12 * 32);
    m.compactCompanionSized(16);
    m.compactBuilt();
    m.plainReleasedNow(99);
    CHECK(m.resultRows() == 0 && m.resultValues() == 0 && m.compactCscOffsets() == 10 && m.compactRowPtrs() == 28);
    // a refused build leaves nothing listed and the matrix as it was
    computeMatrix(m, 5);
    prepare(m, 27, 3);
    m.compactBegins(16, 4, 3 * 32);
    m.compactFailed();
    CHECK(m.hasMatrix() && m.prepared() && !m.compact() && !m.plainReleased());
    CHECK(m.compactSpots(kSpots) == 0 && m.compactCscEntries() == 0 && m.compactCscGroups() == 0 && m.compactRowPtrs() == 0);
    CHECK(m.resultRows() == 5 && m.companionEntries() == 5);
    // an empty matrix: the one-element floors of the table
    computeMatrix(m, 0);
    prepare(m, 0, 0);
    m.compactBegins(16, 4, 0);
    m.compactCompanionSized(0);
    m.compactBuilt();
    CHECK(m.compact() && m.compactCscEntries() == 1 && m.compactCscGroups() == 1 && m.compactRowPtrs() == 1 && m.compactCompanionEntries() == 0);
    // rtd_field_release
    m.released();
    CHECK(!m.hasMatrix() && !m.compact() && !m.plainReleased() && m.compactSpots(kSpots) == 0);
}

void checkRules() {
    using namespace rtd;
    unsigned err = 99;
    // empty or all-zero column: s = 1
    CHECK(dijcScaleBits(0, &err) == bitsOf(1.0f) && err == 0);
    // against frexp over random finite maxima at or above 2^-100
    std::mt19937 rng(5);
    std::uniform_int_distribution<unsigned> any(kDijcTinyBits, kDijcInfBits - 1);
    for (int i = 0; i < 200000; ++i) {
        const unsigned b = i == 0 ? kDijcTinyBits : i == 1 ? kDijcInfBits - 1 : any(rng);
        const float m = floatOf(b);
        int e;
        const float f = std::frexp(m, &e);
        CHECK(f >= 0.5f && f < 1.0f);
        const float s = floatOf(dijcScaleBits(b, &err));
        CHECK(err == 0 && s == std::ldexp(1.0f, e - 15));
        const float inv = floatOf(dijcInvScaleBits(bitsOf(s)));
        CHECK(inv == std::ldexp(1.0f, 15 - e) && std::isnormal(s) && std::isnormal(inv));
        CHECK(m * inv < 32768.0f && m * inv >= 16384.0f);             // the largest code's magnitude lies in [2^14, 2^15)
    }
    // the refusals
    CHECK(dijcScaleBits(bitsOf(std::numeric_limits<float>::infinity()), &err) == bitsOf(1.0f) && err == kDijcErrNotFinite);
    CHECK((dijcScaleBits(bitsOf(std::numeric_limits<float>::quiet_NaN()) & 0x7fffffffu, &err), err == kDijcErrNotFinite));
    CHECK((dijcScaleBits(bitsOf(std::ldexp(1.0f, -101)), &err), err == kDijcErrTiny));
    CHECK((dijcScaleBits(bitsOf(std::nextafter(std::ldexp(1.0f, -100), 0.0f)), &err), err == kDijcErrTiny));
    CHECK((dijcScaleBits(bitsOf(std::numeric_limits<float>::denorm_min()), &err), err == kDijcErrTiny));
    CHECK((dijcScaleBits(bitsOf(std::ldexp(1.0f, -100)), &err), err == 0));
    CHECK(dijcRefusal(0) == nullptr && dijcRefusal(kDijcErrNotFinite) != nullptr && dijcRefusal(kDijcErrTiny) != nullptr);
    CHECK(std::strstr(dijcRefusal(kDijcErrNotFinite | kDijcErrTiny), "not finite") != nullptr);
    CHECK(std::strstr(dijcRefusal(kDijcErrTiny), "2^-100") != nullptr);
    CHECK(dijcSpotsFit(0) && dijcSpotsFit(65536) && !dijcSpotsFit(65537));
    CHECK(dijcOffsetsFit(0) && dijcOffsetsFit(65535) && !dijcOffsetsFit(65536));
    for (int g = 0; g <= 64; ++g)
        for (int e = 0; e <= 8; ++e) CHECK(dijcTreeAllowed(g, e) == ((g == 16 || g == 32) && (e == 1 || e == 2 || e == 4)));
}

}  // namespace

int main() {
    walkMatrix();
    checkRules();
    std::printf("ok %ld\n", checks);
    return 0;
}
