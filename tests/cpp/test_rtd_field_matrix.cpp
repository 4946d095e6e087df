// Stand-alone driver of rtd::FieldMatrix (raytracedicom_amd/csrc/rtd_field_matrix.hpp): the life of a field's dose-influence matrix.
// tests/test_field_matrix_reference.py builds it (also with -fsanitize=address,undefined) and runs it on the CPU.
//
// `Old` below is a literal transcription of the loose members of rtd_field_impl and of every statement that read or assigned them at
// commit a1d1d67, before the header existed (f-> and h-> dropped; a device pointer is a flag "allocated"; hipMalloc is a counter that
// says which allocation of the event fails; everything between the assignments is a draw that says whether the call fails there).
// The comments name the file and line each statement came from. `New` is the same entry points as the engine writes them now, on the
// header and on the buffer table with its three classes. The driver walks both in lock step over random sequences of events (fixed
// seed) and compares every observable after every event: each query, each count and each pointer of the buffer table, what a fetch
// of "dij_batch" reads, and the verdict of a plan set that noted the matrix.
//
// Events: a table set or removed on the handle; rtd_field_dose_influence failing in the staging's allocation, in the first forward,
// in the batches (the staging grown or not), in the result's allocation, behind it, or finishing (nnz drawn, 0 included);
// rtd_field_dose_influence_prepare or a first product (refused, done already, failing early, in its allocation, late, or succeeding);
// rtd_field_let_influence (refused, preparing on demand, failing in its allocation or behind its launches, succeeding); a plan set created on the field;
// rtd_field_release. A released field object stays with the handle until its workspace is taken over and answers calls meanwhile:
// the walk goes on with the same object on both sides.
//
//   test_rtd_field_matrix [walks] [events per walk]      (defaults 4000, 64)
// First the transcription alone: the walk must make every observable take both of its values and reach every sequence named in
// Coverage (else exit code 3, nothing is compared). Then the lock step (first difference: exit code 1, with the walk, the event and
// the observable). Prints one line "ok ..." with the counts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "rtd_field_matrix.hpp"

namespace {

constexpr size_t kSpots = 12;     // nSpot of the walked field
constexpr int kBufs = 15;         // save, rowsB, valsB | colPtr, rows, vals | rowPtr, cCols, cVals, chunkFirst, chunkCol, partial | letVals, letCVals, letDepth

// hipMalloc: the failAt-th allocation of an event fails (-1: none does).
struct Mallocs { int failAt = -1, n = 0; bool operator()() { return n++ != failAt; } };

struct Handle { bool dLetTable = false; unsigned letEpoch = 0; };

enum Outcome { kFailStaging, kFailForward, kFailBatches, kFailResult, kFailGather, kFinish };
struct ComputeDraw { Outcome outcome; size_t nnz; size_t staged; int ownBox[6]; std::vector<int> batch; };
struct PrepareDraw { bool failEarly, failLate; rtd::DijBox box; size_t rows, chunks; };
enum Status { kOk = 0, kFailed = 1, kRefused = 2 };

// ---- the members and statements as they were written by hand ---------------------------------------------------------------------------
struct Old {
    enum : unsigned { kDij = 16, kDijOut = 32 };                       // rtd_engine_impl.hpp:97
    size_t dijCap = 0, dijNnz = 0;                                    // rtd_engine_impl.hpp:186
    bool dijDone = false;                                             // :187
    unsigned dijEpoch = 0;                                            // :188
    std::vector<int> dijBatchOf;                                      // :189
    bool dijPrepared = false;                                         // :194
    int dijOwnBox[6] = {0, 0, 0, -1, -1, -1};                         // :195
    rtd::DijBox dijBox{};                                             // :196
    size_t dijRowsN = 0, dijChunks = 0;                               // :197
    bool letAlloc = false, letDone = false;                           // :201-202
    unsigned letEpoch = 0;                                            // :203
    bool p[kBufs] = {};                                               // the device pointers: allocated or null

    template <typename V> void forEachBuffer(V&& visit) {             // rtd_engine_impl.hpp:251-267
        const size_t nSpot = kSpots;
        visit(0, nSpot, kDij);                                        // :252 (dDijSave, for the class's other buffers of fixed size)
        visit(1, dijCap, kDij); visit(2, dijCap, kDij);               // :257
        visit(3, nSpot + 1, kDijOut); visit(4, std::max<size_t>(dijNnz, 1), kDijOut);   // :258
        visit(5, std::max<size_t>(dijNnz, 1), kDijOut);               // :259
        const size_t ap = dijPrepared ? 1 : 0;                        // :260
        visit(6, ap * (dijRowsN + 1), kDijOut); visit(7, ap * std::max<size_t>(dijNnz, 1), kDijOut);   // :261
        visit(8, ap * std::max<size_t>(dijNnz, 1), kDijOut); visit(9, ap * (nSpot + 1), kDijOut);      // :262
        visit(10, ap * std::max<size_t>(dijChunks, 1), kDijOut);      // :263
        visit(11, ap * std::max<size_t>(dijChunks, 1), kDijOut);      // :264
        const size_t lt = letAlloc ? 1 : 0;                           // :265
        visit(12, lt * std::max<size_t>(dijNnz, 1), kDijOut); visit(13, lt * std::max<size_t>(dijNnz, 1), kDijOut);   // :266
        visit(14, lt * std::max<size_t>(dijRowsN, 1), kDijOut);       // :267
    }
    bool allocBuffers(unsigned classes, Mallocs& mal) {               // rtd_engine_impl.hpp:309-318
        bool ok = true;
        forEachBuffer([&](int i, size_t n, unsigned c) {
            if (!ok || !(classes & c) || n == 0) return;
            ok = mal();
            if (ok) p[i] = true;
        });
        return ok;
    }
    void freeBuffers(unsigned classes) {                              // rtd_engine_impl.hpp:320-322
        forEachBuffer([&](int i, size_t, unsigned c) { if ((classes & c) && p[i]) p[i] = false; });
    }
    bool allocListedAndMissing(Mallocs& mal) {                        // rtd_dij_host.hpp:321-323, rtd_let_host.hpp:81-83
        bool ok = true;
        forEachBuffer([&](int i, size_t n, unsigned c) { if (ok && c == kDijOut && n && !p[i]) { ok = mal(); if (ok) p[i] = true; } });
        return ok;
    }

    Status doseInfluence(const ComputeDraw& d, Mallocs& mal) {        // rtd_dij_host.hpp, rtd_field_dose_influence
        dijDone = false; letDone = false;                             // :59
        ++dijEpoch;                                                   // :60
        if (!p[0]) {                                                  // :61
            dijCap = (size_t)1 << 20;                                 // :62
            if (!allocBuffers(kDij, mal)) { freeBuffers(kDij); dijCap = 0; return kFailed; }   // :63-64
        }
        if (d.outcome == kFailForward) return kFailed;                // :67-71
        dijBatchOf.assign(kSpots, -1);                                // :90
        for (size_t j = 0; j < kSpots; ++j) if (d.batch[j] >= 0) dijBatchOf[j] = d.batch[j];   // :113
        if (d.staged > dijCap) {                                      // :178
            size_t cap = dijCap;                                      // :179
            while (cap < d.staged) cap *= 2;                          // :180
            dijCap = cap;                                             // :187
        }
        if (d.outcome == kFailBatches) return kFailed;                // :211-213
        freeBuffers(kDijOut);                                         // :217
        dijPrepared = false; letAlloc = false;                        // :218
        for (int i = 0; i < 6; ++i) dijOwnBox[i] = d.ownBox[i];       // :219
        dijNnz = d.nnz;                                               // :220
        if (!allocBuffers(kDijOut, mal)) { freeBuffers(kDijOut); dijNnz = 0; return kFailed; }   // :221
        if (d.outcome == kFailGather) return kFailed;                 // :222-227
        dijDone = true;                                               // :228
        return kOk;
    }
    Status prepare(const PrepareDraw& d, Mallocs& mal) {              // rtd_dij_host.hpp, rtd_field_dose_influence_prepare
        if (!dijDone) return kRefused;                                // :273
        if (dijPrepared) return kOk;                                  // :274
        if (d.failEarly) return kFailed;                              // :280-312
        dijBox = d.box; dijRowsN = d.rows; dijChunks = d.chunks;      // :319
        dijPrepared = true;                                           // :320
        const bool ok = allocListedAndMissing(mal);                   // :321-323
        if (!ok || d.failLate) {                                      // :356
            dijPrepared = false;                                      // :325
            for (int i : {6, 7, 8, 9, 10, 11}) if (p[i]) p[i] = false;   // :326-328
            return kFailed;
        }
        return kOk;
    }
    Status letInfluence(const Handle& h, const PrepareDraw& d, bool launchFails, Mallocs& mal) {   // rtd_let_host.hpp, rtd_field_let_influence
        if (!dijDone) return kRefused;                                // :70
        if (!h.dLetTable) return kRefused;                            // :71
        if (!dijPrepared) { const Status st = prepare(d, mal); if (st != kOk) return st; }   // :74
        letDone = false;                                              // :77
        if (!letAlloc) {                                              // :78
            letAlloc = true;                                          // :79
            if (!allocListedAndMissing(mal)) {                        // :81-84
                for (int i : {12, 13, 14}) if (p[i]) p[i] = false;    // :86
                letAlloc = false;                                     // :87
                return kFailed;                                       // :88
            }
        }
        if (launchFails) return kFailed;                              // :104
        letDone = true; letEpoch = h.letEpoch;                        // :105
        return kOk;
    }
    bool letReady(const Handle& h) const { return dijDone && letDone && h.dLetTable && letEpoch == h.letEpoch; }   // rtd_let_host.hpp:10, rtd_optimizer_host.hpp:405
    void release() {                                                  // rtd_engine.hip, rtd_field_release
        freeBuffers(kDij | kDijOut);                                  // :434 (the classes walked here)
        dijDone = false; dijPrepared = false; dijCap = 0; dijNnz = 0; dijBatchOf.clear();   // :437
        letAlloc = false; letDone = false;                            // :438
    }
    // rtd_planset_host.hpp: what rtd_planset_create notes of a field (:179-180, mostChunks starts at 1), what rtd_planset_run asks (:255)
    bool setRefused(unsigned epoch, size_t atChunks) const { return !dijDone || !dijPrepared || dijEpoch != epoch || dijChunks > atChunks; }
};

// ---- the header, driven as the engine drives it --------------------------------------------------------------------------------------
struct New {
    enum : unsigned { kDij = 16, kDijCsc = 32, kDijCompanion = 256, kDijLet = 512 };
    rtd::FieldMatrix matrix;
    bool p[kBufs] = {};

    template <typename V> void forEachBuffer(V&& visit) {
        const size_t nSpot = kSpots;
        visit(0, nSpot, kDij);
        visit(1, matrix.stagingEntries(), kDij); visit(2, matrix.stagingEntries(), kDij);
        visit(3, nSpot + 1, kDijCsc); visit(4, matrix.resultEntries(), kDijCsc); visit(5, matrix.resultEntries(), kDijCsc);
        visit(6, matrix.companionRowPtrs(), kDijCompanion); visit(7, matrix.companionEntries(), kDijCompanion);
        visit(8, matrix.companionEntries(), kDijCompanion); visit(9, matrix.companionChunkFirsts(nSpot), kDijCompanion);
        visit(10, matrix.companionChunks(), kDijCompanion); visit(11, matrix.companionChunks(), kDijCompanion);
        visit(12, matrix.letEntries(), kDijLet); visit(13, matrix.letEntries(), kDijLet); visit(14, matrix.letDepths(), kDijLet);
    }
    bool tryAllocBuffers(unsigned classes, Mallocs& mal) {
        bool ok = true;
        forEachBuffer([&](int i, size_t n, unsigned c) {
            if (!ok || !(classes & c) || n == 0) return;
            ok = mal();
            if (ok) p[i] = true;
        });
        return ok;
    }
    void freeBuffers(unsigned classes) {
        forEachBuffer([&](int i, size_t, unsigned c) { if ((classes & c) && p[i]) p[i] = false; });
    }

    Status doseInfluence(const ComputeDraw& d, Mallocs& mal) {
        rtd::FieldMatrix& m = matrix;
        m.computeBegins();
        if (!p[0]) {
            m.stagingSized((size_t)1 << 20);
            if (!tryAllocBuffers(kDij, mal)) { freeBuffers(kDij); m.stagingSized(0); return kFailed; }
        }
        if (d.outcome == kFailForward) return kFailed;
        std::vector<int> batchOf(kSpots, -1);
        for (size_t j = 0; j < kSpots; ++j) if (d.batch[j] >= 0) batchOf[j] = d.batch[j];
        if (d.staged > m.stagingEntries()) {
            size_t cap = m.stagingEntries();
            while (cap < d.staged) cap *= 2;
            m.stagingSized(cap);
        }
        if (d.outcome == kFailBatches) return kFailed;
        freeBuffers(kDijCsc | kDijCompanion | kDijLet);
        m.resultSized(d.nnz, d.ownBox);
        if (!tryAllocBuffers(kDijCsc, mal)) { freeBuffers(kDijCsc); m.resultAllocationFailed(); return kFailed; }
        if (d.outcome == kFailGather) return kFailed;
        m.computeFinished(std::move(batchOf));
        return kOk;
    }
    Status prepare(const PrepareDraw& d, Mallocs& mal) {
        rtd::FieldMatrix& m = matrix;
        if (!m.hasMatrix()) return kRefused;                          // (matrixRefusal, kMatrix)
        if (m.prepared()) return kOk;
        if (d.failEarly) return kFailed;
        m.companionSized(d.box, d.rows, d.chunks);
        const bool ok = tryAllocBuffers(kDijCompanion, mal);
        if (!ok || d.failLate) { m.companionFailed(); freeBuffers(kDijCompanion); return kFailed; }
        return kOk;
    }
    Status letInfluence(const Handle& h, const PrepareDraw& d, bool launchFails, Mallocs& mal) {
        rtd::FieldMatrix& m = matrix;
        if (!m.hasMatrix()) return kRefused;
        if (!h.dLetTable) return kRefused;
        if (!m.prepared()) { const Status st = prepare(d, mal); if (st != kOk) return st; }   // (matrixOpen, kPrepared)
        m.letBegins();
        if (!m.letListed()) {
            m.letSized();
            if (!tryAllocBuffers(kDijLet, mal)) { freeBuffers(kDijLet); m.letFailed(); return kFailed; }
        }
        if (launchFails) return kFailed;
        m.letComputed(h.letEpoch);
        return kOk;
    }
    bool letReady(const Handle& h) const { return matrix.letValid(h.dLetTable, h.letEpoch); }
    void release() { freeBuffers(kDij | kDijCsc | kDijCompanion | kDijLet); matrix.released(); }
};

struct Coverage {
    long events = 0;
    long hasMatrix[2] = {}, prepared[2] = {}, letReady[2] = {}, verdict[2] = {}, companionListed[2] = {}, letListed[2] = {}, staging[2] = {};
    long outcome[6] = {}, emptyMatrix = 0, grown = 0;
    long prepareFailedEarly = 0, prepareFailedInAllocation = 0, prepareFailedLate = 0, letFailedInAllocation = 0, letFailedOverValues = 0, letPreparedOnDemand = 0;
    long recomputedUnderLet = 0;          // prepared, LET values valid, then the matrix computed again (to the end)
    long staleCompanion = 0;              // no matrix, and the companion of the one before still listed (a computation failed in between)
    long tableGoneUnderLet = 0, newTableUnderLet = 0, releasedWithMatrix = 0, setStale = 0;
    bool complete() const {
        bool ok = emptyMatrix > 0 && grown > 0 && prepareFailedEarly > 0 && prepareFailedInAllocation > 0 && prepareFailedLate > 0 &&
                  letFailedInAllocation > 0 && letFailedOverValues > 0 && letPreparedOnDemand > 0 && recomputedUnderLet > 0 && staleCompanion > 0 && tableGoneUnderLet > 0 &&
                  newTableUnderLet > 0 && releasedWithMatrix > 0 && setStale > 0;
        for (int i = 0; i < 2; ++i)
            ok = ok && hasMatrix[i] > 0 && prepared[i] > 0 && letReady[i] > 0 && verdict[i] > 0 && companionListed[i] > 0 && letListed[i] > 0 && staging[i] > 0;
        for (int i = 0; i < 6; ++i) ok = ok && outcome[i] > 0;
        return ok;
    }
    void print(const char* head) const {
        std::printf("%s events %ld matrix %ld/%ld prepared %ld/%ld let_ready %ld/%ld set_refused %ld/%ld companion_listed %ld/%ld let_listed %ld/%ld "
                    "staging %ld/%ld compute staging_failed %ld forward_failed %ld batches_failed %ld result_failed %ld gather_failed %ld finished %ld "
                    "empty_matrix %ld staging_grown %ld prepare early_failed %ld allocation_failed %ld late_failed %ld let allocation_failed %ld failed_over_values %ld "
                    "prepared_on_demand %ld recomputed_under_let %ld stale_companion %ld table_gone_under_let %ld new_table_under_let %ld "
                    "released_with_matrix %ld set_stale %ld\n", head, events, hasMatrix[0], hasMatrix[1], prepared[0], prepared[1],
                    letReady[0], letReady[1], verdict[0], verdict[1], companionListed[0], companionListed[1], letListed[0], letListed[1], staging[0],
                    staging[1], outcome[0], outcome[1], outcome[2], outcome[3], outcome[4], outcome[5], emptyMatrix, grown, prepareFailedEarly,
                    prepareFailedInAllocation, prepareFailedLate, letFailedInAllocation, letFailedOverValues, letPreparedOnDemand, recomputedUnderLet, staleCompanion,
                    tableGoneUnderLet, newTableUnderLet, releasedWithMatrix, setStale);
    }
};

#define SAME(what, a, b)                                                                                                        \
    do {                                                                                                                        \
        if ((long long)(a) != (long long)(b)) {                                                                                 \
            std::printf("differs: walk %d event %d (%s): %s was %lld, is %lld\n", w, e, name, what, (long long)(a), (long long)(b)); \
            return false;                                                                                                       \
        }                                                                                                                       \
    } while (0)

// One pass. compare = false: the transcription alone.
bool walkAll(int walks, int events, bool compare, Coverage& cov) {
    std::mt19937 rng(20261u);
    auto draw = [&](unsigned n) { return (unsigned)(rng() % n); };
    for (int w = 0; w < walks; ++w) {
        auto old = std::make_unique<Old>();
        auto now = std::make_unique<New>();                              // (on the heap: the sanitizer watches both ends of it)
        Handle h;
        h.letEpoch = draw(3);
        bool haveSet = false; unsigned setEpoch = 0; size_t setChunks = 0;
        for (int e = 0; e < events; ++e) {
            const unsigned r = draw(100);
            const char* name = "";
            ++cov.events;
            Mallocs malOld, malNew;
            auto prepareDraw = [&] {
                PrepareDraw d{draw(12) == 0, draw(12) == 0, rtd::DijBox{(int)draw(4), (int)draw(4), (int)draw(4), (int)draw(3), (int)draw(3) + 1, (int)draw(3) + 1}, 0, 0};
                d.rows = (size_t)d.box.bw * d.box.bh * d.box.bd;          // (0 for a box without voxels)
                d.chunks = draw(3) == 0 ? 0 : draw(40);
                if (draw(10) == 0) malOld.failAt = malNew.failAt = (int)draw(6);
                return d;
            };
            if (r < 8) {
                name = "table set";                                       // rtd_let_host.hpp:46
                if (old->letReady(h)) ++cov.newTableUnderLet;
                h.dLetTable = true; ++h.letEpoch;
            } else if (r < 12) {
                name = "table removed";                                   // rtd_let_host.hpp:30-31
                if (old->letReady(h)) ++cov.tableGoneUnderLet;
                h.dLetTable = false; ++h.letEpoch;
            } else if (r < 40) {
                name = "dose influence";
                ComputeDraw d{};
                const unsigned o = draw(20);
                d.outcome = o < 1 ? kFailStaging : o < 3 ? kFailForward : o < 5 ? kFailBatches : o < 6 ? kFailResult : o < 7 ? kFailGather : kFinish;
                d.nnz = draw(5) == 0 ? 0 : 1 + draw(5000000);
                d.staged = d.nnz + draw(1000);
                for (int i = 0; i < 3; ++i) { d.ownBox[i] = (int)draw(8); d.ownBox[3 + i] = d.ownBox[i] + (int)draw(8) - 1; }
                d.batch.resize(kSpots);
                for (auto& b : d.batch) b = (int)draw(5) - 1;
                if (d.outcome == kFailStaging) malOld.failAt = (int)draw(3);
                if (d.outcome == kFailResult) malOld.failAt = (old->p[0] ? 0 : 3) + (int)draw(3);
                malNew.failAt = malOld.failAt;
                const bool underLet = old->dijDone && old->dijPrepared && old->letReady(h);
                const size_t capBefore = old->p[0] ? old->dijCap : (size_t)1 << 20;
                const Status a = old->doseInfluence(d, malOld);
                // (what the draw asked for is what happened, but for a staging that stands: its allocation cannot fail then)
                Outcome got = d.outcome;
                if (d.outcome == kFailStaging && a == kOk) got = kFinish;
                if (d.outcome == kFailStaging && a == kFailed && old->p[0]) got = kFailResult;
                ++cov.outcome[got];
                if (a == kOk && d.nnz == 0) ++cov.emptyMatrix;
                if (got >= kFailBatches && old->dijCap > capBefore) ++cov.grown;
                if (a == kOk && underLet) ++cov.recomputedUnderLet;
                if (compare) { const Status b = now->doseInfluence(d, malNew); SAME("status", a, b); }
            } else if (r < 62) {
                name = "prepare";
                const PrepareDraw d = prepareDraw();
                const bool todo = old->dijDone && !old->dijPrepared;
                const Status a = old->prepare(d, malOld);
                if (todo && d.failEarly) ++cov.prepareFailedEarly;
                else if (todo && a == kFailed && malOld.failAt >= 0 && malOld.n > malOld.failAt) ++cov.prepareFailedInAllocation;
                else if (todo && a == kFailed) ++cov.prepareFailedLate;
                if (compare) { const Status b = now->prepare(d, malNew); SAME("status", a, b); }
            } else if (r < 80) {
                name = "let influence";
                const PrepareDraw d = prepareDraw();
                const bool launchFails = draw(12) == 0, wasReady = old->letReady(h);
                const bool onDemand = old->dijDone && h.dLetTable && !old->dijPrepared, listed = old->letAlloc;
                const Status a = old->letInfluence(h, d, launchFails, malOld);
                if (onDemand && a == kOk) ++cov.letPreparedOnDemand;
                if (a == kFailed && old->dijPrepared && !listed && !old->letAlloc) ++cov.letFailedInAllocation;
                if (a == kFailed && wasReady) ++cov.letFailedOverValues;
                if (compare) { const Status b = now->letInfluence(h, d, launchFails, malNew); SAME("status", a, b); }
            } else if (r < 92) {
                name = "plan set created";                                // (rtd_optimizer_host.hpp:176-179: a matrix, prepared on demand)
                const PrepareDraw d = prepareDraw();
                const Status a = old->dijDone ? old->prepare(d, malOld) : kRefused;
                if (compare) { const Status b = now->matrix.hasMatrix() ? now->prepare(d, malNew) : kRefused; SAME("status", a, b); }
                if (a == kOk) {
                    haveSet = true; setEpoch = old->dijEpoch; setChunks = std::max<size_t>(1, old->dijChunks);   // rtd_planset_host.hpp:175-182
                    if (compare) { SAME("noted epoch", setEpoch, now->matrix.epoch()); SAME("noted chunks", setChunks, std::max<size_t>(1, now->matrix.chunks())); }
                }
            } else {
                name = "release";                                         // rtd_engine.hip:434-438
                if (old->dijDone) ++cov.releasedWithMatrix;
                old->release();
                if (compare) now->release();
            }
            // what the engine reads between events
            const bool lr = old->letReady(h);
            ++cov.hasMatrix[old->dijDone]; ++cov.prepared[old->dijDone && old->dijPrepared]; ++cov.letReady[lr];
            ++cov.companionListed[old->dijPrepared]; ++cov.letListed[old->letAlloc]; ++cov.staging[old->dijCap > 0];
            if (!old->dijDone && old->dijPrepared) ++cov.staleCompanion;
            if (haveSet) {
                const bool refused = old->setRefused(setEpoch, setChunks);
                ++cov.verdict[refused];
                // (more chunks than noted under the noted epoch cannot be reached: a companion is built once per epoch, in front of the note)
                if (old->dijDone && old->dijPrepared && old->dijEpoch != setEpoch) ++cov.setStale;
                if (compare) SAME("plan set refused", refused, !now->matrix.isMatrixOf(setEpoch, setChunks));
            }
            if (!compare) continue;
            const rtd::FieldMatrix& m = now->matrix;
            SAME("has a matrix", old->dijDone, m.hasMatrix()); SAME("prepared", old->dijPrepared, m.prepared()); SAME("LET ready", lr, now->letReady(h));
            SAME("LET listed", old->letAlloc, m.letListed()); SAME("epoch", old->dijEpoch, m.epoch());
            SAME("nnz", old->dijNnz, m.nnz()); SAME("rows", old->dijRowsN, m.rows()); SAME("chunks", old->dijChunks, m.chunks());
            SAME("staging", old->dijCap, m.stagingEntries());
            const rtd::DijBox &ob = old->dijBox, &nb = m.box();
            SAME("box", ob.x0, nb.x0); SAME("box", ob.y0, nb.y0); SAME("box", ob.z0, nb.z0); SAME("box", ob.bw, nb.bw); SAME("box", ob.bh, nb.bh); SAME("box", ob.bd, nb.bd);
            for (int i = 0; i < 6; ++i) SAME("own box", old->dijOwnBox[i], m.ownBox()[i]);
            if (old->dijDone) {                                           // rtd_engine.hip:1344-1346 (refused without a matrix)
                SAME("dij_batch size", old->dijBatchOf.size(), m.batchOf().size());
                for (size_t j = 0; j < old->dijBatchOf.size(); ++j) SAME("dij_batch", old->dijBatchOf[j], m.batchOf()[j]);
            }
            size_t oldCount[kBufs], newCount[kBufs];
            old->forEachBuffer([&](int i, size_t n, unsigned) { oldCount[i] = n; });
            now->forEachBuffer([&](int i, size_t n, unsigned) { newCount[i] = n; });
            for (int i = 0; i < kBufs; ++i) { SAME("table count", oldCount[i], newCount[i]); SAME("pointer", old->p[i], now->p[i]); }
            SAME("allocations", malOld.n, malNew.n);
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int walks = argc > 1 ? std::atoi(argv[1]) : 4000, events = argc > 2 ? std::atoi(argv[2]) : 64;
    if (walks <= 0 || events <= 0) { std::fprintf(stderr, "usage: %s [walks] [events per walk]\n", argv[0]); return 2; }
    Coverage alone;
    walkAll(walks, events, false, alone);
    alone.print("transcription");
    if (!alone.complete()) { std::printf("the walk leaves an observable at one value: nothing compared\n"); return 3; }
    Coverage both;
    if (!walkAll(walks, events, true, both)) return 1;
    if (!both.complete() || both.events != alone.events) { std::printf("the lock step walked other events than the transcription alone\n"); return 3; }
    both.print("ok");
    return 0;
}
