// rtd_field_matrix.hpp — the life of a field's dose-influence matrix: what exists of it, what it is valid for, and how many elements
// of it the field's buffer table lists. Host only: plain C++17, no HIP, no kernel constant; it holds no device pointer (those are in
// the field's buffer table, classes kDij, kDijCsc, kDijCompanion and kDijLet). tests/cpp/test_rtd_field_matrix.cpp compiles it alone
// and walks it in lock step with the members and assignments the engine once wrote out by hand. DESIGN.md section 4, "What a field's
// matrix is valid for", states the rule; this file is the rule.
//
// The stages, each resting on the one before:
//   a matrix     the CSC result of the last rtd_field_dose_influence that finished              hasMatrix()
//   prepared     the row-major companion and the column chunks built from it                    prepared()
//   LET values   the LET-weighted values on its structure, under one table of the handle        letValid(table present, its number)
//   compact      the 16-bit form of the result and of the companion (rtd_dij_compact.hpp)         compact()
// The compact form rests on `prepared`. Once it stands the plain form's bulk may be given back (plainReleased()): the CSC's rows and
// values, the companion's columns and values and the LET values go, the structure both forms share (column pointers, row pointers,
// the chunk tables and sums) stays, and every consumer of the plain form is refused until the next computation.
// The engine reports the events below where they happen, and nothing but this file writes the state.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace rtd {

struct DijBox { int x0, y0, z0, bw, bh, bd; };   // the voxels that have a row in the companion (x fastest inside the box)

class FieldMatrix {
    bool done_ = false;           // the CSC buffers hold the last computation's result
    bool companion_ = false;      // the buffer table lists the companion, and it belongs to the CSC result ...
    bool letListed_ = false;      // the buffer table lists the three LET buffers
    bool letDone_ = false;        // ... and they hold the values of the CSC result under the handle's table number letTable_
    unsigned epoch_ = 0;          // counts the computations begun: what was sized for a matrix knows it by this number
    unsigned letTable_ = 0;
    size_t staging_ = 0, nnz_ = 0, rows_ = 0, chunks_ = 0;
    int ownBox_[6] = {0, 0, 0, -1, -1, -1};   // the field's dose box (min, max) when the matrix was computed
    DijBox box_{};                // ... united with the bounding box of the matrix's rows: the voxels that have a row
    std::vector<int> batchOf_;    // per spot: its batch in the computation that finished last (-1: empty column)
    // The compact form (rtd_field_dose_influence_compact): listed in the buffer table, and built for the CSC result; its tree (lanes
    // per row, entries per lane and trip), the width of its CSC row indices, the companion's entries with the rows' pads and the
    // 64-entry groups of the CSC side. released_: the plain form's bulk has been freed.
    bool compactListed_ = false, compactDone_ = false, released_ = false;
    int cLanes_ = 0, cPer_ = 0, cRowBits_ = 0;
    size_t cEntries_ = 0, cGroups_ = 0, releasedBytes_ = 0;

public:
    // ---- events of rtd_field_dose_influence ----
    // A computation begins: the result is no longer valid, nor are the LET values made from it; whatever was sized for the matrix (a
    // plan set) no longer is. The companion stays listed until the new result's size is known (resultSized): a computation that fails
    // in between leaves `prepared` over the old companion, which nothing can reach while there is no matrix.
    void computeBegins() { done_ = false; letDone_ = false; compactDone_ = false; ++epoch_; }
    // The batch-major staging is listed with `entries` entries: in front of its first allocation, after growing, 0 when allocating failed.
    void stagingSized(size_t entries) { staging_ = entries; }
    // The batches are through: the old result's buffers, the companion's and the LET values' have been freed, the table lists a
    // result of nnz entries (allocated next).
    void resultSized(size_t nnz, const int ownBox[6]) {
        companion_ = false; letListed_ = false; compactListed_ = false; released_ = false;
        std::copy(ownBox, ownBox + 6, ownBox_);
        nnz_ = nnz;
    }
    void resultAllocationFailed() { nnz_ = 0; }
    void computeFinished(std::vector<int> batchOf) { batchOf_ = std::move(batchOf); done_ = true; }

    // ---- events of rtd_field_dose_influence_prepare ----
    // The companion's sizes are known: the table lists it from here on (allocated next).
    void companionSized(const DijBox& box, size_t rows, size_t chunks) { box_ = box; rows_ = rows; chunks_ = chunks; companion_ = true; }
    void companionFailed() { companion_ = false; }   // (allocating or building it: its buffers have been freed, the sizes stay)

    // ---- events of rtd_field_let_influence ----
    void letBegins() { letDone_ = false; }
    void letSized() { letListed_ = true; }           // the table lists the three from here on (allocated next)
    void letFailed() { letListed_ = false; }
    void letComputed(unsigned handleTable) { letDone_ = true; letTable_ = handleTable; }

    // ---- events of rtd_field_dose_influence_compact ----
    // A build begins with `lanes` lanes per row and `per` entries per lane and trip: the table lists the scales, the scaled weights
    // and the CSC side (codes, 16-bit offsets, `groups` group bases) from here on (allocated next); what an earlier build left has
    // been freed.
    void compactBegins(int lanes, int per, size_t groups) {
        compactListed_ = true; compactDone_ = false; cLanes_ = lanes; cPer_ = per; cGroups_ = groups; cEntries_ = 0; cRowBits_ = 16;
    }
    // The padded rows have been scanned: the companion side is listed with `entries` entries (allocated next).
    void compactCompanionSized(size_t entries) { cEntries_ = entries; }
    // A group of the CSC side spans more than 65 535 voxels: its offsets have been freed, the side reads the result's 32-bit rows.
    void compactRowsStayWide() { cRowBits_ = 32; }
    void compactBuilt() { compactDone_ = true; }
    void compactFailed() { compactListed_ = false; compactDone_ = false; cEntries_ = 0; cGroups_ = 0; }   // (refused, or allocating failed: its buffers have been freed)
    // release_plain: the bulk of the plain form (`bytes` as the table listed it) has been freed, the LET values with it.
    void plainReleasedNow(size_t bytes) { released_ = true; releasedBytes_ = bytes; letListed_ = false; letDone_ = false; }

    // rtd_field_release: every buffer of the matrix has been freed. (The epoch goes on counting; the companion's sizes stay, unread.)
    void released() {
        done_ = false; companion_ = false; staging_ = 0; nnz_ = 0; batchOf_.clear(); letListed_ = false; letDone_ = false;
        compactListed_ = false; compactDone_ = false; released_ = false;
    }

    // ---- queries ----
    bool hasMatrix() const { return done_; }
    bool prepared() const { return companion_; }      // (asked behind hasMatrix(): see computeBegins)
    // The LET values are those of the matrix and of the handle's table as it stands.
    bool letValid(bool tablePresent, unsigned handleTable) const { return done_ && letDone_ && tablePresent && letTable_ == handleTable; }
    bool letListed() const { return letListed_; }
    // An object noted epoch() and room for `chunkCapacity` chunks when it was created: is the matrix still the one it was created on?
    unsigned epoch() const { return epoch_; }
    // (a matrix whose plain form has been released is nobody's who reads that form)
    bool isMatrixOf(unsigned notedEpoch, size_t chunkCapacity) const { return done_ && companion_ && !released_ && epoch_ == notedEpoch && chunks_ <= chunkCapacity; }
    bool compact() const { return done_ && companion_ && compactDone_; }
    bool isCompactOf(unsigned notedEpoch) const { return compact() && epoch_ == notedEpoch; }
    bool plainReleased() const { return released_; }
    size_t releasedBytes() const { return releasedBytes_; }   // what the plain form's bulk held when it was released
    int compactLanes() const { return cLanes_; }
    int compactPer() const { return cPer_; }
    int compactRowBits() const { return cRowBits_; }
    size_t compactEntries() const { return cEntries_; }   // the companion side's, pads included
    size_t compactGroups() const { return cGroups_; }
    size_t nnz() const { return nnz_; }
    size_t rows() const { return rows_; }             // voxels of box()
    size_t chunks() const { return chunks_; }
    size_t stagingEntries() const { return staging_; }
    const DijBox& box() const { return box_; }
    const int* ownBox() const { return ownBox_; }
    const std::vector<int>& batchOf() const { return batchOf_; }   // rtd_field_fetch "dij_batch"

    // ---- element counts of the buffer table (0: the field has no such buffer) ----
    size_t resultEntries() const { return std::max<size_t>(nnz_, 1); }                       // rows and values of the CSC
    size_t resultRows() const { return released_ && cRowBits_ == 16 ? 0 : resultEntries(); } // (released: the rows stay where the compact CSC side reads them)
    size_t resultValues() const { return released_ ? 0 : resultEntries(); }
    size_t companionRowPtrs() const { return companion_ ? rows_ + 1 : 0; }
    size_t companionEntries() const { return companion_ && !released_ ? std::max<size_t>(nnz_, 1) : 0; }   // columns and values of the companion
    size_t companionChunkFirsts(size_t nSpot) const { return companion_ ? nSpot + 1 : 0; }
    size_t companionChunks() const { return companion_ ? std::max<size_t>(chunks_, 1) : 0; }  // chunk columns and chunk sums
    size_t letEntries() const { return letListed_ ? std::max<size_t>(nnz_, 1) : 0; }          // LET values of the CSC and of the companion
    size_t letDepths() const { return letListed_ ? std::max<size_t>(rows_, 1) : 0; }
    size_t compactSpots(size_t nSpot) const { return compactListed_ ? std::max<size_t>(nSpot, 1) : 0; }       // scales, scaled weights
    size_t compactCscEntries() const { return compactListed_ ? std::max<size_t>(nnz_, 1) : 0; }               // codes of the CSC side
    size_t compactCscOffsets() const { return compactListed_ && cRowBits_ == 16 ? std::max<size_t>(nnz_, 1) : 0; }
    size_t compactCscGroups() const { return compactListed_ ? std::max<size_t>(cGroups_, 1) : 0; }
    size_t compactRowPtrs() const { return compactListed_ && cPer_ > 1 ? rows_ + 1 : 0;}        // (without pads the companion's own row pointers serve)
    size_t compactCompanionEntries() const { return compactListed_ ? cEntries_ : 0; }                         // codes and columns of the companion side
};

}  // namespace rtd
