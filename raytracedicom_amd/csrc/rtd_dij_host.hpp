// rtd_dij_host.hpp — host side of a field's dose-influence matrix and of the products with it (include/rtd.h, DESIGN.md sections 10
// and 11; kernels in rtd_dij.hpp and rtd_dij_apply.hpp). Part of rtd_engine.hip's translation unit, included at its end: the batches
// run through its rtd_field_compute_bev and transferImpl. The matrix's buffers are the field's (classes kDij, kDijCsc, kDijCompanion
// and kDijLet of its table); what exists of it and what it is valid for is f->matrix (rtd_field_matrix.hpp), which these files
// tell what happened and ask what holds.
#pragma once

namespace {

// The field's LET values are those of its matrix and of the handle's table as it stands.
bool letReady(const rtd_handle_impl* h, const rtd_field_impl* f) { return f->matrix.letValid(h->dLetTable != nullptr, h->letTableNo); }

// The opening of the matrix entry points, behind the handle and pointer tests of each: what the call needs of the field.
//   kWorkspace   a field that is not remote                         (rtd_field_dose_influence)
//   kMatrix      ... with a matrix
//   kPrepared    ... with a matrix, prepared on demand (the first product of a matrix is synchronous that once)
//   kLetValues   ... with LET values of the matrix and of the handle's table
enum class MatrixStage { kWorkspace, kMatrix, kPrepared, kLetValues };
// What every consumer of the plain form answers (RTD_ERR_NOT_READY) between a release and the next rtd_field_dose_influence.
const char* const kPlainReleasedMsg = ": the plain form of the matrix was freed (rtd_field_dose_influence_compact with release_plain = 1); call rtd_field_dose_influence again";
// The refusals alone, `who` being the entry point the messages name: all that an entry point without launches asks.
int matrixRefusal(rtd_handle_impl* h, const rtd_field_impl* f, const char* who_, MatrixStage need) {
    auto who = [&] { return std::string(who_); };                      // (composed only for a refusal)
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, who() + ": a remote field has no workspace");
    if (need != MatrixStage::kWorkspace && f->matrix.hasMatrix() && f->matrix.plainReleased()) return fail(h, RTD_ERR_NOT_READY, who() + kPlainReleasedMsg);
    if (need == MatrixStage::kLetValues) {
        if (!letReady(h, f)) return fail(h, RTD_ERR_NOT_READY, who() + ": no LET-weighted matrix of the current matrix and table (call rtd_field_let_influence first)");
    } else if (need != MatrixStage::kWorkspace && !f->matrix.hasMatrix())
        return fail(h, RTD_ERR_NOT_READY, who() + ": no dose-influence matrix (call rtd_field_dose_influence first)");
    return RTD_OK;
}
// The refusals, the preparation, and the handle's device made current: a launch may follow.
int matrixOpen(rtd_handle hh, rtd_field ff, const char* who, MatrixStage need) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    { const int st = matrixRefusal(h, f, who, need); if (st != RTD_OK) return st; }
    if (need == MatrixStage::kPrepared && !f->matrix.prepared()) { const int st = rtd_field_dose_influence_prepare(hh, ff); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipSetDevice(h->device));
    return RTD_OK;
}

// The two products' launches with a values array of the matrix's structure: the dose's (rtd_field_dose_influence_apply / _apply_t) or
// the LET-weighted one (rtd_let_host.hpp). cVals: the row-major companion's values; vals: the CSC's.
int dijApplyLaunch(rtd_handle_impl* h, rtd_field_impl* f, const float* cVals, const float* dev_spot_weights, float* dev_dose, int init) {
    const long long nRows = (long long)f->matrix.rows();
    if (nRows == 0 || (!init && f->matrix.nnz() == 0)) return RTD_OK; // nothing to write: no launch
    const unsigned g = (unsigned)((nRows * kDijApGroup + 255) / 256);
    auto launch = [&](auto kern) {
        kern<<<g, 256, 0, h->stream>>>((const long long*)f->dDijRowPtr, (const int*)f->dDijCCols, cVals, dev_spot_weights, dev_dose,
                                       (int)f->doseDims[0], (int)f->doseDims[1], f->matrix.box(), nRows);
    };
    if (init) launch(k_dijap_apply<true>); else launch(k_dijap_apply<false>);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}
int dijApplyTLaunch(rtd_handle_impl* h, rtd_field_impl* f, const float* vals, const float* dev_voxel_weights, float* dev_spot_grad) {
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L, nChunks = (int)f->matrix.chunks();
    if (nChunks)
        k_dijap_apply_t<<<(unsigned)((nChunks + 3) / 4), 256, 0, h->stream>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, vals,
                                                                            (const int*)f->dDijChunkCol, (const int*)f->dDijChunkFirst, dev_voxel_weights,
                                                                            f->dDijPartial, nChunks);
    k_dijap_reduce_t<<<(unsigned)((nSpot + 3) / 4), 256, 0, h->stream>>>((const int*)f->dDijChunkFirst, (const float*)f->dDijPartial, dev_spot_grad, nSpot);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // namespace

extern "C" {

// Dose-influence matrix of a field (include/rtd.h; kernels in rtd_dij.hpp). One forward at the field's own
// weights gives the largest batch radius Rmax and the entry plane; the exact spot -> ray footprints come back from the device; the
// spots are coloured greedily, in spot order, into batches whose footprints grown by Rmax + 2 rays are disjoint; every batch is one
// forward at unit weights on its spots, transferred into a scratch volume and split by owner into per-spot columns. A last forward at
// the field's own weights restores every buffer a later transfer, clear or gradient reads.
int rtd_field_dose_influence(rtd_handle hh, rtd_field ff, float rel_threshold, size_t* nnz) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!nnz) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: null nnz pointer");
    if (!(rel_threshold >= 0.0f && rel_threshold < 1.0f)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: rel_threshold must lie in [0, 1)");
    { const int st = matrixRefusal(h, f, "rtd_field_dose_influence", MatrixStage::kWorkspace); if (st != RTD_OK) return st; }
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: not available with nuclear_corr");
    if (f->fc.rayWeightCutoff != 0.0f)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: needs options.ray_weight_cutoff = 0 when the field is created (only then is the dose linear in the spot weights)");
    if (!h->dCt || !h->haveLuts) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence: set LUTs and CT first");
    const FieldConst& fc = f->fc;
    const size_t nVox = (size_t)f->doseDims[0] * f->doseDims[1] * f->doseDims[2];
    if (nVox > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: more than 2^31 - 1 dose voxels (int32 row indices)");
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nSpot = (size_t)fc.spotNx * fc.spotNy * fc.L;
    FieldMatrix& m = f->matrix;
    m.computeBegins();                                                // (the LET values and whatever a plan set sized belong to the matrix that is replaced)
    if (!f->dDijSave) {
        m.stagingSized((size_t)1 << 20);
        const int st = allocBuffers(h, f, kDij);
        if (st != RTD_OK) { freeBuffers(f, kDij); m.stagingSized(0); return st; }
    }
    // 1. the forward at the field's own weights: Rmax, the entry plane, the field's findings
    { const int st = rtd_field_compute_bev(hh, ff); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipStreamSynchronize(s));
    const FieldState own = *f->hState;
    { const int st = takeFindings(h, f, own); if (st != RTD_OK) return st; }
    if (own.errorFlags & kErrRadiusOverflow) return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
    const int rMax = own.maxRadius;
    const FieldHints savedHints = f->memory.savedHints();
    // 2. footprints, exactly as the convolution's loops visit the spots
    std::vector<int> footX(2 * nSpot / fc.spotNy), footY(2 * nSpot / fc.spotNx);
    {
        const int nT = fc.L * (fc.spotNx + fc.spotNy);
        k_dij_footprint<<<(nT + 255) / 256, 256, 0, s>>>((const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc, f->dDijFoot,
                                                       f->dDijFoot + footX.size());
        RTD_HIP(h, hipGetLastError());
        RTD_HIP(h, hipMemcpyAsync(footX.data(), f->dDijFoot, footX.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        RTD_HIP(h, hipMemcpyAsync(footY.data(), f->dDijFoot + footX.size(), footY.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        RTD_HIP(h, hipStreamSynchronize(s));
    }
    // 3. batches: first fit in spot order over occupancy bitmaps of the padded BEV grid
    const int bevW = fc.bevW, bevH = fc.bevH, words = (bevW + 63) / 64, grow = rMax + 2;
    std::vector<std::array<int, 4>> box(nSpot);
    std::vector<std::vector<uint64_t>> occ;
    std::vector<std::vector<int>> members;
    std::vector<int> batchOf(nSpot, -1);                               // per spot: its batch (-1: empty column); the matrix's once it is finished
    auto meets = [&](const std::vector<uint64_t>& bm, const std::array<int, 4>& b) {
        for (int y = b[1]; y <= b[3]; ++y)
            for (int w = b[0] / 64; w <= b[2] / 64; ++w) {
                const int lo = std::max(b[0], 64 * w) - 64 * w, hi = std::min(b[2], 64 * w + 63) - 64 * w;
                const uint64_t m = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1)) & ~((1ull << lo) - 1);
                if (bm[(size_t)y * words + w] & m) return true;
            }
        return false;
    };
    for (size_t j = 0; j < nSpot; ++j) {
        const size_t l = j / ((size_t)fc.spotNx * fc.spotNy), sy = (j / fc.spotNx) % fc.spotNy, sx = j % fc.spotNx;
        const int* fx = &footX[2 * (l * fc.spotNx + sx)];
        const int* fy = &footY[2 * (l * fc.spotNy + sy)];
        if (fx[1] < fx[0] || fy[1] < fy[0]) continue;                // no ray sees the spot: an empty column
        std::array<int, 4>& b = box[j];
        b = {std::max(fx[0] + kMaxSuperpR - grow, 0), std::max(fy[0] + kMaxSuperpR - grow, 0),
             std::min(fx[1] + kMaxSuperpR + grow, bevW - 1), std::min(fy[1] + kMaxSuperpR + grow, bevH - 1)};
        size_t k = 0;
        while (k < occ.size() && (members[k].size() >= (size_t)kDijMaxSpots || meets(occ[k], b))) ++k;
        if (k == occ.size()) { occ.emplace_back((size_t)bevH * words, 0ull); members.emplace_back(); }
        for (int y = b[1]; y <= b[3]; ++y) for (int x = b[0]; x <= b[2]; ++x) occ[k][(size_t)y * words + x / 64] |= 1ull << (x % 64);
        members[k].push_back((int)j);
        batchOf[j] = (int)k;
    }
    occ.clear();
    std::vector<int> list, boxes;
    std::vector<size_t> first(members.size() + 1, 0);
    for (size_t k = 0; k < members.size(); ++k) {
        first[k] = list.size();
        for (int j : members[k]) { list.push_back(j); boxes.insert(boxes.end(), box[(size_t)j].begin(), box[(size_t)j].end()); }
    }
    first[members.size()] = list.size();
    std::vector<long long> colLen(nSpot, 0);
    long long total = 0;
    int dijErr = 0;
    int st = RTD_OK;
    auto hipFail = [&](hipError_t e) { h->error = std::string("HIP error (dose influence): ") + hipGetErrorString(e); st = RTD_ERR_HIP; };
    hipError_t e = hipSuccess;
    if (!list.empty()) {
        e = hipMemcpyAsync(f->dDijList, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(f->dDijBoxes, boxes.data(), boxes.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(f->dDijSave, f->dSpotWeights, nSpot * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijDose, 0, nVox * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijMisc, 0, 4 * sizeof(int), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijColLen, 0, nSpot * sizeof(long long), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijColSrc, 0, nSpot * sizeof(long long), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);             // (the host vectors above are pageable)
        if (e != hipSuccess) hipFail(e);
        // the batches run without the field's hints: each one is planned (uniform-sigma detection, second sweep launch) on its own
        f->memory.forgetHints();
    }
    // 4. per batch: unit weights, owner map, forward + transfer into the scratch volume, split, clear of its dose box
    for (size_t k = 0; k < members.size() && st == RTD_OK; ++k) {
        const int n = (int)(first[k + 1] - first[k]);
        const int* dList = f->dDijList + first[k];
        e = hipMemsetAsync(f->dSpotWeights, 0, nSpot * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijOwner, 0xFF, (size_t)bevW * bevH * sizeof(unsigned short), s);
        if (e != hipSuccess) { hipFail(e); break; }
        k_dij_weights<<<(n + 255) / 256, 256, 0, s>>>(f->dSpotWeights, dList, n);
        k_dij_owner<<<n, 256, 0, s>>>(f->dDijOwner, bevW, f->dDijBoxes + 4 * first[k]);
        if ((e = hipGetLastError()) != hipSuccess) { hipFail(e); break; }
        f->memory.forgetHints();
        st = rtd_field_compute_bev(hh, ff);
        if (st == RTD_OK) st = transferImpl(hh, ff, f->dDijDose, nullptr, nullptr, false);
        if (st != RTD_OK) break;
        k_dij_check<<<1, 64, 0, s>>>((const FieldState*)f->dState, rMax, f->dDijMisc + 1);
        const size_t lds = (size_t)n * sizeof(unsigned int);
        auto split = [&](auto kern) {
            kern<<<kDijBlocks, 64, lds, s>>>((const float*)f->dDijDose, (int)f->doseDims[0], (int)f->doseDims[1], (const FieldState*)f->dState,
                                            (const unsigned short*)f->dDijOwner, bevW, bevH, n, rel_threshold, f->dDijColMax, f->dDijCnt,
                                            f->dDijRowsB + total, f->dDijValsB + total, f->dDijMisc + 1);
        };
        if (rel_threshold > 0.0f) {
            if ((e = hipMemsetAsync(f->dDijColMax, 0, (size_t)n * sizeof(unsigned int), s)) != hipSuccess) { hipFail(e); break; }
            split(k_dij_split<0>);
        }
        split(k_dij_split<1>);
        k_dij_scan<<<1, 1024, 0, s>>>(f->dDijCnt, kDijBlocks, n, dList, total, f->dDijColLen, f->dDijColSrc, f->dDijMisc);
        int count = 0;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&count, f->dDijMisc, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { hipFail(e); break; }
        f->memory.sigmaFinished(f->hState->errorFlags);               // (the batch's forward has drained: the later batches only replay)
        if (f->hState->errorFlags & kErrRecordExtent) {               // (reported as takeFindings reports it)
            h->error = "a layer's steps exceed the field's sigma and dose records (inputs modified in place?): the records and the trace are dropped, recompute"; st = RTD_ERR_NOT_READY; break;
        }
        if ((size_t)(total + count) > m.stagingEntries()) {          // grow the batch-major staging geometrically (the stream is idle)
            size_t cap = m.stagingEntries();
            while (cap < (size_t)(total + count)) cap *= 2;
            DevBuf<int> r; DevBuf<float> v;
            e = r.alloc(cap);
            if (e == hipSuccess) e = v.alloc(cap);
            if (e == hipSuccess) e = hipMemcpy(r, f->dDijRowsB, (size_t)total * sizeof(int), hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(v, f->dDijValsB, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { hipFail(e); break; }
            std::swap(f->dDijRowsB, r.p); std::swap(f->dDijValsB, v.p); m.stagingSized(cap);   // (r and v free the old staging)
        }
        split(k_dij_split<2>);
        if ((e = hipGetLastError()) != hipSuccess) { hipFail(e); break; }
        total += count;
        st = rtd_field_clear_dose(hh, ff, f->dDijDose);
    }
    // 5. restore: the field's own weights and hints, one forward at them (deterministic: the same bits as before the call)
    if (!list.empty()) {
        (void)hipStreamSynchronize(s);
        if (st == RTD_OK) {
            e = hipMemcpyAsync(&dijErr, f->dDijMisc + 1, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(colLen.data(), f->dDijColLen, nSpot * sizeof(long long), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) hipFail(e);
        }
        const std::string keep = h->error;
        const hipError_t re = hipMemcpyAsync(f->dSpotWeights, f->dDijSave, nSpot * sizeof(float), hipMemcpyDeviceToDevice, s);
        f->memory.restoreHints(savedHints);
        int rst = re == hipSuccess ? rtd_field_compute_bev(hh, ff) : RTD_ERR_HIP;
        if (rst == RTD_OK && hipStreamSynchronize(s) != hipSuccess) rst = RTD_ERR_HIP;
        if (st == RTD_OK && rst != RTD_OK) { st = rst; if (h->error == keep) h->error = "HIP error (dose influence): restoring the field's forward failed"; }
        else h->error = keep;
    }
    if (st != RTD_OK) return st;
    if (dijErr & kDijErrOverflow) return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
    if (dijErr) return fail(h, RTD_ERR_HIP, "rtd_field_dose_influence: internal error: a batch's dose reached beyond the field's superposition radius");
    // 6. CSC: column pointers on the host, the batch-major columns gathered into column order on the device
    std::vector<long long> colPtr(nSpot + 1, 0);
    for (size_t j = 0; j < nSpot; ++j) colPtr[j + 1] = colPtr[j] + colLen[j];
    freeBuffers(f, kDijCsc | kDijCompanion | kDijLet | kDijCompact | kDijCompactRows);   // (with the old result what was built and computed from it)
    const FieldState& fin = *f->hState;
    const int ownBox[6] = {fin.tboxMin[0], fin.tboxMin[1], fin.tboxMin[2], fin.tboxMax[0], fin.tboxMax[1], fin.tboxMax[2]};
    m.resultSized((size_t)colPtr[nSpot], ownBox);
    { const int ast = allocBuffers(h, f, kDijCsc); if (ast != RTD_OK) { freeBuffers(f, kDijCsc); m.resultAllocationFailed(); return ast; } }
    RTD_HIP(h, hipMemcpyAsync(f->dDijColPtr, colPtr.data(), colPtr.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    if (m.nnz())
        k_dij_gather<<<(unsigned)nSpot, 256, 0, s>>>((const long long*)f->dDijColPtr, (const long long*)f->dDijColSrc, (const int*)f->dDijRowsB,
                                                     (const float*)f->dDijValsB, f->dDijRows, f->dDijVals);
    RTD_HIP(h, hipGetLastError());
    RTD_HIP(h, hipStreamSynchronize(s));
    m.computeFinished(std::move(batchOf));
    *nnz = m.nnz();
    return RTD_OK;
}

// Copies the last rtd_field_dose_influence result (host or device memory: hipMemcpyDefault).
int rtd_field_dose_influence_copy(rtd_handle hh, rtd_field ff, int64_t* col_ptr, int32_t* row_idx, float* values) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    // (its own opening: the matrix in front of the pointers, and a remote field is answered like any field without a matrix)
    const size_t nnz = f->matrix.nnz();
    if (!f->matrix.hasMatrix()) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_copy: no dose-influence matrix (call rtd_field_dose_influence first)");
    if (f->matrix.plainReleased()) return fail(h, RTD_ERR_NOT_READY, std::string("rtd_field_dose_influence_copy") + kPlainReleasedMsg);
    if (!col_ptr || (nnz && (!row_idx || !values))) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_copy: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    hipStream_t s = h->stream;
    RTD_HIP(h, hipMemcpyAsync(col_ptr, f->dDijColPtr, (nSpot + 1) * sizeof(int64_t), hipMemcpyDefault, s));
    if (nnz) {
        RTD_HIP(h, hipMemcpyAsync(row_idx, f->dDijRows, nnz * sizeof(int32_t), hipMemcpyDefault, s));
        RTD_HIP(h, hipMemcpyAsync(values, f->dDijVals, nnz * sizeof(float), hipMemcpyDefault, s));
    }
    RTD_HIP(h, hipStreamSynchronize(s));
    return RTD_OK;
}

// The device pointers of the last rtd_field_dose_influence result (no copy; owned by the field).
int rtd_field_dose_influence_device(rtd_handle hh, rtd_field ff, const int64_t** col_ptr, const int32_t** row_idx, const float** values, size_t* nnz) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!col_ptr || !row_idx || !values || !nnz) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_device: null pointer");
    { const int st = matrixRefusal(h, f, "rtd_field_dose_influence_device", MatrixStage::kMatrix); if (st != RTD_OK) return st; }
    *col_ptr = reinterpret_cast<const int64_t*>(f->dDijColPtr); *row_idx = f->dDijRows; *values = f->dDijVals; *nnz = f->matrix.nnz();
    return RTD_OK;
}

// Builds what the products with the last rtd_field_dose_influence result need (include/rtd.h; kernels in
// rtd_dij_apply.hpp): the row-major companion over the field's dose box and the chunk tables of the columns. Synchronous. The
// batch-major staging of rtd_field_dose_influence (dead since its gather into CSC, and at least nnz entries long) is the scratch of
// the placement: the companion costs no memory beyond its own.
int rtd_field_dose_influence_prepare(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    { const int st = matrixRefusal(h, f, "rtd_field_dose_influence_prepare", MatrixStage::kMatrix); if (st != RTD_OK) return st; }
    FieldMatrix& m = f->matrix;
    if (m.prepared()) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    const long long nnz = (long long)m.nnz();
    const int nx = (int)f->doseDims[0], ny = (int)f->doseDims[1];
    if (nnz && (m.stagingEntries() < m.nnz() || !f->dDijRowsB || !f->dDijValsB))
        return fail(h, RTD_ERR_HIP, "rtd_field_dose_influence_prepare: internal error: the staging buffers are smaller than the matrix");
    // column pointers -> the chunks of the transposed product
    std::vector<long long> colPtr(nSpot + 1);
    RTD_HIP(h, hipMemcpyAsync(colPtr.data(), f->dDijColPtr, colPtr.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    RTD_HIP(h, hipStreamSynchronize(s));
    std::vector<int> chunkFirst(nSpot + 1, 0), chunkCol;
    for (size_t j = 0; j < nSpot; ++j) {
        const long long n = (colPtr[j + 1] - colPtr[j] + kDijApChunk - 1) / kDijApChunk;
        if ((long long)chunkCol.size() + n > 0x7fffffffLL) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_prepare: more than 2^31 - 1 column chunks");
        chunkCol.insert(chunkCol.end(), (size_t)n, (int)j);
        chunkFirst[j + 1] = (int)chunkCol.size();
    }
    // the voxels that get a row: the field's dose box, grown (if need be) to hold every row of the matrix
    int lo[3], hi[3];
    for (int i = 0; i < 3; ++i) { lo[i] = m.ownBox()[i]; hi[i] = m.ownBox()[3 + i]; }
    if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) for (int i = 0; i < 3; ++i) { lo[i] = 0x7fffffff; hi[i] = -1; }
    DevBuf<int> dTmp; DevBuf<long long> dBlockSum;                    // scratch: freed when this call returns, after done's synchronise
    hipError_t e = hipSuccess;
    auto done = [&](int st) { (void)hipStreamSynchronize(s); return st; };
    auto hipFailed = [&]() { h->error = std::string("HIP error (dose influence prepare): ") + hipGetErrorString(e); return done(RTD_ERR_HIP); };
    const unsigned streamGrid = (unsigned)std::min<long long>((nnz + 255) / 256, (long long)h->numCUs * 32);
    if (nnz) {
        int mm[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};
        e = dTmp.alloc(sizeof mm / sizeof *mm);
        if (e == hipSuccess) e = hipMemcpyAsync(dTmp, mm, sizeof mm, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipFailed();
        k_dijap_bounds<<<streamGrid, 256, 0, s>>>((const int*)f->dDijRows, nnz, nx, ny, dTmp);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(mm, dTmp, sizeof mm, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipFailed();
        dTmp.reset();
        for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], mm[i]); hi[i] = std::max(hi[i], mm[3 + i]); }
    }
    DijBox box{0, 0, 0, 0, 0, 0};
    if (hi[0] >= lo[0]) box = DijBox{lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
    const long long nRows = (long long)box.bw * box.bh * box.bd;
    m.companionSized(box, (size_t)nRows, chunkCol.size());            // (the buffer table lists the companion from here on)
    e = tryAllocBuffers(f, kDijCompanion);
    auto undo = [&]() { m.companionFailed(); freeBuffers(f, kDijCompanion); };   // the CSC stays; the companion goes
    if (e == hipSuccess) e = hipMemcpyAsync(f->dDijChunkFirst, chunkFirst.data(), chunkFirst.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !chunkCol.empty()) e = hipMemcpyAsync(f->dDijChunkCol, chunkCol.data(), chunkCol.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !nnz) e = hipMemsetAsync(f->dDijRowPtr, 0, (size_t)(nRows + 1) * sizeof(long long), s);
    if (e == hipSuccess && nnz) {
        const int nBlocks = (int)((nRows + kDijApScanItems - 1) / kDijApScanItems);
        e = dTmp.alloc((size_t)nRows);
        if (e == hipSuccess) e = dBlockSum.alloc((size_t)nBlocks);
        if (e == hipSuccess) e = hipMemsetAsync(dTmp, 0, (size_t)nRows * sizeof(int), s);
        if (e == hipSuccess) {
            k_dijap_count<<<streamGrid, 256, 0, s>>>((const int*)f->dDijRows, nnz, nx, ny, box, dTmp);
            k_dijap_scan_sums<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dTmp, nRows, dBlockSum);
            k_dijap_scan_blocks<<<1, 256, 0, s>>>(dBlockSum, nBlocks);
            k_dijap_scan_write<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dTmp, nRows, (const long long*)dBlockSum, f->dDijRowPtr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemsetAsync(dTmp, 0, (size_t)nRows * sizeof(int), s);
        if (e == hipSuccess) {
            k_dijap_fill<<<(unsigned)nSpot, 256, 0, s>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals, nx, ny, box,
                                                         (const long long*)f->dDijRowPtr, dTmp, f->dDijRowsB, f->dDijValsB);
            const unsigned g = (unsigned)std::min<long long>((nRows + 3) / 4, (long long)h->numCUs * 64);
            k_dijap_sort<<<g, 256, 0, s>>>((const long long*)f->dDijRowPtr, nRows, (const int*)f->dDijRowsB, (const float*)f->dDijValsB, f->dDijCCols,
                                           f->dDijCVals);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (the host vectors above are pageable; the scratch is freed below)
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); undo(); return hipFailed(); }
    return done(RTD_OK);
}

// Dij w on the handle's stream: launches only once prepared (the first call prepares, and is synchronous that once).
int rtd_field_dose_influence_apply(rtd_handle hh, rtd_field ff, const float* dev_spot_weights, float* dev_dose, int init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_weights || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply: null device pointer");
    { const int st = matrixOpen(hh, ff, "rtd_field_dose_influence_apply", MatrixStage::kPrepared); if (st != RTD_OK) return st; }
    return dijApplyLaunch(h, f, f->dDijCVals, dev_spot_weights, dev_dose, init);
}

// Dij^T g on the handle's stream (the chunk sums, then their sums per column).
int rtd_field_dose_influence_apply_t(rtd_handle hh, rtd_field ff, const float* dev_voxel_weights, float* dev_spot_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_voxel_weights || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_t: null device pointer");
    { const int st = matrixOpen(hh, ff, "rtd_field_dose_influence_apply_t", MatrixStage::kPrepared); if (st != RTD_OK) return st; }
    return dijApplyTLaunch(h, f, f->dDijVals, dev_voxel_weights, dev_spot_grad);
}

}  // extern "C"
