// rtd_dij_compact_host.hpp — host side of the compact form of a field's dose-influence matrix (include/rtd.h "Compact dose-influence
// matrix"; kernels in rtd_dij_compact.hpp): the build, the release of the plain form, the two products and the
// spectral optimiser that runs on them. Part of rtd_engine.hip's translation unit, included last: the optimiser is the plain one of
// rtd_optimizer_host.hpp with `compact` set. The buffers are the field's (classes kDijCompact and kDijCompactRows of its table); what
// exists of the form is f->matrix (rtd_field_matrix.hpp).
#pragma once

namespace {

// The opening of the entry points that read the compact form.
int compactOpen(rtd_handle_impl* h, const rtd_field_impl* f, const std::string& who) {
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, who + ": a remote field has no workspace");
    if (!f->matrix.hasMatrix()) return fail(h, RTD_ERR_NOT_READY, who + ": no dose-influence matrix (call rtd_field_dose_influence first)");
    if (!f->matrix.compact()) return fail(h, RTD_ERR_NOT_READY, who + ": no compact form of the matrix (call rtd_field_dose_influence_compact first)");
    return RTD_OK;
}

const long long* compactRowPtr(const rtd_field_impl* f) { return f->matrix.compactPer() > 1 ? f->dDijcRowPtr : f->dDijRowPtr; }

template <int G, int E>
void compactLaunchApply(rtd_handle_impl* h, rtd_field_impl* f, float* dev_dose, int init, long long nRows) {
    const unsigned g = (unsigned)((nRows * G + 255) / 256);
    auto launch = [&](auto kern) {
        kern<<<g, 256, 0, h->stream>>>(compactRowPtr(f), (const unsigned short*)f->dDijcCCode, (const unsigned short*)f->dDijcCCol, (const float*)f->dDijcWs,
                                       dev_dose, (int)f->doseDims[0], (int)f->doseDims[1], f->matrix.box(), nRows);
    };
    if (init) launch(k_dijc_apply<G, E, true>); else launch(k_dijc_apply<G, E, false>);
}

// Bytes of the plain form's bulk as the table lists it now: the CSC's rows and values, the companion's columns and values, the LET values.
size_t compactPlainBytes(const FieldMatrix& m) {
    return m.resultRows() * sizeof(int) + m.resultValues() * sizeof(float) + m.companionEntries() * (sizeof(int) + sizeof(float)) +
           m.letEntries() * 2 * sizeof(float) + m.letDepths() * sizeof(float);
}

}  // namespace

extern "C" {

void rtd_default_dij_compact_options(rtd_dij_compact_options* o) { std::memset(o, 0, sizeof *o); }

int rtd_field_dose_influence_compact(rtd_handle hh, rtd_field ff, const rtd_dij_compact_options* opt) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    const std::string who = "rtd_field_dose_influence_compact";
    rtd_dij_compact_options o;
    rtd_default_dij_compact_options(&o);
    if (opt) o = *opt;
    for (int r : o.reserved)
        if (r) return fail(h, RTD_ERR_INVALID_ARG, who + ": a reserved word is not zero");
    if (o.release_plain > 1) return fail(h, RTD_ERR_INVALID_ARG, who + ": release_plain must be 0 or 1");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, who + ": a remote field has no workspace");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, who + ": not available with nuclear_corr");
    FieldMatrix& m = f->matrix;
    if (!m.hasMatrix()) return fail(h, RTD_ERR_NOT_READY, who + ": no dose-influence matrix (call rtd_field_dose_influence first)");
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    if (!dijcSpotsFit(nSpot)) return fail(h, RTD_ERR_INVALID_ARG, who + ": more than 65 536 spots (16-bit column indices)");
    // the forward tree: the default, or the one the profiles ask for (read here, once per build)
    int G = kDijcLanes, E = kDijcPer;
    if (const char* v = std::getenv("RTD_DIJC_LANES")) G = std::atoi(v);
    if (const char* v = std::getenv("RTD_DIJC_PER")) E = std::atoi(v);
    if (!dijcTreeAllowed(G, E)) return fail(h, RTD_ERR_INVALID_ARG, who + ": RTD_DIJC_LANES must be 16 or 32 and RTD_DIJC_PER 1, 2 or 4");
    bool wide = false;                                                // RTD_DIJC_ROWS32=1: the CSC side keeps the 32-bit rows whatever the spans are
    if (const char* v = std::getenv("RTD_DIJC_ROWS32")) wide = std::atoi(v) != 0;
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const bool stands = m.compact() && (m.plainReleased() || (m.compactLanes() == G && m.compactPer() == E && (!wide || m.compactRowBits() == 32)));
    if (!stands) {
        if (!m.prepared()) { const int st = rtd_field_dose_influence_prepare(hh, ff); if (st != RTD_OK) return st; }
        RTD_HIP(h, hipStreamSynchronize(s));
        freeBuffers(f, kDijCompact | kDijCompactRows);
        const long long nnz = (long long)m.nnz(), nRows = (long long)m.rows();
        const int nChunks = (int)m.chunks();
        m.compactBegins(G, E, (size_t)nChunks * kDijcChunkGroups);
        DevBuf<unsigned> dFlags, dChunkMax;
        DevBuf<int> dCnt; DevBuf<long long> dBlockSum;                // scratch: freed when this call returns, after the synchronise
        hipError_t e = tryAllocBuffers(f, kDijCompact);
        auto undo = [&]() { (void)hipStreamSynchronize(s); freeBuffers(f, kDijCompact | kDijCompactRows); m.compactFailed(); };
        auto hipFailed = [&]() {
            undo();
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, who + ": a device allocation failed; the compact form is dropped, the matrix stays"); }
            h->error = std::string("HIP error (dose influence compact): ") + hipGetErrorString(e);
            return (int)RTD_ERR_HIP;
        };
        if (e == hipSuccess) e = dFlags.alloc(2);
        if (e == hipSuccess) e = dChunkMax.alloc(std::max<size_t>((size_t)nChunks, 1));
        if (e == hipSuccess) e = hipMemsetAsync(dFlags, 0, 2 * sizeof(unsigned), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijcBase, 0, m.compactCscGroups() * sizeof(int), s);   // (the groups a short chunk does not have read 0)
        if (e != hipSuccess) return hipFailed();
        // 1. column maxima -> scales and the refusal flags; 2. the CSC side and the largest group span
        if (nChunks)
            k_dijc_chunk_max<<<(unsigned)((nChunks + 3) / 4), 256, 0, s>>>((const long long*)f->dDijColPtr, (const float*)f->dDijVals, (const int*)f->dDijChunkCol,
                                                                         (const int*)f->dDijChunkFirst, dChunkMax, nChunks, dFlags);
        k_dijc_scales<<<(unsigned)((nSpot + 3) / 4), 256, 0, s>>>((const int*)f->dDijChunkFirst, (const unsigned*)dChunkMax, f->dDijcScale, (int)nSpot, dFlags);
        if (nChunks)
            k_dijc_pack_csc<<<(unsigned)((nChunks + 3) / 4), 256, 0, s>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals,
                                                                        (const int*)f->dDijChunkCol, (const int*)f->dDijChunkFirst, (const float*)f->dDijcScale,
                                                                        f->dDijcCode, f->dDijcOff, f->dDijcBase, nChunks, dFlags);
        e = hipGetLastError();
        // 3. the companion side's rows, padded to a multiple of E
        long long entries = nnz;
        if (e == hipSuccess && E > 1 && nRows) {
            const int nBlocks = (int)((nRows + kDijApScanItems - 1) / kDijApScanItems);
            e = dCnt.alloc((size_t)nRows);
            if (e == hipSuccess) e = dBlockSum.alloc((size_t)nBlocks);
            if (e == hipSuccess) {
                k_dijc_pad_count<<<(unsigned)((nRows + 255) / 256), 256, 0, s>>>((const long long*)f->dDijRowPtr, nRows, E, dCnt);
                k_dijap_scan_sums<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dCnt, nRows, dBlockSum);
                k_dijap_scan_blocks<<<1, 256, 0, s>>>(dBlockSum, nBlocks);
                k_dijap_scan_write<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dCnt, nRows, (const long long*)dBlockSum, f->dDijcRowPtr);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&entries, f->dDijcRowPtr + nRows, sizeof entries, hipMemcpyDeviceToHost, s);
        } else if (e == hipSuccess && E > 1) {
            e = hipMemsetAsync(f->dDijcRowPtr, 0, sizeof(long long), s);
        }
        unsigned flags[2] = {0, 0};
        if (e == hipSuccess) e = hipMemcpyAsync(flags, dFlags, sizeof flags, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);             // the one read of the device's decisions
        if (e != hipSuccess) return hipFailed();
        if (const char* why = dijcRefusal(flags[0])) { undo(); return fail(h, RTD_ERR_INVALID_ARG, who + ": " + why); }
        if (wide || !dijcOffsetsFit(flags[1])) {                       // a group spans more than 65 535 voxels: the side keeps the 32-bit rows
            (void)hipFree(f->dDijcOff); f->dDijcOff = nullptr;
            m.compactRowsStayWide();
        }
        m.compactCompanionSized((size_t)entries);
        if (entries) {
            e = tryAllocBuffers(f, kDijCompactRows);
            if (e != hipSuccess) return hipFailed();
            k_dijc_pack_rows<<<(unsigned)((nRows * kDijApGroup + 255) / 256), 256, 0, s>>>((const long long*)f->dDijRowPtr, E > 1 ? (const long long*)f->dDijcRowPtr : nullptr,
                                                                                         (const int*)f->dDijCCols, (const float*)f->dDijCVals, (const float*)f->dDijcScale,
                                                                                         f->dDijcCCode, f->dDijcCCol, nRows);
            if (E > 1) k_dijc_tag_pads<<<(unsigned)((nRows + 255) / 256), 256, 0, s>>>((const long long*)f->dDijRowPtr, f->dDijcRowPtr, nRows, E);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hipFailed();
        }
        m.compactBuilt();
    }
    if (o.release_plain && !m.plainReleased()) {
        RTD_HIP(h, hipStreamSynchronize(s));
        const size_t before = compactPlainBytes(m);
        auto drop = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
        drop(f->dDijVals); drop(f->dDijCCols); drop(f->dDijCVals);
        if (m.compactRowBits() == 16) drop(f->dDijRows);
        freeBuffers(f, kDijLet);
        m.plainReleasedNow(before);
    }
    return RTD_OK;
}

int rtd_field_dose_influence_compact_info(rtd_handle hh, rtd_field ff, rtd_dij_compact_info* info) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!info) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_compact_info: null pointer");
    { const int st = compactOpen(h, f, "rtd_field_dose_influence_compact_info"); if (st != RTD_OK) return st; }
    const FieldMatrix& m = f->matrix;
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    std::memset(info, 0, sizeof *info);
    info->value_bits = 16; info->col_bits = 16; info->row_bits = (uint32_t)m.compactRowBits();
    info->lanes_per_row = (uint32_t)m.compactLanes(); info->entries_per_lane = (uint32_t)m.compactPer();
    info->plain_released = m.plainReleased() ? 1 : 0;
    info->nnz = m.nnz(); info->row_entries = m.compactEntries();
    info->compact_bytes = m.compactSpots(nSpot) * 2 * sizeof(float) + (m.compactCscEntries() + m.compactCscOffsets()) * sizeof(unsigned short) +
                          m.compactCscGroups() * sizeof(int) + m.compactRowPtrs() * sizeof(long long) +
                          m.compactCompanionEntries() * 2 * sizeof(unsigned short);
    info->released_bytes = m.plainReleased() ? m.releasedBytes() - compactPlainBytes(m) : 0;
    info->plain_bytes = m.plainReleased() ? m.releasedBytes() : compactPlainBytes(m);
    return RTD_OK;
}

int rtd_field_dose_influence_compact_device(rtd_handle hh, rtd_field ff, rtd_dij_compact_device* d) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!d) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_compact_device: null pointer");
    { const int st = compactOpen(h, f, "rtd_field_dose_influence_compact_device"); if (st != RTD_OK) return st; }
    const FieldMatrix& m = f->matrix;
    std::memset(d, 0, sizeof *d);
    d->scale = f->dDijcScale; d->col_ptr = reinterpret_cast<const int64_t*>(f->dDijColPtr);
    d->csc_code = f->dDijcCode; d->csc_offset = f->dDijcOff; d->csc_base = f->dDijcBase;
    d->csc_rows = m.compactRowBits() == 32 ? f->dDijRows : nullptr;
    d->row_ptr = reinterpret_cast<const int64_t*>(compactRowPtr(f)); d->row_code = f->dDijcCCode; d->row_col = f->dDijcCCol;
    d->nnz = m.nnz(); d->n_groups = m.compactGroups(); d->n_rows = m.rows(); d->row_entries = m.compactEntries();
    const DijBox& b = m.box();
    const int box[6] = {b.x0, b.y0, b.z0, b.bw, b.bh, b.bd};
    std::copy(box, box + 6, d->box);
    return RTD_OK;
}

// Dij w with the compact form on the handle's stream: the scaled weights, then the rows. Launches only.
int rtd_field_dose_influence_apply_compact(rtd_handle hh, rtd_field ff, const float* dev_spot_weights, float* dev_dose, int init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_weights || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_compact: null device pointer");
    { const int st = compactOpen(h, f, "rtd_field_dose_influence_apply_compact"); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipSetDevice(h->device));
    const FieldMatrix& m = f->matrix;
    const long long nRows = (long long)m.rows();
    if (nRows == 0 || (!init && m.nnz() == 0)) return RTD_OK;         // nothing to write: no launch
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L;
    k_dijc_scale_w<<<(unsigned)((nSpot + 255) / 256), 256, 0, h->stream>>>(dev_spot_weights, (const float*)f->dDijcScale, f->dDijcWs, nSpot);
    switch (m.compactLanes() * 8 + m.compactPer()) {
        case 16 * 8 + 1: compactLaunchApply<16, 1>(h, f, dev_dose, init, nRows); break;
        case 16 * 8 + 2: compactLaunchApply<16, 2>(h, f, dev_dose, init, nRows); break;
        case 16 * 8 + 4: compactLaunchApply<16, 4>(h, f, dev_dose, init, nRows); break;
        case 32 * 8 + 1: compactLaunchApply<32, 1>(h, f, dev_dose, init, nRows); break;
        case 32 * 8 + 2: compactLaunchApply<32, 2>(h, f, dev_dose, init, nRows); break;
        default: compactLaunchApply<32, 4>(h, f, dev_dose, init, nRows); break;
    }
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// Dij^T g with the compact form on the handle's stream (the chunk sums, then their sums per column times the scale). Launches only.
int rtd_field_dose_influence_apply_t_compact(rtd_handle hh, rtd_field ff, const float* dev_voxel_weights, float* dev_spot_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_voxel_weights || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_t_compact: null device pointer");
    { const int st = compactOpen(h, f, "rtd_field_dose_influence_apply_t_compact"); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipSetDevice(h->device));
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L, nChunks = (int)f->matrix.chunks();
    if (nChunks) {
        auto launch = [&](auto kern) {
            kern<<<(unsigned)((nChunks + 3) / 4), 256, 0, h->stream>>>((const long long*)f->dDijColPtr, (const unsigned short*)f->dDijcCode, (const unsigned short*)f->dDijcOff,
                                                                     (const int*)f->dDijcBase, (const int*)f->dDijRows, (const int*)f->dDijChunkCol,
                                                                     (const int*)f->dDijChunkFirst, dev_voxel_weights, f->dDijPartial, nChunks);
        };
        if (f->matrix.compactRowBits() == 32) launch(k_dijc_apply_t<true>); else launch(k_dijc_apply_t<false>);
    }
    k_dijc_reduce_t<<<(unsigned)((nSpot + 3) / 4), 256, 0, h->stream>>>((const int*)f->dDijChunkFirst, (const float*)f->dDijPartial, (const float*)f->dDijcScale,
                                                                       dev_spot_grad, nSpot);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The spectral optimisers of rtd_optimizer_create, _create_robust and _create_voxelwise whose two products are the compact ones
// (the last two: DESIGN.md section 29; the checks and the iteration are optCreate's and rtd_optimizer_run's).
int rtd_optimizer_create_compact(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_optimizer_options* opt,
                                 rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    return optCreate(hh, fields, n_fields, nullptr, oo, opt, out, false, true);
}

int rtd_optimizer_create_robust_compact(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_robust_options* robust, rtd_objective oo,
                                        const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!robust) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust_compact: null pointer");
    if (out) *out = nullptr;
    return optCreate(hh, fields, n_fields, robust, oo, opt, out, false, true);
}

int rtd_optimizer_create_voxelwise_compact(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, uint32_t n_scenarios, rtd_objective oo,
                                           const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    rtd_robust_options ro{};
    ro.mode = RTD_ROBUST_EXPECTED; ro.n_scenarios = n_scenarios;
    return optCreate(hh, fields, n_fields, &ro, oo, opt, out, true, true);
}

}  // extern "C"
