// rtd_roi_host.hpp — contours -> ROI voxel lists (include/rtd.h; kernels in rtd_roi.hpp). Part of rtd_engine.hip's
// translation unit. Plain owned allocations (DevBuf), like an objective. The host does what is per point and per plane (the transform,
// the planarity check, the planes, the slice assignment); the device does what is per voxel.
#pragma once

namespace {

struct rtd_roi_impl {
    uint32_t dims[3] = {0, 0, 0};
    size_t nVox = 0, nVoxels = 0;
    int nSlots = 0, maskWords = 0;
    rtd_roi_info info{};
    float kernelMs = 0.0f;
    DevBuf<unsigned> dRowMask; DevBuf<int> dSliceSlot, dVoxels;
};

// What every ROI ends with once its packed row mask is on the stream: count, scan, one wait for the total, emit, info. The kernels and
// their order are those rtd_roi_rasterize has always launched; derived ROIs (rtd_roi_ops_host.hpp) end the same way.
struct RoiTail {
    DevBuf<unsigned> dWork; DevBuf<RoiBox> dBox;                       // scratch: freed with this object
    hipEvent_t ev[4] = {};
    int nRows = 0, nRowBlocks = 0;
    ~RoiTail() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    // work: rowCnt[nRows] | rowOff[nRows] | blockSum[nRowBlocks] | total[1]
    hipError_t alloc(int rows) {
        nRows = rows; nRowBlocks = (rows + kRoiBlock - 1) / kRoiBlock;
        RoiBox box;
        for (int a = 0; a < 3; ++a) { box.lo[a] = 0xffffffffu; box.hi[a] = 0u; }
        hipError_t e = dWork.alloc(2 * (size_t)nRows + (size_t)nRowBlocks + 1);
        if (e == hipSuccess) e = dBox.alloc(1);
        if (e == hipSuccess) e = hipMemcpy(dBox, &box, sizeof box, hipMemcpyHostToDevice);
        for (hipEvent_t& evt : ev) if (e == hipSuccess) e = hipEventCreate(&evt);
        return e;
    }
    void begin(rtd_handle_impl* h) { (void)hipEventRecord(ev[0], h->stream); }   // before the kernels that write the row mask
    // r->dRowMask holds nRows rows (slot-major) on the stream; dSlots: the slots' slices. Sets the list, n_voxels, the box and kernelMs.
    hipError_t finish(rtd_handle_impl* h, rtd_roi_impl* r, const RoiSlot* dSlots) {
        const int nx = (int)r->dims[0], ny = (int)r->dims[1];
        unsigned *dRowCnt = dWork, *dRowOff = dWork + nRows, *dBlockSum = dWork + 2 * (size_t)nRows, *dTotal = dBlockSum + nRowBlocks;
        unsigned total = 0u;
        RoiBox box;
        k_roi_count<<<(unsigned)nRowBlocks, kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, dSlots, ny, r->maskWords, nRows, dRowCnt, dBlockSum, dBox);
        k_roi_sums<<<1, kRoiBlock, 0, h->stream>>>(dBlockSum, nRowBlocks, dTotal);
        k_roi_row_offsets<<<(unsigned)nRowBlocks, kRoiBlock, 0, h->stream>>>((const unsigned*)dRowCnt, (const unsigned*)dBlockSum, nRows, dRowOff);
        (void)hipEventRecord(ev[1], h->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, dTotal, sizeof total, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&box, dBox, sizeof box, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess && total) {
            e = r->dVoxels.alloc(total);
            if (e == hipSuccess) {
                (void)hipEventRecord(ev[2], h->stream);
                k_roi_emit<<<(unsigned)((nRows + kRoiBlock / 64 - 1) / (kRoiBlock / 64)), kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, dSlots, (const unsigned*)dRowCnt,
                                                                                                                    (const unsigned*)dRowOff, nx, ny, r->maskWords, nRows, r->dVoxels);
                (void)hipEventRecord(ev[3], h->stream);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            }
        }
        if (e != hipSuccess) return e;
        float a = 0.0f, b = 0.0f;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        if (total) (void)hipEventElapsedTime(&b, ev[2], ev[3]);
        r->kernelMs = a + b;
        r->nVoxels = total;
        r->info.n_voxels = total;
        if (total) for (int i = 0; i < 3; ++i) { r->info.box_lo[i] = box.lo[i]; r->info.box_hi[i] = box.hi[i]; }
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

int rtd_roi_rasterize(rtd_handle hh, const rtd_roi_grid* grid, const rtd_contour_set* cs, rtd_roi* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!grid || !cs || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: null pointer");
    *out = nullptr;
    if (!cs->points || !cs->offsets) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: null pointer");
    const uint32_t nx = grid->dims[0], ny = grid->dims[1], nz = grid->dims[2];
    const size_t nVox = (size_t)nx * ny * nz;
    if (!nx || !ny || !nz || (size_t)nx * ny > (size_t)0x7fffffff || nVox > (size_t)0x7fffffff)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a zero dimension or more than 2^31 - 1 voxels");
    if (!cs->n_contours) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: no contours");
    const float* m = grid->world_to_idx.m;
    const float* v = grid->world_to_idx.v;
    for (int i = 0; i < 9; ++i) if (!std::isfinite(m[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a matrix entry is not finite");
    for (int i = 0; i < 3; ++i) if (!std::isfinite(v[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a matrix entry is not finite");
    if (!(grid->plane_thickness_mm > 0.0f) || !std::isfinite(grid->plane_thickness_mm))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: plane_thickness_mm must be positive and finite");
    const uint32_t nC = cs->n_contours;
    for (uint32_t c = 0; c < nC; ++c) {
        if (cs->offsets[c + 1] < cs->offsets[c]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: the offsets must ascend");
        if (cs->offsets[c + 1] - cs->offsets[c] < 3u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a contour needs at least 3 points");
    }
    if (cs->offsets[nC] > 0x7fffffffu) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: more than 2^31 - 1 points");
    for (size_t i = (size_t)cs->offsets[0] * 3; i < (size_t)cs->offsets[nC] * 3; ++i)
        if (!std::isfinite(cs->points[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a coordinate is not finite");

    // the transform (float64, every operation rounded: this file is built without contraction), the plane coordinate of every contour
    const size_t p0 = cs->offsets[0], nPts = cs->offsets[nC] - p0;
    std::vector<double> pu(nPts), pv(nPts);
    std::vector<double> kcOf(nC);
    for (uint32_t c = 0; c < nC; ++c) {
        for (size_t p = cs->offsets[c]; p < cs->offsets[c + 1]; ++p) {
            const double x = (double)cs->points[3 * p], y = (double)cs->points[3 * p + 1], z = (double)cs->points[3 * p + 2];
            pu[p - p0] = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)v[0];
            pv[p - p0] = (((double)m[3] * x + (double)m[4] * y) + (double)m[5] * z) + (double)v[1];
            const double kc = (((double)m[6] * x + (double)m[7] * y) + (double)m[8] * z) + (double)v[2];
            if (p == cs->offsets[c]) kcOf[c] = kc;
            else if (std::fabs(kc - kcOf[c]) > 1e-3) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a contour is not planar in the grid's k");
        }
    }
    // planes: contours sorted stably by plane coordinate; a plane ends where a contour lies more than 1e-3 above the plane's first one
    std::vector<uint32_t> order(nC);
    for (uint32_t c = 0; c < nC; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kcOf[a] < kcOf[b]; });
    std::vector<double> planeKc;
    std::vector<int> planeEdge;                                        // plane p: edges planeEdge[p] .. planeEdge[p + 1]
    std::vector<RoiEdge> edges;
    edges.reserve(nPts);
    for (uint32_t oi = 0; oi < nC; ++oi) {
        const uint32_t c = order[oi];
        if (planeKc.empty() || kcOf[c] - planeKc.back() > 1e-3) { planeKc.push_back(kcOf[c]); planeEdge.push_back((int)edges.size()); }
        const size_t a0 = cs->offsets[c] - p0, a1 = cs->offsets[c + 1] - p0;
        for (size_t a = a0; a < a1; ++a) { const size_t b = a + 1 < a1 ? a + 1 : a0; edges.push_back(RoiEdge{pu[a], pv[a], pu[b], pv[b]}); }
    }
    planeEdge.push_back((int)edges.size());
    // slices: the nearest plane, a tie to the lower coordinate, within half a slab
    const double slab = (double)grid->plane_thickness_mm * std::sqrt(((double)m[6] * (double)m[6] + (double)m[7] * (double)m[7]) + (double)m[8] * (double)m[8]);
    std::vector<RoiSlot> slots;
    std::vector<int> sliceSlot(nz, -1);
    for (uint32_t k = 0; k < nz; ++k) {
        // the planes ascend, so the nearest is one of the two around k
        const size_t hiP = (size_t)(std::lower_bound(planeKc.begin(), planeKc.end(), (double)k) - planeKc.begin());
        int best = -1;
        double bestD = 0.0;
        for (size_t p = hiP ? hiP - 1 : 0; p < planeKc.size() && p <= hiP; ++p) {
            const double d = std::fabs((double)k - planeKc[p]);
            if (best < 0 || d < bestD) { best = (int)p; bestD = d; }
        }
        if (best >= 0 && bestD <= slab / 2) { sliceSlot[k] = (int)slots.size(); slots.push_back(RoiSlot{(int)k, planeEdge[(size_t)best], planeEdge[(size_t)best + 1], 0}); }
    }

    auto* r = new rtd_roi_impl();
    r->dims[0] = nx; r->dims[1] = ny; r->dims[2] = nz;
    r->nVox = nVox;
    r->nSlots = (int)slots.size();
    r->maskWords = (int)((nx + 31u) / 32u);
    r->info.n_planes = (uint32_t)planeKc.size();
    r->info.n_slices_covered = (uint32_t)slots.size();
    const int nRows = r->nSlots * (int)ny;                             // (rows: at most nz * ny < 2^31)
    DevBuf<RoiEdge> dEdges; DevBuf<RoiSlot> dSlots;                    // scratch: freed when this call returns
    RoiTail tail;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = r->dSliceSlot.alloc(nz);
    if (e == hipSuccess) e = hipMemcpy(r->dSliceSlot, sliceSlot.data(), (size_t)nz * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->dVoxels.alloc(1);      // (replaced by the tail when the list is not empty)
    if (e == hipSuccess && nRows > 0) {
        e = r->dRowMask.alloc((size_t)nRows * r->maskWords);
        if (e == hipSuccess) e = dEdges.alloc(edges.size());
        if (e == hipSuccess) e = dSlots.alloc(slots.size());
        if (e == hipSuccess) e = tail.alloc(nRows);
        if (e == hipSuccess) e = hipMemcpy(dEdges, edges.data(), edges.size() * sizeof(RoiEdge), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dSlots, slots.data(), slots.size() * sizeof(RoiSlot), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            const int nGroups = (int)((ny + kRoiRows - 1) / kRoiRows), nSegs = (int)((nx + kRoiSegBits - 1) / kRoiSegBits);
            const size_t nScanBlocks = (size_t)r->nSlots * nGroups * nSegs;    // (every block holds a voxel of its own: below 2^31)
            tail.begin(h);
            for (size_t base = 0; base < nScanBlocks; base += kRoiMaxBlocks)
                k_roi_scan<<<(unsigned)std::min<size_t>(kRoiMaxBlocks, nScanBlocks - base), kRoiBlock, 0, h->stream>>>(dEdges, dSlots, (int)nx, (int)ny, nGroups, nSegs, r->maskWords,
                                                                                                                     (unsigned)base, r->dRowMask);
            e = tail.finish(h, r, dSlots);
        }
    }
    if (e != hipSuccess) { delete r; RTD_HIP(h, e); }
    *out = reinterpret_cast<rtd_roi>(r);
    return RTD_OK;
}

int rtd_roi_get_info(rtd_handle hh, rtd_roi rr, rtd_roi_info* info) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !info) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_get_info: null pointer");
    *info = r->info;
    return RTD_OK;
}

int rtd_roi_voxels(rtd_handle hh, rtd_roi rr, int32_t* host_out, size_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || (!host_out && r->nVoxels)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_voxels: null pointer");
    if (capacity < r->nVoxels) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_voxels: the capacity is below n_voxels");
    if (!r->nVoxels) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipMemcpy(host_out, r->dVoxels, r->nVoxels * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RTD_OK;
}

int rtd_roi_device(rtd_handle hh, rtd_roi rr, const int32_t** dev_voxels, size_t* n) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_voxels || !n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_device: null pointer");
    *dev_voxels = r->dVoxels;
    *n = r->nVoxels;
    return RTD_OK;
}

int rtd_roi_fill_mask(rtd_handle hh, rtd_roi rr, uint8_t* dev_mask) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_mask) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_fill_mask: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!r->nSlots) {                                                  // no slice took a plane: there is no packed mask to read
        RTD_HIP(h, hipMemsetAsync(dev_mask, 0, r->nVox, h->stream));
        return RTD_OK;
    }
    k_roi_fill<<<(unsigned)((r->nVox + kRoiBlock - 1) / kRoiBlock), kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, (const int*)r->dSliceSlot, (int)r->dims[0], (int)r->dims[1],
                                                                                              r->maskWords, (unsigned)r->nVox, dev_mask);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_roi_kernel_ms(rtd_handle hh, rtd_roi rr, float* ms) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_kernel_ms: null pointer");
    *ms = r->kernelMs;
    return RTD_OK;
}

int rtd_roi_destroy(rtd_handle hh, rtd_roi rr) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h || !r) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete r;
    return RTD_OK;
}

}  // extern "C"
