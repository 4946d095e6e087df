// rtd_roi_ops_host.hpp — derived ROIs: margins, boolean algebra, an ROI from a byte mask (include/rtd.h; kernels in
// rtd_roi_ops.hpp, the cost tables in rtd_roi_tables.hpp). Part of rtd_engine.hip's translation unit, after rtd_roi_host.hpp. Synchronous
// set-up calls like rtd_roi_rasterize: allocations, the kernels that write the packed row mask of the result, then the tail every ROI
// shares (RoiTail: count, scan, one wait for the total, emit). A derived ROI has a slot for every slice of its working region and none
// elsewhere; n_planes and n_slices_covered stay 0.
#pragma once

namespace {

// A result under construction: slots for the slices z0 .. z1 (none when z0 > z1), the row mask allocated but not written.
struct RoiDerived {
    rtd_roi_impl* r = nullptr;
    DevBuf<RoiSlot> dSlots;
    RoiTail tail;
    int nRows = 0;
    ~RoiDerived() { delete r; }                                        // (release() hands the ROI to the caller)
    rtd_roi_impl* release() { rtd_roi_impl* p = r; r = nullptr; return p; }
    hipError_t alloc(rtd_handle_impl* h, const uint32_t dims[3], int z0, int z1) {
        r = new rtd_roi_impl();
        for (int a = 0; a < 3; ++a) r->dims[a] = dims[a];
        r->nVox = (size_t)dims[0] * dims[1] * dims[2];
        r->maskWords = (int)((dims[0] + 31u) / 32u);
        r->nSlots = z0 <= z1 ? z1 - z0 + 1 : 0;
        nRows = r->nSlots * (int)dims[1];
        std::vector<int> sliceSlot(dims[2], -1);
        std::vector<RoiSlot> slots;
        for (int z = z0; z <= z1; ++z) { sliceSlot[(size_t)z] = z - z0; slots.push_back(RoiSlot{z, 0, 0, 0}); }
        hipError_t e = hipSetDevice(h->device);
        if (e == hipSuccess) e = r->dSliceSlot.alloc(dims[2]);
        if (e == hipSuccess) e = hipMemcpy(r->dSliceSlot, sliceSlot.data(), (size_t)dims[2] * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = r->dVoxels.alloc(1);                  // (replaced by the tail when the list is not empty)
        if (e == hipSuccess && nRows > 0) {
            e = r->dRowMask.alloc((size_t)nRows * r->maskWords);
            if (e == hipSuccess) e = dSlots.alloc(slots.size());
            if (e == hipSuccess) e = tail.alloc(nRows);
            if (e == hipSuccess) e = hipMemcpy(dSlots, slots.data(), slots.size() * sizeof(RoiSlot), hipMemcpyHostToDevice);
        }
        return e;
    }
    hipError_t finish(rtd_handle_impl* h) { return nRows > 0 ? tail.finish(h, r, dSlots) : hipSuccess; }
};

// launch(blocks of this piece, the first block's number) for nBlocks blocks, at most kRoiMaxBlocks a launch.
template <typename F>
void roiLaunchPieces(size_t nBlocks, F launch) {
    for (size_t base = 0; base < nBlocks; base += kRoiMaxBlocks) launch((unsigned)std::min<size_t>(kRoiMaxBlocks, nBlocks - base), base);
}

}  // namespace

extern "C" {

int rtd_roi_margin(rtd_handle hh, rtd_roi ss, const float spacing_mm[3], const float margin_mm[6], int contract, rtd_roi* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* src = reinterpret_cast<rtd_roi_impl*>(ss);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!src || !spacing_mm || !margin_mm || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_margin: null pointer");
    if (contract != 0 && contract != 1) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_margin: contract must be 0 or 1");
    RoiTables T;
    if (const char* why = roiMarginTables(spacing_mm, margin_mm, contract == 1, T)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_roi_margin: ") + why);
    const int nx = (int)src->dims[0], ny = (int)src->dims[1], nz = (int)src->dims[2];
    MarginRegion g{};
    g.nx = nx; g.ny = ny; g.nz = nz; g.maskWords = src->maskWords; g.invert = contract;
    for (int i = 0; i < 6; ++i) g.len[i] = T.len[i];
    const bool empty = src->nVoxels == 0;
    if (!empty) {
        const uint32_t *lo = src->info.box_lo, *hi = src->info.box_hi;
        // p = q + d with d in [-len[-], +len[+]]: the source's box grown by the tables; a contraction stays inside the source's box
        const int grow = contract ? 0 : 1;
        g.x0 = std::max(0, (int)lo[0] - grow * g.len[0]); g.x1 = std::min(nx - 1, (int)hi[0] + grow * g.len[1]);
        g.y0 = std::max(0, (int)lo[1] - grow * g.len[2]); g.y1 = std::min(ny - 1, (int)hi[1] + grow * g.len[3]);
        g.z0 = std::max(0, (int)lo[2] - grow * g.len[4]); g.z1 = std::min(nz - 1, (int)hi[2] + grow * g.len[5]);
        g.wx0 = g.x0 & ~31;
        g.nXT = (g.x1 - g.wx0) / 64 + 1;
        // the sources q = p - d of the region; the complement a contraction expands has voxels everywhere in the grid
        g.ly0 = contract ? 0 : (int)lo[1]; g.ly1 = contract ? ny - 1 : (int)hi[1];
        g.zr0 = std::max(g.z0 - g.len[5], contract ? 0 : (int)lo[2]); g.zr1 = std::min(g.z1 + g.len[4], contract ? nz - 1 : (int)hi[2]);
    }
    RoiDerived d;
    DevBuf<float> dTables; DevBuf<unsigned short> dReach;              // scratch: freed when this call returns
    hipError_t e = d.alloc(h, src->dims, empty ? 0 : g.z0, empty ? -1 : g.z1);
    if (e == hipSuccess && !empty) {
        const int RY = g.y1 - g.y0 + 1, nYT = (RY + kMarginRows - 1) / kMarginRows, nYG = (RY + 3) / 4;
        const int nZr = g.zr1 - g.zr0 + 1, nZ = g.z1 - g.z0 + 1, nZG = (nZ + kMarginSlices - 1) / kMarginSlices;
        e = dTables.alloc(3 * kTableWords);
        if (e == hipSuccess && !h->roiMarginNaive) e = dReach.alloc((size_t)nZr * RY * 64 * g.nXT);
        if (e == hipSuccess) e = hipMemcpy(dTables, &T.cost[0][0], sizeof T.cost, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            d.tail.begin(h);
            e = hipMemsetAsync(d.r->dRowMask, 0, (size_t)d.nRows * g.maskWords * sizeof(unsigned), h->stream);
        }
        if (e == hipSuccess) {
            const unsigned* sm = src->dRowMask; const int* ss2 = src->dSliceSlot; const float* tb = dTables;
            unsigned* dm = d.r->dRowMask; unsigned short* rc = dReach; hipStream_t st = h->stream;
            if (h->roiMarginNaive) {
                roiLaunchPieces((size_t)g.nXT * nYG * nZ, [&](unsigned n, size_t base) { k_roi_margin_naive<<<n, kRoiBlock, 0, st>>>(sm, ss2, g, tb, nYG, (unsigned)base, dm); });
            } else {
                roiLaunchPieces((size_t)g.nXT * nYT * nZr, [&](unsigned n, size_t base) { k_roi_margin_xy<<<n, kRoiBlock, 0, st>>>(sm, ss2, g, tb, nYT, (unsigned)base, rc); });
                roiLaunchPieces((size_t)g.nXT * nYG * nZG, [&](unsigned n, size_t base) { k_roi_margin_z<<<n, kRoiBlock, 0, st>>>((const unsigned short*)rc, g, nYG, (unsigned)base, dm); });
            }
            e = d.finish(h);
        }
    }
    RTD_HIP(h, e);
    *out = reinterpret_cast<rtd_roi>(d.release());
    return RTD_OK;
}

int rtd_roi_combine(rtd_handle hh, rtd_roi aa, rtd_roi bb, int op, rtd_roi* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* a = reinterpret_cast<rtd_roi_impl*>(aa);
    auto* b = reinterpret_cast<rtd_roi_impl*>(bb);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!a || !b || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_combine: null pointer");
    if (op != RTD_ROI_OR && op != RTD_ROI_AND && op != RTD_ROI_ANDNOT && op != RTD_ROI_XOR) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_combine: unknown op");
    for (int i = 0; i < 3; ++i) if (a->dims[i] != b->dims[i]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_combine: the two ROIs have different dims");
    // the slices the result can have voxels in (z0 > z1: none)
    const int big = (int)a->dims[2];
    const int a0 = a->nVoxels ? (int)a->info.box_lo[2] : big, a1 = a->nVoxels ? (int)a->info.box_hi[2] : -1;
    const int b0 = b->nVoxels ? (int)b->info.box_lo[2] : big, b1 = b->nVoxels ? (int)b->info.box_hi[2] : -1;
    int z0, z1;
    if (op == RTD_ROI_AND) { z0 = std::max(a0, b0); z1 = std::min(a1, b1); }
    else if (op == RTD_ROI_ANDNOT) { z0 = a0; z1 = a1; }
    else { z0 = std::min(a0, b0); z1 = std::max(a1, b1); }
    if (z0 > z1) { z0 = 0; z1 = -1; }
    RoiDerived d;
    hipError_t e = d.alloc(h, a->dims, z0, z1);
    if (e == hipSuccess && d.nRows > 0) {
        const size_t nWords = (size_t)d.nRows * d.r->maskWords;
        d.tail.begin(h);
        k_roi_combine<<<(unsigned)((nWords + kRoiBlock - 1) / kRoiBlock), kRoiBlock, 0, h->stream>>>((const unsigned*)a->dRowMask, (const int*)a->dSliceSlot, (const unsigned*)b->dRowMask,
                                                                                                  (const int*)b->dSliceSlot, (int)a->dims[1], d.r->maskWords, z0, nWords, op, d.r->dRowMask);
        e = d.finish(h);
    }
    RTD_HIP(h, e);
    *out = reinterpret_cast<rtd_roi>(d.release());
    return RTD_OK;
}

int rtd_roi_from_mask(rtd_handle hh, const uint32_t dims[3], const uint8_t* dev_mask, rtd_roi* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!dims || !dev_mask || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_from_mask: null pointer");
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2];
    if (!nx || !ny || !nz || (size_t)nx * ny > (size_t)0x7fffffff || (size_t)nx * ny * nz > (size_t)0x7fffffff)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_from_mask: a zero dimension or more than 2^31 - 1 voxels");
    RoiDerived d;
    hipError_t e = d.alloc(h, dims, 0, (int)nz - 1);
    if (e == hipSuccess) {
        const int nPieces = (int)((nx + kRoiSegBits - 1) / kRoiSegBits);
        const size_t nWaves = (size_t)d.nRows * nPieces;
        unsigned* dm = d.r->dRowMask; hipStream_t st = h->stream; const int mw = d.r->maskWords;
        d.tail.begin(h);
        roiLaunchPieces((nWaves + kRoiBlock / 64 - 1) / (kRoiBlock / 64), [&](unsigned n, size_t base) { k_roi_from_mask<<<n, kRoiBlock, 0, st>>>(dev_mask, (int)nx, mw, nPieces, nWaves, base, dm); });
        e = d.finish(h);
    }
    RTD_HIP(h, e);
    *out = reinterpret_cast<rtd_roi>(d.release());
    return RTD_OK;
}

}  // extern "C"
