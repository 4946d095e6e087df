// rtd_rbe_host.hpp — host side of the variable-RBE dose (include/rtd.h; kernels in rtd_rbe.hpp). Part of
// rtd_engine.hip's translation unit, included at its end, after rtd_let_host.hpp: an rtd_rbe object is a class volume (one byte per
// voxel) and a table of six floats per class, both plain owned allocations; the optimiser's RBE mode lives in the object of
// rtd_optimizer_host.hpp, which launches the two kernels through rbeOptForward / rbeOptBackward below.
#pragma once

namespace {

struct rtd_rbe_impl {
    uint32_t dims[3] = {0, 0, 0};
    size_t nVox = 0;
    int nClasses = 0;
    DevBuf<unsigned char> dClasses;
    DevBuf<float> dTable;          // [kRbeCoefs][kRbeMaxClasses]: a0 a1 b0 b1 alpha_x beta_x, zero beyond nClasses
};

// The six numbers of a tissue, each formed in float64 from the float fields and rounded once; false when the tissue is refused.
bool rbeCoefficients(const rtd_rbe_tissue* t, float out[kRbeCoefs]) {
    if (!(t->alpha_x > 0.0f) || !std::isfinite(t->alpha_x) || !(t->beta_x > 0.0f) || !std::isfinite(t->beta_x)) return false;
    for (int i = 0; i < 2; ++i)
        if (!std::isfinite(t->rbe_max[i]) || !std::isfinite(t->rbe_min[i]) || t->reserved[i] != 0u) return false;
    const double ax = (double)t->alpha_x, sb = std::sqrt((double)t->beta_x);
    out[0] = (float)(ax * (double)t->rbe_max[0]); out[1] = (float)(ax * (double)t->rbe_max[1]);
    out[2] = (float)(sb * (double)t->rbe_min[0]); out[3] = (float)(sb * (double)t->rbe_min[1]);
    out[4] = t->alpha_x; out[5] = t->beta_x;
    return true;
}

// Class c's column of the device table, on the handle's stream like everything that reads it. Synchronous (coef is the caller's).
hipError_t rbeUploadClass(rtd_handle_impl* h, rtd_rbe_impl* r, int c, const float coef[kRbeCoefs]) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < kRbeCoefs && e == hipSuccess; ++k)
        e = hipMemcpyAsync(r->dTable + k * kRbeMaxClasses + c, &coef[k], sizeof(float), hipMemcpyHostToDevice, h->stream);
    const hipError_t w = hipStreamSynchronize(h->stream);
    return e == hipSuccess ? w : e;
}

// box: NULL (the grid) or inclusive min[3], max[3] inside the grid.
bool rbeBoxOf(const rtd_rbe_impl* r, const int32_t* box, DijBox& out) {
    if (!box) { out = DijBox{0, 0, 0, (int)r->dims[0], (int)r->dims[1], (int)r->dims[2]}; return true; }
    for (int a = 0; a < 3; ++a)
        if (box[a] < 0 || box[a] > box[3 + a] || (uint32_t)box[3 + a] >= r->dims[a]) return false;
    out = DijBox{box[0], box[1], box[2], box[3] - box[0] + 1, box[4] - box[1] + 1, box[5] - box[2] + 1};
    return true;
}

unsigned rbeGrid(const rtd_handle_impl* h, const DijBox& b) {          // a wave per line, four to a block, grid-stride beyond 8 blocks per CU
    const long long lines = (long long)b.bh * b.bd;
    return (unsigned)std::max<long long>(1, std::min<long long>((lines + 3) / 4, (long long)h->numCUs * 8));
}
bool rbeAligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

void rbeForwardLaunch(rtd_handle_impl* h, const rtd_rbe_impl* r, const float* dose, const float* letDose, const DijBox& b, float* out) {
    const int wide = rbeAligned(dose, 16) && rbeAligned(letDose, 16) && rbeAligned(out, 16) && rbeAligned(r->dClasses.p, 4) ? 1 : 0;
    k_rbe_forward<<<rbeGrid(h, b), 256, 0, h->stream>>>(dose, letDose, (const unsigned char*)r->dClasses, (const float*)r->dTable, r->nClasses, (int)r->dims[0],
                                                        (int)r->dims[1], b, wide, out);
}
void rbeBackwardLaunch(rtd_handle_impl* h, const rtd_rbe_impl* r, const float* dose, const float* letDose, const float* gRbe, const DijBox& b, float* gDose,
                       float* gLet) {
    const int wide = rbeAligned(dose, 16) && rbeAligned(letDose, 16) && rbeAligned(gRbe, 16) && rbeAligned(gDose, 16) && rbeAligned(gLet, 16) &&
                     rbeAligned(r->dClasses.p, 4) ? 1 : 0;
    k_rbe_backward<<<rbeGrid(h, b), 256, 0, h->stream>>>(dose, letDose, gRbe, (const unsigned char*)r->dClasses, (const float*)r->dTable, r->nClasses,
                                                         (int)r->dims[0], (int)r->dims[1], b, wide, gDose, gLet);
}

// Steps 3 and 5 of an iteration with an RBE model (rtd_optimizer_run): on the union of the fields' row boxes, nothing when it is empty.
int rbeOptForward(rtd_handle_impl* h, rtd_optimizer_impl* p) {
    if (p->rbeBox.bw > 0) rbeForwardLaunch(h, p->rbe, p->dDose, p->dLetDose, p->rbeBox, p->dRbeDose);
    return RTD_OK;
}
int rbeOptBackward(rtd_handle_impl* h, rtd_optimizer_impl* p) {
    if (p->rbeBox.bw > 0) rbeBackwardLaunch(h, p->rbe, p->dDose, p->dLetDose, p->dRbeG, p->rbeBox, p->dG, p->dLetG);
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_rbe_create(rtd_handle hh, const uint32_t dose_dims[3], const rtd_rbe_tissue* default_tissue, rtd_rbe* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dose_dims || !default_tissue || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_create: null pointer");
    *out = nullptr;
    const size_t nVox = (size_t)dose_dims[0] * dose_dims[1] * dose_dims[2];
    if (!dose_dims[0] || !dose_dims[1] || !dose_dims[2] || (size_t)dose_dims[0] * dose_dims[1] > (size_t)0x7fffffff || nVox > (size_t)0x7fffffff)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_create: a zero dimension or more than 2^31 - 1 voxels");
    float coef[kRbeCoefs];
    if (!rbeCoefficients(default_tissue, coef))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_create: the tissue needs finite alpha_x > 0 and beta_x > 0, finite line coefficients and zero reserved words");
    RTD_HIP(h, hipSetDevice(h->device));
    auto* r = new rtd_rbe_impl();
    for (int a = 0; a < 3; ++a) r->dims[a] = dose_dims[a];
    r->nVox = nVox; r->nClasses = 1;
    hipError_t e = r->dClasses.alloc(nVox);
    if (e == hipSuccess) e = r->dTable.alloc((size_t)kRbeCoefs * kRbeMaxClasses);
    if (e == hipSuccess) e = hipMemsetAsync(r->dClasses, 0, nVox, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->dTable, 0, (size_t)kRbeCoefs * kRbeMaxClasses * sizeof(float), h->stream);
    if (e == hipSuccess) e = rbeUploadClass(h, r, 0, coef);
    if (e != hipSuccess) {
        (void)hipGetLastError(); (void)hipStreamSynchronize(h->stream);
        delete r;
        return fail(h, e == hipErrorOutOfMemory ? RTD_ERR_OUT_OF_MEMORY : RTD_ERR_HIP, std::string("rtd_rbe_create: ") + hipGetErrorString(e));
    }
    *out = reinterpret_cast<rtd_rbe>(r);
    return RTD_OK;
}

int rtd_rbe_add_tissue(rtd_handle hh, rtd_rbe rr, const rtd_rbe_tissue* tissue, int32_t* class_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !tissue || !class_id) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_add_tissue: null pointer");
    float coef[kRbeCoefs];
    if (!rbeCoefficients(tissue, coef))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_add_tissue: the tissue needs finite alpha_x > 0 and beta_x > 0, finite line coefficients and zero reserved words");
    if (r->nClasses >= kRbeMaxClasses) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_add_tissue: 256 classes at the most");
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, rbeUploadClass(h, r, r->nClasses, coef));              // (beyond nClasses: nothing reads the column until the count moves)
    *class_id = r->nClasses++;
    return RTD_OK;
}

int rtd_rbe_assign_voxels(rtd_handle hh, rtd_rbe rr, const int32_t* host_voxels, size_t n, int32_t class_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || (!host_voxels && n)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_voxels: null pointer");
    if (class_id < 0 || class_id >= r->nClasses) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_voxels: unknown class");
    for (size_t i = 0; i < n; ++i)
        if (host_voxels[i] < 0 || (size_t)host_voxels[i] >= r->nVox) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_voxels: a voxel index is outside the grid");
    if (!n) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    DevBuf<int> dList;                                                // scratch: freed when this call returns, after the wait
    hipError_t e = dList.alloc(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dList, host_voxels, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        k_rbe_scatter<<<(unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->numCUs * 8), 256, 0, h->stream>>>((const int*)dList, n, (unsigned char)class_id, r->dClasses);
        e = hipGetLastError();
    }
    const hipError_t w = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = w;
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, e == hipErrorOutOfMemory ? RTD_ERR_OUT_OF_MEMORY : RTD_ERR_HIP, std::string("rtd_rbe_assign_voxels: ") + hipGetErrorString(e)); }
    return RTD_OK;
}

int rtd_rbe_assign_roi(rtd_handle hh, rtd_rbe rr, rtd_roi roi, int32_t class_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    auto* q = reinterpret_cast<rtd_roi_impl*>(roi);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !q) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_roi: null pointer");
    if (class_id < 0 || class_id >= r->nClasses) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_roi: unknown class");
    for (int a = 0; a < 3; ++a)
        if (q->dims[a] != r->dims[a]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_assign_roi: the ROI must be on the object's dose grid");
    if (!q->nVoxels) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    k_rbe_scatter<<<(unsigned)std::min<size_t>((q->nVoxels + 255) / 256, (size_t)h->numCUs * 8), 256, 0, h->stream>>>((const int*)q->dVoxels, q->nVoxels,
                                                                                                                    (unsigned char)class_id, r->dClasses);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_rbe_classes_device(rtd_handle hh, rtd_rbe rr, const uint8_t** dev_classes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_classes) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_classes_device: null pointer");
    *dev_classes = r->dClasses;
    return RTD_OK;
}

int rtd_rbe_dose(rtd_handle hh, rtd_rbe rr, const float* dev_dose, const float* dev_let_dose, const int32_t box[6], float* dev_rbe_dose) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_dose || !dev_let_dose || !dev_rbe_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_dose: null pointer");
    DijBox b;
    if (!rbeBoxOf(r, box, b)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_dose: the box must lie inside the grid with min <= max");
    RTD_HIP(h, hipSetDevice(h->device));
    rbeForwardLaunch(h, r, dev_dose, dev_let_dose, b, dev_rbe_dose);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_rbe_backward(rtd_handle hh, rtd_rbe rr, const float* dev_dose, const float* dev_let_dose, const float* dev_g_rbe, const int32_t box[6],
                     float* dev_g_dose, float* dev_g_let) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_dose || !dev_let_dose || !dev_g_rbe || !dev_g_dose || !dev_g_let) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_backward: null pointer");
    if (dev_g_dose == dev_g_let) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_backward: the two outputs must be two volumes");
    DijBox b;
    if (!rbeBoxOf(r, box, b)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_rbe_backward: the box must lie inside the grid with min <= max");
    RTD_HIP(h, hipSetDevice(h->device));
    rbeBackwardLaunch(h, r, dev_dose, dev_let_dose, dev_g_rbe, b, dev_g_dose, dev_g_let);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_rbe_destroy(rtd_handle hh, rtd_rbe rr) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h || !r) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete r;
    return RTD_OK;
}

// The RBE model of a plain optimiser: everything it needs is allocated here, never in rtd_optimizer_run.
int rtd_optimizer_set_rbe(rtd_handle hh, rtd_optimizer pp, rtd_rbe rr) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    auto* r = reinterpret_cast<rtd_rbe_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: null optimiser");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!r) {                                                         // removes it (the stream may still read the volumes)
        if (!p->rbe) return RTD_OK;
        // g_d filled the box of the voxel gradient: g_R * fd, which outside the objective's voxels is 0 * fd (a -0, or a NaN where fd
        // overflowed). Without a model only the objective's voxels are written and the rest is read as the +0 of the allocation.
        RTD_HIP(h, hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        p->rbe = nullptr; p->rbeBox = DijBox{0, 0, 0, 0, 0, 0};
        p->dRbeDose.reset(); p->dRbeG.reset(); p->dLetDose.reset(); p->dLetG.reset(); p->dLetGrad.reset();
        return RTD_OK;
    }
    if (p->robust) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: not available for a robust or voxel-wise optimiser");
    if (p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: not available for an L-BFGS optimiser");
    if (p->constrained) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: not available for a constrained optimiser");
    if (p->compact) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: not available for a compact optimiser (no compact LET values)");
    if (p->letObj) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: the optimiser has a LET objective (one or the other)");
    for (int a = 0; a < 3; ++a)
        if (r->dims[a] != p->obj->dims[a]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_rbe: the RBE object must be on the optimiser's dose grid");
    for (const rtd_field_impl* f : p->fields)
        if (!letReady(h, f)) return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_set_rbe: a field has no LET-weighted matrix (call rtd_field_let_influence first)");
    if (!p->rbe) {
        const size_t nGrad = std::max<size_t>((size_t)p->n, 1);
        hipError_t e = p->dLetDose.alloc(p->nVox);
        if (e == hipSuccess) e = p->dLetG.alloc(p->nVox);
        if (e == hipSuccess) e = p->dRbeDose.alloc(p->nVox);
        if (e == hipSuccess) e = p->dRbeG.alloc(p->nVox);
        if (e == hipSuccess) e = p->dLetGrad.alloc(nGrad);
        for (float* v : {p->dLetDose.p, p->dLetG.p, p->dRbeDose.p, p->dRbeG.p})
            if (e == hipSuccess) e = hipMemsetAsync(v, 0, p->nVox * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->dLetGrad, 0, nGrad * sizeof(float), h->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError(); (void)hipStreamSynchronize(h->stream);
            p->dRbeDose.reset(); p->dRbeG.reset(); p->dLetDose.reset(); p->dLetG.reset(); p->dLetGrad.reset();
            return fail(h, e == hipErrorOutOfMemory ? RTD_ERR_OUT_OF_MEMORY : RTD_ERR_HIP, std::string("rtd_optimizer_set_rbe: ") + hipGetErrorString(e));
        }
    }
    // the union of the fields' row boxes, once: dose and LET-weighted dose are zero outside it, and so stay R, g_d and g_n
    int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
    bool any = false;
    for (const rtd_field_impl* f : p->fields) {
        if (!f->matrix.rows()) continue;
        const DijBox& b = f->matrix.box();
        const int fl[3] = {b.x0, b.y0, b.z0}, fh[3] = {b.x0 + b.bw - 1, b.y0 + b.bh - 1, b.z0 + b.bd - 1};
        for (int a = 0; a < 3; ++a) { lo[a] = any ? std::min(lo[a], fl[a]) : fl[a]; hi[a] = any ? std::max(hi[a], fh[a]) : fh[a]; }
        any = true;
    }
    p->rbeBox = any ? DijBox{lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1} : DijBox{0, 0, 0, 0, 0, 0};
    p->rbe = r;
    return RTD_OK;
}

int rtd_optimizer_rbe_dose(rtd_handle hh, rtd_optimizer pp, const float** dev) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_rbe_dose: null pointer");
    if (!p->rbe) return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_rbe_dose: the optimiser has no RBE model");
    *dev = p->dRbeDose;
    return RTD_OK;
}

}  // extern "C"
